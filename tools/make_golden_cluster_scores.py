#!/usr/bin/env python3
"""Golden vectors of the clustering scores and the hits-per-cluster histogram, FROM THE REFERENCE ITSELF:
``tests/golden/g21_cluster_scores.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``, default
``/root/reference``) with pandas and scikit-learn, through the stand-ins of ``oracle/_ref_standins.py`` (as
``tools/make_golden_tracking_metrics.py``).  The file holds data only.  Per case ``<name>``:

* ``<name>/truth``, ``<name>/predicted``: the inputs (int64);
* ``<name>/scores``: the reference's ``common_metrics`` ``v_measure``, ``homogeneity``, ``completeness``,
  ``adjusted_rand``, ``fowlkes_mallows`` (``score_keys``) of ``truth=``, ``predicted=``, fp64;
* ``<name>/hist``: the reference's ``count_hits_per_cluster(predicted)``;
* ``<name>/flat_keys``, ``<name>/flat_values``: its ``hits_per_cluster_count_to_flat_dict`` of that.

Cases: ``td3_0, td3_1, blobs, ptedge, naneta, recomix`` of ``g17_tracking_metrics.npz`` (labels and particle
ids), its three scan batches with the reference's DBSCAN labels kept in ``g20_tracking_binned.npz``, and hand
cases that pin the rules for zero entropy and for labels as categories (``HAND``).  ``sklearn_version``: the
version the reference delegated to.

Usage:  python tools/make_golden_cluster_scores.py [--ref PATH]
"""

from __future__ import annotations

import argparse
import os
import pathlib
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
G17 = REPO / "tests" / "golden" / "g17_tracking_metrics.npz"
G20 = REPO / "tests" / "golden" / "g20_tracking_binned.npz"
OUT = REPO / "tests" / "golden" / "g21_cluster_scores.npz"
EVENTS = ("td3_0", "td3_1", "blobs", "ptedge", "naneta", "recomix")
SCORE_KEYS = ("v_measure", "homogeneity", "completeness", "adjusted_rand", "fowlkes_mallows")

_T12 = [5, 5, 5, 5, 9, 9, 9, 0, 0, 0, 0, 2]
#: name -> (truth, predicted)
HAND = {
    "identical": (_T12, _T12),                                                  # every score 1
    "renamed": (_T12, [-1, -1, -1, -1, 3, 3, 3, 70, 70, 70, 70, 0]),            # a permutation of the label names
    "one_cluster": (_T12, [4] * 12),                                            # H(K) = 0: completeness 1, v 0
    "singletons": (_T12, list(range(12))),                                      # every hit its own cluster
    "one_class": ([7] * 12, [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2]),              # H(C) = 0: homogeneity 1
    "one_class_one_cluster": ([7] * 12, [-1] * 12),                             # both entropies 0
    "singletons_vs_one_class": ([0] * 6, list(range(6))),
    "n1": ([3], [-1]),
    "any_int64": ([2 ** 62, -2 ** 62, 0, 0, -2 ** 62, 2 ** 62, 0, 1, 1, 2 ** 62],
                  [-1, -7, 2 ** 62, -2 ** 62, -7, -1, 2 ** 62, -1, -7, -1]),    # labels are categories of any value
    "ref_test": ([0, 0, 1, 1, 1, 2, 2, 3, 3], [0, 0, 0, 1, 1, 2, 3, 3, 3]),     # test_cluster_metrics.py: hist [1, 1, 2]
}


def install(ref: pathlib.Path):
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", default="/root/reference", type=pathlib.Path)
    args = ap.parse_args()
    install(args.ref)
    import sklearn
    from gnn_tracking.metrics.cluster_metrics import (common_metrics, count_hits_per_cluster,
                                                      hits_per_cluster_count_to_flat_dict)

    assert list(common_metrics) == ["v_measure", "homogeneity", "completeness", "trk", "adjusted_rand",
                                    "fowlkes_mallows"], list(common_metrics)
    g17, g20 = np.load(G17), np.load(G20)
    cases = {name: (g17[f"{name}/pid"], g17[f"{name}/labels"]) for name in EVENTS}
    for i in range(3):
        cases[f"scan_b{i}"] = (g17[f"scan/b{i}/pid"], g20[f"scan/b{i}/labels"])
    cases.update(HAND)

    arrs = {"score_keys": np.array(SCORE_KEYS, dtype=np.str_), "sklearn_version": np.array(sklearn.__version__),
            "names": np.array(list(cases), dtype=np.str_)}
    g = np.random.default_rng(210)
    for name, (truth, predicted) in cases.items():
        truth, predicted = np.asarray(truth, dtype=np.int64), np.asarray(predicted, dtype=np.int64)
        assert truth.shape == predicted.shape and truth.ndim == 1
        scores = np.array([float(common_metrics[k](truth=truth, predicted=predicted)) for k in SCORE_KEYS])
        hist = np.asarray(count_hits_per_cluster(predicted), dtype=np.int64)
        # the ClusterMetricType convention: further keyword arguments are ignored
        assert float(common_metrics["v_measure"](truth=truth, predicted=predicted, pts=None)) == scores[0]
        # the histogram does not depend on the hit order; the scores may in their last bits (sklearn's sums
        # run in the order of the sorted labels, which a permutation of the hits keeps)
        perm = g.permutation(len(truth))
        assert np.array_equal(count_hits_per_cluster(predicted[perm]), hist)
        flat = hits_per_cluster_count_to_flat_dict(hist)
        arrs[f"{name}/truth"], arrs[f"{name}/predicted"] = truth, predicted
        arrs[f"{name}/scores"], arrs[f"{name}/hist"] = scores, hist
        arrs[f"{name}/flat_keys"] = np.array(list(flat), dtype=np.str_)
        arrs[f"{name}/flat_values"] = np.array([float(v) for v in flat.values()], dtype=np.float64)
        print(f"  {name}: n = {len(truth)}, scores {scores.tolist()}, hist of {len(hist)} sizes")
    assert arrs["ref_test/hist"].tolist() == [1, 1, 2]
    np.savez_compressed(OUT, **arrs)
    size = OUT.stat().st_size
    assert size < 200_000, size
    print(f"wrote {OUT.relative_to(REPO)} ({size / 1024:.1f} KiB), sklearn {sklearn.__version__}")


if __name__ == "__main__":
    main()
