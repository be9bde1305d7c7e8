#!/usr/bin/env python3
"""Golden vectors of the edge-classifier validation metrics, FROM THE REFERENCE ITSELF:
``tests/golden/g16_ec_metrics.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``,
default ``/root/reference``).  It installs the stand-ins of ``oracle/_ref_standins.py`` for the
third-party packages the reference imports, and replaces ``torchmetrics.classification.BinaryAUROC``
(not installed) by a class backed by ``sklearn.metrics.roc_auc_score``: torchmetrics' ``max_fpr`` code
is a port of sklearn's (linear interpolation at ``max_fpr``, McClish standardisation), so this is the
closest stand-in available; both raise for a single class, which the reference's wrapper turns into
NaN, and sklearn also raises for NaN scores.  It then runs the reference's own
``get_maximized_bcs``, ``get_roc_auc_scores``, ``BinaryClassificationStats`` and the loop body of
``ECModule.validation_step`` (training/ec.py:66-80) on:

* ``g1``: the reference ``W`` of the golden test graph (tests/golden/g1_ec_testgraph.npz) with its BCE
  loss (the ``total`` of the validation step);
* ``ties``: scores drawn from seven values (exact linspace thresholds, both signed zeros), pt values
  exactly 0.5, 0.9 and 1.5 as fp32 and a NaN pt;
* ``saturated``: a trained classifier's {0.001, 0.999} scores;
* ``nanscore``: NaN scores on low-pt edges (AUCs NaN for the cuts that keep them);
* ``nopos`` / ``empty``: a cut with no positives, a cut with no edges.

Usage:  python tools/make_golden_ec_metrics.py [--ref PATH]
"""

from __future__ import annotations

import argparse
import os
import pathlib
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "g16_ec_metrics.npz"
PT_THLDS = (0.0, 0.5, 0.9, 1.5)
MAX_FPRS = (None, 0.01, 0.001)
BCS_THLDS = (0.5, 0.25)


def install(ref: pathlib.Path):
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins
    from sklearn.metrics import roc_auc_score as sk_auc

    _ref_standins.install()

    class BinaryAUROC:
        """torchmetrics.classification.BinaryAUROC stand-in: sklearn's roc_auc_score in float64."""

        def __init__(self, max_fpr=None, **_kw):
            self.max_fpr = max_fpr

        def to(self, *a, **k):
            return self

        def __call__(self, preds, target):
            return torch.tensor(sk_auc(target.cpu().numpy(), preds.cpu().numpy(), max_fpr=self.max_fpr),
                                dtype=torch.float64)

    sys.modules["torchmetrics.classification"].BinaryAUROC = BinaryAUROC


def graph(seed, n_nodes, n_edges):
    g = np.random.default_rng(seed)
    ei = g.integers(0, n_nodes, size=(2, n_edges)).astype(np.int64)
    pt = g.lognormal(0.0, 0.7, size=n_nodes).astype(np.float32)
    return g, ei, pt


def cases():
    z = np.load(REPO / "tests" / "golden" / "g1_ec_testgraph.npz")
    out = {"g1": dict(w=z["W"], y=z["y"], pt=z["pt"], edge_index=z["edge_index"])}
    thl = torch.linspace(0.0, 1.0, 200).numpy()

    g, ei, pt = graph(16, 300, 3001)
    pt[:12] = np.float32(0.5)
    pt[12:24] = np.float32(0.9)
    pt[24:36] = np.float32(1.5)
    pt[36:40] = np.nan
    vals = np.array([-0.0, 0.0, thl[37], thl[100], thl[199], 0.25, 0.5], dtype=np.float32)
    w = vals[g.integers(0, len(vals), size=ei.shape[1])]
    y = g.random(ei.shape[1]) < 0.3 + 0.4 * (w > 0.3)
    out["ties"] = dict(w=w, y=y, pt=pt, edge_index=ei)

    g, ei, pt = graph(17, 500, 4097)
    y = g.random(ei.shape[1]) < 0.31
    good = g.random(ei.shape[1]) < 0.93
    w = np.where(y == good, np.float32(0.999), np.float32(0.001)).astype(np.float32)
    out["saturated"] = dict(w=w, y=y, pt=pt, edge_index=ei)

    g, ei, pt = graph(18, 200, 1500)
    w = g.random(ei.shape[1]).astype(np.float32)
    y = g.random(ei.shape[1]) < 0.2 + 0.6 * w
    low = (pt[ei[0]] <= 0.9) & (pt[ei[1]] <= 0.9)
    w[np.nonzero(low)[0][:3]] = np.nan
    out["nanscore"] = dict(w=w, y=y, pt=pt, edge_index=ei)

    g, ei, pt = graph(19, 150, 900)
    pt = np.minimum(pt, np.float32(1.2))
    pt[:5] = np.float32(3.0)
    w = g.random(ei.shape[1]).astype(np.float32)
    high = (pt[ei[0]] > 1.5) | (pt[ei[1]] > 1.5)
    y = (g.random(ei.shape[1]) < 0.4) & ~high
    out["nopos"] = dict(w=w, y=y, pt=pt, edge_index=ei)

    g, ei, pt = graph(20, 100, 640)
    pt = np.minimum(pt, np.float32(1.4))
    w = g.random(ei.shape[1]).astype(np.float32)
    y = g.random(ei.shape[1]) < 0.5
    out["empty"] = dict(w=w, y=y, pt=pt, edge_index=ei)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", default="/root/reference", type=pathlib.Path)
    args = ap.parse_args()
    install(args.ref)
    from gnn_tracking.metrics.binary_classification import (BinaryClassificationStats, get_maximized_bcs,
                                                            get_roc_auc_scores)
    from gnn_tracking.utils.nomenclature import denote_pt

    torch.set_num_threads(4)
    arrs = {}
    for name, c in cases().items():
        W = torch.from_numpy(c["w"])
        Y = torch.from_numpy(c["y"])
        PT = torch.from_numpy(c["pt"])
        EI = torch.from_numpy(c["edge_index"])
        metrics = {}
        for pt in PT_THLDS:   # training/ec.py:66-80
            if pt > 0:
                pt_mask = (PT[EI[0]] > pt) | (PT[EI[1]] > pt)
                w, y = W[pt_mask], Y[pt_mask]
            else:
                w, y = W, Y
            _metrics = get_roc_auc_scores(true=y, predicted=w, max_fprs=[None, 0.01, 0.001]) | get_maximized_bcs(
                y=y, output=w)
            metrics |= denote_pt(_metrics, pt)
        assert len(metrics) == 44, len(metrics)
        for k, v in c.items():
            arrs[f"{name}/{k}"] = v
        arrs[f"{name}/keys"] = np.array(list(metrics), dtype=np.str_)
        arrs[f"{name}/values"] = np.array([float(v) for v in metrics.values()], dtype=np.float64)
        bcs = [BinaryClassificationStats(output=W, y=Y, thld=t).get_all() for t in BCS_THLDS]
        arrs[f"{name}/bcs_keys"] = np.array(list(bcs[0]), dtype=np.str_)
        arrs[f"{name}/bcs_values"] = np.array([[float(v) for v in b.values()] for b in bcs], dtype=np.float64)
        print(f"  {name}: E={W.numel()}  roc_auc={metrics['roc_auc']:.6f}  max_mcc_pt0.9={metrics['max_mcc_pt0.9']:.6f}")
    arrs["bcs_thlds"] = np.array(BCS_THLDS, dtype=np.float64)
    arrs["g1/total"] = np.load(REPO / "tests" / "golden" / "g1_ec_testgraph.npz")["loss"]
    np.savez_compressed(OUT, **arrs)
    print(f"wrote {OUT.relative_to(REPO)} ({OUT.stat().st_size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
