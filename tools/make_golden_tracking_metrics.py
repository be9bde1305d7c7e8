#!/usr/bin/env python3
"""Golden vectors of the object-condensation tracking metrics, FROM THE REFERENCE ITSELF:
``tests/golden/g17_tracking_metrics.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``,
default ``/root/reference``) with pandas, scikit-learn and scipy.  It installs the stand-ins of
``oracle/_ref_standins.py`` for the other third-party packages the reference imports, then runs the
reference's own ``tracking_metrics`` + ``flatten_track_metrics`` (metrics/cluster_metrics.py) on:

* ``td3``: sklearn DBSCAN labels, two (eps, min_samples), of condensed latent coordinates (one blob
  per particle, see ``scan_batches``) of G5's ``td3`` hits (1500 hits, 120 particles);
* ``blobs``: hand-made clusters with noise (-1 and other negative labels), clusters below 3 hits,
  split and merged particles;
* ``ptedge``: pt exactly 0.5f / 0.9f / 1.5f, particles whose hits differ in pt so that the mean decides;
* ``naneta``: NaN pt and eta on some hits, |eta| = 4.0 exactly;
* ``recomix`` / ``recobool``: reconstructable mixed within a particle, as float and as bool;
* ``nocut``: a cut no particle passes (NaN rates);
* ``noise``: all-noise labels;  ``empty``: no hits;
* ``scan``: ``DBSCANHyperParamScannerFixed`` (the reference's DBSCANFastRescan on sklearn) over three
  batches, then ``get_foms()``: its per-trial records and the figures of merit.

Every case is accepted only if the reference gives identical results on several random row
permutations of its hits AND on several random one-to-one relabellings of its particle ids: pandas
orders the ties of ``value_counts`` by its own sort of the (cluster, id) groups, which a row permutation
leaves alone and a relabelling does not - so the golden values do not depend on how ties are broken.

Usage:  python tools/make_golden_tracking_metrics.py [--ref PATH]
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
OUT = REPO / "tests" / "golden" / "g17_tracking_metrics.npz"
PT_THLDS = (0.0, 0.5, 0.9, 1.5)
SCAN_TRIALS = ({"eps": 0.12, "min_samples": 2}, {"eps": 0.2, "min_samples": 3}, {"eps": 0.35, "min_samples": 1},
               {"eps": 0.2, "min_samples": 4})


def install(ref: pathlib.Path):
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()


def td3():
    z = np.load(REPO / "tests" / "golden" / "g5_oc.npz")
    return (z["td3/x"].astype(np.float32), z["td3/particle_id"], z["td3/pt"].astype(np.float32),
            z["td3/eta"].astype(np.float32), z["td3/reconstructable"].astype(np.float32))


def cases():
    from sklearn.cluster import DBSCAN

    out = {}
    b = scan_batches()[0]
    for k, (eps, ms) in enumerate(((0.15, 3), (0.3, 2))):
        lab = DBSCAN(eps=eps, min_samples=ms).fit_predict(b["H"])
        out[f"td3_{k}"] = dict(labels=lab, pid=b["pid"], pt=b["pt"], eta=b["eta"], reco=b["reco"], cuts=PT_THLDS)

    g = np.random.default_rng(170)
    # blobs: 40 particles of 4..14 hits (ids x 2^40), clusters = particles with split / merged / mixed
    sizes = g.integers(4, 15, size=40)
    pidl = np.repeat(np.arange(40, dtype=np.int64) * 2 ** 40, sizes)
    lab = np.repeat(np.arange(40, dtype=np.int64), sizes) * 3
    n = len(pidl)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for p in range(0, 40, 5):        # split: the last hits of the particle in a cluster of their own
        lab[first[p] + sizes[p] - 2:first[p] + sizes[p]] = 3 * p + 1
    for p in range(1, 39, 7):        # merged with the next particle
        lab[first[p + 1]:first[p + 1] + sizes[p + 1]] = 3 * p
    for p in range(2, 40, 6):        # a foreign hit
        lab[first[p]] = 3 * ((p + 3) % 40)
    noise = g.random(n) < 0.08
    lab[noise] = g.choice([-1, -5, -1], size=noise.sum())
    lab[first[3]:first[3] + sizes[3]] = np.array([7000, 7000] + [-1] * (sizes[3] - 2))   # below 3 hits
    ptp = np.exp(g.normal(0, 0.8, size=40)).astype(np.float32)
    etap = g.uniform(-4.5, 4.5, size=40).astype(np.float32)
    out["blobs"] = dict(labels=lab, pid=pidl, pt=ptp[pidl >> 40], eta=etap[pidl >> 40],
                        reco=(g.random(40) < 0.85).astype(np.float32)[pidl >> 40], cuts=PT_THLDS)

    # pt edges: per-particle exact cut values, and particles whose mean decides
    sizes = np.full(24, 5)
    pidl = np.repeat(np.arange(24, dtype=np.int64) + 11, sizes)
    lab = np.repeat(np.arange(24, dtype=np.int64), sizes)
    base = np.array([0.5, 0.9, 1.5, 0.4999, 0.8999, 1.4999, 0.5001, 0.9001] * 3, dtype=np.float32)
    pt = base[pidl - 11].copy()
    for p in range(12, 24):   # hits differ: the mean is the cut value or straddles it
        sel = pidl == p + 11
        d = np.float32(0.25) * np.array([-1, 1, -2, 2, 0], dtype=np.float32)
        pt[sel] = base[p] + d * (1 if p % 2 else 1.0001)
    out["ptedge"] = dict(labels=lab, pid=pidl, pt=pt, eta=np.zeros_like(pt), reco=np.ones_like(pt), cuts=PT_THLDS)

    # NaN pt / eta on some hits, |eta| = 4.0 exactly
    c = out["blobs"]
    pt, eta = c["pt"].copy(), c["eta"].copy()
    pt[::17] = np.nan
    eta[5::19] = np.nan
    eta[(c["pid"] >> 40) % 6 == 1] = np.float32(4.0)
    eta[(c["pid"] >> 40) % 6 == 2] = np.float32(-4.0)
    out["naneta"] = dict(c, pt=pt, eta=eta)

    # reconstructable mixed within a particle
    reco = (g.random(len(c["pid"])) < 0.4).astype(np.float32)
    reco[(c["pid"] >> 40) % 3 == 0] = 0.0
    out["recomix"] = dict(c, reco=reco)
    out["recobool"] = dict(c, reco=reco.astype(bool))

    out["nocut"] = dict(c, cuts=(0.0, 0.9, 50.0))
    out["noise"] = dict(c, labels=np.full_like(c["labels"], -1))
    out["empty"] = dict(labels=np.zeros(0, np.int64), pid=np.zeros(0, np.int64), pt=np.zeros(0, np.float32),
                        eta=np.zeros(0, np.float32), reco=np.zeros(0, np.float32), cuts=PT_THLDS)
    return out


def scan_batches():
    """Three batches of G5 td3's hits with condensed latent points: one Gaussian blob (sigma 0.06) per
    particle around a centre uniform in [-3, 3]^4, a tenth of the hits scattered uniformly."""
    _, pid, pt, eta, reco = td3()
    g = np.random.default_rng(171)
    upid, inv = np.unique(pid, return_inverse=True)
    out = []
    for b in range(3):
        centres = g.uniform(-3, 3, size=(len(upid), 4))
        h = centres[inv] + 0.06 * g.normal(size=(len(pid), 4))
        scat = g.random(len(pid)) < 0.1
        h[scat] = g.uniform(-3, 3, size=(scat.sum(), 4))
        perm = g.permutation(len(pid))
        out.append(dict(H=h[perm].astype(np.float32), pid=pid[perm], pt=pt[perm], eta=eta[perm], reco=reco[perm]))
    return out


def relabel(c, g):
    """The case with its particle ids mapped one-to-one onto a random order of the same ids."""
    u, inv = np.unique(c["pid"], return_inverse=True)
    return dict(c, pid=g.permutation(u)[inv])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", default="/root/reference", type=pathlib.Path)
    args = ap.parse_args()
    install(args.ref)
    from gnn_tracking.metrics.cluster_metrics import flatten_track_metrics, tracking_metrics
    from gnn_tracking.postprocessing.dbscanscanner import DBSCANHyperParamScannerFixed
    from torch_geometric.data import Data

    def run(c, perm):
        r = tracking_metrics(truth=c["pid"][perm], predicted=c["labels"][perm], pts=c["pt"][perm],
                             reconstructable=c["reco"][perm], eta=c["eta"][perm], pt_thlds=list(c["cuts"]))
        return flatten_track_metrics(r)

    def same(a, b):
        return list(a) == list(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)

    arrs = {}
    g = np.random.default_rng(172)
    for name, c in cases().items():
        n = len(c["pid"])
        flat = run(c, np.arange(n))
        for _ in range(4):
            assert same(flat, run(c, g.permutation(n))), f"{name}: the reference's result depends on the hit order"
            assert same(flat, run(relabel(c, g), np.arange(n))), f"{name}: the reference's result depends on ties"
        for k in ("labels", "pid", "pt", "eta", "reco"):
            arrs[f"{name}/{k}"] = np.asarray(c[k])
        arrs[f"{name}/cuts"] = np.array(c["cuts"], dtype=np.float64)
        arrs[f"{name}/keys"] = np.array(list(flat), dtype=np.str_)
        arrs[f"{name}/values"] = np.array([float(v) for v in flat.values()], dtype=np.float64)
        print(f"  {name}: n={n}  " + "  ".join(f"{k}={flat[k]:.4g}" for k in list(flat)[:5]))

    from gnn_tracking.postprocessing.fastrescanner import DBSCANFastRescan

    batches = scan_batches()
    scanner = DBSCANHyperParamScannerFixed([dict(t) for t in SCAN_TRIALS])
    for i, b in enumerate(batches):
        data = Data(particle_id=torch.from_numpy(b["pid"]), pt=torch.from_numpy(b["pt"]),
                    eta=torch.from_numpy(b["eta"]), reconstructable=torch.from_numpy(b["reco"]))
        scanner(data, {"H": torch.from_numpy(b["H"])}, i)
        # (DBSCAN's labels depend on the hit order; the metrics of those labels must not)
        fr = DBSCANFastRescan(b["H"], max_eps=max(t["eps"] for t in SCAN_TRIALS))
        for t in SCAN_TRIALS:
            c = dict(labels=fr.cluster(eps=t["eps"], min_pts=t["min_samples"]), pid=b["pid"], pt=b["pt"],
                     eta=b["eta"], reco=b["reco"], cuts=PT_THLDS)
            n = len(b["pid"])
            r0 = run(c, np.arange(n))
            assert same(r0, run(c, g.permutation(n))) and same(r0, run(relabel(c, g), np.arange(n))), \
                "scan: tie-dependent trial"
    foms_all, rec0 = scanner.get_foms(), scanner._results
    assert len(foms_all) == 68, len(foms_all)
    for i, b in enumerate(batches):
        for k, v in b.items():
            arrs[f"scan/b{i}/{k}"] = v
    arrs["scan/trials"] = np.array([[t["eps"], t["min_samples"]] for t in SCAN_TRIALS], dtype=np.float64)
    rkeys = list(rec0[0])
    arrs["scan/record_keys"] = np.array(rkeys, dtype=np.str_)
    arrs["scan/records"] = np.array([[float(r[k]) for k in rkeys] for r in rec0], dtype=np.float64)
    arrs["scan/fom_keys"] = np.array(list(foms_all), dtype=np.str_)
    arrs["scan/fom_values"] = np.array([float(v) for v in foms_all.values()], dtype=np.float64)
    print(f"  scan: {len(rec0)} records, {len(foms_all)} foms, best eps {foms_all['best_dbscan_eps']}")
    np.savez_compressed(OUT, **arrs)
    print(f"wrote {OUT.relative_to(REPO)} ({OUT.stat().st_size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
