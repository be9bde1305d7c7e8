#!/usr/bin/env python3
"""Golden vectors of the metric-learning k-scan, FROM THE REFERENCE ITSELF: ``tests/golden/g18_kscan.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``, default
``/root/reference``) with networkx, pandas and scipy.  It installs the stand-ins of
``oracle/_ref_standins.py`` for the other third-party packages the reference imports, swaps in a ``Data``
class of its own (the stand-in's has no ``detach()`` and takes no ``num_nodes=``), then runs the
reference's own ``GraphConstructionKNNScanner`` (graph_construction/k_scanner.py), and on the first
batch of every case ``get_largest_segment_fracs``, ``get_cc_labels`` (analysis/graphs.py) and
``get_efficiency_purity_edges`` (metrics/graph_construction.py) by themselves.

Events: curved "tracks" of 3-14 hits plus 10-15 % noise hits (id 0) in 4-8 dimensions; per-hit eta on both
sides of 4.0 (a particle is partly masked); non-reconstructable particles; per-particle pt around the
threshold; one particle per event whose middle hit alone is masked out, so that its two good segments are
joined only through that hit (the segment components and the upper-bound components differ).

Cases (every one is in the file or the tool fails):
  base      three batches averaged, ids x 2^40, ks 1..7; targets with one crossing each, one above
            max(frac50) (NaN) and one below frac50(k_min) (no crossing: the end point)
  unsorted  ks given as 5, 2, 7, 1, 3; small ids
  maxedges  max_edges exceeded at the third k (a two-k table is left)
  twok      two ks (the spline is a line);  onek  one k (NaN at every target)
  threek    three ks (a parabola)
  nanfake   pt_thld 0.5 with every pt below 0.9: the max_fake_* columns are NaN and left out of the spline

Acceptance, checked for every batch of every case:
  * for every k the stand-in's brute-force edges (float64 distances, float32 radius filter) are those of
    the repository's CPU search contract (oracle/knn_ref.c: fmaf chain, ties by index): no count depends on
    a near-tie in distance;
  * on a grid of 2 001 points the reference's spline crosses every target that has a finite result exactly
    once; a target without a crossing has the reference's optimiser end exactly at an end point.

``fom_rel_dev``: over all tables, the largest relative deviation between the reference's figures of merit
at a target (L-BFGS-B) and its own spline evaluated at the bracketed root (scipy ``brentq``); the tool fails
on a table where it exceeds 1e-6.  Tests compare at 100 x this value.

Usage:  python tools/make_golden_kscan.py [--ref PATH]
"""

from __future__ import annotations

import argparse
import os
import pathlib
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "g18_kscan.npz"

CASES = {
    "base": dict(seeds=(180, 181, 182), n_tracks=90, dim=6, big_ids=True, ks=[1, 2, 3, 4, 5, 6, 7],
                 targets=(0.05, 0.4, 0.6, 0.9)),
    "unsorted": dict(seeds=(183,), n_tracks=60, dim=4, big_ids=False, ks=[5, 2, 7, 1, 3], targets=(0.4, 0.6)),
    "maxedges": dict(seeds=(184, 185), n_tracks=50, dim=8, big_ids=True, ks=[1, 2, 3, 4, 5], targets=(0.2, 0.4),
                     max_edges="third"),
    "twok": dict(seeds=(186,), n_tracks=50, dim=5, big_ids=True, ks=[2, 6], targets=(0.45, 0.61)),
    "onek": dict(seeds=(187,), n_tracks=40, dim=4, big_ids=False, ks=[3], targets=(0.4,)),
    "threek": dict(seeds=(188,), n_tracks=50, dim=7, big_ids=True, ks=[1, 3, 6], targets=(0.4, 0.65)),
    "nanfake": dict(seeds=(189, 190), n_tracks=60, dim=6, big_ids=True, ks=[1, 2, 4, 6], targets=(0.3, 0.6),
                    pt_thld=0.5, pt_max=0.85),
}


def event(seed, n_tracks, dim, big_ids, pt_max=None):
    """One event: hits in `dim` dimensions, true edges between consecutive hits of a track (both
    directions), shuffled."""
    g = np.random.default_rng(seed)
    xs, pids, pts, etas, recos, te = [], [], [], [], [], []
    box = np.where(np.arange(dim) < 3, 1.0, 0.25)   # three wide directions, the others narrow
    jitter = 0.2
    at = 0
    for p in range(1, n_tracks + 1):
        m = int(g.integers(3, 15))
        t = np.linspace(0, 1, m)[:, None]
        start, v, c = box * g.uniform(-1, 1, dim), box * g.normal(size=dim), box * g.normal(size=dim)
        v *= g.uniform(0.5, 2.2) / np.linalg.norm(v)
        # (an imperfect embedding: the jitter of a hit is comparable to the spacing of its track, tracks
        # overlap - the longer and faster a track, the larger the k that joins its pieces)
        x = start + v * t + 0.4 * c * t ** 2 + jitter * g.normal(size=(m, dim))
        pt = float(np.exp(g.normal(0.1, 0.6)))
        if pt_max is not None:
            pt = min(pt, pt_max * float(g.uniform(0.7, 1.0)))
        eta0 = float(g.uniform(-4.4, 4.4))
        eta = eta0 + 0.25 * np.linspace(-1, 1, m) * g.choice([-1, 1])
        if p == 1:   # two good segments joined only through a masked-out hit of its own
            m_mid = m // 2
            pt, eta = max(pt, 1.2) if pt_max is None else pt, np.full(m, 1.0)
            eta[m_mid] = 4.3
        xs.append(x)
        pids.append(np.full(m, p, np.int64))
        pts.append(np.full(m, pt, np.float32))
        etas.append(eta.astype(np.float32))
        recos.append(np.full(m, float(g.random() < 0.88), np.float32))
        a = np.arange(at, at + m - 1)
        te.append(np.stack([np.concatenate([a, a + 1]), np.concatenate([a + 1, a])]))
        at += m
    n_noise = int(g.uniform(0.10, 0.15) * at / 0.87)
    xs.append(box * g.uniform(-1.6, 1.6, size=(n_noise, dim)))
    pids.append(np.zeros(n_noise, np.int64))
    noise_pt = np.exp(g.normal(0, 0.5, n_noise))
    pts.append((noise_pt if pt_max is None else np.minimum(noise_pt, pt_max)).astype(np.float32))
    etas.append(g.uniform(-4.5, 4.5, n_noise).astype(np.float32))
    recos.append(np.ones(n_noise, np.float32))
    x = np.concatenate(xs).astype(np.float32)
    pid = np.concatenate(pids)
    if big_ids:
        pid = pid * 2 ** 40
    n = len(pid)
    perm = g.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return dict(x=x[perm], pid=pid[perm], pt=np.concatenate(pts)[perm], eta=np.concatenate(etas)[perm],
                reco=np.concatenate(recos)[perm], true_edge_index=inv[np.concatenate(te, axis=1)])


def install(ref: pathlib.Path):
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()

    class Data(_ref_standins.Data):
        """The stand-in plus what the k-scan touches: ``num_nodes=``, ``detach()``."""

        def __init__(self, num_nodes=None, **kw):
            super().__init__(**kw)
            self.__dict__["_num_nodes"] = num_nodes

        @property
        def num_nodes(self):
            if self.__dict__.get("_num_nodes") is not None:
                return self.__dict__["_num_nodes"]
            for k in ("particle_id", "x"):
                if k in self.__dict__:
                    return int(self.__dict__[k].shape[0])
            raise AttributeError("num_nodes")

        def detach(self):
            return self

    import torch_geometric.data

    torch_geometric.data.Data = Data
    return Data


def same_edges(a, b):
    ka = np.lexsort((a[0], a[1]))
    kb = np.lexsort((b[0], b[1]))
    return a.shape == b.shape and np.array_equal(a[:, ka], b[:, kb])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", default="/root/reference", type=pathlib.Path)
    args = ap.parse_args()
    Data = install(args.ref)
    warnings.filterwarnings("ignore")
    from scipy.optimize import brentq

    import ref_cpu
    from gnn_tracking.analysis.graphs import get_cc_labels, get_largest_segment_fracs
    from gnn_tracking.graph_construction.k_scanner import GraphConstructionKNNScanner
    from gnn_tracking.metrics.graph_construction import get_efficiency_purity_edges
    from gnn_tracking.models.graph_construction import knn_with_max_radius

    arrs, fom_rel_dev = {}, 0.0
    for name, cfg in CASES.items():
        batches = [event(s, cfg["n_tracks"], cfg["dim"], cfg["big_ids"], cfg.get("pt_max")) for s in cfg["seeds"]]
        ks, pt_thld, max_radius = cfg["ks"], cfg.get("pt_thld", 0.9), 1.0
        datas = [Data(x=torch.from_numpy(b["x"]), particle_id=torch.from_numpy(b["pid"]), pt=torch.from_numpy(b["pt"]),
                      eta=torch.from_numpy(b["eta"]), reconstructable=torch.from_numpy(b["reco"]),
                      true_edge_index=torch.from_numpy(b["true_edge_index"])) for b in batches]
        # acceptance 1: the stand-in's edges are the search contract's, for every batch and k
        n_edges = {}
        for i, d in enumerate(datas):
            for k in ks:
                e_ref = knn_with_max_radius(d.x, k=k, max_radius=max_radius).numpy()
                e_own = ref_cpu.knn_graph_c(d.x, k, max_radius).numpy()
                assert same_edges(e_ref, e_own), f"{name}: batch {i}, k = {k}: the neighbour sets depend on a near-tie"
                n_edges[i, k] = e_ref.shape[1]
        max_edges = 5_000_000
        if cfg.get("max_edges") == "third":   # between the second and the third k's edge counts, in every batch
            lo = max(n_edges[i, ks[1]] for i in range(len(datas)))
            hi = min(n_edges[i, ks[2]] for i in range(len(datas)))
            assert lo < hi, f"{name}: no max_edges separates the second from the third k"
            max_edges = (lo + hi) // 2
        scanner = GraphConstructionKNNScanner(ks=ks, targets=cfg["targets"], max_radius=max_radius, pt_thld=pt_thld,
                                              max_eta=4.0, max_edges=max_edges)
        for i, d in enumerate(datas):
            scanner(d, i)
        recs = scanner._results
        res = scanner.get_results()
        foms = scanner.get_foms()
        df = res.df
        # acceptance 2 and the optimiser's stopping noise
        kmin, kmax = float(df["k"].min()), float(df["k"].max())
        for t in cfg["targets"]:
            fin = np.isfinite(foms[f"k_at_segment50_{t * 100:.0f}"])
            if len(df) < 2:
                assert not fin
                continue
            if t > df["frac50"].max():
                assert not fin, f"{name}: target {t} above max(frac50) must be NaN"
                continue
            assert fin, f"{name}: target {t}"
            f = lambda k: res._eval_spline(k)["frac50"] - t   # noqa: E731
            grid = np.linspace(kmin, kmax, 2001)
            g = np.array([f(k) for k in grid])
            assert not (g == 0).any(), f"{name}: target {t} hit on a grid point"
            cross = np.flatnonzero(g[:-1] * g[1:] < 0)
            k_ref = foms[f"k_at_segment50_{t * 100:.0f}"]
            if len(cross) == 0:
                i = int(np.argmin(np.abs(g)))
                assert i in (0, 2000) and k_ref == grid[i], f"{name}: target {t}: no crossing and no end point"
                continue
            assert len(cross) == 1, f"{name}: target {t} is crossed {len(cross)} times"
            root = brentq(f, grid[cross[0]], grid[cross[0] + 1], xtol=1e-15, rtol=8.9e-16)
            at = res._eval_spline(root)
            for key, stem in [("n_edges", "n_edges_frac_segment50")] + [(v, f"{v}_at_segment50")
                                                                       for v in res._extra_metrics]:
                a, b = foms[f"{stem}_{t * 100:.0f}"], at[key]
                dev = abs(a - b) / max(abs(b), 1e-300)
                assert dev <= 1e-6, f"{name}: target {t}: {key} deviates by {dev:.3g} (a flat crossing?)"
                fom_rel_dev = max(fom_rel_dev, dev)
        nan_cols = [c for c in df.columns if df[c].isna().any()]
        if name == "nanfake":
            assert any(c.startswith("max_fake_") for c in nan_cols), f"{name}: no NaN max_fake_ column"
        if cfg.get("max_edges") == "third":
            assert sorted(set(r["k"] for r in recs)) == ks[:2], f"{name}: max_edges did not stop at the third k"
        # the free functions on the first batch at the first k
        d = datas[0]
        d.edge_index = knn_with_max_radius(d.x, k=ks[0], max_radius=max_radius)
        d.y = d.particle_id[d.edge_index[0]] == d.particle_id[d.edge_index[1]]
        lsf = np.sort(get_largest_segment_fracs(d, pt_thld=pt_thld, max_eta=4.0))
        cc_true = get_cc_labels(d.edge_index[:, d.y], num_nodes=len(d.particle_id)).numpy()
        cc_all = get_cc_labels(d.edge_index, num_nodes=len(d.particle_id)).numpy()
        ep = get_efficiency_purity_edges(d, pt_thld=pt_thld, max_eta=4.0)

        for i, b in enumerate(batches):
            for key, v in b.items():
                arrs[f"{name}/b{i}/{key}"] = v
        rkeys = list(recs[0])
        arrs[f"{name}/n_batches"] = np.array(len(batches))
        arrs[f"{name}/ks"] = np.array(ks, dtype=np.int64)
        arrs[f"{name}/targets"] = np.array(cfg["targets"], dtype=np.float64)
        arrs[f"{name}/settings"] = np.array([max_radius, pt_thld, 4.0, max_edges], dtype=np.float64)
        arrs[f"{name}/record_keys"] = np.array(rkeys, dtype=np.str_)
        arrs[f"{name}/records"] = np.array([[float(r[k]) for k in rkeys] for r in recs], dtype=np.float64)
        arrs[f"{name}/fom_keys"] = np.array(list(foms), dtype=np.str_)
        arrs[f"{name}/fom_values"] = np.array([float(v) for v in foms.values()], dtype=np.float64)
        arrs[f"{name}/nan_columns"] = np.array(nan_cols, dtype=np.str_)
        arrs[f"{name}/first/edge_index"] = d.edge_index.numpy()
        arrs[f"{name}/first/lsf_sorted"] = lsf
        arrs[f"{name}/first/cc_true"] = cc_true
        arrs[f"{name}/first/cc_all"] = cc_all
        arrs[f"{name}/first/eff_pur"] = np.array([ep["efficiency"], ep["purity"]], dtype=np.float64)
        f50 = "  ".join(f"{v:.3f}" for v in df["frac50"])
        print(f"  {name}: {len(batches)} batches of {[len(b['pid']) for b in batches]} hits, {len(recs)} records, "
              f"frac50 = {f50}, NaN columns {len(nan_cols)}")
    arrs["fom_rel_dev"] = np.array(fom_rel_dev)
    arrs["cases"] = np.array(list(CASES), dtype=np.str_)
    np.savez_compressed(OUT, **arrs)
    print(f"fom_rel_dev = {fom_rel_dev:.3g}")
    print(f"wrote {OUT.relative_to(REPO)} ({OUT.stat().st_size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
