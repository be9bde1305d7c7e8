#!/usr/bin/env python3
"""Golden vectors of the binned tracking metrics, the cluster table and ``DBSCANPerformanceDetails``,
FROM THE REFERENCE ITSELF: ``tests/golden/g20_tracking_binned.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``,
default ``/root/reference``) with pandas, scikit-learn and scipy, through the stand-ins of
``oracle/_ref_standins.py`` (as ``tools/make_golden_tracking_metrics.py``).  The file holds expected
values and key names only: the inputs are the cases of ``g17_tracking_metrics.npz``, read by name.

* ``single/<case>/vs_pt``, ``single/<case>/vs_eta``: the reference's ``tracking_metrics_vs_pt`` (edges 0, 0.5, 0.9,
  1.5, inf; ``max_eta=4``) and ``tracking_metrics_vs_eta`` (edges -4, -2, 0, 2, 4; ``pt_thld=0.9``) of one
  batch, for ``td3_0, td3_1, blobs, ptedge, naneta, recomix, recobool``: rows x columns, fp64;
* ``multi/vs_pt``, ``multi/vs_eta``: the same over the three batches ``blobs, naneta, recomix`` (mean
  and ``_err`` over batches);
* ``table/<case>/<column>``: ``tracking_metric_df`` (rows with ``c >= 0``) for the six tie-free cases
  (``td3_1`` has a tied cluster: the reference's own table depends on the id numbering there);
* ``scan/...``: the reference's ``DBSCANPerformanceDetails(eps=0.2, min_samples=3)`` over ``scan/b0..b2``
  of G17: its per-batch labels and tables and the ``vs_pt`` / ``vs_eta`` rows of its results.

Every case is accepted only if the reference gives identical results on 4 random row permutations of
its hits and on 4 random one-to-one relabellings of its particle ids (``maj_pid`` mapped back).

Usage:  python tools/make_golden_tracking_binned.py [--ref PATH]
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
G17 = REPO / "tests" / "golden" / "g17_tracking_metrics.npz"
OUT = REPO / "tests" / "golden" / "g20_tracking_binned.npz"
BINNED = ("td3_0", "td3_1", "blobs", "ptedge", "naneta", "recomix", "recobool")
MULTI = ("blobs", "naneta", "recomix")
TABLES = ("td3_0", "blobs", "ptedge", "naneta", "recomix", "recobool")
PT_EDGES = [0.0, 0.5, 0.9, 1.5, float("inf")]
ETA_EDGES = [-4.0, -2.0, 0.0, 2.0, 4.0]
MAX_ETA, PT_THLD = 4.0, 0.9
EPS, MIN_SAMPLES = 0.2, 3
PROPS = ("maj_reconstructable", "maj_eta", "maj_pt")
COLUMNS = ("maj_pid", "maj_hits", "cluster_size", "valid_cluster", *PROPS, "maj_pid_hits", "maj_frac", "maj_pid_frac",
           "perfect_match", "double_majority", "lhc_match")


def install(ref: pathlib.Path):
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()


def same(x: np.ndarray, y: np.ndarray) -> bool:
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind == "f":
        return bool(np.all((x == y) | ((x != x) & (y != y))))
    return bool(np.all(x == y))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", default="/root/reference", type=pathlib.Path)
    args = ap.parse_args()
    install(args.ref)
    import pandas as pd
    from gnn_tracking.metrics.cluster_metrics import (tracking_metric_df, tracking_metrics_vs_eta,
                                                      tracking_metrics_vs_pt)
    from gnn_tracking.postprocessing.dbscanscanner import DBSCANPerformanceDetails, dbscan
    from torch_geometric.data import Data

    g17 = np.load(G17)
    g = np.random.default_rng(200)

    def case(name):
        return {k: g17[f"{name}/{k}"] for k in ("labels", "pid", "pt", "eta", "reco")}

    def hdf(c, perm=None):
        perm = np.arange(len(c["pid"])) if perm is None else perm
        return pd.DataFrame({"c": c["labels"][perm], "id": c["pid"][perm], "reconstructable": c["reco"][perm],
                             "pt": c["pt"][perm], "eta": c["eta"][perm]})

    def binned(cs, perms=None):
        hs = [hdf(c, None if perms is None else p) for c, p in zip(cs, perms or [None] * len(cs))]
        cds = [tracking_metric_df(h) for h in hs]
        return (tracking_metrics_vs_pt(hs, cds, pts=PT_EDGES, max_eta=MAX_ETA),
                tracking_metrics_vs_eta(hs, cds, etas=ETA_EDGES, pt_thld=PT_THLD))

    def table(c, perm=None, back=None):
        cd = tracking_metric_df(hdf(c, perm))
        cd = cd[cd.index >= 0].sort_index()
        # (the reference takes the three property columns from a set of strings: their order among
        # themselves changes from process to process with the string hash.  Fixed here.)
        assert sorted(cd.columns) == sorted(COLUMNS), list(cd.columns)
        assert [k for k in cd.columns if k not in PROPS] == [k for k in COLUMNS if k not in PROPS]
        assert all(k in PROPS for k in cd.columns[4:7])
        cd = cd[list(COLUMNS)]
        if back is not None:
            cd = cd.assign(maj_pid=cd["maj_pid"].map(back))
        return cd

    def variants(c):
        """4 row permutations and 4 id relabellings of the case: (case, perm, maj_pid map back)."""
        n = len(c["pid"])
        u, inv = np.unique(c["pid"], return_inverse=True)
        for _ in range(4):
            yield c, g.permutation(n), None
            pu = g.permutation(u)
            yield dict(c, pid=pu[inv]), None, dict(zip(pu.tolist(), u.tolist()))

    def check_binned(name, cs):
        vp, ve = binned(cs)
        for vs in zip(*(list(variants(c)) for c in cs)):
            vp2, ve2 = binned([v[0] for v in vs], [v[1] for v in vs])
            assert list(vp2.columns) == list(vp.columns) and list(ve2.columns) == list(ve.columns)
            assert same(vp.to_numpy(dtype=float), vp2.to_numpy(dtype=float)) and \
                same(ve.to_numpy(dtype=float), ve2.to_numpy(dtype=float)), \
                f"{name}: the reference's binned metrics depend on the hit order or on ties"
        return vp, ve

    def check_table(name, c):
        cd = table(c)
        for c2, perm, back in variants(c):
            cd2 = table(c2, perm, back)
            assert cd.index.equals(cd2.index) and list(cd.columns) == list(cd2.columns) and \
                all(same(cd[k].to_numpy(), cd2[k].to_numpy()) for k in cd.columns), \
                f"{name}: the reference's table depends on the hit order or on ties"
        return cd

    arrs = {"pt_edges": np.array(PT_EDGES), "eta_edges": np.array(ETA_EDGES), "max_eta": np.float64(MAX_ETA),
            "pt_thld": np.float64(PT_THLD), "scan/eps": np.float64(EPS), "scan/min_samples": np.int64(MIN_SAMPLES)}

    def put_binned(prefix, vp, ve):
        arrs.setdefault("vs_pt_keys", np.array(list(vp.columns), dtype=np.str_))
        arrs.setdefault("vs_eta_keys", np.array(list(ve.columns), dtype=np.str_))
        assert list(vp.columns) == [str(k) for k in arrs["vs_pt_keys"]]
        assert list(ve.columns) == [str(k) for k in arrs["vs_eta_keys"]]
        arrs[f"{prefix}vs_pt"] = vp.to_numpy(dtype=np.float64)
        arrs[f"{prefix}vs_eta"] = ve.to_numpy(dtype=np.float64)

    def put_table(prefix, cd):
        arrs.setdefault("table_columns", np.array(list(cd.columns), dtype=np.str_))
        assert list(cd.columns) == [str(k) for k in arrs["table_columns"]]
        # (the columns keep the reference's dtypes: maj_reconstructable is float64 where reconstructable is bool)
        arrs[f"{prefix}c"] = cd.index.to_numpy(dtype=np.int64)
        for k in cd.columns:
            arrs[f"{prefix}{k}"] = cd[k].to_numpy()

    for name in BINNED:
        vp, ve = check_binned(name, [case(name)])
        put_binned(f"single/{name}/", vp, ve)
        print(f"  {name}: n_particles per pt bin {vp['n_particles'].tolist()}, clusters "
              f"{vp['n_cleaned_clusters'].tolist()}; per eta bin {ve['n_particles'].tolist()}")
    vp, ve = check_binned("multi", [case(n) for n in MULTI])
    arrs["multi/names"] = np.array(MULTI, dtype=np.str_)
    put_binned("multi/", vp, ve)
    print(f"  multi: perfect {vp['perfect'].tolist()} +- {vp['perfect_err'].tolist()}")
    for name in TABLES:
        cd = check_table(name, case(name))
        put_table(f"table/{name}/", cd)
        print(f"  table {name}: {len(cd)} clusters, {int(cd['valid_cluster'].sum())} valid")

    # the scanner over the three scan batches of G17
    scanner = DBSCANPerformanceDetails(eps=EPS, min_samples=MIN_SAMPLES)
    for i in range(3):
        b = {k: g17[f"scan/b{i}/{k}"] for k in ("H", "pid", "pt", "eta", "reco")}
        data = Data(particle_id=torch.from_numpy(b["pid"]), pt=torch.from_numpy(b["pt"]),
                    eta=torch.from_numpy(b["eta"]), reconstructable=torch.from_numpy(b["reco"]))
        scanner(data, {"H": torch.from_numpy(b["H"])}, i)
        c = dict(labels=dbscan(b["H"], eps=EPS, min_samples=MIN_SAMPLES), pid=b["pid"], pt=b["pt"], eta=b["eta"],
                 reco=b["reco"])
        cd = check_table(f"scan/b{i}", c)
        check_binned(f"scan/b{i}", [c])
        ref_cd = scanner._c_dfs[i]
        ref_cd = ref_cd[ref_cd.index >= 0].sort_index()
        ref_cd = ref_cd[list(COLUMNS)]
        assert all(same(cd[k].to_numpy(), ref_cd[k].to_numpy()) for k in cd.columns)
        put_table(f"scan/b{i}/table/", cd)
        assert same(scanner._h_dfs[i]["c"].to_numpy(), c["labels"])
        arrs[f"scan/b{i}/labels"] = c["labels"].astype(np.int16)   # (the reference's DBSCAN labels: its h_df's c)
    h_dfs, c_dfs = scanner.get_results()
    assert scanner.get_foms() == {} and len(h_dfs) == 3
    put_binned("scan/", tracking_metrics_vs_pt(h_dfs, c_dfs, pts=PT_EDGES, max_eta=MAX_ETA),
               tracking_metrics_vs_eta(h_dfs, c_dfs, etas=ETA_EDGES, pt_thld=PT_THLD))
    print(f"  scan: clusters per batch {[int((c.index >= 0).sum()) for c in c_dfs]}")
    np.savez_compressed(OUT, **arrs)
    size = OUT.stat().st_size
    assert size < 200_000, size
    print(f"wrote {OUT.relative_to(REPO)} ({size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
