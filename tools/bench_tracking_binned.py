#!/usr/bin/env python3
"""The binned tracking metrics of one 200 k-hit batch in 20 pt bins (tracking_metrics_vs_pt: one
windows call and one host copy) and its cluster table (tracking_metric_table) on the device, against
the reference's algorithm on the host (a pandas value_counts / groupby chain and masked sums per bin
when pandas is importable, otherwise the numpy restatement of tests/tracking_binned_ref.py; the
output says which).

With ``--events B`` it measures a collated batch instead: B events of ``--hits`` hits each (default 6000) through
``DBSCANPerformanceDetails.__call__`` and ``tracking_metrics_vs_pt`` - one DBSCAN, one batched table call and one batched
windows call per 32 bins for all events - against the per-event loop that preceded the batched entries (one DBSCAN, then
per event a table call and a windows call with a host copy each), alternating the two in one process.

Usage:  python tools/bench_tracking_binned.py [--hits 200000] [--bins 20] [--reps 10] [--host-reps 1] [--events B]
Prints one JSON line.
"""

from __future__ import annotations

import argparse
import itertools
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def event(seed, n, n_particles=6000, noise_frac=0.1):
    """Per-particle pt / eta, ids x 2^40; clusters = particles, a tenth of the hits moved to a random
    cluster, a tenth noise."""
    g = np.random.default_rng(seed)
    which = g.integers(0, n_particles, size=n)
    pid = (which + 1).astype(np.int64) * 2 ** 40
    labels = which.astype(np.int64)
    moved = g.random(n) < 0.1
    labels[moved] = g.integers(0, n_particles, size=int(moved.sum()))
    labels[g.random(n) < noise_frac] = -1
    pt = np.exp(g.normal(-0.5, 0.9, size=n_particles)).astype(np.float32)[which]
    eta = np.clip(g.normal(0, 2, size=n_particles), -4.6, 4.6).astype(np.float32)[which]
    reco = (g.random(n_particles) < 0.9).astype(np.float32)[which]
    return labels, pid, pt, eta, reco


def pandas_binned(pd, labels, pid, pt, eta, reco, edges, thld=3, max_eta=4.0):
    """The reference's chain of frame operations (value_counts of (c, id), first per cluster, groupby
    means, merge, then per bin the masked sums), written out for timing."""
    h = pd.DataFrame({"c": labels, "id": pid, "pt": pt, "reconstructable": reco, "eta": eta})
    vc = h[["c", "id"]].value_counts().reset_index()
    gb = vc.groupby("c")
    c = gb.first().rename({"id": "maj_pid", "count": "maj_hits"}, axis=1)
    c["cluster_size"] = gb["count"].sum()
    u, cnt = np.unique(h["c"], return_counts=True)
    c["valid_cluster"] = (u >= 0) & (cnt >= thld)
    props = h[["id", "pt", "reconstructable", "eta"]].groupby("id").mean()
    c = c.merge(props, left_on="maj_pid", right_index=True).rename(
        columns={k: f"maj_{k}" for k in ("pt", "reconstructable", "eta")})
    c["maj_pid_hits"] = c["maj_pid"].map(h["id"].value_counts())
    frac = c["maj_hits"] / c["cluster_size"]
    pfrac = c["maj_hits"] / c["maj_pid_hits"]
    out = []
    for lo, hi in itertools.pairwise(edges):
        cm = ((c["maj_pt"] < hi) & (c["maj_pt"] >= lo) & (c["maj_reconstructable"] != 0) & (c["maj_eta"] < max_eta)
              & c["valid_cluster"])
        hm = (h["pt"] < hi) & (h["pt"] >= lo) & (h["eta"] < max_eta) & h["reconstructable"].astype(bool)
        out.append((len(np.unique(h["id"][hm])), int(cm.sum()),
                    int(((c["maj_pid_hits"] == c["maj_hits"]) & (frac > 0.99) & cm).sum()),
                    int(((pfrac > 0.5) & (frac > 0.5) & cm).sum()), int(((frac > 0.75) & cm).sum())))
    return out


class PerEventDetails:
    """``DBSCANPerformanceDetails.__call__`` as it was before the batched entries: one DBSCAN for the batch, then per event
    a plain hit record and one ``gnntrk_cluster_table`` launch sequence with its host copy."""

    def __init__(self, eps, min_samples):
        self.eps, self.min_samples, self.h_dfs, self.c_dfs = eps, min_samples, [], []

    def __call__(self, data, out, i_batch):
        from gnn_tracking_amd import cluster_metrics as CM
        from gnn_tracking_amd.postprocessing import DBSCANFastRescan

        fr = DBSCANFastRescan(out["H"].detach(), max_eps=self.eps, ptr=data.ptr)
        labels = fr.cluster_device(eps=self.eps, min_pts=self.min_samples)
        pid, pt, reco, eta = CM._hits(data.particle_id, data.pt, data.reconstructable, data.eta, labels.device)
        rows = data.ptr.tolist()
        for a, b in zip(rows, rows[1:]):
            lab, cols = labels[a:b], [v[a:b] for v in (pid, pt, reco, eta)]
            self.h_dfs.append({"c": lab, "id": cols[0], "reconstructable": cols[2], "pt": cols[1], "eta": cols[3]})
            self.c_dfs.append(CM._table(lab.contiguous(), None, *(c.contiguous() for c in cols), 3))


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def events_main(args) -> None:
    import gnn_tracking_amd as G
    from gnn_tracking_amd import cluster_metrics as CM
    from gnn_tracking_amd import synthetic
    from gnn_tracking_amd.postprocessing import DBSCANPerformanceDetails

    dev = torch.device("cuda")
    n = args.hits if args.hits != 200_000 else 6000
    events = []
    for i in range(args.events):
        ev = synthetic.make_pileup_event(900 + i, n, 8, n_particles=max(8, n // 10), n_clusters=max(4, n // 30))
        events.append(G.Data(x=ev["x"].to(dev), edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev),
                             **{k: ev[k].to(dev) for k in ("particle_id", "pt", "eta", "reconstructable")}))
    data = G.collate(events)
    edges = np.concatenate([np.linspace(0.0, 3.0, args.bins), [np.inf]]).tolist()
    eps, min_samples = 0.25, 2

    def run(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = make(eps, min_samples)
        sc(data, {"H": data.x}, 0)
        h_dfs, c_dfs = (sc.h_dfs, sc.c_dfs) if isinstance(sc, PerEventDetails) else sc.get_results()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = CM.tracking_metrics_vs_pt(h_dfs, c_dfs, edges)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, rows, c_dfs

    ms = {"batched": ([], []), "per_event": ([], [])}
    kinds = {"batched": DBSCANPerformanceDetails, "per_event": PerEventDetails}
    for rep in range(args.reps + 2):
        got = {}
        for name in (("batched", "per_event") if rep % 2 else ("per_event", "batched")):   # (alternating)
            call_ms, vs_ms, rows, c_dfs = run(kinds[name])
            got[name] = (rows, c_dfs)
            if rep >= 2:   # (two repetitions warm up)
                ms[name][0].append(call_ms)
                ms[name][1].append(vs_ms)
        same = all(a == b or (a != a and b != b) for ra, rb in zip(got["batched"][0], got["per_event"][0])
                   for a, b in zip(ra.values(), rb.values()))
        same = same and all(np.array_equal(ta[k], tb[k], equal_nan=ta[k].dtype.kind == "f")
                            for ta, tb in zip(got["batched"][1], got["per_event"][1]) for k in ta)
        assert same, "the batched path and the per-event loop differ"
    line = {"bench": "tracking_binned_events", "events": args.events, "hits_per_event": n, "bins": len(edges) - 1,
            "clusters": int(sum(len(t["c"]) for t in got["batched"][1])), "device": torch.cuda.get_device_name(dev),
            "reps": args.reps}
    for name, (call_ms, vs_ms) in ms.items():
        line[name + "_call_ms"] = spread(call_ms)
        line[name + "_vs_pt_ms"] = spread(vs_ms)
        line[name + "_total_ms"] = spread([a + b for a, b in zip(call_ms, vs_ms)])
    print(json.dumps(line))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--events", type=int, default=0, help="a collated batch of this many events of --hits hits (default 6000)")
    args = ap.parse_args()
    if args.events:
        return events_main(args)
    from gnn_tracking_amd import cluster_metrics as CM

    dev = torch.device("cuda")
    labels, pid, pt, eta, reco = event(17, args.hits)
    edges = np.concatenate([np.linspace(0.0, 3.0, args.bins), [np.inf]]).tolist()
    h = {"c": torch.from_numpy(labels).to(dev), "id": torch.from_numpy(pid).to(dev),
         "reconstructable": torch.from_numpy(reco).to(dev), "pt": torch.from_numpy(pt).to(dev),
         "eta": torch.from_numpy(eta).to(dev)}

    def sync_t():
        torch.cuda.synchronize()
        return time.perf_counter()

    rec = {"vs_pt": [], "table": []}
    for rep in range(args.reps + 1):
        t0 = sync_t()
        rows = CM.tracking_metrics_vs_pt([h], [None], edges)
        t1 = sync_t()
        table = CM.tracking_metric_table(h["c"], truth=h["id"], pts=h["pt"], reconstructable=h["reconstructable"],
                                         eta=h["eta"])
        t2 = sync_t()
        if rep:   # (the first repetition warms up)
            rec["vs_pt"].append((t1 - t0) * 1e3)
            rec["table"].append((t2 - t1) * 1e3)
    med = {k + "_ms": round(statistics.median(v), 3) for k, v in rec.items()}

    try:
        import pandas as pd
        host_kind = "pandas chain"
    except ImportError:
        pd = None
        import tracking_binned_ref as B
        host_kind = "numpy restatement (pandas not importable)"
    h_ms = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        if pd is not None:
            host = pandas_binned(pd, labels, pid, pt, eta, reco, edges)
        else:
            n_part, counts = B.window_counts(labels, pid, pt, eta, reco, B.pt_windows(edges))
            host = [(int(n_part[j]), *map(int, counts[j])) for j in range(len(edges) - 1)]
        h_ms.append((time.perf_counter() - t0) * 1e3)
    line = {"bench": "tracking_binned", "hits": args.hits, "bins": len(edges) - 1, "clusters": int(len(table["c"])),
            "device": torch.cuda.get_device_name(dev), **med,
            "n_cleaned_clusters": int(sum(r["n_cleaned_clusters"] for r in rows)),
            "host_n_cleaned_clusters": int(sum(r[1] for r in host)),
            "host": host_kind, "host_vs_pt_ms": round(statistics.median(h_ms), 1)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
