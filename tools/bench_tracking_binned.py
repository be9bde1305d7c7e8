#!/usr/bin/env python3
"""The binned tracking metrics of one 200 k-hit batch in 20 pt bins (tracking_metrics_vs_pt: one
windows call and one host copy) and its cluster table (tracking_metric_table) on the device, against
the reference's algorithm on the host (a pandas value_counts / groupby chain and masked sums per bin
when pandas is importable, otherwise the numpy restatement of tests/tracking_binned_ref.py; the
output says which).

Usage:  python tools/bench_tracking_binned.py [--hits 200000] [--bins 20] [--reps 10] [--host-reps 1]
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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
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
