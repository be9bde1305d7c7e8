#!/usr/bin/env python3
"""One OC validation batch of the DBSCAN scanner on a 200 k-hit event: radius graph, ten rescans,
the tracking metrics of all ten trials and the host copy - on the device, against the reference's
algorithm on the host (sklearn DBSCAN + a pandas value_counts / groupby chain when importable,
otherwise the numpy restatement of tests/tracking_metrics_ref.py; the output says which).

Usage:  python tools/bench_tracking_metrics.py [--hits 200000] [--reps 5] [--host-reps 1]
Prints one JSON line.
"""

from __future__ import annotations

import argparse
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

TRIALS = [(0.05, 1), (0.08, 2), (0.1, 3), (0.12, 4), (0.15, 2), (0.18, 3), (0.2, 1), (0.25, 4), (0.3, 2), (0.07, 3)]
CUTS = (0.0, 0.5, 0.9, 1.5)


def event(seed, n, dim=8, n_particles=6000, sigma=0.05, noise_frac=0.1):
    g = np.random.default_rng(seed)

    def ball(m):
        v = g.normal(size=(m, dim))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * (3.0 * g.random((m, 1)) ** (1.0 / dim))

    centres = ball(n_particles)
    n_noise = int(noise_frac * n)
    which = g.integers(0, n_particles, size=n - n_noise)
    x = np.concatenate([centres[which] + sigma * g.normal(size=(n - n_noise, dim)), ball(n_noise)]).astype(np.float32)
    pid = np.concatenate([(which + 1).astype(np.int64) * 2 ** 40, np.zeros(n_noise, np.int64)])
    k = pid >> 40
    pt = np.exp(g.normal(-0.5, 0.9, size=n_particles + 1)).astype(np.float32)[k]
    eta = np.clip(g.normal(0, 2, size=n_particles + 1), -4.6, 4.6).astype(np.float32)[k]
    perm = g.permutation(n)
    return x[perm], pid[perm], pt[perm], eta[perm], np.ones(n, np.float32)


def pandas_metrics(pd, labels, pid, pt, eta, reco, cuts, thld=3, max_eta=4.0):
    """The reference's chain of frame operations (value_counts of (c, id), first per cluster, groupby
    means, merge, masked sums), written out for timing."""
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
    out = {}
    for p in cuts:
        cm = (c["maj_pt"] >= p) & (c["maj_reconstructable"] != 0) & (c["maj_eta"].abs() < max_eta) & c["valid_cluster"]
        hm = (h["pt"] >= p) & h["reconstructable"].astype(bool) & (h["eta"].abs() < max_eta)
        out[p] = (len(np.unique(h["id"][hm])), int(cm.sum()),
                  int(((c["maj_pid_hits"] == c["maj_hits"]) & (frac > 0.99) & cm).sum()),
                  int(((pfrac > 0.5) & (frac > 0.5) & cm).sum()), int(((frac > 0.75) & cm).sum()))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
    from gnn_tracking_amd import cluster_metrics as CM
    from gnn_tracking_amd.postprocessing import DBSCANFastRescan

    dev = torch.device("cuda")
    x, pid, pt, eta, reco = event(17, args.hits)
    X, PID, PT, ETA, RECO = (torch.from_numpy(a).to(dev) for a in (x, pid, pt, eta, reco))
    max_eps = max(e for e, _ in TRIALS)

    def sync_t():
        torch.cuda.synchronize()
        return time.perf_counter()

    rec = {"graph": [], "rescans": [], "metrics": [], "total": []}
    for rep in range(args.reps + 1):
        t0 = sync_t()
        fr = DBSCANFastRescan(X, max_eps=max_eps)
        t1 = sync_t()
        labels = torch.empty((len(TRIALS), args.hits), dtype=torch.int64, device=dev)
        for k, (e, m) in enumerate(TRIALS):
            labels[k] = fr.cluster_device(eps=e, min_pts=m)
        t2 = sync_t()
        res = CM.tracking_metrics_trials(labels, truth=PID, pts=PT, eta=ETA, reconstructable=RECO, pt_thlds=CUTS)
        t3 = sync_t()
        if rep:   # (the first repetition warms up)
            for k, v in zip(rec, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                rec[k].append(v * 1e3)
    med = {k + "_ms": round(statistics.median(v), 3) for k, v in rec.items()}
    med["metrics_ms_per_trial"] = round(med["metrics_ms"] / len(TRIALS), 4)

    host_labels = labels.cpu().numpy()
    try:
        import pandas as pd
        from sklearn.cluster import DBSCAN
        host_kind = "sklearn DBSCAN + pandas chain"
    except ImportError:
        pd = DBSCAN = None
        import tracking_metrics_ref as R
        host_kind = "numpy restatement (metrics only; sklearn / pandas not importable)"
    h_db, h_m = [], []
    for _ in range(args.host_reps):
        if DBSCAN is not None:
            t0 = time.perf_counter()
            for e, m in TRIALS:
                DBSCAN(eps=e, min_samples=m).fit_predict(x)
            h_db.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for t in range(len(TRIALS)):
            if pd is not None:
                pandas_metrics(pd, host_labels[t], pid, pt, eta, reco, CUTS)
            else:
                R.tracking_counts(host_labels[t], pid, pt, eta, reco, CUTS)
        h_m.append((time.perf_counter() - t0) * 1e3)
    line = {"bench": "tracking_metrics", "hits": args.hits, "trials": len(TRIALS), "cuts": len(CUTS),
            "device": torch.cuda.get_device_name(dev), **med,
            "best_double_majority_pt0.9": max(r["double_majority_pt0.9"] for r in res),
            "host": host_kind, "host_metrics_ms": round(statistics.median(h_m), 1),
            "host_dbscan_ms": round(statistics.median(h_db), 1) if h_db else None}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
