#!/usr/bin/env python3
"""The five clustering scores (v-measure, homogeneity, completeness, adjusted Rand, Fowlkes-Mallows) of 10
DBSCAN-like labellings of one 200 k-hit event on the device (clustering_scores_trials: one C call and one
host copy for all trials) against the host: sklearn's five functions per trial, as the reference's
common_metrics call them, when sklearn is importable, otherwise the numpy restatement of
tests/cluster_scores_ref.py (the output says which).

With ``--events B`` it measures a collated batch instead: B events of ``--hits`` hits each (default 6000), scored per
event by one ``clustering_scores_trials(..., ptr=ptr)`` call, against the loop of one call per event on the event's rows,
alternating the two in one process.

Usage:  python tools/bench_cluster_scores.py [--hits 200000] [--trials 10] [--reps 10] [--host-reps 1] [--events B]
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


def event(seed, n, n_trials, n_particles=6000):
    """Particle ids x 2^40; per trial clusters = particles with a growing share of the hits moved to a random
    cluster and a growing share of noise (label -1): from 2 % to 30 % each."""
    g = np.random.default_rng(seed)
    which = g.integers(0, n_particles, size=n)
    truth = (which + 1).astype(np.int64) * 2 ** 40
    labels = np.empty((n_trials, n), dtype=np.int64)
    for t in range(n_trials):
        frac = 0.02 + 0.28 * t / max(1, n_trials - 1)
        lab = which.astype(np.int64)
        moved = g.random(n) < frac
        lab[moved] = g.integers(0, n_particles, size=int(moved.sum()))
        lab[g.random(n) < frac] = -1
        labels[t] = lab
    return truth, labels


def events_main(args) -> None:
    from gnn_tracking_amd import cluster_metrics as CM

    dev = torch.device("cuda")
    n = args.hits if args.hits != 200_000 else 6000
    parts = [event(21 + i, n, args.trials, n_particles=max(8, n // 10)) for i in range(args.events)]
    truth_d = torch.from_numpy(np.concatenate([p[0] for p in parts])).to(dev)
    labels_d = torch.from_numpy(np.concatenate([p[1] for p in parts], axis=1)).to(dev)
    ptr = torch.arange(args.events + 1, device=dev) * n
    rows = ptr.tolist()

    def batched():
        return CM.clustering_scores_trials(labels_d, truth=truth_d, ptr=ptr)

    def per_event():
        per = [CM.clustering_scores_trials(labels_d[:, a:b], truth=truth_d[a:b]) for a, b in zip(rows, rows[1:])]
        return [[per[e][t] for e in range(args.events)] for t in range(args.trials)]

    ms = {"batched": [], "per_event": []}
    fns = {"batched": batched, "per_event": per_event}
    for rep in range(args.reps + 2):
        got = {}
        for name in (("batched", "per_event") if rep % 2 else ("per_event", "batched")):   # (alternating)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = fns[name]()
            torch.cuda.synchronize()
            if rep >= 2:   # (two repetitions warm up)
                ms[name].append((time.perf_counter() - t0) * 1e3)
        assert got["batched"] == got["per_event"], "the batched call and the per-event loop differ"
    line = {"bench": "cluster_scores_events", "events": args.events, "hits_per_event": n, "trials": args.trials,
            "device": torch.cuda.get_device_name(dev), "reps": args.reps,
            "v_measure_first_last": [round(got["batched"][0][0]["v_measure"], 6), round(got["batched"][-1][-1]["v_measure"], 6)]}
    for name, v in ms.items():
        line[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(line))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--events", type=int, default=0, help="a collated batch of this many events of --hits hits (default 6000)")
    args = ap.parse_args()
    if args.events:
        return events_main(args)
    from gnn_tracking_amd import cluster_metrics as CM

    dev = torch.device("cuda")
    truth, labels = event(21, args.hits, args.trials)
    truth_d, labels_d = torch.from_numpy(truth).to(dev), torch.from_numpy(labels).to(dev)

    def sync_t():
        torch.cuda.synchronize()
        return time.perf_counter()

    ms = []
    for rep in range(args.reps + 1):
        t0 = sync_t()
        scores = CM.clustering_scores_trials(labels_d, truth=truth_d)
        t1 = sync_t()
        if rep:   # (the first repetition warms up)
            ms.append((t1 - t0) * 1e3)

    try:
        from sklearn import metrics as M

        host_kind = "sklearn, five scores per trial"
        fns = (M.v_measure_score, M.homogeneity_score, M.completeness_score, M.adjusted_rand_score,
               M.fowlkes_mallows_score)

        def host_scores(t):
            return [float(f(truth, labels[t])) for f in fns]
    except ImportError:
        import cluster_scores_ref as R

        host_kind = "numpy restatement (sklearn not importable)"

        def host_scores(t):
            return list(R.scores(truth, labels[t]).values())
    h_ms = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host = [host_scores(t) for t in range(args.trials)]
        h_ms.append((time.perf_counter() - t0) * 1e3)
    worst = max(abs(a - b) for s, h in zip(scores, host) for a, b in zip(s.values(), h))
    line = {"bench": "cluster_scores", "hits": args.hits, "trials": args.trials,
            "device": torch.cuda.get_device_name(dev), "scores_ms": round(statistics.median(ms), 3),
            "v_measure_first_last": [round(scores[0]["v_measure"], 6), round(scores[-1]["v_measure"], 6)],
            "max_abs_diff_to_host": worst, "host": host_kind, "host_ms": round(statistics.median(h_ms), 1)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
