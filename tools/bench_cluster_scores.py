#!/usr/bin/env python3
"""The five clustering scores (v-measure, homogeneity, completeness, adjusted Rand, Fowlkes-Mallows) of 10
DBSCAN-like labellings of one 200 k-hit event on the device (clustering_scores_trials: one C call and one
host copy for all trials) against the host: sklearn's five functions per trial, as the reference's
common_metrics call them, when sklearn is importable, otherwise the numpy restatement of
tests/cluster_scores_ref.py (the output says which).

Usage:  python tools/bench_cluster_scores.py [--hits 200000] [--trials 10] [--reps 10] [--host-reps 1]
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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
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
