#!/usr/bin/env python3
"""Times the EC threshold scan (``graph_analysis.ec_threshold_scan``) against the loop of single-threshold calls it
replaces - per threshold ``BinaryClassificationStats`` on all and on the masked edges and
``summarize_track_graph_info(get_track_graph_info_from_data(data, w=w, threshold=t))``, with ``get_orphan_counts`` once -
on the "bridged" pile-up events of tools/time_track_graph.py (6 000 hits, kNN k = 6, plus 3 000 random edges), for one
event and for 32 collated events, at T = 1, 20 and 200 thresholds.  Weights: true edges ~ Beta(5, 2), false ~ Beta(2, 5).
Per input: the scan, its parts (prepare with its host read, steps, host finish with its host copy) and the loop, as wall
time around work that ends in a device synchronise, median [min, max] of ``--reps`` repetitions after two warm-up rounds
(``--loop-reps`` for the loop), the kernel launches of ``gnntrk_ec_scan_steps`` per threshold, and whether the scan's
records equal the loop's.

Without ``--step`` the tool is a driver: it runs every step as a child process under its own ``timeout`` and stops at
the first one that fails.

Usage:  python tools/time_ec_scan.py [--hits 6000] [--events 32] [--reps 20] [--loop-reps 20]
Prints one JSON line per step and number of thresholds.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import subprocess
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

STEPS = {"single": 600, "batch": 900}   # seconds of `timeout` per step
N_THR = (1, 20, 200)
LAUNCHES_PER_THRESHOLD = 3   # es_union_kernel, es_count_kernel, es_emit_kernel


def loop(data, w, thresholds):
    import gnn_tracking_amd as G
    from gnn_tracking_amd.graph_masks import get_edge_mask_from_node_mask, get_good_node_mask

    em = get_edge_mask_from_node_mask(get_good_node_mask(data), data.edge_index)
    w_m, y_m = w[em], data.y[em]
    orphans = G.get_orphan_counts(data)._asdict()
    out = []
    for t in thresholds:
        bcs = G.BinaryClassificationStats(w, data.y, t).get_all()
        thld = G.BinaryClassificationStats(w_m, y_m, t).get_all()
        summary = G.summarize_track_graph_info(G.get_track_graph_info_from_data(data, w=w, threshold=t))
        out.append({"threshold": t, **bcs, **{f"{k}_thld": v for k, v in thld.items()}, **orphans, **summary})
    return out


def step(name, args):
    import numpy as np
    import torch

    import gnn_tracking_amd as G
    from gnn_tracking_amd import graph_analysis as GA
    from time_track_graph import make_data, timed

    dev = torch.device("cuda:0")
    if name == "single":
        data = make_data(100, args.hits, dev, True)
    else:
        data = G.collate([make_data(100 + i, args.hits, dev, True) for i in range(args.events)])
    g = np.random.default_rng(2200)
    y = data.y.cpu().numpy()
    w = torch.from_numpy(np.where(y, g.beta(5, 2, size=len(y)), g.beta(2, 5, size=len(y))).astype(np.float32)).to(dev)
    ok = True
    for n_thr in N_THR:
        thresholds = np.linspace(0.0, 1.0, n_thr + 2)[1:-1].tolist()
        out = {"step": name, "hits": int(data.particle_id.shape[0]), "edges": int(w.shape[0]),
               "events": 1 if name == "single" else args.events, "thresholds": n_thr,
               "step_launches_per_threshold": LAUNCHES_PER_THRESHOLD}
        out["scan_ms"] = timed(lambda: G.ec_threshold_scan(data, w, thresholds), args.reps)
        st = {}

        def prepare():
            st["s"] = GA._scan_prepare(data, w, thresholds, 0.9, 4.0, False)

        out["prepare_ms"] = timed(prepare, args.reps)
        out["steps_ms"] = timed(lambda: GA._scan_steps(st["s"]), args.reps)
        out["finish_ms"] = timed(lambda: GA._scan_finish(st["s"]), args.reps)
        out["particles"] = int(st["s"].n_rows)
        out["loop_ms"] = timed(lambda: loop(data, w, thresholds), args.loop_reps)
        out["loop_reps"] = args.loop_reps
        out["loop_over_scan"] = round(out["loop_ms"][0] / out["scan_ms"][0], 2)
        got, want = G.ec_threshold_scan(data, w, thresholds), loop(data, w, thresholds)
        out["equal_to_loop"] = len(got) == len(want) and all(
            list(a) == list(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a) for a, b in zip(got, want))
        ok = ok and out["equal_to_loop"]
        print(json.dumps(out), flush=True)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=6000)
    ap.add_argument("--events", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=20)
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--step", name, "--hits", str(args.hits),
               "--events", str(args.events), "--reps", str(args.reps), "--loop-reps", str(args.loop_reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"time_ec_scan: step {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
