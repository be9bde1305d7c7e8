#!/usr/bin/env python3
"""The k-scan of the metric-learning validation (GraphConstructionKNNScanner: one neighbour search at max(ks), the
components and counts of all ks, the tracking metrics of all ks) on the event generator of tools/bench_kscan.py
(particles as short chains in an 8-d latent space, 10 % noise hits), B events of N hits each, ks = 1..9:
  (a) as B single-event scanner calls,
  (b) as ONE call on the collated batch (every event its own scan).
Both in one process, alternating, after a warm-up of both; every timed window runs for at least --window seconds;
per-event time = median over the windows, with their spread.  Kernel launches of one pass of each come from the
profiler's device activity, and those of the collated call once more on the first two events alone: the number does
not depend on the number of events.  Needs a GPU.

    python tools/bench_kscan_batch.py                        # 32 events of 6 000 hits
    python tools/bench_kscan_batch.py --events 4 --hits 50000
    python tools/bench_kscan_batch.py --only single          # (a) alone, e.g. on another commit
"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnn_tracking_amd as G
from gnn_tracking_amd import GraphConstructionKNNScanner
from bench_kscan import KS, event
from bench_oc_batch import launches, window

FIELDS = ("x", "particle_id", "pt", "eta", "reconstructable", "true_edge_index")


def launch_names(fn):
    """as bench_oc_batch.launches, by name: {kernel or memory operation: launches of one pass}"""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def make_events(n_events, hits, dev):
    return [G.Data(**{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in zip(FIELDS, event(800 + i, hits))})
            for i in range(n_events)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=32)
    ap.add_argument("--hits", type=int, default=6000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--only", choices=("single", "collated"), help="time one of the two alone (e.g. (a) on another commit)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kscan_batch.py needs a GPU")
    dev = torch.device("cuda")
    events = make_events(a.events, a.hits, dev)
    scanner = GraphConstructionKNNScanner(ks=KS)

    def singles():
        for i, ev in enumerate(events):
            scanner(ev, i)

    runs = {"single": singles}
    if a.only != "single":
        batch, pair = G.collate(events), G.collate(events[:2])
        runs["collated"] = lambda: scanner(batch, 0)
    if a.only == "collated":
        del runs["single"]
    for _ in range(3):
        for f in runs.values():
            f()
    res = {"events": a.events, "hits_per_event": a.hits, "ks": len(KS)}
    for k, f in runs.items():
        f()
        res[f"records_{k}"] = len(scanner.results_raw)
    if not a.no_launch_count:
        for k, f in runs.items():
            res[f"launches_{k}"] = launches(f)
        if "collated" in runs and a.events > 2:
            # the same call on two events: the k-scan's own launches (ks_*, cc_*) do not depend on the number of
            # events; what differs is listed by name as [all events, two events]
            scanner(pair, 0)
            many, two = launch_names(runs["collated"]), launch_names(lambda: scanner(pair, 0))
            res["launches_collated_2_events"] = sum(two.values())
            res["kscan_launches_collated"] = [sum(v for k, v in c.items() if "ks_" in k) for c in (many, two)]
            res["launches_differ_in"] = {k[:60]: [many[k], two[k]] for k in sorted(set(many) | set(two)) if many[k] != two[k]}
    t = {k: [] for k in runs}
    for _ in range(a.windows):
        for k, f in runs.items():   # alternating
            t[k].append(window(f, a.window) / a.events * 1e3)
    for k, v in t.items():
        res[f"ms_per_event_{k}"] = round(statistics.median(v), 4)
        res[f"ms_per_event_{k}_min_max"] = [round(min(v), 4), round(max(v), 4)]
    if len(runs) == 2:
        res["speedup"] = round(res["ms_per_event_single"] / res["ms_per_event_collated"], 3)
    print(json.dumps(res), flush=True)
