#!/usr/bin/env python3
"""The DBSCAN scan of the object-condensation validation (DBSCANHyperParamScannerFixed: one radius graph, 10 DBSCAN
trials, the tracking metrics of all trials) on the latent cloud of cfg5's generator, B events of N hits each:
  (a) as B single-event scanner calls,
  (b) as ONE call on the collated batch (every event its own problem).
Both in one process, alternating, after a warm-up of both; every timed window runs for at least --window seconds;
per-event time = median over the windows, with their spread.  Kernel launches of one pass of each come from the
profiler's device activity.  Needs a GPU.

    python tools/bench_oc_validation_batch.py                        # 32 events of 6 000 hits
    python tools/bench_oc_validation_batch.py --events 4 --hits 50000
    python tools/bench_oc_validation_batch.py --only single          # (a) alone, e.g. on another commit
"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnn_tracking_amd as G
from gnn_tracking_amd import synthetic
from gnn_tracking_amd.postprocessing import DBSCANHyperParamScannerFixed
from bench_oc_batch import launches, window

DIM = 8
TRIALS = [(0.05, 1), (0.08, 2), (0.1, 3), (0.12, 4), (0.15, 2), (0.18, 3), (0.2, 1), (0.25, 4), (0.3, 2), (0.07, 3)]


def make_events(n_events, hits, dev):
    """cfg5's cloud scaled to the event size: 3 clusters and 7 particles per 100 hits, as at 200 000 hits"""
    out = []
    for i in range(n_events):
        ev = synthetic.make_pileup_event(700 + i, hits, DIM, n_particles=max(hits * 7 // 100, 2), n_clusters=max(hits * 3 // 100, 1))
        out.append(G.Data(x=ev["x"].to(dev), edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev),
                          particle_id=ev["particle_id"].to(dev), pt=ev["pt"].to(dev), eta=ev["eta"].to(dev),
                          reconstructable=ev["reconstructable"].to(dev)))
    return out


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
        sys.exit("bench_oc_validation_batch.py needs a GPU")
    dev = torch.device("cuda")
    events = make_events(a.events, a.hits, dev)
    batch = G.collate(events)
    scanner = DBSCANHyperParamScannerFixed([{"eps": e, "min_samples": m} for e, m in TRIALS])

    def singles():
        for i, ev in enumerate(events):
            scanner(ev, {"H": ev.x}, i)

    def collated():
        scanner(batch, {"H": batch.x}, 0)

    runs = {k: f for k, f in (("single", singles), ("collated", collated)) if a.only in (None, k)}
    for _ in range(3):
        for f in runs.values():
            f()
    res = {"events": a.events, "hits_per_event": a.hits, "trials": len(TRIALS)}
    for k, f in runs.items():
        f()
        res[f"records_{k}"] = len(scanner._results)
    if not a.no_launch_count:
        for k, f in runs.items():
            res[f"launches_{k}"] = launches(f)
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
