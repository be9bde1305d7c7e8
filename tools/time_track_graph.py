#!/usr/bin/env python3
"""Times ``get_track_graph_info_from_data`` on the device: one event of the pile-up generator
(``synthetic.make_pileup_event``: 6 000 hits in 600 clusters, 600 particle ids drawn independently of the positions, so
that every selected particle is split into single hits) with its kNN graph (k = 6, radius 1), and the collation of 32
such events.  That graph is one component per cluster and the hits of a particle lie in different clusters: no
particle needs a search.  The ``*_bridged`` steps add one random edge inside the event per two hits, which joins the
clusters: then nearly every selected particle is searched, through a graph of short paths and wide levels - the
worst case for the search kernel.  Per input: the whole call and its parts - labels
(two ``gnntrk_cc_labels``), adjacency, table, distance search - as wall time around work that ends in a device
synchronise, median [min, max] of ``--reps`` repetitions after two warm-up rounds.  The single event is also timed
through the networkx restatement ``tests/track_graph_ref.py`` (the reference's algorithm with one search per particle
instead of one per pair of hits), and the two tables are compared.

Without ``--step`` the tool is a driver: it runs every step as a child process under its own ``timeout`` and stops at
the first one that fails.

Usage:  python tools/time_track_graph.py [--hits 6000] [--events 32] [--reps 20]
Prints one JSON line per step.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

STEPS = {"single": 240, "single_bridged": 240, "batch": 240, "batch_bridged": 240}   # seconds of `timeout` per step
BRIDGES = 0.5   # random edges per hit of the *_bridged steps
K, RADIUS = 6, 1.0


def make_data(seed, hits, device, bridged):
    import torch

    import gnn_tracking_amd as G
    from gnn_tracking_amd.synthetic import make_pileup_event

    ev = make_pileup_event(seed, hits, n_particles=max(hits // 10, 2), n_clusters=max(hits // 10, 2))
    d = G.Data(**{k: v.to(device) for k, v in ev.items() if k != "beta"})
    d.edge_index = G.knn_with_max_radius(d.x, K, RADIUS)
    if bridged:
        g = torch.Generator().manual_seed(seed)
        extra = torch.randint(0, hits, (2, int(BRIDGES * hits)), generator=g).to(device)
        d.edge_index = torch.cat([d.edge_index, extra], dim=1)
    d.y = d.particle_id[d.edge_index[0]] == d.particle_id[d.edge_index[1]]
    torch.cuda.synchronize()
    return d


def timed(fn, reps):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(v, 4) for v in (statistics.median(ts), min(ts), max(ts))]


def parts(data, reps):
    """the calls of ``graph_analysis.track_graph_table``, one at a time"""
    import torch

    from gnn_tracking_amd import _capi, events, ops
    from gnn_tracking_amd import graph_analysis as GA
    from gnn_tracking_amd.graph_masks import get_good_node_mask

    lib, p = _capi.load(), ops._p
    ei, pid = data.edge_index.contiguous(), data.particle_id.contiguous()
    mask = get_good_node_mask(data).to(torch.uint8)
    n, m, dev = int(pid.shape[0]), int(ei.shape[1]), ei.device
    ptr = events.event_ptr(data)
    seg_ptr = torch.tensor([0, n], device=dev) if ptr is None else ptr.to(dev)
    n_ev = seg_ptr.numel() - 1
    stream = ops._stream(ei)
    st = {}

    def labels():
        st["seg"], st["comp"] = GA.cc_labels(ei, n, same_pid=pid, check=False), GA.cc_labels(ei, n, check=False)

    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbrs = torch.empty(2 * m, dtype=torch.int32, device=dev)
    table = torch.empty((n, 9), dtype=torch.int64, device=dev)
    search = torch.empty(n, dtype=torch.int32, device=dev)
    head = torch.empty(4, dtype=torch.int64, device=dev)
    ws_a = ops._ws(lib.gnntrk_track_graph_adjacency_workspace_bytes(n), ei)
    ws_t = ops._ws(lib.gnntrk_track_graph_table_workspace_bytes(n), ei)
    ws_d = ops._ws(lib.gnntrk_track_graph_distance_workspace_bytes(n, 0), ei)

    def adjacency():
        _capi.check(lib.gnntrk_track_graph_adjacency(p(ei), m, n, p(seg_ptr), n_ev, p(rowptr), p(nbrs), p(head[2:]),
                                                     p(ws_a), ws_a.numel(), stream), lib)

    def table_call():
        _capi.check(lib.gnntrk_track_graph_table(p(st["seg"]), p(st["comp"]), p(pid), p(mask), n, p(seg_ptr), n_ev,
                                                 p(table), p(search), p(head), p(ws_t), ws_t.numel(), stream), lib)

    def distance():
        _capi.check(lib.gnntrk_track_graph_distance(p(table), p(search), p(head), p(st["seg"]), p(rowptr), p(nbrs), n,
                                                    p(seg_ptr), n_ev, p(ws_d), ws_d.numel(), stream), lib)

    out = {"labels_ms": timed(labels, reps), "adjacency_ms": timed(adjacency, reps), "table_ms": timed(table_call, reps)}
    # (a search only writes its row's distance: repeating it on the same table repeats the same work)
    out["distance_ms"] = timed(distance, reps)
    rows, searches = (int(v) for v in head[:2].tolist())
    out.update(rows=rows, searches=searches, edges=m)
    return out


def step(name, args):
    import numpy as np
    import torch

    import gnn_tracking_amd as G

    dev = torch.device("cuda:0")
    single, bridged = name.startswith("single"), name.endswith("bridged")
    if single:
        data = make_data(100, args.hits, dev, bridged)
    else:
        data = G.collate([make_data(100 + i, args.hits, dev, bridged) for i in range(args.events)])
    out = {"step": name, "hits": int(data.particle_id.shape[0]), "events": 1 if single else args.events}
    out["whole_call_ms"] = timed(lambda: G.get_track_graph_info_from_data(data), args.reps)
    out.update(parts(data, args.reps))
    total = sum(out[k][0] for k in ("labels_ms", "adjacency_ms", "table_ms", "distance_ms"))
    out["distance_share_of_parts"] = round(out["distance_ms"][0] / total, 3)
    if single:
        import track_graph_ref as R
        from gnn_tracking_amd.graph_masks import get_good_node_mask

        got = G.get_track_graph_info_from_data(data)
        ei, pid = data.edge_index.cpu().numpy(), data.particle_id.cpu().numpy()
        mask = get_good_node_mask(data).cpu().numpy()
        t0 = time.perf_counter()
        want = R.table(ei, pid, mask)
        out["networkx_restatement_s"] = round(time.perf_counter() - t0, 3)
        out["equal_to_restatement"] = all(np.array_equal(got[c], want[c]) for c in R.COLUMNS)
        d = want["distance_largest_segments"]
        out["split"], out["no_path"] = int((want["n_segments"] > 1).sum()), int(np.isinf(d).sum())
        out["max_distance"] = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
    print(json.dumps(out), flush=True)
    return 0 if out.get("equal_to_restatement", True) else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=6000)
    ap.add_argument("--events", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--step", name, "--hits", str(args.hits),
               "--events", str(args.events), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"time_track_graph: step {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
