#!/usr/bin/env python3
"""One validation batch of the metric-learning k-scan on a 200 k-hit event (8-d latent space, ks 1..9):
the neighbour search at k = 9, the component + count kernels of all nine ks (gnntrk_kscan_counts), the
tracking-metrics call for the upper bounds, the host copy, and the whole batch - medians after a
warm-up - next to the reference's algorithm on the host for the same input (networkx components + the
Python loops of analysis/graphs.py, restated here; pandas for the upper bounds when importable, otherwise
the numpy restatement of tests/tracking_metrics_ref.py; the output says which), on the largest input it
finishes within a minute.

Usage:  python tools/bench_kscan.py [--hits 200000] [--reps 5] [--host-hits 20000]
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

KS = list(range(1, 10))


def event(seed, n, dim=8, particles_per_hit=0.03):
    """Particles as short chains (step 0.03 along a random direction) in a ball, 10 % noise hits (id 0)."""
    g = np.random.default_rng(seed)
    n_particles = max(2, int(particles_per_hit * n))

    def ball(m):
        v = g.normal(size=(m, dim))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * (3.0 * g.random((m, 1)) ** (1.0 / dim))

    centres, direction = ball(n_particles), g.normal(size=(n_particles, dim))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    n_noise = int(0.1 * n)
    which = np.sort(g.integers(0, n_particles, size=n - n_noise))
    start = np.flatnonzero(np.r_[True, which[1:] != which[:-1]])
    rank = np.arange(len(which)) - np.repeat(start, np.diff(np.r_[start, len(which)]))
    x = centres[which] + 0.03 * rank[:, None] * direction[which] + 0.01 * g.normal(size=(len(which), dim))
    x = np.concatenate([x, ball(n_noise)]).astype(np.float32)
    pid = np.concatenate([(which + 1).astype(np.int64) * 2 ** 40, np.zeros(n_noise, np.int64)])
    nxt = np.flatnonzero(which[1:] == which[:-1])
    te = np.stack([np.concatenate([nxt, nxt + 1]), np.concatenate([nxt + 1, nxt])])
    k = pid >> 40
    pt = np.exp(g.normal(-0.5, 0.9, size=n_particles + 1)).astype(np.float32)[k]
    eta = np.clip(g.normal(0, 2, size=n_particles + 1), -4.6, 4.6).astype(np.float32)[k]
    perm = g.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return x[perm], pid[perm], pt[perm], eta[perm], np.ones(n, np.float32), inv[te]


def host_scan(x, pid, pt, eta, reco, te):
    """The reference's per-k work on the host, given the edge lists (the neighbour search is not timed):
    networkx components twice, the Python loop over segments, the per-node label dict, tracking metrics."""
    import networkx as nx

    import kscan_ref as R
    import tracking_metrics_ref as TR

    nbr, cnt = R.neighbour_table(x, max(KS), 1.0) if len(x) <= 4000 else device_table(x)
    mask = R.good_node_mask(pid, pt, eta, reco)
    t0 = time.perf_counter()
    for k in KS:
        e = R.table_edges(nbr, cnt, k)
        y = pid[e[0]] == pid[e[1]]
        upid, counts = np.unique(pid[mask], return_counts=True)
        pid2count = dict(zip(upid.tolist(), counts.tolist()))
        keep = y & mask[e[0]] & mask[e[1]]
        gx = nx.Graph()
        gx.add_edges_from(e[:, keep].T)
        largest = {}
        for seg in nx.connected_components(gx):
            p = int(pid[next(iter(seg))])
            largest[p] = max(largest.get(p, 0), len(seg) / pid2count[p])
        for p in set(upid.tolist()) - set(largest):
            largest[p] = 1 / pid2count[p]
        gx = nx.Graph()
        gx.add_nodes_from(range(len(pid)))
        gx.add_edges_from(e[:, y].T)
        index = {node: i for i, comp in enumerate(nx.connected_components(gx)) for node in comp}
        labels = np.array([index[node] for node in gx.nodes()])
        TR.tracking_metrics_flat(labels, pid, pt, eta, reco, (0.9,))
    return time.perf_counter() - t0


def device_table(x):
    from gnn_tracking_amd import _capi, ops

    d = torch.from_numpy(x).cuda()
    n = len(x)
    nbr = torch.empty(n * max(KS), dtype=torch.int32, device=d.device)
    cnt = torch.empty(n, dtype=torch.int32, device=d.device)
    ops._knn_search(_capi.load(), d, max(KS), 1.0, None, nbr, cnt, ops._stream(d))
    return nbr.cpu().numpy().reshape(n, -1), cnt.cpu().numpy()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-hits", type=int, default=20_000)
    args = ap.parse_args()
    from gnn_tracking_amd import Data, GraphConstructionKNNScanner, _capi, ops
    from gnn_tracking_amd import k_scanner as KSC
    from gnn_tracking_amd.cluster_metrics import _counts, _cut_plan
    from gnn_tracking_amd.graph_masks import get_good_node_mask

    dev = torch.device("cuda:0")
    ev = event(1, args.hits)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    d = Data(x=t(ev[0]), particle_id=t(ev[1]), pt=t(ev[2]), eta=t(ev[3]), reconstructable=t(ev[4]),
             true_edge_index=t(ev[5]))
    n, kmax, lib = args.hits, max(KS), _capi.load()
    nbr = torch.empty(n * kmax, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    mask = get_good_node_mask(d)
    _, cuts, _ = _cut_plan([0.9])
    state = {}

    def search():
        ops._knn_search(lib, d.x, kmax, 1.0, None, nbr, cnt, ops._stream(d.x))

    def counts():
        state["c"], state["l"] = KSC.kscan_counts(nbr, cnt, kmax, KS, d.particle_id, mask, d.true_edge_index)

    def tracking():
        state["t"] = _counts(state["l"], d.particle_id, d.pt, d.reconstructable, d.eta, cuts, 3, 4)

    def copy():
        torch.cat([state["c"].reshape(-1), state["t"]]).cpu()

    scanner = GraphConstructionKNNScanner(ks=KS)
    out = {"hits": n, "ks": KS, "dim": 8}
    out["search_k9_ms"] = timed(search, args.reps)
    out["components_and_counts_ms"] = timed(counts, args.reps)
    out["tracking_metrics_ms"] = timed(tracking, args.reps)
    out["host_copy_ms"] = timed(copy, args.reps)
    out["whole_batch_ms"] = timed(lambda: scanner(d, 0), args.reps)
    # launches of one gnntrk_kscan_counts call: init, particles, true edges; per k union, compress, segmax,
    # segments; finish (+ 2 clears); host reads per batch: the one copy
    out["kscan_kernel_launches"] = 3 + 4 * len(KS) + 1
    out["host_reads_per_batch"] = 1
    out["n_edges_k9"] = int(state["c"][-1, 0])
    try:
        hev = event(1, args.host_hits)
        out["host_reference_hits"] = args.host_hits
        out["host_reference_s"] = host_scan(*hev)
        out["host_reference"] = "networkx components + python loops + numpy restatement of the tracking metrics"
    except ImportError as e:
        out["host_reference"] = f"not run: {e}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
