#!/usr/bin/env python3
"""Timings of the EFMLP edge filter at event size.

One synthetic event: ``--hits`` hits (default 150 000, the bench.py default), the kNN graph of the first 8
node features with ``--k`` neighbours (default 33: about 5 M edges), ``EFMLP(node 14, edge 28, hidden 128,
depth 5)`` on ``[x_i, x_j, edge_features]``.  Reports, as medians of ``--iters`` runs after ``--warmup``
(HIP events on the current stream), one JSON line:

* forward alone, kernel and composed, and the share of the fp32 matrix peak the kernel forward reaches;
* forward + BCE + backward: composed, kernel, composed again (the same process, the same card);
* ``MLGraphConstruction.forward`` with the filter scored before / after the edge features are written.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import pathlib

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import gnn_tracking_amd as G  # noqa: E402
from gnn_tracking_amd import edge_filter, graph_construction, ops  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12   # MI355X, dense fp32 MFMA


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=150_000)
    ap.add_argument("--k", type=int, default=33)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = G.synthetic.make_event(3, args.hits, 2 * args.hits, dev)
    x = ev.x.contiguous()
    edge_index = G.knn_with_max_radius(x[:, :8].contiguous(), args.k, 1e9)
    edge_attr = ops.edge_features(x, edge_index)
    E = int(edge_index.shape[1])
    y = (torch.rand(E, device=dev) < 0.3).float()
    torch.manual_seed(0)
    model = G.EFMLP(node_indim=14, edge_indim=28, hidden_dim=args.hidden, depth=args.depth).to(dev)
    loss_fct = G.EdgeWeightBCELoss()
    data = G.Data(x=x, edge_index=edge_index, edge_attr=edge_attr)

    def forward():
        with torch.no_grad():
            model(data)

    def step():
        model.zero_grad(set_to_none=True)
        loss_fct(w=model(data)["W"], y=y, edge_index=edge_index, pt=ev.pt).backward()

    def with_kernel(on, fn):
        old, edge_filter._EFMLP_KERNEL = edge_filter._EFMLP_KERNEL, on
        try:
            return timed(fn, args.warmup, args.iters)
        finally:
            edge_filter._EFMLP_KERNEL = old

    res = dict(hits=args.hits, k=args.k, edges=E, hidden=args.hidden, depth=args.depth)
    res["step_composed_first_ms"] = with_kernel(False, step)
    res["step_kernel_ms"] = with_kernel(True, step)
    res["step_composed_last_ms"] = with_kernel(False, step)
    res["fwd_composed_ms"] = with_kernel(False, forward)
    res["fwd_kernel_ms"] = with_kernel(True, forward)
    flops = 2.0 * E * (56 * args.hidden + (args.depth - 1) * args.hidden**2 + args.hidden)
    res["fwd_flop"] = flops
    res["fwd_share_of_fp32_matrix_peak"] = flops / (res["fwd_kernel_ms"][0] * 1e-3) / FP32_MATRIX_PEAK

    gdata = G.Data(x=x, particle_id=torch.randint(0, 5000, (args.hits,), device=dev), pt=ev.pt,
                   reconstructable=torch.ones(args.hits, dtype=torch.bool, device=dev), eta=x[:, 3].contiguous(),
                   edge_index=ev.edge_index)

    def gc_forward(fused):
        gc = G.MLGraphConstruction(ec=model, ec_threshold=0.5, max_num_neighbors=args.k, max_radius=1e9,
                                   embedding_slice=(0, 8))
        old, graph_construction._EF_FUSED_CUT = graph_construction._EF_FUSED_CUT, fused
        old_k, edge_filter._EFMLP_KERNEL = edge_filter._EFMLP_KERNEL, True   # (the filter on its kernel in both orders)

        def run():
            with torch.no_grad():
                return gc(gdata)
        try:
            out = run()
            return timed(run, args.warmup, args.iters), int(out.edge_index.shape[1])
        finally:
            graph_construction._EF_FUSED_CUT, edge_filter._EFMLP_KERNEL = old, old_k

    res["gc_features_first_ms"], kept = gc_forward(False)
    res["gc_score_first_ms"], kept2 = gc_forward(True)
    res["gc_features_first_again_ms"], _ = gc_forward(False)
    assert kept == kept2
    res["gc_edges_kept"] = kept
    print(json.dumps(res))


if __name__ == "__main__":
    main()
