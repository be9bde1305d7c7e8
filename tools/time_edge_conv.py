#!/usr/bin/env python3
"""Times the dynamic edge convolution (``ops.edge_conv``): the fused kNN edge-conv kernel (csrc/edge_conv.hip)
against the same operator composed from the library's other operators, at event size.  Needs the GPU.

* Clouds of ``--hits`` (100 000) random hits, ``D`` in {14, 10}, ``H`` = 100, ``O`` = 10, ``k`` in {1, 3, 16} (the
  query itself included), add / mean / max: forward, and forward + backward with a gradient for ``x``, of both
  paths on the same neighbour table (searched once per ``D``, outside the timed windows).
* One ``PointCloudTCN`` training step (forward, ``CondensationLossRG``, backward) at the model's defaults on a
  ``--model-hits`` cloud, with the kernel path on and off.
* ``--composed-only``: the composed path alone.  It is written here from ``ops.knn_graph``, ``ops.graph_index``,
  ``ops.fused_mlp``, ``ops.segment_sum`` and torch's ``scatter_reduce`` - operators the package had before the
  kernel - so that this mode runs on a checkout from before the kernel and gives that checkout's times.

Per configuration ``--reps`` windows of ``--iters`` calls per path, the paths alternating inside a repetition, HIP
events around a window, everything warmed up first: the median window and the spread (smallest, largest) in
milliseconds per call, and the largest difference between the two paths' outputs.  One JSON line each.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

sys.dont_write_bytecode = True

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

import gnn_tracking_amd as G  # noqa: E402
from gnn_tracking_amd import ops  # noqa: E402

DIMS, KS, AGGRS, HIDDEN, OUT = (14, 10), (1, 3, 16), ("add", "mean", "max"), 100, 10


def self_first_edges(x, k):
    """``(edge_index, nbr, cnt)``: the k - 1 nearest other hits of every hit with the hit itself in front"""
    n, dev = int(x.shape[0]), x.device
    q = torch.arange(n, device=dev)
    if k == 1:
        return torch.stack([q, q]), torch.zeros(n, 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    knn = ops.knn_graph(x, k - 1)
    assert int(knn.shape[1]) == n * (k - 1)
    ids = torch.cat([q[:, None], knn[0].view(n, k - 1)], dim=1)
    ei = torch.stack([ids.reshape(-1), q[:, None].expand(n, k).reshape(-1)]).contiguous()
    return ei, knn[0].view(n, k - 1).to(torch.int32).contiguous(), torch.full((n,), k - 1, dtype=torch.int32, device=dev)


def composed(x, ei, weights, biases, aggr):
    """the operator from what the package had before the kernel"""
    n, m = int(x.shape[0]), int(ei.shape[1])
    gi = ops.graph_index(ei, n)
    xt = ops._GatherRows.apply(x, gi.tgt, ("tgt", gi))
    xs = ops._GatherRows.apply(x, gi.src, ("src", gi))
    msg = ops.fused_mlp([ops.Seg(torch.cat([xt, xs - xt], dim=1))], weights, biases, n_rows=m)
    if aggr == "max":
        idx = gi.tgt.to(torch.int64)[:, None].expand(m, msg.shape[1])
        return torch.zeros(n, msg.shape[1], device=x.device).scatter_reduce(0, idx, msg, "amax", include_self=False)
    h = ops.segment_sum(msg, gi, "tgt")
    return h / float(ei.shape[1] // n) if aggr == "mean" else h


def kernel(x, nbr, cnt, weights, biases, aggr, ei):
    old, ops._EDGE_CONV_KERNEL = ops._EDGE_CONV_KERNEL, True
    try:
        return ops.edge_conv(x, nbr, cnt, weights, biases, aggr=aggr, include_self=True, edge_index=ei)
    finally:
        ops._EDGE_CONV_KERNEL = old


def window(fn, iters):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fns: dict, iters, reps, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(window(fn, iters))
    return {name: dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
            for name, t in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=100_000)
    ap.add_argument("--model-hits", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--composed-only", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-operator", action="store_true")
    ap.add_argument("--out", type=pathlib.Path, default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_edge_conv: no GPU; there is no time without one")
    dev = torch.device("cuda")
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out is not None:
            with args.out.open("a") as f:
                f.write(line + "\n")

    g = torch.Generator().manual_seed(0)
    for D in (() if args.skip_operator else DIMS):
        x0 = torch.randn(args.hits, D, generator=g).to(dev)
        W = [(torch.randn(HIDDEN, 2 * D, generator=g) / (2 * D) ** 0.5).to(dev).requires_grad_(),
             (torch.randn(OUT, HIDDEN, generator=g) / HIDDEN ** 0.5).to(dev).requires_grad_()]
        b = [(0.1 * torch.randn(HIDDEN, generator=g)).to(dev).requires_grad_(),
             (0.1 * torch.randn(OUT, generator=g)).to(dev).requires_grad_()]
        r = torch.randn(args.hits, OUT, generator=g).to(dev)
        for k in KS:
            ei, nbr, cnt = self_first_edges(x0, k)
            for aggr in AGGRS:
                x = x0.clone().requires_grad_()
                paths = {"composed": lambda: composed(x, ei, W, b, aggr)}
                if not args.composed_only:
                    paths["kernel"] = lambda: kernel(x, nbr, cnt, W, b, aggr, ei)
                diff = None
                if not args.composed_only:
                    with torch.no_grad():
                        diff = float((paths["kernel"]() - paths["composed"]()).abs().max())

                def fwd(fn):
                    def go():
                        with torch.no_grad():
                            fn()
                    return go

                def fwd_bwd(fn):
                    def go():
                        for t in (x, *W, *b):
                            t.grad = None
                        (fn() * r).sum().backward()
                    return go

                rec = dict(what="edge_conv", hits=args.hits, D=D, H=HIDDEN, O=OUT, k=k, aggr=aggr, max_abs_diff=diff,
                           forward=measure({n_: fwd(f) for n_, f in paths.items()}, args.iters, args.reps),
                           forward_backward=measure({n_: fwd_bwd(f) for n_, f in paths.items()}, args.iters, args.reps))
                emit(rec)

    if not args.skip_model and hasattr(G, "PointCloudTCN"):
        from gnn_tracking_amd import synthetic
        from gnn_tracking_amd.training import TCModule

        data = synthetic.make_event(0, args.model_hits, 2, dev)
        data.particle_id = torch.arange(args.model_hits, device=dev) // 10
        torch.manual_seed(0)
        model = G.PointCloudTCN(14).to(dev)
        mod = TCModule(model, loss_fct=G.CondensationLossRG())

        def step(on):
            def go():
                old, ops._EDGE_CONV_KERNEL = ops._EDGE_CONV_KERNEL, on
                try:
                    model.zero_grad(set_to_none=True)
                    loss, _ = mod.training_step(data)
                    loss.backward()
                finally:
                    ops._EDGE_CONV_KERNEL = old
            return go

        paths = {"composed": step(False)} if args.composed_only else {"composed": step(False), "kernel": step(True)}
        emit(dict(what="PointCloudTCN training step", hits=args.model_hits,
                  step=measure(paths, max(1, args.iters // 4), args.reps, warmup=2)))
    elif not args.skip_model:
        emit(dict(what="PointCloudTCN training step", note="this checkout has no PointCloudTCN"))


if __name__ == "__main__":
    main()
