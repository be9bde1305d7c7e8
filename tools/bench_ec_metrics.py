"""Edge-classifier validation metrics (gnntrk_bcs_counts, gnntrk_roc_auc, metrics.ec_validation_metrics) at
the cfg3 size (32 synthetic events x 150 k hits x 2 M edges = 64 M edges), saturated and uniform W, in
edge_index order (int64 ids) and held in CSR order (EdgeOrdered: int32 ids, labels through perm), against
the reference algorithm restated in plain torch on the device (200 BinaryClassificationStats per pt cut
with their .item() syncs, boolean-mask indexing, a torch.sort AUROC per cut and max_fpr).  HIP-event
times; one JSON line on stdout (and in --out).

    python tools/bench_ec_metrics.py [--events 32] [--reps 10] [--ref-reps 1] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_tracking_amd as G  # noqa: E402
from gnn_tracking_amd import _capi, ops, synthetic  # noqa: E402
from gnn_tracking_amd import metrics as M  # noqa: E402
from gnn_tracking_amd.edge_order import EdgeOrdered  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--events", type=int, default=32)
ap.add_argument("--hits", type=int, default=150_000)
ap.add_argument("--edges", type=int, default=2_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--ref-reps", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
HBM = 6.3e12   # achievable copy bandwidth of the MI355X (bytes / s)
PT_THLDS, MAX_FPRS = (0.0, 0.5, 0.9, 1.5), (None, 0.01, 0.001)

batch = G.collate([synthetic.make_event(100 + i, args.hits, args.edges, dev) for i in range(args.events)])
ei, N, E = batch.edge_index, batch.num_nodes, int(batch.edge_index.shape[1])
gi = ops.graph_index(ei, N)
print(f"N = {N}, E = {E}", file=sys.stderr)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def make_w(dist):
    g = torch.Generator(device=dev).manual_seed(5)
    if dist == "uniform":
        return torch.rand(E, generator=g, device=dev)
    good = torch.rand(E, generator=g, device=dev) < 0.95
    return torch.where(good == batch.y, torch.tensor(0.999, device=dev), torch.tensor(0.001, device=dev))


def counts_bytes(e):
    """Algorithmic bytes of the counts pass: score, label, permutation, two ids and two pt gathers per edge."""
    per = 4 + 1 + (4 if e.perm is not None else 0) + 2 * (8 if e.ids_i64 else 4) + 2 * 4
    return per * e.n, per


# -------------------------------------------------- the reference's algorithm in plain torch
def ref_bcs(w, y, thld):
    yi = y.int()
    true = yi == 1
    n_true = torch.sum(true).item()
    pf = w < thld
    n_pf = torch.sum(pf).item()
    ptrue = ~pf
    TP = torch.sum(true & ptrue).item()
    TN = torch.sum(~true & pf).item()
    FP = torch.sum(~true & ptrue).item()
    FN = torch.sum(true & pf).item()
    del n_true, n_pf
    TPR, TNR = M.zero_divide(TP, TP + FN), M.zero_divide(TN, TN + FP)
    mcc = M.zero_divide(TP * TN - FP * FN, np.sqrt(float((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN))))
    return (TPR + TNR) / 2, M.zero_divide(2 * TP, 2 * TP + FP + FN), TPR, TNR, mcc


def ref_auroc(w, y, max_fpr):
    """torchmetrics' binary ROC on the device: descending sort, distinct-value cumsums, trapezoids."""
    order = torch.argsort(w, descending=True)
    ws, ys = w[order], y[order].to(torch.float64)
    distinct = torch.nonzero(ws[1:] - ws[:-1]).squeeze(1)
    idx = torch.cat([distinct, torch.tensor([ws.numel() - 1], device=w.device)])
    tps = torch.cumsum(ys, 0)[idx]
    fps = 1 + idx - tps
    tpr = torch.cat([torch.zeros(1, device=w.device, dtype=torch.float64), tps / tps[-1]])
    fpr = torch.cat([torch.zeros(1, device=w.device, dtype=torch.float64), fps / fps[-1]])
    if max_fpr is not None:
        stop = int(torch.bucketize(torch.tensor(max_fpr, device=w.device, dtype=torch.float64), fpr, right=True))
        wgt = (max_fpr - fpr[stop - 1]) / (fpr[stop] - fpr[stop - 1])
        itp = torch.lerp(tpr[stop - 1], tpr[stop], wgt)
        tpr, fpr = torch.cat([tpr[:stop], itp.view(1)]), torch.cat([fpr[:stop], fpr.new_tensor([max_fpr])])
    return torch.trapz(tpr, fpr).item()


def ref_validation(w, y, pt, ei):
    out = {}
    for cut in PT_THLDS:
        if cut > 0:
            m = (pt[ei[0]] > cut) | (pt[ei[1]] > cut)
            wm, ym = w[m], y[m]
        else:
            wm, ym = w, y
        for f in MAX_FPRS:
            out[f"auc{f}_{cut}"] = ref_auroc(wm, ym, f)
        rows = [ref_bcs(wm, ym, t) for t in torch.linspace(0.0, 1.0, 200)]
        out[f"bcs_{cut}"] = torch.asarray(rows, device=w.device).T.max(dim=1).values.sum().item()
    return out


rec = {"metric": "ec_validation_metrics", "E": E, "N": N, "events": args.events, "hbm_bytes_per_s": HBM}
for dist in ("saturated", "uniform"):
    w = make_w(dist)
    thr = torch.linspace(0.0, 1.0, 200).to(dev)
    for form in ("edge_index", "csr"):
        if form == "csr":
            wf = EdgeOrdered(w[gi.perm.long()], gi)
            e = M._Edges(wf, batch.y, batch.pt, ei)
            assert e.perm is not None
        else:
            wf = w
            e = M._Edges(w, batch.y, batch.pt, ei)
        cbuf = torch.empty(len(PT_THLDS) * 2 * 201, dtype=torch.int64, device=dev)
        abuf = torch.empty(len(PT_THLDS) * _capi.AUC_STRIDE, dtype=torch.int64, device=dev)
        t_counts = timed(lambda: M._launch_counts(e, PT_THLDS, thr, cbuf), args.reps)
        t_auc = timed(lambda: M._launch_auc(e, PT_THLDS, [0.01, 0.001], abuf), args.reps)
        t_all = timed(lambda: M.ec_validation_metrics(wf, batch.y, batch.pt, ei), args.reps)
        nbytes, per = counts_bytes(e)
        key = f"{dist}/{form}"
        rec[key] = {"counts_ms": t_counts[0], "counts_min_ms": t_counts[1],
                    "counts_bytes_per_edge": per, "counts_GBps": nbytes / (t_counts[1] * 1e-3) / 1e9,
                    "counts_floor_ms": nbytes / HBM * 1e3, "auroc_ms": t_auc[0], "auroc_min_ms": t_auc[1],
                    "validation_metrics_ms": t_all[0], "validation_metrics_min_ms": t_all[1]}
        print(f"{key}: counts {t_counts[0]:.3f} ms ({rec[key]['counts_GBps']:.0f} GB/s, floor "
              f"{rec[key]['counts_floor_ms']:.3f} ms at {per} B/edge), auroc {t_auc[0]:.3f} ms, "
              f"ec_validation_metrics {t_all[0]:.3f} ms", file=sys.stderr)
    if args.ref_reps > 0:
        t_ref = timed(lambda: ref_validation(w, batch.y, batch.pt, ei), args.ref_reps, warm=1)
        rec[f"{dist}/reference_form_ms"] = t_ref[0]
        print(f"{dist}: reference form in torch {t_ref[0]:.1f} ms", file=sys.stderr)

line = json.dumps(rec)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
