#!/usr/bin/env python3
"""The object-condensation optimisation step (MLGraphConstruction -> GraphTCN -> CondensationLossRG -> backward -> Adam,
cfg5's model and loss settings) on B events of N hits each:
  (a) as B single-event steps,
  (b) as ONE step on the collated batch (every event its own problem).
Both in one process, alternating, after a warm-up of both; every timed window runs for at least --window seconds;
per-event time = median over the windows, with their spread.  Kernel launches of one step of each come from the
profiler's device activity.  Needs a GPU.

    python tools/bench_oc_batch.py                        # 32 events of 6 000 hits, fp32 and bf16 storage
    python tools/bench_oc_batch.py --events 4 --hits 50000
"""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_tracking_amd as G
from gnn_tracking_amd import dist as gdist, ops, synthetic, training

DIM, K_NN = 8, 16


def make_events(n_events, hits, dev):
    """cfg5's cloud scaled to the event size: 3 particles and 7 hits per 100 hits and per cluster, as at 200 000 hits"""
    out = []
    for i in range(n_events):
        ev = synthetic.make_pileup_event(700 + i, hits, DIM, n_particles=max(hits * 7 // 100, 2), n_clusters=max(hits * 3 // 100, 1))
        g = np.random.default_rng(700 + i)
        x = torch.cat([ev["x"], torch.from_numpy(g.uniform(0, 1.5, size=(hits, 6)).astype(np.float32))], dim=1)
        out.append(G.Data(x=x.to(dev), edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev),
                          particle_id=ev["particle_id"].to(dev), pt=ev["pt"].to(dev), eta=ev["eta"].to(dev),
                          reconstructable=ev["reconstructable"].to(dev)))
    return out


def make_module(dev, bf16):
    torch.manual_seed(0)
    model = G.GraphTCN(14, 28, h_outdim=DIM, hidden_dim=40, L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=DIM).to(dev)
    flat = gdist.FlatParameters(model)
    mod = training.TCModule(model, loss_fct=G.CondensationLossRG(lw_repulsive=1.0, lw_noise=0.1, lw_coward=0.1),
                            preproc=G.MLGraphConstruction(ml=None, embedding_slice=(0, DIM), max_radius=1.0, max_num_neighbors=K_NN),
                            flat=flat, scheduler=None, bf16=bf16, optimizer=lambda p: torch.optim.Adam(p, lr=1e-4))
    return mod


def step(mod, data):
    import copy
    opt = mod.configure_optimizers()
    mod.zero_grad()
    ops.clear_graph_index_cache()
    d = mod.data_preproc(copy.copy(data))
    with G.bf16_storage(mod.bf16):
        out = mod(d, _preprocessed=True)
        loss, _ = mod.get_losses(out, d, metrics=False)
        with ops.grad_sinks_armed():
            loss.backward()
    opt.step()
    return loss.detach()


def window(fn, min_seconds):
    """seconds per call of fn over a window of at least min_seconds"""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 2 == 0 or n == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


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
        sys.exit("bench_oc_batch.py needs a GPU")
    dev = torch.device("cuda")
    events = make_events(a.events, a.hits, dev)
    batch = G.collate(events)
    for dtype in ("f32", "bf16"):
        mod = make_module(dev, dtype == "bf16")

        def singles():
            for ev in events:
                step(mod, ev)

        def collated():
            step(mod, batch)

        runs = {k: f for k, f in (("single", singles), ("collated", collated)) if a.only in (None, k)}
        for _ in range(3):
            for f in runs.values():
                f()
        res = {"dtype": dtype, "events": a.events, "hits_per_event": a.hits}
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
