#!/usr/bin/env python3
"""Times the geometric graph builder (``gnn_tracking_amd.GraphBuilder``).

* default (needs the GPU): the device time of ``build`` for a synthetic whole-pixel-event cloud of ``--hits`` hits
  (default 50 000) over the 18 pixel layers - straight tracks from the beam line plus noise, as in
  tools/make_golden_graph_builder.py - with HIP events around ``--iters`` builds after ``--warmup``; also the number of
  candidate pairs (the work of the reference's cross join) and of edges.  One JSON line.
* ``--ref PATH`` (CPU, next to a checkout of the reference, with pandas): the wall time of the reference's
  ``GraphBuilder.build_edges`` + ``to_pyg_data`` on the two sector point clouds of tests/golden/g23_graph_builder.npz.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
BARREL_R = np.array([32.0, 72.0, 116.0, 172.0])                                  # layers 7..10
ENDCAP_Z = np.array([600.0, 700.0, 820.0, 960.0, 1120.0, 1300.0, 1500.0])       # |z| of layers 6..0 and 11..17


def event_cloud(n_hits: int, seed: int = 0):
    """(x float32 [n, 14], layer, particle_id, pt): about 80 % track hits, 20 % noise"""
    g = np.random.default_rng(seed)
    n_tracks = max(1, int(0.8 * n_hits / 7.5))
    phi0, k = g.uniform(-np.pi, np.pi, n_tracks), g.uniform(-0.003, 0.003, n_tracks)
    z0, cot = g.uniform(-80, 80, n_tracks), np.sinh(g.uniform(-2.8, 2.8, n_tracks))
    pt = g.choice(np.array([0.05, 0.3, 0.7, 0.95, 2.0]), n_tracks)
    rows = []
    for i, r in enumerate(BARREL_R):
        z = z0 + r * cot
        ok = np.abs(z) < 480
        rows.append(np.stack([np.full(ok.sum(), r), (phi0 + k * r)[ok], z[ok], np.full(ok.sum(), 7.0 + i),
                              np.flatnonzero(ok) + 1.0, pt[ok]], axis=1))
    for i, az in enumerate(ENDCAP_Z):
        for lay, z in ((6 - i, -az), (11 + i, az)):
            with np.errstate(all="ignore"):
                r = (z - z0) / cot
            ok = (cot * z > 0) & (r > 30) & (r < 175)
            rows.append(np.stack([r[ok], (phi0 + k * r)[ok], np.full(ok.sum(), z), np.full(ok.sum(), float(lay)),
                                  np.flatnonzero(ok) + 1.0, pt[ok]], axis=1))
    a = np.concatenate(rows)
    n_noise = max(0, n_hits - len(a))
    lay = g.integers(0, 18, n_noise)
    barrel = (lay >= 7) & (lay <= 10)
    r = np.where(barrel, BARREL_R[np.clip(lay - 7, 0, 3)], g.uniform(30, 175, n_noise))
    z = np.where(barrel, g.uniform(-480, 480, n_noise),
                 np.where(lay <= 6, -ENDCAP_Z[np.clip(6 - lay, 0, 6)], ENDCAP_Z[np.clip(lay - 11, 0, 6)]))
    a = np.concatenate([a, np.stack([r, g.uniform(-np.pi, np.pi, n_noise), z, lay.astype(np.float64), np.zeros(n_noise),
                                     np.zeros(n_noise)], axis=1)])[:n_hits]
    a = a[g.permutation(len(a))]
    a[:, :3] += g.normal(0, 0.02, (len(a), 3))
    a[:, 1] = (a[:, 1] + np.pi) % (2 * np.pi) - np.pi
    x = np.zeros((len(a), 14), np.float32)
    x[:, :3] = a[:, :3]
    return x, a[:, 3].astype(np.int64), a[:, 4].astype(np.int64), a[:, 5].astype(np.float32)


def time_device(args) -> dict:
    import torch

    import gnn_tracking_amd as G

    x, layer, pid, pt = event_cloud(args.hits)
    n = len(layer)
    t = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    pc = G.Data(x=t(x), layer=t(layer), particle_id=t(pid), pt=t(pt), reconstructable=t((pid > 0).astype(np.int64)),
                sector=t(np.zeros(n, np.int64)), eta=t(np.zeros(n, np.float32)))
    b = G.GraphBuilder()
    per_layer = np.bincount(layer, minlength=18)
    pairs = sum(int(per_layer[l1]) * int(per_layer[l2]) for l1, l2 in b._layer_pairs())
    for _ in range(args.warmup):
        data = b.build(pc)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        data = b.build(pc)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"hits": n, "candidate_pairs": pairs, "edges": data.num_edges, "true_edges": int(data.y.sum()),
            "build_ms_median": float(np.median(times)), "build_ms_min": float(min(times)), "iters": args.iters}


def time_reference(ref: pathlib.Path, iters: int) -> dict:
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()
    import tempfile

    import torch
    from gnn_tracking.graph_construction.graph_builder import GraphBuilder
    from torch_geometric.data import Data

    tmp = tempfile.mkdtemp(prefix="gbt_")
    b = GraphBuilder(tmp, tmp, collect_data=False)
    keys = ("x", "layer", "particle_id", "pt", "reconstructable", "sector", "eta")
    with np.load(REPO / "tests" / "golden" / "g23_graph_builder.npz") as f:
        clouds = [Data(**{k: torch.from_numpy(f[f"sector{s}_{k}"]) for k in keys}) for s in (0, 1)]
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        for c in clouds:
            be = b.build_edges(b.get_dataframe(c, 0))
            b.to_pyg_data(c, be[0], be[1], be[2])
        times.append(time.perf_counter() - t0)
    return {"reference_two_sectors_s_median": float(np.median(times)), "hits": [int(c.x.shape[0]) for c in clouds],
            "iters": iters}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=50000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ref", type=pathlib.Path, default=None, help="time the reference on the CPU instead")
    args = ap.parse_args()
    print(json.dumps(time_reference(args.ref, args.iters) if args.ref else time_device(args)))


if __name__ == "__main__":
    main()
