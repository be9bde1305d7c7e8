#!/usr/bin/env python3
"""Times the point cloud builder (``gnn_tracking_amd.PointCloudBuilder``).

* default (needs the GPU): a synthetic full-size event (``--hits`` 120 000 hits, 5 cells per hit, ``--particles``
  10 000 particles) and, with ``--bundled``, the reference's bundled event of tests/golden/g24_point_cloud.npz, each
  with 1 and 64 sectors (and 2 with the truth edges): the wall time of ``build`` per event (tables already on the
  device, synchronised) and the device time of every C entry, with HIP events around the call (an entry is a few
  launches; their list is in csrc/point_cloud.hip).  One JSON line per configuration.
* ``--ref PATH`` (CPU, next to a checkout of the reference, with pandas): the wall time of the reference's
  ``PointCloudBuilder.process()`` on its bundled event with the CSV load taken out (the loader returns copies of the
  parsed frames), for the same sector counts.
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
sys.path.insert(0, str(REPO / "tests"))
PIXEL = [(8, l) for l in (2, 4, 6, 8)] + [(v, l) for v in (7, 9) for l in range(2, 16, 2)]
CONFIGS = (dict(n_sectors=1), dict(n_sectors=64, measurement_mode=True), dict(n_sectors=2, add_true_edges=True))


def synthetic_event(n_hits: int, n_particles: int, cells_per_hit: int = 5, seed: int = 0):
    """(tables, detector columns): hits of random particles (10 % noise) on the pixel layers, 3 000 modules"""
    g = np.random.default_rng(seed)
    modules = 200
    rows = [(v, l, m) for v, l in PIXEL for m in range(modules)]
    det = {k: np.array([r[i] for r in rows], np.int64) for i, k in enumerate(("volume_id", "layer_id", "module_id"))}
    for k in ("rot_xu", "rot_xv", "rot_xw", "rot_yu", "rot_yv", "rot_yw", "rot_zu", "rot_zv", "rot_zw"):
        det[k] = g.uniform(-1, 1, len(rows))
    det["module_t"], det["pitch_u"], det["pitch_v"] = (np.full(len(rows), v) for v in (0.15, 0.05, 0.05625))
    pids = (np.arange(1, n_particles + 1, dtype=np.int64) * 4503599627370517) % 2 ** 60     # (distinct: the factor is odd)
    phi0 = g.uniform(-np.pi, np.pi, n_particles)
    owner = g.integers(0, n_particles, n_hits)
    noise = g.uniform(size=n_hits) < 0.1
    phi = np.where(noise, g.uniform(-np.pi, np.pi, n_hits), phi0[owner] + g.normal(0, 0.05, n_hits))
    r = g.uniform(30, 1000, n_hits)
    lay = g.integers(0, len(PIXEL), n_hits)
    hit_id = np.arange(1, n_hits + 1, dtype=np.int64)
    hits = dict(hit_id=hit_id, x=r * np.cos(phi), y=r * np.sin(phi), z=g.uniform(-1500, 1500, n_hits),
                volume_id=np.array([PIXEL[i][0] for i in lay]), layer_id=np.array([PIXEL[i][1] for i in lay]),
                module_id=g.integers(0, modules, n_hits))
    chit = np.repeat(hit_id, cells_per_hit)
    cells = dict(hit_id=chit, ch0=g.integers(0, 400, len(chit)), ch1=g.integers(0, 1200, len(chit)),
                 value=g.uniform(0.01, 1, len(chit)))
    parts = dict(particle_id=pids, px=g.normal(0, 0.6, n_particles), py=g.normal(0, 0.6, n_particles),
                 pz=g.normal(0, 1, n_particles), q=np.ones(n_particles), vx=np.zeros(n_particles), vy=np.zeros(n_particles))
    truth = dict(hit_id=hit_id, particle_id=np.where(noise, 0, pids[owner]))
    return dict(hits=hits, cells=cells, particles=parts, truth=truth), det


class _Timed:
    """the library with HIP events around every compute entry of the point cloud builder"""

    def __init__(self, lib, torch):
        self._lib, self._torch, self.records = lib, torch, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("gnntrk_point_cloud_", "gnntrk_truth_edges_")) or name.endswith("workspace_bytes"):
            return fn

        def timed(*a):
            e0, e1 = (self._torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            rc = fn(*a)
            e1.record()
            self.records.append((name[7:], e0, e1))
            return rc

        return timed


def time_device(args) -> None:
    import torch

    import gnn_tracking_amd as G
    from gnn_tracking_amd import _capi

    events = {"synthetic": synthetic_event(args.hits, args.particles)}
    if args.bundled:
        import point_cloud_cases as C

        events["bundled"] = (C.golden_tables(), C.golden_detector())
    lib = _Timed(_capi.load(), torch)
    _capi.load = lambda: lib
    for name, (tables, det) in events.items():
        dev = {t: {c: torch.from_numpy(np.ascontiguousarray(v)).cuda() for c, v in cols.items()} for t, cols in tables.items()}
        detector = G.load_detector(det)
        for kw in CONFIGS:
            b = G.PointCloudBuilder(detector=detector, **kw)
            for _ in range(args.warmup):
                out = b.build(dev)
            torch.cuda.synchronize()
            wall, entries = [], {}
            for _ in range(args.iters):
                lib.records.clear()
                t0 = time.perf_counter()
                out = b.build(dev)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                for entry, e0, e1 in lib.records:
                    entries.setdefault(entry, []).append(e0.elapsed_time(e1))
            print(json.dumps({"event": name, **{k: v for k, v in kw.items()}, "hits": len(tables["hits"]["hit_id"]),
                              "cells": len(tables["cells"]["hit_id"]), "rows": sum(int(c.x.shape[0]) for c in out),
                              "truth_edges": sum(int(c.edge_index.shape[1]) for c in out),
                              "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(min(wall)),
                              "entry_ms_median": {k: float(np.median(v)) for k, v in entries.items()}, "iters": args.iters}))


def time_reference(ref: pathlib.Path, iters: int) -> None:
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(ref / "src"))
    import _ref_standins

    _ref_standins.install()
    import tempfile

    from gnn_tracking.preprocessing import point_cloud_builder as pcb

    trackml = ref / "tests" / "test_data" / "trackml"
    frames = pcb.simple_data_loader(trackml / "event000000001")
    pcb.simple_data_loader = lambda f: tuple(x.copy() for x in frames)
    for kw in CONFIGS:
        b = pcb.PointCloudBuilder(indir=trackml, outdir=tempfile.mkdtemp(prefix="pct_"), write_output=False,
                                  collect_data=False, detector_config=trackml / "detectors.csv.gz", **kw)
        times = []
        for _ in range(iters):
            t0 = time.perf_counter()
            b.process()
            times.append(time.perf_counter() - t0)
        print(json.dumps({"event": "bundled", **kw, "reference_process_s_median": float(np.median(times)),
                          "reference_process_s_min": float(min(times)), "iters": iters}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=120000)
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--bundled", action="store_true", help="also the bundled event of the golden file")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ref", type=pathlib.Path, default=None, help="time the reference on the CPU instead")
    args = ap.parse_args()
    time_reference(args.ref, args.iters) if args.ref else time_device(args)


if __name__ == "__main__":
    main()
