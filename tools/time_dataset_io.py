#!/usr/bin/env python3
"""Times the device-to-disk path of the dataset writer for a collated batch (needs the GPU).

Two paths over the same batch, alternating window by window:

* ``packed``   - ``io.pack_events`` (one ``gnntrk_pack_segments`` launch), ONE copy of the image into a pinned buffer,
                 then per event ``torch.save`` of the views of the host image;
* ``composed`` - what there is without the kernel: ``uncollate``'s slices, one ``.cpu()`` per field and event, then the
                 same ``torch.save`` per event.

Per shape: the wall time until the data is on the host (``host_ms``: ends in a device synchronise) and until the files
are written (``total_ms``), each the median over ``--windows`` windows of ``--iters`` iterations with [min, max]; and
the device time of the pack launch alone (HIP events) against its byte floor.  Files go to ``--dir`` (default: a
directory under /dev/shm where there is one, else the system's temporary directory).  Shapes: 1 and 32 events of about
6 000 hits and 35 000 edges, and one full-size event (``--full-hits``, ``--full-edges``).  One JSON line per shape and a
markdown table.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import shutil
import sys
import tempfile
import time

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
HBM_BYTES_PER_S = 6.3e12          # MI355X, achievable (a float4 copy)


def make_event(seed: int, n: int, e: int, device):
    """the fields of ``GraphBuilder.build`` with random contents"""
    import torch

    import gnn_tracking_amd as G

    g = torch.Generator(device="cpu").manual_seed(seed)
    i64 = lambda hi, *s: torch.randint(0, hi, s, generator=g)   # noqa: E731
    f32 = lambda *s: torch.rand(*s, generator=g)                  # noqa: E731
    d = G.Data(x=f32(n, 14), edge_index=i64(n, 2, e), edge_attr=f32(e, 4), pt=f32(n), particle_id=i64(1 << 40, n),
               y=f32(e).round(), reconstructable=i64(2, n), sector=i64(8, n), evtid=torch.tensor([seed]),
               s=torch.tensor([0]), eta=f32(n), layer=i64(18, n))
    return d.to(device)


def measure(batch, n_events: int, out: pathlib.Path, windows: int, iters: int, warmup: int) -> dict:
    import torch

    import gnn_tracking_amd as G
    from gnn_tracking_amd import io as gio

    names = [out / f"e{i}.pt" for i in range(n_events)]
    pinned = {}

    def packed():
        t0 = time.perf_counter()
        p = gio.pack_events(batch)
        total = p.event_ptr[-1]
        if "buf" not in pinned or pinned["buf"].numel() < total:
            pinned["buf"] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = pinned["buf"][:total]
        host.copy_(p.image[:total], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for d, path in zip(p.event_dicts(host), names):
            gio._write(d, path)
        return t1 - t0, time.perf_counter() - t0

    def composed():
        t0 = time.perf_counter()
        dicts = [gio._event_dict(d) for d in (G.uncollate(batch) if n_events > 1 else [batch])]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for d, path in zip(dicts, names):
            gio._write(d, path)
        return t1 - t0, time.perf_counter() - t0

    paths = {"packed": packed, "composed": composed}
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    # the two paths write the same files
    composed()
    want = [G.load_graph(p) for p in names]
    packed()
    for a, b in zip([G.load_graph(p) for p in names], want):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a.keys())
    file_bytes = sum(p.stat().st_size for p in names)
    rec = {k: {"host": [], "total": []} for k in paths}
    for w in range(windows):
        for k in (("packed", "composed") if w % 2 == 0 else ("composed", "packed")):
            h = t = 0.0
            for _ in range(iters):
                a, b = paths[k]()
                h, t = h + a, t + b
            rec[k]["host"].append(1e3 * h / iters)
            rec[k]["total"].append(1e3 * t / iters)
    # the pack launch alone (with the upload of its plan), device time
    p = gio.pack_events(batch)
    image_bytes = p.event_ptr[-1]
    torch.cuda.synchronize()
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        gio.pack_events(batch, image=p.image)
    e1.record()
    torch.cuda.synchronize()
    pack_ms = e0.elapsed_time(e1) / reps
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731
    res = {"events": n_events, "image_bytes": int(image_bytes), "file_bytes": int(file_bytes),
           "pack_launch_ms": pack_ms, "pack_floor_ms": 1e3 * 2 * image_bytes / HBM_BYTES_PER_S,
           "windows": windows, "iters": iters}
    for k in paths:
        res[k] = {"host_ms": stat(rec[k]["host"]), "total_ms": stat(rec[k]["total"])}
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hits", type=int, default=6000)
    ap.add_argument("--edges", type=int, default=35000)
    ap.add_argument("--full-hits", type=int, default=120000)
    ap.add_argument("--full-edges", type=int, default=2000000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", type=pathlib.Path, default=None)
    args = ap.parse_args()
    import torch

    import gnn_tracking_amd as G

    if not torch.cuda.is_available():
        raise SystemExit("time_dataset_io: needs the GPU (a CPU run gives no time)")
    base = args.dir or pathlib.Path("/dev/shm" if pathlib.Path("/dev/shm").is_dir() else tempfile.gettempdir())
    out = pathlib.Path(tempfile.mkdtemp(prefix="gnntrk_io_", dir=base))
    rows = []
    try:
        for label, b, n, e in (("1 event", 1, args.hits, args.edges), ("32 events", 32, args.hits, args.edges),
                               ("1 full-size event", 1, args.full_hits, args.full_edges)):
            events = [make_event(i, n + 37 * i, e + 101 * i, "cuda") for i in range(b)]
            batch = G.collate(events) if b > 1 else events[0]
            if b == 1:                      # (one event goes through the packer as a batch of one)
                batch.ptr = torch.tensor([0, batch.num_nodes], device="cuda")
            r = measure(batch, b, out, args.windows, args.iters, args.warmup)
            r.update(shape=label, hits=n, edges=e)
            print(json.dumps(r), flush=True)
            rows.append(r)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    f = lambda s: f"{s['median']:.2f} [{s['min']:.2f}, {s['max']:.2f}]"   # noqa: E731
    print("| shape | image MB | packed: host ms | composed: host ms | packed: total ms | composed: total ms | pack launch ms (floor) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['shape']} | {r['image_bytes'] / 1e6:.1f} | {f(r['packed']['host_ms'])} | {f(r['composed']['host_ms'])} | "
              f"{f(r['packed']['total_ms'])} | {f(r['composed']['total_ms'])} | {r['pack_launch_ms']:.3f} ({r['pack_floor_ms']:.3f}) |")


if __name__ == "__main__":
    main()
