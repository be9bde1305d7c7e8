"""Cases of the graph-index build around its chunk geometry, the renumbered (``node_rank``) path, the slow paths and
the table scan, shared by the emulator file and the GPU file.  Every case compares ``perm``, ``tgt``, ``src``,
``rowptr_t``, ``spos``, ``spos_inv`` and ``rowptr_s`` with torch's stable argsort of the translated ids
(``parity_cases._check_graph_index``), the carried labels with ``y[perm]`` and the carried rows with
``bf16(edge_attr)[perm]`` as bit patterns."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import parity_cases as P
from gnn_tracking_amd import ops

CHUNK = 16384       # edges per chunk of the edge list up to 512 chunks (own_plan)
SCAN_TILE = 4096    # table entries per tile of the scan (kScanTile)


def _unaligned(t: torch.Tensor, skip: int) -> torch.Tensor:
    """A contiguous copy of ``t`` that starts ``skip`` elements into a larger buffer."""
    buf = torch.empty(t.numel() + skip, dtype=t.dtype, device=t.device)
    out = buf[skip:].view(t.shape)
    out.copy_(t)
    return out


def events(g, sizes, device, feat=3):
    """A collated batch: ``sizes`` = ((nodes, edges), ...); ids of an event in its own range, its edges contiguous."""
    offs, parts, batch = 0, [], []
    for i, (n, e) in enumerate(sizes):
        parts.append(g.integers(0, max(n, 1), size=(2, e)) + offs)
        batch.append(torch.full((n,), i, dtype=torch.long))
        offs += n
    ei = torch.from_numpy(np.concatenate(parts, axis=1)).long().to(device)
    x = torch.from_numpy(g.standard_normal((offs, feat)).astype(np.float32)).to(device)
    return ei, offs, x, torch.cat(batch).to(device)


def carried(g, E, device, stride=4, label_skip=0, special=False):
    y = torch.from_numpy(g.random(E) < 0.3)
    y = _unaligned(y.to(device), label_skip) if label_skip else y.to(device)
    r = g.normal(size=(E, stride)).astype(np.float32) * 3
    if special and E >= 8:
        r[1, 0], r[2, 1], r[3, 2], r[5, 3] = np.nan, np.inf, -np.inf, -0.0
    rows = torch.from_numpy(r).to(device)
    return y, (rows[:, :4] if stride > 4 else rows)


def bf16_bits(rows: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 bit patterns (int16): round to nearest even on the bits; a NaN keeps its sign and its top payload
    bits and gets the quiet bit (the IEEE 754 narrowing; torch's own CPU cast of a NaN is not that - it returns
    0xffff - so it is the reference for every other value only)."""
    r = rows.detach().cpu().contiguous()
    u = r.view(torch.int32).long() & 0xffffffff
    out = torch.where(torch.isnan(r), (u >> 16) | 0x40, (u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)
    ok = ~torch.isnan(r)
    assert torch.equal(out[ok], r.to(torch.bfloat16).view(torch.int16)[ok])
    return out


def build_and_check(ei, N, y, rows, order_by=None, flags=2, tag=""):
    """``flags`` = 2: the own counting sort whatever the density (0: the build's own choice)."""
    E = int(ei.shape[1])
    gi = ops.graph_index(ei, N, cache=False, flags=flags, carry_label=y, carry_rows=rows, order_by=order_by)
    eic = ei.cpu().clamp(0, max(N - 1, 0))   # (ids out of range are clamped; the cases that have none are unchanged)
    if order_by is not None:
        assert gi.node_rank is not None and torch.equal(gi.node_perm.cpu().long()[gi.node_rank.cpu().long()], torch.arange(N))
        eic = gi.node_rank.cpu().long()[eic]
    P._check_graph_index(gi, eic, N, tag)
    if E == 0:
        return gi
    perm = gi.perm.cpu().long()
    lab, rc = ops.carried_label(gi, y), ops.carried_rows(gi, rows)
    assert lab is not None and rc is not None, tag + ": nothing was carried"
    assert torch.equal(lab.cpu(), y.cpu().to(torch.uint8)[perm]), tag + ": label_csr == y[perm]"
    assert torch.equal(rc.cpu().contiguous().view(torch.int16), bf16_bits(rows)[perm]), tag + ": carried rows"
    return gi


# ------------------------------------------------------------------ chunk geometry of the fused remap / count
# (nodes, edges) per event; id rows off the 16-byte grid; labels off the 4-byte grid
GEOMETRY = {
    "two_chunks_second_holds_one_edge": (((700, CHUNK + 1),), 0, 0),
    "tail_of_three_edges": (((700, CHUNK + 3),), 0, 0),
    "one_edge": (((5, 1),), 0, 0),
    "no_edge": (((5, 0),), 0, 0),
    "id_rows_off_the_16_byte_grid": (((900, CHUNK + 6),), 1, 0),
    "labels_off_the_4_byte_grid": (((900, CHUNK + 6),), 0, 1),
    "chunk_straddles_two_events": (((5000, 20000), (4000, 13000)), 0, 0),
}


def case_geometry(device, name):
    sizes, ei_skip, label_skip = GEOMETRY[name]
    g = np.random.default_rng(21)
    ei, N, x, batch = events(g, sizes, device)
    E = int(ei.shape[1])
    if ei_skip:
        ei = _unaligned(ei, ei_skip)
        assert ei.is_contiguous() and ei.data_ptr() % 16 == 8 and E % 2 == 0
    y, rows = carried(g, E, device, label_skip=label_skip)
    if label_skip:
        assert y.data_ptr() % 4 != 0
    build_and_check(ei, N, y, rows, order_by=(x, 1, batch, len(sizes)), tag=name)
    build_and_check(ei, N, y, rows, order_by=None, tag=name + " (caller's numbering)")


# ------------------------------------------------------------------ renumbering
RENUMBER = {
    "one_event_own_order": (((6000, 18001),), 1),
    "two_events_own_order": (((4100, 12000), (2500, 7003)), 2),
    "64_events_own_order": (tuple((90 + i, 270 + 3 * i) for i in range(64)), 64),
    "small_radix_order": (((700, 5000), (300, 2500), (1, 3), (900, 9000)), 0),
    "event_count_not_stated_radix_order": (((5000, 17000),), 0),
}


def case_renumber(device, name):
    sizes, n_ev = RENUMBER[name]
    g = np.random.default_rng(22)
    ei, N, x, batch = events(g, sizes, device)
    x[::7, 1] = 0.25   # ties keep the old order
    y, rows = carried(g, int(ei.shape[1]), device)
    for flags in ((2,) if n_ev == 64 else (0, 2)):   # (64 events: a table of 16 384 buckets - once)
        build_and_check(ei, N, y, rows, order_by=(x, 1, batch, n_ev), flags=flags, tag=f"{name} flags={flags}")


# ------------------------------------------------------------------ slow paths, with node_rank and carried rows
def case_window_slow_path(device):
    """More buckets than a chunk's LDS window holds (4096 x 256 nodes), ids unsorted: cursors in the table itself."""
    g = np.random.default_rng(23)
    N = 1_200_000
    ei = torch.from_numpy(g.integers(0, N, size=(2, 20000))).long().to(device)
    x = torch.from_numpy(g.standard_normal((N, 2)).astype(np.float32)).to(device)
    y, rows = carried(g, 20000, device)
    build_and_check(ei, N, y, rows, order_by=(x, 1, None, 0), tag="window slow path")


HUBS = {"hub_14000_run_walk": 14000, "hub_30000_run_bitmaps_on_the_emulator": 30000}


def case_hub(device, name):
    """Half of the edges into one node: a bucket over the LDS capacity of the bucket sort, a hub over it alone."""
    E = HUBS[name]
    g = np.random.default_rng(24)
    arr = g.integers(0, 600, size=(2, E))
    arr[1, ::2] = 333
    arr[0, 1::3] = 17
    ei = torch.from_numpy(arr).long().to(device)
    x = torch.from_numpy(g.standard_normal((600, 2)).astype(np.float32)).to(device)
    y, rows = carried(g, E, device)
    build_and_check(ei, 600, y, rows, order_by=(x, 1, None, 1), tag=name)


def case_out_of_range(device):
    """One id equal to N and one negative id through the renumbered path: counted (the validating build raises what it
    raised before), clamped to N - 1 and 0."""
    g = np.random.default_rng(25)
    ei, N, x, batch = events(g, ((3000, CHUNK + 5),), device)
    ei[1, 11] = N
    ei[0, CHUNK + 2] = -3
    y, rows = carried(g, int(ei.shape[1]), device)
    build_and_check(ei, N, y, rows, order_by=(x, 1, batch, 1), tag="ids out of range, clamped")
    with pytest.raises(IndexError, match=rf"^edge_index: 2 node ids out of range \[0, {N}\)$"):
        ops.graph_index(ei, N, cache=False, flags=2, validate=True, carry_label=y, carry_rows=rows, order_by=(x, 1, batch, 1))
    ok = ei.clamp(0, N - 1)
    ops.graph_index(ok, N, cache=False, flags=2, validate=True, carry_label=y, carry_rows=rows, order_by=(x, 1, batch, 1))


def case_rows(device):
    """A row stride over 4 floats; NaN, infinities and -0 among the features."""
    g = np.random.default_rng(26)
    ei, N, x, batch = events(g, ((2000, 9001),), device)
    y, rows = carried(g, 9001, device, stride=8, special=True)
    assert rows.stride(0) == 8
    build_and_check(ei, N, y, rows, order_by=(x, 1, batch, 1), tag="row stride 8, special values")
    build_and_check(ei, N, y, rows, order_by=None, tag="row stride 8, special values (caller's numbering)")


# ------------------------------------------------------------------ the scan of the (bucket, chunk) table
# table entries incl. the total = buckets x chunks + 1: one tile short by one, exact, over by one, two tiles and one
SCAN = {
    "2_entries": (200, CHUNK - 5),
    "3_entries": (200, CHUNK + 5),
    "tile_minus_1": (2047 * 256, CHUNK + 5),          # 2047 x 2 + 1
    "tile": (1365 * 256, 2 * CHUNK + 5),              # 1365 x 3 + 1
    "tile_plus_1": (2048 * 256 - 9, CHUNK + 5),       # 2048 x 2 + 1
    "two_tiles_plus_1": (2048 * 256, 3 * CHUNK + 5),  # 2048 x 4 + 1
}


def scan_entries(N, E):
    nc = -(-E // CHUNK)
    chunk = -(-(-(-E // nc)) // 4) * 4
    return -(-N // 256) * -(-E // chunk) + 1


def case_scan(device, name):
    N, E = SCAN[name]
    want = {"2_entries": 2, "3_entries": 3, "tile_minus_1": SCAN_TILE - 1, "tile": SCAN_TILE, "tile_plus_1": SCAN_TILE + 1,
            "two_tiles_plus_1": 2 * SCAN_TILE + 1}[name]
    assert scan_entries(N, E) == want
    g = np.random.default_rng(27)
    ei = torch.from_numpy(g.integers(0, N, size=(2, E))).long().to(device)
    y, rows = carried(g, E, device)
    build_and_check(ei, N, y, rows, order_by=None, tag=name)
