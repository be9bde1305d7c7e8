"""The track-graph statistics on the CPU wave64 emulator (the real kernel sources of csrc/track_graph.hip): every case
of tests/track_graph_cases.py against the networkx restatement, and the host-side argument checks of the new C
entries."""

import contextlib
import ctypes

import pytest
import torch

import track_graph_cases as C
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@contextlib.contextmanager
def emulated_cpu():
    """the emulator takes host pointers: nothing may move its inputs to a GPU that happens to be there"""
    old = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with emulated():
            yield
    finally:
        torch.cuda.is_available = old


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    with emulated_cpu():
        case(DEVICE)


def test_entries_validate_on_the_host():
    lib = emulator_lib()
    err = lambda: lib.gnntrk_last_error()   # noqa: E731
    n, m = 5, 4
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)   # noqa: E731
    seg, mask = i64(0, 1, 5), (ctypes.c_uint8 * n)(1, 1, 1, 1, 1)
    ei = i64(1, 2, 3, 0, 2, 3, 4, 1)           # the path 1-2-3-4 and the cross-event edge 0-1
    table, search, counts = (ctypes.c_int64 * (9 * n))(), (ctypes.c_int32 * n)(), i64(-1, -1)
    rowptr, nbrs, bad = (ctypes.c_int64 * (n + 1))(), (ctypes.c_int32 * (2 * m))(), i64(-1, -1)

    # ---- gnntrk_track_graph_adjacency
    need = lib.gnntrk_track_graph_adjacency_workspace_bytes(n)
    assert need >= 4 * n and lib.gnntrk_track_graph_adjacency_workspace_bytes(-1) == 0
    ws = (ctypes.c_uint8 * need)()

    def adjacency(**kw):
        a = dict(dict(ei=ei, m=m, n=n, seg=seg, n_seg=2, rowptr=rowptr, nbrs=nbrs, bad=bad, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_track_graph_adjacency(a["ei"], a["m"], a["n"], a["seg"], a["n_seg"], a["rowptr"], a["nbrs"],
                                                a["bad"], a["ws"], a["ws_bytes"], None)

    assert adjacency() == 0, err()
    assert list(rowptr) == [0, 0, 1, 3, 5, 6] and list(bad) == [0, 1] and sorted(nbrs[1:3]) == [1, 3]
    assert adjacency(seg=None) == 1 and b"seg_ptr" in err() and adjacency(n_seg=0) == 1
    assert adjacency(n_seg=65537) == 4 and b"65536" in err()
    assert adjacency(n=-1) == 1 and adjacency(n=1 << 30) == 4 and adjacency(m=-1) == 1 and adjacency(m=1 << 30) == 4
    assert adjacency(ei=None) == 1 and adjacency(nbrs=None) == 1 and adjacency(rowptr=None) == 1 and b"NULL" in err()
    assert adjacency(bad=None) == 1
    assert adjacency(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"track_graph_adjacency" in err()
    assert adjacency(ws=None) == 1 and b"workspace" in err()
    assert adjacency(n=0, m=0, ei=None, nbrs=None, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and rowptr[0] == 0
    assert adjacency() == 0

    # ---- gnntrk_track_graph_table (the segments {1, 2} and {4} of particle 2 share a component through the noise hit 3)
    need_t = lib.gnntrk_track_graph_table_workspace_bytes(n)
    assert need_t > 0 and lib.gnntrk_track_graph_table_workspace_bytes(1000) > need_t
    ws_t = (ctypes.c_uint8 * need_t)()
    segs, comps = i64(0, 1, 1, 3, 4), i64(0, 1, 1, 1, 1)
    pid2 = i64(1, 2, 2, 0, 2)

    def table_call(**kw):
        a = dict(dict(segs=segs, comps=comps, pid=pid2, mask=mask, n=n, seg=seg, n_seg=2, table=table, search=search,
                      counts=counts, ws=ws_t, ws_bytes=need_t), **kw)
        return lib.gnntrk_track_graph_table(a["segs"], a["comps"], a["pid"], a["mask"], a["n"], a["seg"], a["n_seg"],
                                            a["table"], a["search"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert table_call() == 0, err()
    assert list(counts) == [2, 1]
    rows = sorted(tuple(table[9 * r:9 * r + 9]) for r in range(2))
    assert rows == [(0, 1, 1, 1, 1, 1, 0, 0, -1), (1, 2, 3, 2, 2, 3, -2, 1, 4)]
    assert tuple(table[9 * search[0]:9 * search[0] + 2]) == (1, 2)
    # the two segments in different components: "no path" (-1) without an entry in the search list
    assert table_call(comps=i64(0, 1, 1, 3, 4)) == 0 and list(counts) == [2, 0]
    assert sorted(tuple(table[9 * r:9 * r + 9]) for r in range(2))[1] == (1, 2, 3, 2, 2, 2, -1, 1, 4)
    assert table_call() == 0 and list(counts) == [2, 1]
    assert table_call(seg=None) == 1 and b"seg_ptr" in err() and table_call(n_seg=-1) == 1
    assert table_call(n_seg=65537) == 4 and table_call(n=-1) == 1 and table_call(n=1 << 30) == 4
    for name in ("segs", "comps", "pid", "mask", "table", "search", "counts"):
        assert table_call(**{name: None}) == 1 and b"NULL" in err(), name
    assert table_call(ws_bytes=need_t - 1) == 1 and b"workspace" in err() and b"track_graph_table" in err()
    assert table_call(ws=None) == 1
    counts[0] = counts[1] = -1
    assert table_call(n=0, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and list(counts) == [0, 0]
    assert table_call() == 0 and list(counts) == [2, 1]

    # ---- gnntrk_track_graph_distance / _ex
    assert lib.gnntrk_track_graph_distance_workspace_bytes(n, 0) == 0
    assert lib.gnntrk_track_graph_distance_workspace_bytes(163840, 0) == 0
    assert lib.gnntrk_track_graph_distance_workspace_bytes(163841, 0) > 0
    need_d = lib.gnntrk_track_graph_distance_workspace_bytes(n, 2)
    assert need_d >= 3 * 4
    ws_d = (ctypes.c_uint8 * need_d)()

    def distance(ex=True, **kw):
        a = dict(dict(table=table, search=search, counts=counts, segs=segs, rowptr=rowptr, nbrs=nbrs, n=n, seg=seg,
                      n_seg=2, lds=2, ws=ws_d, ws_bytes=need_d), **kw)
        head = (a["table"], a["search"], a["counts"], a["segs"], a["rowptr"], a["nbrs"], a["n"], a["seg"], a["n_seg"])
        if ex:
            return lib.gnntrk_track_graph_distance_ex(*head, a["lds"], a["ws"], a["ws_bytes"], None)
        return lib.gnntrk_track_graph_distance(*head, a["ws"], a["ws_bytes"], None)

    assert distance(lds=0) == 1 and b"lds_hits" in err() and distance(lds=163841) == 1
    assert distance(seg=None) == 1 and distance(n_seg=0) == 1 and distance(n_seg=65537) == 4
    assert distance(n=-1) == 1 and distance(n=1 << 30) == 4
    for name in ("table", "search", "counts", "segs", "rowptr"):
        assert distance(**{name: None}) == 1 and b"NULL" in err(), name
    assert distance(ws_bytes=need_d - 1) == 1 and b"workspace" in err() and distance(ws=None) == 1
    assert distance(n=0, ws=None, ws_bytes=0) == 0
    row = 9 * search[0]
    assert table[row + 6] == -2
    assert distance() == 0, err()                # the event of 4 hits against lds_hits = 2: the workspace's bitmaps
    assert table[row + 6] == 2
    table[row + 6] = -2
    assert distance(ex=False, ws=None, ws_bytes=0) == 0, err()      # LDS bitmaps: no workspace needed
    assert table[row + 6] == 2
