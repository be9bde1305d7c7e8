"""The geometric graph builder on the CPU wave64 emulator (the real kernel sources of csrc/graph_builder.hip): every case
of tests/graph_builder_cases.py, and the host-side argument checks of the new C entries."""

import contextlib
import ctypes

import pytest
import torch

import graph_builder_cases as C
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
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)   # noqa: E731
    f32 = lambda *v: (ctypes.c_float * len(v))(*v)   # noqa: E731
    n, n_pairs = 5, 2
    # hits 0, 1 on layer 7, hits 2, 3 on layer 8, hit 4 on layer 9 (event 1); columns r, phi, z
    x = f32(32, 0, 0, 32, 0.1, 5, 72, 0, 0, 72, 0.1, 11, 116, 0, 0)
    layer, pid, pt = i64(7, 7, 8, 8, 9), i64(1, 2, 1, 2, 1), f32(1, 1, 1, 1, 1)
    seg, one = i64(0, 4, 5), i64(0, 5)
    pairs, radius = (ctypes.c_int32 * 4)(7, 8, 8, 9), (ctypes.c_double * 2)(0, 0)
    cuts = (ctypes.c_double * 4)(0.005, 200, 1.7, 1)
    head = i64(-1, -1)

    # ---- gnntrk_graph_builder_count
    need = lib.gnntrk_graph_builder_count_workspace_bytes(n, 2, pairs, n_pairs)
    assert need > 0 and lib.gnntrk_graph_builder_count_workspace_bytes(0, 1, pairs, n_pairs) == 0
    assert lib.gnntrk_graph_builder_count_workspace_bytes(n, 2, pairs, 0) == 0
    assert lib.gnntrk_graph_builder_count_workspace_bytes(1000, 2, pairs, n_pairs) > need
    ws = (ctypes.c_uint8 * need)()

    def count(**kw):
        a = dict(dict(x=x, stride=3, layer=layer, n=n, seg=seg, n_seg=2, pairs=pairs, radius=radius, n_pairs=n_pairs,
                      cuts=cuts, head=head, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_graph_builder_count(a["x"], a["stride"], a["layer"], a["n"], a["seg"], a["n_seg"], a["pairs"],
                                              a["radius"], a["n_pairs"], a["cuts"], a["head"], a["ws"], a["ws_bytes"], None)

    assert count() == 0, err()
    assert list(head) == [4, 0]                      # the four (7, 8) pairs of event 0; (8, 9) crosses the events
    assert count(seg=None) == 1 and b"seg_ptr" in err() and count(n_seg=0) == 1
    assert count(n_seg=65537) == 4 and b"65536" in err()
    assert count(n=-1) == 1 and count(n=1 << 30) == 4
    for name in ("x", "layer", "pairs", "radius", "cuts", "head"):
        assert count(**{name: None}) == 1 and b"NULL" in err() and b"graph_builder_count" in err(), name
    assert count(stride=2) == 1 and count(n_pairs=-1) == 1
    assert count(n_pairs=129) == 4 and b"128" in err()
    assert count(pairs=(ctypes.c_int32 * 4)(7, 64, 8, 9)) == 1 and b"[0, 64)" in err()
    assert count(pairs=(ctypes.c_int32 * 4)(-1, 8, 8, 9)) == 1
    assert count(radius=(ctypes.c_double * 2)(-1, 0)) == 1
    assert count(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"graph_builder_count" in err()
    assert count(ws=None) == 1 and b"workspace" in err()
    head[0] = head[1] = -1
    assert count(n=0, x=None, layer=None, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and list(head) == [0, 0]
    head[0] = -1
    assert count(n_pairs=0, pairs=None, radius=None, ws=None, ws_bytes=0) == 0 and list(head) == [0, 0]
    assert count(layer=i64(7, 7, 8, 64, -1)) == 0 and list(head) == [2, 2]       # two hits on no layer
    one_need = lib.gnntrk_graph_builder_count_workspace_bytes(n, 1, pairs, n_pairs)
    assert count(seg=one, n_seg=1, ws_bytes=one_need) == 0 and list(head) == [6, 0]
    assert count() == 0 and list(head) == [4, 0]

    # ---- gnntrk_graph_builder_fill
    m = 4
    ei, ea, y, ept, eptr = (ctypes.c_int64 * (2 * m))(), (ctypes.c_float * (4 * m))(), f32(*[9] * m), f32(*[9] * m), i64(9, 9, 9)

    def fill(**kw):
        a = dict(dict(x=x, stride=3, layer=layer, pid=pid, pt=pt, n=n, seg=seg, n_seg=2, pairs=pairs, radius=radius,
                      n_pairs=n_pairs, cuts=cuts, m=m, ei=ei, ea=ea, y=y, ept=ept, eptr=eptr, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_graph_builder_fill(a["x"], a["stride"], a["layer"], a["pid"], a["pt"], a["n"], a["seg"], a["n_seg"],
                                             a["pairs"], a["radius"], a["n_pairs"], a["cuts"], a["m"], a["ei"], a["ea"],
                                             a["y"], a["ept"], a["eptr"], a["ws"], a["ws_bytes"], None)

    assert fill() == 0, err()
    assert list(ei) == [0, 0, 1, 1, 2, 3, 2, 3] and list(y) == [1, 0, 0, 1] and list(eptr) == [0, 4, 4]
    assert list(ept) == [1, 1, 1, 1] and abs(ea[0] - 0.04) < 1e-8 and abs(ea[3 * m + 1] - (0.1 ** 2 + 0.152 ** 2) ** 0.5) < 1e-2
    assert fill(seg=None) == 1 and b"seg_ptr" in err() and fill(n_seg=65537) == 4
    assert fill(n=-1) == 1 and fill(n=1 << 30) == 4 and fill(m=-1) == 1 and fill(m=1 << 30) == 4
    for name in ("x", "layer", "pid", "pt", "pairs", "radius", "cuts", "ei", "ea", "y", "ept", "eptr"):
        assert fill(**{name: None}) == 1 and b"NULL" in err() and b"graph_builder_fill" in err(), name
    assert fill(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"graph_builder_fill" in err()
    assert fill(ws=None) == 1
    assert fill(n=0, m=0, x=None, layer=None, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and list(eptr) == [0, 0, 0]
    assert fill(n=0, m=1, ws=None, ws_bytes=0) == 1 and b"without" in err()
    # a smaller edge count than the rows hold: the slots beyond it are not written
    for i in range(2 * m):
        ei[i] = -7
    assert fill(m=3) == 0 and list(ei)[:6] == [0, 0, 1, 2, 3, 2] and list(ei)[6:] == [-7, -7]
    assert count() == 0 and fill() == 0 and list(ei) == [0, 0, 1, 1, 2, 3, 2, 3]

    # ---- gnntrk_graph_builder_truth
    need_t = lib.gnntrk_graph_builder_truth_workspace_bytes(n)
    assert need_t > 0 and lib.gnntrk_graph_builder_truth_workspace_bytes(1000) > need_t
    assert lib.gnntrk_graph_builder_truth_workspace_bytes(-1) == lib.gnntrk_graph_builder_truth_workspace_bytes(0)
    ws_t = (ctypes.c_uint8 * need_t)()
    counts = (ctypes.c_int64 * 28)()

    def truth(**kw):
        a = dict(dict(ei=ei, m=m, y=y, ept=ept, layer=layer, pid=pid, pt=pt, n=n, seg=seg, n_seg=2, relabel=1,
                      counts=counts, ws=ws_t, ws_bytes=need_t), **kw)
        return lib.gnntrk_graph_builder_truth(a["ei"], a["m"], a["y"], a["ept"], a["layer"], a["pid"], a["pt"], a["n"],
                                              a["seg"], a["n_seg"], a["relabel"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert truth() == 0, err()
    # event 0: 4 edges, 2 true (pt 1 > 0, 0.1, 0.5, 0.9, not > 1), none relabelled, particles 1 and 2 with one hit on 7
    # and one on 8 each; event 1: the lone hit of particle 1
    assert list(counts)[:14] == [4, 2, 2, 2, 2, 2, 0, 0, 2, 2, 2, 2, 0, 0] and not any(list(counts)[14:])
    assert truth(seg=one, n_seg=1) == 0 and list(counts)[8:13] == [3, 3, 3, 3, 0]      # 1 x 1 + 1 x 1 | 1 x 1
    assert truth(m=0, ei=None, y=None, ept=None) == 0 and list(counts)[:9] == [0] * 8 + [2]
    assert truth(layer=i64(7, 7, 8, 8, 70)) == 0 and counts[14 + 13] == 1
    assert truth(seg=None) == 1 and b"seg_ptr" in err() and truth(n_seg=0) == 1 and truth(n_seg=65537) == 4
    assert truth(n=-1) == 1 and truth(n=1 << 30) == 4 and truth(m=-1) == 1 and truth(m=1 << 30) == 4
    for name in ("ei", "y", "ept", "layer", "pid", "pt", "counts"):
        assert truth(**{name: None}) == 1 and b"NULL" in err() and b"graph_builder_truth" in err(), name
    assert truth(ws_bytes=need_t - 1) == 1 and b"workspace" in err() and b"graph_builder_truth" in err()
    assert truth(ws=None) == 1
    assert truth(n=0, m=0, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and not any(counts)
    assert truth(n=0, ws=None, ws_bytes=0) == 1 and b"without hits" in err()
    # an edge with an end outside [0, n) or a label of an id <= 0 is no transition and faults nothing
    assert truth(ei=(ctypes.c_int64 * 8)(0, 99, -1, 1, 2, 3, 2, 3)) == 0
    assert truth() == 0 and list(counts)[:2] == [4, 2]
