"""The point cloud builder on the CPU wave64 emulator (the real kernel sources of csrc/point_cloud.hip): every case of
tests/point_cloud_cases.py, and the host-side argument checks of the new C entries."""

import contextlib
import ctypes

import pytest
import torch

import point_cloud_cases as C
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
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)   # noqa: E731
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)   # noqa: E731
    # two hits on (8, 2) and (8, 4) of particle 5, one noise hit on (8, 2); one cell each
    H = 3
    a = dict(hit_id=i64(10, 11, 12), xyz=f64(50, 0, 0, 0, 80, 0, -50, 0, 0), vlm=i32(8, 2, 0, 8, 4, 0, 8, 2, 0), H=H,
             cell_hit=i64(10, 11, 12), cell_ch=i32(1, 1, 2, 2, 3, 3), cell_val=f64(0.5, 0.25, 1.0), Cn=3,
             part_id=i64(5), part_p=f64(1, 0, 0), P=1, truth_hit=i64(12, 11, 10), truth_pid=i64(0, 5, 5), T=3,
             layer_map=i32(*[(7 if j == 8 * 64 + 2 else 8 if j == 8 * 64 + 4 else -1) for j in range(64 * 64)]),
             det_index=i32(-1, 0), det_dims=i32(9, 5, 1), det_rows=f64(1, 0, 0, 0, 1, 0, 0, 0, 1, 0.15, 0.05, 0.05), M=1,
             codes=i32(3, 9), scale=f64(1000, 1), F=2, remove_noise=0, x=(ctypes.c_float * (2 * H))(),
             cols=(ctypes.c_int64 * (6 * H))(), pt_eta=(ctypes.c_float * (2 * H))(), uv=(ctypes.c_double * (2 * H))(),
             slot=(ctypes.c_int32 * H)(), head=(ctypes.c_int64 * 12)())
    a["det_index"] = i32(*[(0 if j in (8 * 5 + 2, 8 * 5 + 4) else -1) for j in range(9 * 5)])
    need = lib.gnntrk_point_cloud_select_workspace_bytes(3, 3, 1)
    assert need > 0 and lib.gnntrk_point_cloud_select_workspace_bytes(0, 3, 1) == 0
    assert lib.gnntrk_point_cloud_select_workspace_bytes(300, 3, 1) > need
    a.update(ws=(ctypes.c_uint8 * need)(), ws_bytes=need)
    order = ("hit_id", "xyz", "vlm", "H", "cell_hit", "cell_ch", "cell_val", "Cn", "part_id", "part_p", "P", "truth_hit",
             "truth_pid", "T", "layer_map", "det_index", "det_dims", "det_rows", "M", "codes", "scale", "F", "remove_noise",
             "x", "cols", "pt_eta", "uv", "slot", "head", "ws", "ws_bytes")

    def select(**kw):
        b = dict(a, **kw)
        return lib.gnntrk_point_cloud_select(*[b[k] for k in order], None)

    assert select() == 0, err()
    assert list(a["head"])[:9] == [3, 0, 0, 0, 0, 0, 0, 2, 1]
    assert list(a["cols"])[:3] == [7, 8, 7] and list(a["cols"])[3:6] == [5, 5, 0] and list(a["slot"]) == [0, 0, 1]
    assert list(a["cols"])[9:12] == [2, 2, 1] and list(a["cols"])[12:15] == [2, 2, 1] and list(a["cols"])[15:18] == [0, 1, 2]
    assert [round(v, 6) for v in a["x"]] == [0.05, 1, 0.08, 1, 0.05, 1] and a["pt_eta"][0] == 1 and a["pt_eta"][2] == 0
    assert select(remove_noise=1) == 0 and list(a["head"])[:9] == [2, 0, 0, 0, 0, 0, 0, 1, 0]
    assert select(hit_id=i64(10, 10, 12)) == 0 and a["head"][1] == 1
    assert select(vlm=i32(8, 2, 0, 8, 64, 0, -1, 2, 0)) == 0 and a["head"][4] == 2
    assert select(truth_hit=i64(12, 12, 10)) == 0 and a["head"][5] == 1
    assert select(cell_hit=i64(10, 11, 11)) == 0 and a["head"][2] == 1
    assert select(vlm=i32(8, 2, 0, 8, 4, 3, 8, 2, 0)) == 0 and a["head"][3] == 1
    for name in ("hit_id", "xyz", "vlm", "cell_hit", "cell_ch", "cell_val", "part_id", "part_p", "truth_hit", "truth_pid",
                 "layer_map", "det_index", "det_dims", "det_rows", "codes", "scale", "x", "cols", "pt_eta", "uv", "slot", "head"):
        assert select(**{name: None}) == 1 and b"NULL" in err() and b"point_cloud_select" in err(), name
    for name in ("H", "Cn", "P", "T"):
        assert select(**{name: -1}) == 1 and select(**{name: 1 << 30}) == 4, name
    assert select(M=-1) == 1 and select(F=0) == 1 and select(F=33) == 4 and b"GNNTRK_PC_MAX_FEATURES" in err()
    assert select(codes=i32(3, 27)) == 1 and select(codes=i32(-1, 3)) == 1 and select(scale=f64(1, float("nan"))) == 1
    assert select(ws_bytes=need - 1) == 1 and b"workspace" in err() and select(ws=None) == 1
    assert select(H=0, hit_id=None, xyz=None, vlm=None, ws=None, ws_bytes=0) == 0 and not any(a["head"])
    assert select() == 0 and list(a["head"])[:9] == [3, 0, 0, 0, 0, 0, 0, 2, 1]

    # ---- gnntrk_point_cloud_sectors / _gather: two sectors; hits 0 (phi 0) and 1 (phi 90 degrees), noise at phi 180
    S = 2
    s_need = lib.gnntrk_point_cloud_sectors_workspace_bytes(H, 1, S)
    assert s_need > 0 and lib.gnntrk_point_cloud_sectors_workspace_bytes(0, 1, S) == 0
    assert lib.gnntrk_point_cloud_sectors_workspace_bytes(H, 1, 0) == 0
    b = dict(uv=a["uv"], slot=a["slot"], n_kept=a["head"], cap=H, part_p=a["part_p"], P=1, S=S, cs=f64(1, 0, -1, 1.2e-16),
             slope=1.0038848218538872, ds=1.1, di=1e-4, thld=0.5, counts=(ctypes.c_int64 * (6 * S))(), head=i64(-1, -1),
             ws=(ctypes.c_uint8 * s_need)(), ws_bytes=s_need)
    s_order = ("uv", "slot", "n_kept", "cap", "part_p", "P", "S", "cs", "slope", "ds", "di", "thld", "counts", "head", "ws", "ws_bytes")

    def sectors(**kw):
        c = dict(b, **kw)
        return lib.gnntrk_point_cloud_sectors(*[c[k] for k in s_order], None)

    assert sectors() == 0, err()
    # sector 0: hit 0; sector 1: the noise hit.  Particle 5 (pt 1 > thld) has one hit in each test of sector 0
    assert list(b["head"]) == [2, 0] and list(b["counts"]) == [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0]
    for name in ("uv", "slot", "n_kept", "part_p", "cs", "counts", "head"):
        assert sectors(**{name: None}) == 1 and b"NULL" in err() and b"point_cloud_sectors" in err(), name
    assert sectors(S=0) == 1 and sectors(cap=-1) == 1 and sectors(P=-1) == 1
    assert sectors(cap=1 << 30) == 4 and sectors(cap=1 << 20, S=1 << 10) == 4 and b"2^30" in err()
    assert sectors(ws_bytes=s_need - 1) == 1 and b"workspace" in err() and sectors(ws=None) == 1
    assert sectors(cap=0, uv=None, slot=None, ws=None, ws_bytes=0) == 0 and list(b["head"]) == [0, 0]
    assert sectors() == 0 and list(b["head"]) == [2, 0]
    g = dict(x=a["x"], cols=a["cols"], pt_eta=a["pt_eta"], slot=a["slot"], cap=H, F=2, P=1, S=S, n_rows=2,
             x_out=(ctypes.c_float * 4)(), cols_out=(ctypes.c_int64 * 12)(), pte_out=(ctypes.c_float * 4)(), ws=b["ws"],
             ws_bytes=s_need)

    def gather(**kw):
        c = dict(g, **kw)
        return lib.gnntrk_point_cloud_gather(*[c[k] for k in g], None)

    assert gather() == 0, err()
    assert list(g["cols_out"]) == [7, 7, 5, 0, 0, 0, 2, 1, 2, 1, 0, -1] and [round(v, 6) for v in g["x_out"]] == [0.05, 1, 0.05, 1]
    for name in ("x", "cols", "pt_eta", "slot", "x_out", "cols_out", "pte_out"):
        assert gather(**{name: None}) == 1 and b"NULL" in err() and b"point_cloud_gather" in err(), name
    assert gather(n_rows=-1) == 1 and gather(n_rows=7) == 1 and gather(F=0) == 1 and gather(F=33) == 4 and gather(S=0) == 1
    assert gather(ws_bytes=s_need - 1) == 1 and b"workspace" in err() and gather(ws=None) == 1
    assert gather(n_rows=0, x_out=None, cols_out=None, pte_out=None) == 0

    # ---- gnntrk_truth_edges_count / _fill
    n = 6
    pid, seg, one = i64(4, 0, 4, 4, 9, 9), i64(0, 3, 6), i64(0, 6)
    t_need = lib.gnntrk_truth_edges_workspace_bytes(n)
    assert t_need > 0 and lib.gnntrk_truth_edges_workspace_bytes(0) == 0 and lib.gnntrk_truth_edges_workspace_bytes(600) > t_need
    t = dict(pid=pid, n=n, seg=seg, n_seg=2, counts=i64(-1, -1), ws=(ctypes.c_uint8 * t_need)(), ws_bytes=t_need)

    def count(**kw):
        c = dict(t, **kw)
        return lib.gnntrk_truth_edges_count(*[c[k] for k in t], None)

    assert count() == 0 and list(t["counts"]) == [1, 1], err()
    assert count(seg=one, n_seg=1) == 0 and t["counts"][0] == 4
    assert count(pid=None) == 1 and b"NULL" in err() and count(counts=None) == 1 and count(seg=None) == 1 and b"seg_ptr" in err()
    assert count(n=-1) == 1 and count(n=1 << 30) == 4 and count(n_seg=0) == 1 and count(n_seg=65537) == 4
    assert count(ws_bytes=t_need - 1) == 1 and b"workspace" in err() and count(ws=None) == 1
    assert count(n=0, pid=None, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and list(t["counts"]) == [0, 0]
    f = dict(pid=pid, n=n, seg=seg, n_seg=2, m=2, global_ids=0, ei=i64(*[-7] * 4), eptr=i64(-1, -1, -1), ws=t["ws"], ws_bytes=t_need)

    def fill(**kw):
        c = dict(f, **kw)
        return lib.gnntrk_truth_edges_fill(*[c[k] for k in f], None)

    assert fill() == 0 and list(f["ei"]) == [0, 2, 1, 2] and list(f["eptr"]) == [0, 1, 2], err()
    assert fill(global_ids=1) == 0 and list(f["ei"]) == [0, 4, 2, 5]
    big = i64(*[-7] * 8)
    assert fill(seg=one, n_seg=1, m=4, ei=big, global_ids=1) == 0 and list(big) == [0, 0, 2, 4, 2, 3, 3, 5]
    assert fill(pid=None) == 1 and fill(ei=None) == 1 and fill(eptr=None) == 1 and b"NULL" in err() and fill(seg=None) == 1
    assert fill(n=-1) == 1 and fill(n=1 << 30) == 4 and fill(m=-1) == 1 and fill(m=1 << 30) == 4 and fill(n_seg=65537) == 4
    assert fill(ws_bytes=t_need - 1) == 1 and b"workspace" in err() and fill(ws=None) == 1
    assert fill(n=0, m=1, ws=None, ws_bytes=0) == 1 and b"without hits" in err()
    assert fill(n=0, m=0, pid=None, ei=None, ws=None, ws_bytes=0, seg=i64(0, 0, 0)) == 0 and list(f["eptr"]) == [0, 0, 0]
    # a smaller edge count than the hits hold: nothing beyond it is written
    small = i64(*[-7] * 8)
    assert fill(seg=one, n_seg=1, m=3, ei=small, global_ids=1) == 0 and list(small)[6:] == [-7, -7]
