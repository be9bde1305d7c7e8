"""The EC threshold scan on the CPU wave64 emulator (the real kernel sources of csrc/ec_scan.hip): every case of
tests/ec_scan_cases.py against the composition of the single-threshold functions and the networkx / numpy restatement, the
reference's own records of tests/golden/g22_ec_scan.npz, and the host-side argument checks of the two C entries with a
hand-checked example."""

import ctypes

import pytest

import ec_scan_cases as C
import ec_scan_golden as GOLD
from emul_util import emulator_lib
from test_track_graph_emul import emulated_cpu

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    with emulated_cpu():
        case(DEVICE)


@pytest.mark.parametrize("name", GOLD.GRAPHS)
def test_reference_records(name):
    with emulated_cpu():
        GOLD.check_device(name, DEVICE)


def test_entries_validate_on_the_host():
    lib = emulator_lib()
    err = lambda: lib.gnntrk_last_error()   # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)   # noqa: E731
    f32 = lambda *v: (ctypes.c_float * len(v))(*v)   # noqa: E731
    u8 = lambda *v: (ctypes.c_uint8 * len(v))(*v)   # noqa: E731
    # event 0: hit 0 of particle 1; event 1: hits 1, 2, 4 of particle 2 and the noise hit 3, outside the mask.
    # Edges: 1-2 (0.9, true), 2-3 and 3-4 (0.5, false), 1-4 (0.2, true) and the cross-event edge 0-1 (0.9, false).
    n, m, n_thr = 5, 5, 3
    seg, pid, mask = i64(0, 1, 5), i64(1, 2, 2, 0, 2), u8(1, 1, 1, 0, 1)
    ei = i64(1, 2, 3, 1, 0, 2, 3, 4, 4, 1)
    w, y, thr = f32(0.9, 0.5, 0.5, 0.2, 0.9), u8(1, 0, 0, 1, 0), f32(0.3, 0.5, 0.7)
    head, particles = i64(-1, -1, -1, -1), (ctypes.c_int64 * (3 * n))()
    bcs, orphans = (ctypes.c_int64 * (2 * 4 * (n_thr + 1)))(), (ctypes.c_int64 * (2 * 3))()
    need = lib.gnntrk_ec_scan_prepare_workspace_bytes(n, m, n_thr)
    assert need > 4 * 3 * n + 6 * m and lib.gnntrk_ec_scan_prepare_workspace_bytes(1000, 5000, 200) > need
    assert lib.gnntrk_ec_scan_prepare_workspace_bytes(-1, -1, 0) == lib.gnntrk_ec_scan_prepare_workspace_bytes(0, 0, 1)
    ws = (ctypes.c_uint8 * need)()

    def prepare(**kw):
        a = dict(dict(ei=ei, m=m, w=w, y=y, y_kind=0, pid=pid, mask=mask, n=n, seg=seg, n_seg=2, thr=thr, n_thr=n_thr,
                      per_event=0, head=head, particles=particles, bcs=bcs, orphans=orphans, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_ec_scan_prepare(a["ei"], a["m"], a["w"], a["y"], a["y_kind"], a["pid"], a["mask"], a["n"],
                                          a["seg"], a["n_seg"], a["thr"], a["n_thr"], a["per_event"], a["head"],
                                          a["particles"], a["bcs"], a["orphans"], a["ws"], a["ws_bytes"], None)

    steps = (ctypes.c_int32 * (n_thr * 2 * 3))()

    def run_steps(**kw):
        a = dict(dict(ei=ei, m=m, pid=pid, n=n, n_thr=n_thr, rows=2, steps=steps, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_ec_scan_steps(a["ei"], a["m"], a["pid"], a["n"], a["n_thr"], a["rows"], a["steps"], a["ws"],
                                        a["ws_bytes"], None)

    # ---- the example
    assert prepare() == 0, err()
    assert list(head) == [2, 0, 0, 1]
    rows = sorted(tuple(particles[3 * r:3 * r + 3]) for r in range(2))
    assert rows == [(0, 1, 1), (1, 2, 3)]
    # [mask class][label][bin k = #{j : !(w < t_j)}]: 0.9 -> 3, 0.5 -> 2 (w == t counts as predicted true), 0.2 -> 0
    assert list(bcs[:16]) == [0, 0, 2, 0,  0, 0, 0, 0,    # an end outside the mask: the two false edges at 0.5
                              0, 0, 0, 1,  1, 0, 0, 1]    # inside: the cross-event edge (false) | 1-4 and 1-2 (true)
    assert list(orphans[:3]) == [0, 0, 0]
    assert run_steps() == 0, err()
    by_row = {tuple(particles[3 * r:3 * r + 2]): r for r in range(2)}

    def step(j, key):
        r = by_row[key]
        return tuple(steps[(j * 2 + r) * 3:(j * 2 + r) * 3 + 3])

    # (segments, largest segment, largest component): t = 0.7 and 0.5 keep 1-2 only (0.5 > 0.5 is false); t = 0.3
    # joins {1, 2} and {4} through the noise hit 3; 1-4 (0.2) and the cross-event edge are in no graph
    assert [step(j, (0, 1)) for j in range(3)] == [(1, 1, 1)] * 3
    assert [step(j, (1, 2)) for j in range(3)] == [(2, 2, 3), (2, 2, 2), (2, 2, 2)]
    # per event: the cross-event edge counts for the event of its first end
    assert prepare(per_event=1) == 0, err()
    assert list(bcs[:16]) == [0] * 11 + [1, 0, 0, 0, 0] and list(bcs[16:]) == [0, 0, 2, 0] + [0] * 8 + [1, 0, 0, 1]
    assert list(orphans) == [0] * 6
    # float32 labels, an edge out of range, a hit without an edge
    yf = f32(1.5, 0.0, 2.0, 1.0, float("nan"))
    assert prepare(y=yf, y_kind=1, ei=i64(1, 2, 3, 1, 4, 2, 3, 4, 4, 5)) == 0, err()
    assert list(head) == [2, 0, 1, 0] and list(orphans[:3]) == [0, 1, 1]
    assert list(bcs[:16]) == [0, 0, 2, 0,  0, 0, 0, 0,  0, 0, 0, 0,  1, 0, 0, 1]   # (int(2.0) != 1, int(1.5) == 1)

    # ---- refusals of gnntrk_ec_scan_prepare
    assert prepare(n=-1) == 1 and b"ec_scan_prepare" in err() and prepare(n=1 << 30) == 4
    assert prepare(m=-1) == 1 and prepare(m=1 << 30) == 4
    assert prepare(n_thr=0) == 1 and b"n_thr" in err() and prepare(n_thr=257) == 4 and b"256" in err()
    assert prepare(seg=None) == 1 and b"seg_ptr" in err() and prepare(n_seg=0) == 1
    assert prepare(n_seg=65537) == 4 and b"65536" in err()
    assert prepare(y_kind=2) == 1 and b"y_kind" in err()
    for name in ("ei", "w", "y", "pid", "mask", "thr", "head", "particles", "bcs", "orphans"):
        assert prepare(**{name: None}) == 1 and b"NULL" in err() and b"ec_scan_prepare" in err(), name
    assert prepare(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"ec_scan_prepare" in err()
    assert prepare(ws=None) == 1 and b"workspace" in err()
    head[0] = -1
    assert prepare(n=0, m=0, ei=None, w=None, y=None, pid=None, mask=None, particles=None, ws=None, ws_bytes=0,
                   seg=i64(0, 0, 0)) == 0, err()
    assert list(head) == [0, 0, 0, 0] and not any(bcs[:16])
    assert prepare(m=0, ei=None, w=None, y=None) == 0, err()
    assert list(head) == [2, 0, 0, 0] and list(orphans[:3]) == [1, 4, 5] and not any(bcs[:16])
    assert run_steps(m=0, ei=None) == 0, err()
    assert [step(j, (1, 2)) for j in range(3)] == [(3, 1, 1)] * 3

    # ---- refusals of gnntrk_ec_scan_steps
    assert prepare() == 0
    assert run_steps(n=-1) == 1 and b"ec_scan_steps" in err() and run_steps(n=1 << 30) == 4
    assert run_steps(m=-1) == 1 and run_steps(m=1 << 30) == 4
    assert run_steps(n_thr=0) == 1 and run_steps(n_thr=257) == 4
    assert run_steps(rows=-1) == 1 and b"n_particles" in err() and run_steps(rows=n + 1) == 1
    for name in ("ei", "pid", "steps"):
        assert run_steps(**{name: None}) == 1 and b"NULL" in err(), name
    assert run_steps(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"ec_scan_steps" in err()
    assert run_steps(ws=None) == 1
    assert run_steps(n=0, m=0, rows=0, ei=None, pid=None, steps=None, ws=None, ws_bytes=0) == 0, err()
    assert run_steps(rows=0, steps=None) == 0, err()
    assert run_steps() == 0 and [step(j, (1, 2)) for j in range(3)] == [(2, 2, 3), (2, 2, 2), (2, 2, 2)]
