"""The k-scan on a collated batch on the CPU wave64 emulator (the real kernel sources of csrc/kscan.hip): every case of
tests/kscan_batch_cases.py against the single-event restatement applied per event, and the host-side argument checks
of the two batched C entries."""

import contextlib
import ctypes

import pytest
import torch

import kscan_batch_cases as C
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@contextlib.contextmanager
def emulated_cpu():
    """the emulator takes host pointers: the scanner must not move its inputs to a GPU that happens to be there"""
    old = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with emulated():
            yield
    finally:
        torch.cuda.is_available = old


def test_random_tables_per_event():
    with emulated_cpu():
        C.case_random_tables(DEVICE)


def test_cross_event_entries_are_bad_and_join_nothing():
    with emulated_cpu():
        C.case_cross_event_entries(DEVICE)


def test_many_small_events():
    with emulated_cpu():
        C.case_many_small_events(DEVICE)


def test_scanner_on_a_collated_batch():
    with emulated_cpu():
        C.case_scanner_batch(DEVICE)


def test_scanner_one_event_is_todays_call():
    with emulated_cpu():
        C.case_scanner_one_event(DEVICE)


def test_scanner_max_edges_stops_one_event(caplog):
    with emulated_cpu():
        C.case_scanner_max_edges(DEVICE, caplog)


def test_scanner_skips_a_one_hit_event():
    with emulated_cpu():
        C.case_scanner_small_event(DEVICE)


def test_scanner_refuses_a_true_edge_across_events():
    with emulated_cpu():
        C.case_scanner_refuses_cross_event_true_edge(DEVICE)


def test_batched_entries_validate_on_the_host():
    lib = emulator_lib()
    err = lambda: lib.gnntrk_last_error()   # noqa: E731
    buf = (ctypes.c_int64 * 256)()
    i32 = (ctypes.c_int32 * 64)()
    u8 = (ctypes.c_uint8 * 64)()
    ks = (ctypes.c_int32 * 3)(1, 2, 3)
    seg = (ctypes.c_int64 * 3)(0, 1, 4)
    need = lib.gnntrk_kscan_counts_batched_workspace_bytes(4, 2, 3)
    ws = (ctypes.c_uint8 * need)()
    # the counter rows live in the workspace: it grows with n_seg * n_ks
    assert lib.gnntrk_kscan_counts_batched_workspace_bytes(4, 4096, 64) >= need + 4095 * 64 * 3 * 8
    assert lib.gnntrk_kscan_counts_batched_workspace_bytes(4, 1, 64) == lib.gnntrk_kscan_counts_workspace_bytes(4)
    pid = (ctypes.c_int64 * 4)()
    lab = (ctypes.c_int64 * 12)()

    def call(**kw):
        a = dict(dict(nbr=i32, cnt=i32, n=4, k_stride=3, ks=ks, n_ks=3, pid=pid, mask=u8, te=None, n_te=0, seg=seg,
                      n_seg=2, out=buf, labels=lab, ws=ws, ws_bytes=need), **kw)
        return lib.gnntrk_kscan_counts_batched(a["nbr"], a["cnt"], a["n"], a["k_stride"], a["ks"], a["n_ks"], a["pid"],
                                               a["mask"], a["te"], a["n_te"], a["seg"], a["n_seg"], a["out"],
                                               a["labels"], a["ws"], a["ws_bytes"], None)

    assert call() == 0, err()
    assert call(seg=None) == 1 and b"seg_ptr" in err()
    assert call(n_seg=0) == 1 and b"n_seg" in err() and call(n_seg=-1) == 1
    assert call(ws_bytes=need - 1) == 1 and b"workspace" in err() and b"kscan_counts_batched" in err()
    assert call(ws=None) == 1 and b"workspace" in err()
    assert call(n_seg=65537) == 4 and b"65536" in err()
    # everything gnntrk_kscan_counts refuses
    assert call(n=-1) == 1
    assert call(n_ks=0) == 1 and call(n_ks=65) == 1
    assert call(ks=None) == 1 and b"NULL" in err()
    assert call(ks=(ctypes.c_int32 * 3)(1, 0, 3)) == 1 and b"k = 0" in err()
    assert call(k_stride=2) == 1 and b"k = 3" in err()
    assert call(nbr=None) == 1 and call(mask=None) == 1 and call(labels=None) == 1 and b"NULL" in err()
    assert call(out=None) == 1
    assert call(n_te=2) == 1 and call(n_te=-1) == 1
    assert call(n=1 << 30) == 4
    # no hits: the tables of all events are cleared, nothing is launched
    for i in range(2 * 3 * 9):
        buf[i] = -1
    assert call(n=0, seg=(ctypes.c_int64 * 3)(0, 0, 0), ws=None, ws_bytes=0) == 0
    assert not any(buf[i] for i in range(2 * 3 * 9))
