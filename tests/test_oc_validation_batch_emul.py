"""Validation of a collated batch on the CPU wave64 emulator (the real kernel sources of csrc/dbscan.hip and
csrc/tracking_metrics.hip): every case of tests/oc_validation_batch_cases.py against the single-event oracles applied
per event, and the host-side argument checks of the batched C entries."""

import contextlib
import ctypes

import pytest
import torch

import neighbor_cases as N
import oc_validation_batch_cases as C
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@contextlib.contextmanager
def emulated_cpu():
    """the emulator takes host pointers: the scanners must not move their inputs to a GPU that happens to be there"""
    old = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with emulated():
            yield
    finally:
        torch.cuda.is_available = old


# ------------------------------------------------------------------------------------------------- radius graph
@pytest.mark.parametrize("flags", N.FLAGS)
@pytest.mark.parametrize("dim", C.RADIUS_WIDTHS)
def test_radius_graph_per_event_every_width(dim, flags):
    with emulated_cpu():
        C.case_radius_events(DEVICE, dim, flags)


def test_radius_graph_per_event_chunk_edges():
    with emulated_cpu():
        C.case_radius_chunk_edges(DEVICE)


def test_radius_graph_per_event_above_the_pruned_threshold():
    with emulated_cpu():
        C.case_radius_big_events(DEVICE)


@pytest.mark.parametrize("flags", N.FLAGS)
def test_colliding_events_share_no_edge(flags):
    with emulated_cpu():
        C.case_colliding_events(DEVICE, flags)


# ------------------------------------------------------------------------------------------------- DBSCAN labels
@pytest.mark.parametrize("flags", N.FLAGS)
def test_dbscan_labels_per_event(flags):
    with emulated_cpu():
        C.case_dbscan_events(DEVICE, flags)


@pytest.mark.parametrize("flags", N.FLAGS)
def test_one_event_takes_todays_path(flags):
    with emulated_cpu():
        C.case_one_event_is_todays_call(DEVICE, flags)


# ----------------------------------------------------------------------------------------------- tracking metrics
def test_tracking_metrics_per_event():
    with emulated_cpu():
        C.case_metrics_events(DEVICE)


def test_label_beyond_its_event_is_refused():
    with emulated_cpu():
        C.case_metrics_bad_label(DEVICE)


def test_majority_tie_inside_the_event():
    with emulated_cpu():
        C.case_metrics_tie(DEVICE)


def test_tracking_metrics_one_event_is_todays_call():
    with emulated_cpu():
        C.case_metrics_one_event(DEVICE)


# ------------------------------------------------------------------------------------------------------- scanners
def test_scanner_on_a_collated_batch():
    with emulated_cpu():
        C.case_scanner_batch(DEVICE)


def test_performance_details_on_a_collated_batch():
    with emulated_cpu():
        C.case_performance_details_batch(DEVICE)


# ------------------------------------------------------------------------------------------ host-side validation
def test_batched_entries_validate_on_the_host():
    lib = emulator_lib()
    n = 16
    x = (ctypes.c_float * (3 * n))()
    cnt = (ctypes.c_int32 * n)()
    off = (ctypes.c_int64 * (n + 1))()
    seg = (ctypes.c_int64 * 3)(0, 6, n)
    assert lib.gnntrk_radius_count_batched_ws(x, n, 3, 3, 1.0, seg, 0, cnt, off, None, 0, 0, None) == 1
    assert b"n_seg" in lib.gnntrk_last_error()
    assert lib.gnntrk_radius_fill_batched_ws(x, n, 3, 3, 1.0, seg, 0, off, 0, None, None, None, 0, None, 0, 0, None) == 1
    assert lib.gnntrk_radius_count_batched_ws(x, n, 3, 3, -1.0, seg, 2, cnt, off, None, 0, 0, None) == 1
    assert b"radius must be >= 0" in lib.gnntrk_last_error()
    # (NULL seg_ptr: one event, the unbatched entry)
    assert lib.gnntrk_radius_count_batched_ws(x, n, 3, 3, 1.0, None, 0, cnt, off, None, 0, 0, None) == 0
    assert off[n] == n * n
    assert lib.gnntrk_radius_count_batched_ws(x, n, 3, 3, 1.0, seg, 2, cnt, off, None, 0, 0, None) == 0
    assert off[n] == 6 * 6 + 10 * 10
    core = (ctypes.c_uint8 * n)()
    root = (ctypes.c_int32 * n)()
    lab = (ctypes.c_int64 * n)()
    cptr = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.gnntrk_dbscan_labels_batched(off, None, None, n, 1.0, core, root, None, 2, lab, cptr, None, 0, None) == 1
    assert b"seg_ptr" in lib.gnntrk_last_error()
    assert lib.gnntrk_dbscan_labels_batched(off, None, None, n, 1.0, core, root, seg, 2, lab, cptr, None, 0, None) == 1
    assert b"workspace" in lib.gnntrk_last_error()
    assert lib.gnntrk_dbscan_labels_batched(off, None, None, 0, 1.0, core, root, seg, 2, lab, cptr, None, 0, None) == 0
    assert list(cptr) == [0, 0, 0]
    ids = (ctypes.c_int64 * n)()
    f = (ctypes.c_float * n)()
    out = (ctypes.c_int64 * (2 * 1 * (1 + 2 * 4) + 1))()
    need = lib.gnntrk_tracking_metrics_workspace_bytes(n, 2)
    ws = (ctypes.c_uint8 * need)()
    cuts = (ctypes.c_float * 1)(0.0)

    def call(sp=seg, n_seg=2, wb=need, o=out):
        return lib.gnntrk_tracking_metrics_batched(lab, 2, ids, f, f, f, n, sp, n_seg, cuts, 1, 4.0, 3, o, ws, wb, None)

    assert call(sp=None) == 1 and b"seg_ptr" in lib.gnntrk_last_error()
    assert call(n_seg=0) == 1 and b"n_seg" in lib.gnntrk_last_error()
    assert call(wb=need - 1) == 1 and b"workspace" in lib.gnntrk_last_error()
    assert call(o=None) == 1 and b"NULL" in lib.gnntrk_last_error()
