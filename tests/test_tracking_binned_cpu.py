"""Binned tracking metrics, the cluster table and DBSCANPerformanceDetails' results without a GPU
(gnntrk_tracking_metrics_windows, gnntrk_cluster_table, cluster_metrics.py): the numpy restatement
against the reference's golden values (G20, inputs of G17), the kernels on the wave64 emulator against
both, and the C entries' host-side argument checks."""

import ctypes

import numpy as np
import pytest
import torch

import tracking_binned_ref as B
from emul_util import emulated
from gnn_tracking_amd import _capi
from gnn_tracking_amd import cluster_metrics as CM
from tracking_binned_cases import (BINNED, G20, MULTI, TABLES, assert_rows, assert_table, batch, golden_rows,
                                   golden_table, hit_record, random_event, random_windows, scan_batch)

PT_EDGES, ETA_EDGES = G20["pt_edges"].tolist(), G20["eta_edges"].tolist()
MAX_ETA, PT_THLD = float(G20["max_eta"]), float(G20["pt_thld"])


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", BINNED)
def test_restatement_reproduces_binned_golden(name):
    assert_rows(B.vs_pt([batch(name)], PT_EDGES, MAX_ETA), golden_rows(f"single/{name}/", "vs_pt"), name)
    assert_rows(B.vs_eta([batch(name)], ETA_EDGES, PT_THLD), golden_rows(f"single/{name}/", "vs_eta"), name)


def test_restatement_reproduces_multi_batch_golden():
    bs = [batch(n) for n in MULTI]
    assert_rows(B.vs_pt(bs, PT_EDGES, MAX_ETA), golden_rows("multi/", "vs_pt"), "multi")
    assert_rows(B.vs_eta(bs, ETA_EDGES, PT_THLD), golden_rows("multi/", "vs_eta"), "multi")


@pytest.mark.parametrize("name", TABLES)
def test_restatement_reproduces_table_golden(name):
    b = batch(name)
    assert_table(B.cluster_table(b["labels"], b["pid"], b["pt"], b["eta"], b["reco"]), golden_table(f"table/{name}/"),
                 name)


def test_restatement_reproduces_scanner_golden():
    bs = [scan_batch(i) for i in range(3)]
    for i, b in enumerate(bs):
        assert_table(B.cluster_table(b["labels"], b["pid"], b["pt"], b["eta"], b["reco"]),
                     golden_table(f"scan/b{i}/table/"), f"scan b{i}")
    assert_rows(B.vs_pt(bs, PT_EDGES, MAX_ETA), golden_rows("scan/", "vs_pt"), "scan")
    assert_rows(B.vs_eta(bs, ETA_EDGES, PT_THLD), golden_rows("scan/", "vs_eta"), "scan")


# ------------------------------------------------------------------ the emulator
@pytest.mark.parametrize("name", BINNED)
def test_emulated_binned_metrics_match_golden(name):
    h = [hit_record(batch(name))]
    with emulated():
        vp = CM.tracking_metrics_vs_pt(h, [None], PT_EDGES, max_eta=MAX_ETA)
        ve = CM.tracking_metrics_vs_eta(h, [None], ETA_EDGES, pt_thld=PT_THLD)
    assert_rows(vp, golden_rows(f"single/{name}/", "vs_pt"), name)
    assert_rows(ve, golden_rows(f"single/{name}/", "vs_eta"), name)


def test_emulated_multi_batch_matches_golden():
    h = [hit_record(batch(n)) for n in MULTI]
    with emulated():
        vp = CM.tracking_metrics_vs_pt(h, [None] * 3, PT_EDGES, max_eta=MAX_ETA)
        ve = CM.tracking_metrics_vs_eta(h, [None] * 3, ETA_EDGES, pt_thld=PT_THLD)
    assert_rows(vp, golden_rows("multi/", "vs_pt"), "multi")
    assert_rows(ve, golden_rows("multi/", "vs_eta"), "multi")
    with pytest.raises(ValueError, match="differ in length"):
        CM.tracking_metrics_vs_pt(h, [None] * 2, PT_EDGES)


@pytest.mark.parametrize("name", TABLES)
def test_emulated_table_matches_golden(name):
    b = batch(name)
    with emulated():
        got = CM.tracking_metric_table(b["labels"], truth=b["pid"], pts=b["pt"], reconstructable=b["reco"],
                                       eta=b["eta"])
    assert_table(got, golden_table(f"table/{name}/"), name, dtypes=True)


def test_emulated_scanner_results_match_golden():
    """The scanner's results from the reference's DBSCAN labels (the device DBSCAN is the GPU test's)."""
    bs = [scan_batch(i) for i in range(3)]
    with emulated():
        for i, b in enumerate(bs):
            got = CM.tracking_metric_table(b["labels"], truth=b["pid"], pts=b["pt"], reconstructable=b["reco"],
                                           eta=b["eta"])
            assert_table(got, golden_table(f"scan/b{i}/table/"), f"scan b{i}", dtypes=True)
        h = [hit_record(b) for b in bs]
        vp = CM.tracking_metrics_vs_pt(h, [None] * 3, PT_EDGES, max_eta=MAX_ETA)
        ve = CM.tracking_metrics_vs_eta(h, [None] * 3, ETA_EDGES, pt_thld=PT_THLD)
    assert_rows(vp, golden_rows("scan/", "vs_pt"), "scan")
    assert_rows(ve, golden_rows("scan/", "vs_eta"), "scan")


def windows_call(labels, pid, pt, eta, reco, windows, thld=3):
    """gnntrk_tracking_metrics_windows on host arrays through the emulator: (n_particles, counts [T, W, 4])."""
    lib = _capi.load()
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    n_trials, n = labels.shape
    win = np.ascontiguousarray(windows, dtype=np.float32)
    nw = len(win)
    out = np.full(nw + n_trials * nw * 4 + 1, -1, dtype=np.int64)
    ws = np.zeros(lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, n_trials), dtype=np.uint8)
    arrs = [np.ascontiguousarray(a) for a in (pid, pt, eta, reco)]
    _capi.check(lib.gnntrk_tracking_metrics_windows(labels.ctypes.data, n_trials, arrs[0].ctypes.data,
                                                    arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, n,
                                                    win.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nw, thld,
                                                    out.ctypes.data, ws.ctypes.data, ws.size, None), lib)
    assert out[-1] == 0
    return out[:nw], out[nw:-1].reshape(n_trials, nw, 4)


@pytest.mark.parametrize("n,n_trials,big_ids", [(200, 1, False), (3000, 4, True)])
def test_emulated_windows_match_restatement(n, n_trials, big_ids):
    g = np.random.default_rng(n)
    pid, pt, eta, reco = random_event(g, n, max(2, n // 12), big_ids)
    labels = g.integers(-3, max(2, n // 8), size=(n_trials, n)).astype(np.int64)
    win = random_windows(g)
    assert len(win) == 32
    with emulated():
        n_part, counts = windows_call(labels, pid, pt, eta, reco, win)
    assert counts[:, :, 0].sum() > 0 and n_part.sum() > 0
    for t in range(n_trials):
        want_part, want = B.window_counts(labels[t], pid, pt, eta, reco, win)
        assert np.array_equal(n_part, want_part), f"trial {t}"
        assert np.array_equal(counts[t], want), f"trial {t}"


def test_forty_bins_are_two_calls_worth():
    b = batch("blobs")
    edges = np.linspace(0.0, 4.0, 41).tolist()
    h = [hit_record(b), hit_record(batch("naneta"))]
    with emulated():
        rows = CM.tracking_metrics_vs_pt(h, [None, None], edges, max_eta=MAX_ETA)
        first = CM.tracking_metrics_vs_pt(h, [None, None], edges[:33], max_eta=MAX_ETA)
        second = CM.tracking_metrics_vs_pt(h, [None, None], edges[32:], max_eta=MAX_ETA)
    assert len(rows) == 40 and len(first) == 32 and len(second) == 8
    assert_rows(rows, first + second, "40 bins")
    assert_rows(rows, B.vs_pt([b, batch("naneta")], edges, MAX_ETA), "40 bins (restatement)")
    assert sum(r["n_cleaned_clusters"] for r in rows) > 0


def test_table_ties_follow_the_smallest_id_rule():
    # a cluster of 4 hits split 2:2 between particles 9 and 5, and one 3:1
    pid = np.array([9, 9, 5, 5, 7, 7, 7, 3, 5], dtype=np.int64)
    lab = np.array([4, 4, 4, 4, 2, 2, 2, 2, -1], dtype=np.int64)
    pt = np.where(pid == 5, np.float32(2.0), np.float32(0.5)).astype(np.float32)
    eta, reco = np.zeros(9, np.float32), np.ones(9, np.float32)
    with emulated():
        got = CM.tracking_metric_table(lab, truth=pid, pts=pt, reconstructable=reco, eta=eta)
    assert got["c"].tolist() == [2, 4]
    assert got["maj_pid"].tolist() == [7, 5] and got["maj_hits"].tolist() == [3, 2]
    assert got["maj_pid_hits"].tolist() == [3, 3] and got["maj_pt"].tolist() == [0.5, 2.0]
    assert got["maj_frac"].tolist() == [0.75, 0.5] and got["lhc_match"].tolist() == [False, False]
    assert got["perfect_match"].tolist() == [False, False] and got["double_majority"].tolist() == [True, False]
    assert_table(got, B.cluster_table(lab, pid, pt, eta, reco), "ties", dtypes=True, exact_means=True)
    # the largest-id rule would name 9: the tie decides
    swapped = np.where(pid == 5, 11, pid)
    with emulated():
        got2 = CM.tracking_metric_table(lab, truth=swapped, pts=pt, reconstructable=reco, eta=eta)
    assert got2["maj_pid"].tolist() == [7, 9] and got2["maj_pt"].tolist() == [0.5, 0.5]


def test_labels_beyond_the_hits_are_refused():
    pid, pt, eta, reco = random_event(np.random.default_rng(3), 100, 10, False)
    labels = np.zeros((1, 100), dtype=np.int64)
    labels[0, 7] = 100
    with emulated():
        # (the C entry counts them in its last value; the Python layer raises on it)
        lib = _capi.load()
        out = np.zeros(2 * 5 + 1, dtype=np.int64)
        win = np.zeros((2, 4), dtype=np.float32)
        ws = np.zeros(lib.gnntrk_tracking_metrics_windows_workspace_bytes(100, 1), dtype=np.uint8)
        _capi.check(lib.gnntrk_tracking_metrics_windows(labels.ctypes.data, 1, pid.ctypes.data, pt.ctypes.data,
                                                        eta.ctypes.data, reco.ctypes.data, 100,
                                                        win.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2, 3,
                                                        out.ctypes.data, ws.ctypes.data, ws.size, None), lib)
        assert out[-1] == 1
        # labels that are handed through as they are (the scanner's DBSCAN labels, in [-1, n) by construction)
        cpu = torch.device("cpu")
        with pytest.raises(ValueError, match=">= the number of hits"):
            CM._table(torch.from_numpy(labels[0]), None, *CM._hits(pid, pt, reco, eta, cpu), 3)


# ------------------------------------------------------------ host-side validation
@pytest.fixture(scope="module", params=["gfx950", "emulator"])
def lib(request):
    if request.param == "emulator":
        import emul_util
        return emul_util.emulator_lib()
    from gnn_tracking_amd import _build
    return _capi.bind(ctypes.CDLL(str(_build.build_lib())))


def test_windows_entry_validates_on_the_host(lib):
    n = 16
    lab, ids, f = (ctypes.c_int64 * (2 * n))(), (ctypes.c_int64 * n)(), (ctypes.c_float * n)()
    out = (ctypes.c_int64 * (32 + 2 * 32 * 4 + 1))()
    win = (ctypes.c_float * (4 * 33))()
    need = lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, 2)
    assert need > 0 and lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, 4) > need
    ws = (ctypes.c_uint8 * need)()

    def call(n_trials=2, n_win=1, wn=win, labels=lab, pid=ids, pt=f, o=out, w=ws, wb=need, nn=n):
        return lib.gnntrk_tracking_metrics_windows(labels, n_trials, pid, pt, f, f, nn, wn, n_win, 3, o, w, wb, None)

    def err():
        return lib.gnntrk_last_error()

    assert call(n_win=0) == 1 and b"n_win" in err()
    assert call(n_win=33) == 1 and b"n_win" in err()
    assert call(wn=None) == 1 and b"NULL" in err()
    assert call(n_trials=0) == 1 and b"n_trials" in err()
    assert call(n_trials=_capi.TRACKING_MAX_TRIALS + 1) == 1 and b"n_trials" in err()
    assert call(labels=None) == 1 and b"NULL" in err()
    assert call(pid=None) == 1 and b"NULL" in err()
    assert call(pt=None) == 1 and b"NULL" in err()
    assert call(o=None) == 1 and b"NULL" in err()
    assert call(w=None) == 1 and b"workspace" in err()
    assert call(wb=need - 1) == 1 and b"workspace" in err()
    assert call(nn=-1) == 1
    assert call(nn=1 << 30) == 4 and b"2^30" in err()
    assert _capi.TRACKING_MAX_WINDOWS == 32


def test_cluster_table_entry_validates_on_the_host(lib):
    n = 16
    lab, f = (ctypes.c_int64 * n)(), (ctypes.c_float * n)()
    col, bad = (ctypes.c_int64 * n)(), (ctypes.c_int64 * 1)()
    need = lib.gnntrk_cluster_table_workspace_bytes(n)
    assert need > 0 and lib.gnntrk_cluster_table_workspace_bytes(4 * n) > need
    ws = (ctypes.c_uint8 * need)()

    def call(labels=lab, pid=lab, pt=f, size=col, mpid=col, mpt=f, nb=bad, w=ws, wb=need, nn=n):
        return lib.gnntrk_cluster_table(labels, pid, pt, f, f, nn, size, col, mpid, col, mpt, f, f, nb, w, wb, None)

    def err():
        return lib.gnntrk_last_error()

    assert call(labels=None) == 1 and b"NULL" in err()
    assert call(pid=None) == 1 and b"NULL" in err()
    assert call(pt=None) == 1 and b"NULL" in err()
    assert call(size=None) == 1 and b"NULL" in err()
    assert call(mpid=None) == 1 and b"NULL" in err()
    assert call(mpt=None) == 1 and b"NULL" in err()
    assert call(nb=None) == 1 and b"NULL" in err()
    assert call(w=None) == 1 and b"workspace" in err()
    assert call(wb=need - 1) == 1 and b"workspace" in err()
    assert call(nn=-1) == 1
    assert call(nn=1 << 30) == 4 and b"2^30" in err()
