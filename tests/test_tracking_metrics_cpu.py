"""Tracking metrics of the OC validation (gnntrk_tracking_metrics, cluster_metrics.py, OCScanResults)
without a GPU: the numpy restatement against the reference's golden values (G17), the kernels on the
wave64 emulator against both, and the C entries' host-side argument checks."""

import ctypes
import pathlib

import numpy as np
import pytest
import torch

import tracking_metrics_ref as R
from emul_util import emulated
from gnn_tracking_amd import _capi
from gnn_tracking_amd import cluster_metrics as CM
from gnn_tracking_amd.postprocessing import OCScanResults

GOLD = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "g17_tracking_metrics.npz")
CASES = ("td3_0", "td3_1", "blobs", "ptedge", "naneta", "recomix", "recobool", "nocut", "noise", "empty")


def golden(name):
    return dict(zip([str(k) for k in GOLD[f"{name}/keys"]], GOLD[f"{name}/values"].tolist()))


def case(name):
    return {k: GOLD[f"{name}/{k}"] for k in ("labels", "pid", "pt", "eta", "reco")}, tuple(GOLD[f"{name}/cuts"])


def assert_same(got: dict, want: dict, what: str):
    assert list(got) == list(want), f"{what}: keys {list(got)} vs {list(want)}"
    for k, v in want.items():
        g = float(got[k])
        assert g == v or (g != g and v != v), f"{what}: {k} = {got[k]!r}, want {v!r}"


@pytest.mark.parametrize("name", [c for c in CASES if c != "empty"])
def test_restatement_reproduces_reference_golden(name):
    c, cuts = case(name)
    got = R.tracking_metrics_flat(c["labels"], c["pid"], c["pt"], c["eta"], c["reco"], cuts)
    assert_same(got, golden(name), name)


@pytest.mark.parametrize("name", CASES)
def test_emulated_tracking_metrics_match_golden(name):
    c, cuts = case(name)
    with emulated():
        got = CM.tracking_metrics(truth=c["pid"], predicted=c["labels"], pts=c["pt"], reconstructable=c["reco"],
                                  eta=c["eta"], pt_thlds=list(cuts))
    assert list(got) == list(cuts)
    assert_same(CM.flatten_track_metrics(got), golden(name), name)


def random_event(g, n, n_part, n_lab, big_ids):
    pid = g.integers(0, n_part, n).astype(np.int64)
    if big_ids:
        pid = pid * (2 ** 40) - 2 ** 41
    pt = g.choice(np.array([0.3, 0.5, 0.9, 0.95, 1.5, 2.0, np.nan], np.float32), n)
    eta = g.choice(np.array([0.1, -3.9, 4.0, -4.0, 2.5, np.nan], np.float32), n)
    reco = g.choice(np.array([0, 1, np.nan], np.float32), n, p=[0.2, 0.75, 0.05])
    return pid, pt, eta, reco


@pytest.mark.parametrize("n,n_trials,big_ids", [(200, 3, False), (3000, 4, True), (20000, 2, True)])
def test_emulated_trials_match_restatement(n, n_trials, big_ids):
    g = np.random.default_rng(n)
    pid, pt, eta, reco = random_event(g, n, max(2, n // 12), n // 8, big_ids)
    labels = g.integers(-3, max(2, n // 8), size=(n_trials, n)).astype(np.int64)
    with emulated():
        got = CM.tracking_metrics_trials(torch.from_numpy(labels), truth=pid, pts=pt, eta=eta, reconstructable=reco)
    for t in range(n_trials):
        assert_same(got[t], R.tracking_metrics_flat(labels[t], pid, pt, eta, reco), f"trial {t}")


def test_ties_follow_the_smallest_id_rule():
    # clusters of 4 hits split 2:2 between a particle that passes the 0.9 cut and one that does not: the
    # smaller id decides whether the cluster counts at 0.9
    pid = np.array([5, 5, 9, 9, 9, 9, 5, 5] * 2 + [7, 7, 3, 3], dtype=np.int64)
    pt = np.where(np.isin(pid, (5, 3)), np.float32(2.0), np.float32(0.5)).astype(np.float32)
    lab = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
    eta, reco = np.zeros(20, np.float32), np.ones(20, np.float32)
    with emulated():
        got = CM.tracking_metrics(truth=pid, predicted=lab, pts=pt, reconstructable=reco, eta=eta, pt_thlds=[0.0, 0.9])
    # majority particle: 5 for clusters 0..3 (5 < 9), 3 for cluster 4 (3 < 7): all pass 0.9
    assert got[0.9]["n_cleaned_clusters"] == 5
    assert_same(CM.flatten_track_metrics(got), R.tracking_metrics_flat(lab, pid, pt, eta, reco, (0.0, 0.9)), "ties")
    # the largest-id rule would give another answer: the tie decides
    swapped = np.where(pid == 5, 11, np.where(pid == 3, 13, pid))
    with emulated():
        got2 = CM.tracking_metrics(truth=swapped, predicted=lab, pts=pt, reconstructable=reco, eta=eta,
                                   pt_thlds=[0.0, 0.9])
    assert got2[0.9]["n_cleaned_clusters"] == 0


def test_arbitrary_labels_and_unsorted_cuts():
    c, _ = case("blobs")
    lab = np.where(c["labels"] < 0, -7, c["labels"] * 1000 + 10 ** 12)
    with emulated():
        got = CM.tracking_metrics(truth=c["pid"], predicted=lab, pts=c["pt"], reconstructable=c["reco"],
                                  eta=c["eta"], pt_thlds=[0.9, 0.0, 1.5, 0.5])
    want = golden("blobs")
    assert list(got) == [0.9, 0.0, 1.5, 0.5]
    flat = CM.flatten_track_metrics(got)
    assert_same({k: flat[k] for k in want}, want, "relabelled")


def test_labels_beyond_the_hits_are_refused():
    pid, pt, eta, reco = random_event(np.random.default_rng(3), 100, 10, 10, False)
    labels = torch.zeros((2, 100), dtype=torch.int64)
    labels[1, 7] = 100
    with emulated(), pytest.raises(ValueError, match=">= the number of hits"):
        CM.tracking_metrics_trials(labels, truth=pid, pts=pt, eta=eta, reconstructable=reco)


def test_oc_scan_results_match_golden():
    keys = [str(k) for k in GOLD["scan/record_keys"]]
    records = []
    for row in GOLD["scan/records"]:
        r = dict(zip(keys, row.tolist()))
        r["i_batch"], r["min_samples"] = int(r["i_batch"]), int(r["min_samples"])
        records.append(r)
    want = dict(zip([str(k) for k in GOLD["scan/fom_keys"]], GOLD["scan/fom_values"].tolist()))
    assert len(want) == 68
    foms = OCScanResults(records).get_foms()
    assert list(foms) == list(want)
    for k, v in want.items():
        assert foms[k] == pytest.approx(v, rel=1e-12, abs=1e-15, nan_ok=True), k
    assert R.get_foms(records) == pytest.approx(want, rel=1e-12, abs=1e-15, nan_ok=True)
    assert isinstance(foms["best_dbscan_min_samples"], float)


# ------------------------------------------------------------ host-side validation
@pytest.fixture(scope="module", params=["gfx950", "emulator"])
def lib(request):
    if request.param == "emulator":
        import emul_util
        return emul_util.emulator_lib()
    from gnn_tracking_amd import _build
    return _capi.bind(ctypes.CDLL(str(_build.build_lib())))


def test_tracking_metrics_entry_validates_on_the_host(lib):
    n = 16
    lab = (ctypes.c_int64 * n)()
    ids = (ctypes.c_int64 * n)()
    f = (ctypes.c_float * n)()
    out = (ctypes.c_int64 * (8 + 8 * 8 * 4 + 1))()
    need = lib.gnntrk_tracking_metrics_workspace_bytes(n, 2)
    assert need > 0 and lib.gnntrk_tracking_metrics_workspace_bytes(n, 4) > need
    ws = (ctypes.c_uint8 * need)()

    def cuts(*v):
        return (ctypes.c_float * max(1, len(v)))(*v)

    def call(n_trials=2, n_cuts=1, c=None, labels=lab, pid=ids, pt=f, o=out, w=ws, wb=need, nn=n):
        return lib.gnntrk_tracking_metrics(labels, n_trials, pid, pt, f, f, nn, c or cuts(*([0.0] * max(1, n_cuts))),
                                           n_cuts, 4.0, 3, o, w, wb, None)

    def err():
        return lib.gnntrk_last_error()

    assert call(n_cuts=9) == 1 and b"n_cuts" in err()
    assert call(n_cuts=0) == 1 and b"n_cuts" in err()
    assert call(n_cuts=2, c=cuts(0.9, 0.5)) == 1 and b"ascending" in err()
    assert call(n_cuts=2, c=cuts(0.5, float("nan"))) == 1 and b"ascending" in err()
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
