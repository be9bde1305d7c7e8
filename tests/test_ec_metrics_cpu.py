"""Edge-classifier validation metrics without a GPU: the float64 restatement against the golden
vectors from the reference (tests/golden/g16_ec_metrics.npz, tools/make_golden_ec_metrics.py) and
sklearn, the kernels of csrc/metrics.hip on the wave64 emulator against both, and the host-side
argument checks of the new C entries."""

import ctypes

import numpy as np
import pytest
import torch

import ec_metrics_ref as R
from emul_util import emulated
from gnn_tracking_amd import _capi
from gnn_tracking_amd import metrics as M

GOLD = np.load(__import__("pathlib").Path(__file__).resolve().parent / "golden" / "g16_ec_metrics.npz")
CASES = ("g1", "ties", "saturated", "nanscore", "nopos", "empty")


def case(name):
    return tuple(GOLD[f"{name}/{k}"] for k in ("w", "y", "pt", "edge_index"))


def golden(name):
    return dict(zip([str(k) for k in GOLD[f"{name}/keys"]], GOLD[f"{name}/values"].tolist()))


def assert_metrics(got: dict, want: dict, what: str, auc_tol=1e-12):
    assert list(got) == list(want), f"{what}: keys {list(got)} vs {list(want)}"
    for k, v in want.items():
        tol = auc_tol if k.startswith("roc_auc") else 0.0
        assert R.same_value(float(got[k]), float(v), tol), f"{what}: {k} = {got[k]!r}, want {v!r}"


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_golden(name):
    w, y, pt, ei = case(name)
    assert_metrics(R.ec_metrics(w, y, pt, ei), golden(name), f"restatement/{name}")
    keys = [str(k) for k in GOLD[f"{name}/bcs_keys"]]
    for t, row in zip(GOLD["bcs_thlds"], GOLD[f"{name}/bcs_values"]):
        got = R.bcs_at(w, y, float(t))
        assert list(got) == keys
        assert [float(v) for v in got.values()] == row.tolist(), f"BinaryClassificationStats({t})"


def test_golden_has_the_validation_keys():
    keys = list(golden("ties"))
    assert len(keys) == 44 and keys[:3] == ["roc_auc", "roc_auc_0.01FPR", "roc_auc_0.001FPR"]
    assert "max_mcc_pt0.9" in keys and "tpr_eq_tnr_pt0.9" in keys and keys[-1] == "tpr_eq_tnr_loc_pt1.5"
    assert np.isfinite(GOLD["g1/total"])


def test_restatement_auc_matches_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    g = np.random.default_rng(3)
    for n, levels in ((500, None), (2000, 9), (3000, 2)):
        w = g.random(n).astype(np.float32) if levels is None else \
            g.integers(0, levels, n).astype(np.float32) / np.float32(levels)
        y = g.random(n) < 0.2 + 0.5 * w
        for f in (None, 0.01, 0.001, 0.3, 1.0):
            want = skm.roc_auc_score(y, w, max_fpr=f)
            assert abs(R.roc_auc(y, w, f) - want) <= 1e-12, (n, levels, f)


# ---------------------------------------------------------------- emulated kernels
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", CASES)
def test_emulated_validation_metrics_match_golden(name):
    w, y, pt, ei = case(name)
    with emulated():
        got = M.ec_validation_metrics(t(w), t(y), t(pt), t(ei))
        full = M.get_roc_auc_scores(t(y), t(w), [None, 0.01, 0.001]) | M.get_maximized_bcs(output=t(w), y=t(y))
        bcs = [M.BinaryClassificationStats(t(w), t(y), float(th)).get_all() for th in GOLD["bcs_thlds"]]
    gold = golden(name)
    assert_metrics(got, gold, f"emulated/{name}")
    assert_metrics(full, {k: v for k, v in gold.items() if "_pt" not in k}, f"emulated full/{name}")
    for b, row in zip(bcs, GOLD[f"{name}/bcs_values"]):
        assert list(b) == [str(k) for k in GOLD[f"{name}/bcs_keys"]]
        assert [float(v) for v in b.values()] == row.tolist()


def _counts(w, y, pt, src, tgt, cuts, thr, perm=None):
    e = M._Edges.__new__(M._Edges)
    e.w, e.perm, e.pt = w, perm, pt
    e.src, e.tgt, e.ids_i64 = src, tgt, int(src is not None and src.dtype == torch.int64)
    e.y, e.y_kind = (y.view(torch.uint8), 0) if y.dtype == torch.bool else (y, 1)
    e.n = w.numel()
    out = torch.empty(len(cuts) * 2 * (thr.numel() + 1), dtype=torch.int64)
    M._launch_counts(e, cuts, thr, out)
    auc = torch.empty(len(cuts) * _capi.AUC_STRIDE, dtype=torch.int64)
    M._launch_auc(e, cuts, [0.01, 0.001, 0.3], auc)
    return out.numpy().reshape(len(cuts), 2, -1), auc.numpy().reshape(len(cuts), -1)


@pytest.mark.parametrize("n,dist,n_thr,n_cuts,csr", [
    (1, "uniform", 200, 4, False), (255, "saturated", 1, 1, True), (4097, "ties", 200, 4, True),
    (9001, "uniform", 1024, 8, False), (3 * 4096 * 4 + 17, "saturated", 200, 4, True),
    (20000, "ties", 37, 3, False)])
def test_emulated_kernels_several_workgroups(n, dist, n_thr, n_cuts, csr):
    """Count tables exact against np.bincount, AUC rows against the float64 restatement; sizes of
    several workgroups / sort tiles with odd tails, int32 ids through a permutation (CSR form) and
    int64 ids, bool and fp32 labels, the small and the large LDS histogram."""
    g = np.random.default_rng(n)
    n_nodes = max(2, n // 7)
    ei = g.integers(0, n_nodes, size=(2, n)).astype(np.int64)
    pt = g.lognormal(0.0, 0.7, n_nodes).astype(np.float32)
    pt[: n_nodes // 10] = np.float32(0.9)
    if dist == "uniform":
        w = g.random(n).astype(np.float32)
    elif dist == "saturated":
        w = np.where(g.random(n) < 0.7, np.float32(0.001), np.float32(0.999)).astype(np.float32)
    else:
        w = np.array([-0.0, 0.0, 0.25, 0.5, 1.0, np.float32(1 / 3)], np.float32)[g.integers(0, 6, n)]
    y = g.random(n) < 0.2 + 0.5 * w
    cuts = sorted(g.choice([0.0, 0.3, 0.5, 0.9, 1.2, 1.5, 2.0, 3.0], n_cuts, replace=False).tolist())
    thr = torch.linspace(0.0, 1.0, n_thr) if n_thr > 1 else torch.tensor([0.5])
    want = R.counts_table(w, y, pt, ei, cuts, thr.numpy())
    with emulated():
        if csr:   # scores and ids in a permuted order, labels read through the permutation (fp32 labels)
            perm = g.permutation(n).astype(np.int32)
            got, auc = _counts(t(w[perm]), t(y.astype(np.float32)), t(pt), t(ei[0][perm].astype(np.int32)),
                               t(ei[1][perm].astype(np.int32)), cuts, thr, t(perm))
        else:
            got, auc = _counts(t(w), t(y), t(pt), t(ei[0]), t(ei[1]), cuts, thr)
    assert np.array_equal(got, want)
    for c, cut in enumerate(cuts):
        m = R.cut_mask(pt, ei, cut)
        ref = R.roc_aucs(y[m], w[m], [None, 0.01, 0.001, 0.3])
        vals = M._auc_from_row(auc[c], [0.01, 0.001, 0.3])
        assert int(auc[c, 0]) == int((y & m).sum()) and int(auc[c, 1]) == int((~y & m).sum())
        for a, b in zip(vals, ref):
            assert R.same_value(a, b, 1e-12), (cut, vals, ref)


def test_product_path_refuses_cpu_tensors():
    w = torch.rand(10)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.ec_validation_metrics(w, w > 0.5, torch.rand(4), torch.zeros(2, 10, dtype=torch.int64))


# ------------------------------------------------------------ host-side validation
@pytest.fixture(scope="module", params=["gfx950", "emulator"])
def lib(request):
    if request.param == "emulator":
        import emul_util
        return emul_util.emulator_lib()
    from gnn_tracking_amd import _build
    return _capi.bind(ctypes.CDLL(str(_build.build_lib())))


def test_metrics_entries_validate_on_the_host(lib):
    buf = (ctypes.c_float * 64)()
    ids = (ctypes.c_int64 * 64)()
    out = (ctypes.c_int64 * (8 * _capi.AUC_STRIDE + 2 * 9 * 2 * 1025))()

    def cuts(*v):
        return (ctypes.c_float * max(1, len(v)))(*v)

    fpr = (ctypes.c_double * 4)(0.01, 0.001, 0.5, 1.0)

    def counts(n_cuts=1, n_thr=4, n=16, w=buf, y=buf, thr=buf, c=None, pt=None, counts_out=out):
        return lib.gnntrk_bcs_counts(w, y, 1, None, ids, ids, 1, pt, c or cuts(*([0.0] * max(1, n_cuts))), n_cuts, thr,
                                     n_thr, n, counts_out, None)

    def auc(n_cuts=1, n_fpr=2, n=16, ws=None, ws_bytes=0, f=fpr, c=None, pt=None, w=buf):
        return lib.gnntrk_roc_auc(w, buf, 1, None, ids, ids, 1, pt, c or cuts(*([0.0] * max(1, n_cuts))), n_cuts, f,
                                  n_fpr, n, out, ws, ws_bytes, None)

    def err():
        return lib.gnntrk_last_error()

    assert counts(n_cuts=9) == 1 and b"n_cuts" in err()
    assert counts(n_cuts=0) == 1
    assert counts(n_thr=1025) == 1 and b"n_thr" in err()
    assert counts(w=None) == 1 and b"NULL" in err()
    assert counts(thr=None) == 1 and b"NULL" in err()
    assert counts(counts_out=None) == 1 and b"NULL" in err()
    assert counts(n_cuts=2, c=cuts(0.9, 0.5), pt=buf) == 1 and b"ascending" in err()
    assert counts(n=1 << 31) == 4 and b"2^31" in err()
    need = lib.gnntrk_roc_auc_workspace_bytes(16)
    assert need >= 16 * 16 and lib.gnntrk_roc_auc_workspace_bytes(1 << 26) >= 16 * (1 << 26)
    assert auc(ws=None) == 1 and b"workspace" in err()
    ws = (ctypes.c_uint8 * 64)()
    assert auc(ws=ws, ws_bytes=64) == 1 and b"workspace" in err()
    assert auc(n_fpr=5) == 1 and b"n_fpr" in err()
    bad = (ctypes.c_double * 1)(0.0)
    assert auc(n_fpr=1, f=bad) == 1 and b"max_fpr" in err()
    assert auc(n_cuts=9) == 1 and b"n_cuts" in err()
    assert auc(w=None) == 1 and b"NULL" in err()
    assert auc(n=1 << 31) == 4
