"""The k-scan of the metric-learning validation (gnntrk_cc_labels, gnntrk_kscan_counts, graph_analysis.py,
k_scanner.py) without a GPU: the numpy restatement against the reference's golden values (G18), the kernels
on the wave64 emulator against both, random graphs against the restatement, the C entries' host-side
argument checks and ``KScanResults`` on hand-written tables.

FOM tolerance: G18 stores ``fom_rel_dev``, the largest relative deviation between the reference's figures
of merit (L-BFGS-B) and its own spline at the bracketed root; the tests compare at 100 x that value
(optimiser stopping noise that may move with the scipy build).  Records and the ``max_frac_segment50``
block involve no optimiser and are compared exactly."""

import ctypes
import pathlib

import numpy as np
import pytest
import torch

import kscan_ref as R
from emul_util import emulated, emulator_lib
from gnn_tracking_amd import Data, GraphConstructionKNNScanner, KScanResults
from gnn_tracking_amd import graph_analysis as GA
from gnn_tracking_amd import k_scanner as KS

GOLD = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "g18_kscan.npz")
CASES = [str(c) for c in GOLD["cases"]]
FOM_RTOL = 100 * float(GOLD["fom_rel_dev"])


def batches(name):
    return [{k: GOLD[f"{name}/b{i}/{k}"] for k in ("x", "pid", "pt", "eta", "reco", "true_edge_index")}
            for i in range(int(GOLD[f"{name}/n_batches"]))]


def settings(name):
    max_radius, pt_thld, max_eta, max_edges = GOLD[f"{name}/settings"].tolist()
    return dict(ks=GOLD[f"{name}/ks"].tolist(), targets=tuple(GOLD[f"{name}/targets"].tolist()),
                max_radius=max_radius, pt_thld=pt_thld, max_eta=max_eta, max_edges=int(max_edges))


def golden_records(name):
    keys = [str(k) for k in GOLD[f"{name}/record_keys"]]
    return [dict(zip(keys, row.tolist())) for row in GOLD[f"{name}/records"]]


def golden_foms(name):
    return dict(zip([str(k) for k in GOLD[f"{name}/fom_keys"]], GOLD[f"{name}/fom_values"].tolist()))


def assert_records(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), f"{what}: record {i} keys {list(g)} vs {list(w)}"
        for k, v in w.items():
            assert float(g[k]) == v or (g[k] != g[k] and v != v), f"{what}: record {i} {k} = {g[k]!r}, want {v!r}"


def assert_foms(got, want, what, rtol=FOM_RTOL):
    assert list(got) == list(want), f"{what}: keys {list(got)} vs {list(want)}"
    for k, v in want.items():
        g = float(got[k])
        if "max_frac_segment50" in k:
            assert g == v or (g != g and v != v), f"{what}: {k} = {g!r}, want {v!r} (exact)"
        else:
            assert (g != g and v != v) or abs(g - v) <= rtol * abs(v), f"{what}: {k} = {g!r}, want {v!r}"


def data_of(b, dev="cpu"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return Data(x=t(b["x"]), particle_id=t(b["pid"]), pt=t(b["pt"]), eta=t(b["eta"]), reconstructable=t(b["reco"]),
                true_edge_index=t(b["true_edge_index"]))


def scan(name, dev="cpu"):
    s = settings(name)
    scanner = GraphConstructionKNNScanner(**s)
    for i, b in enumerate(batches(name)):
        scanner(data_of(b, dev), i)
    return scanner


def test_fom_tolerance_comes_from_the_golden_file():
    assert 0 < FOM_RTOL < 1e-4


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_golden(name):
    s = settings(name)
    recs = []
    for b in batches(name):
        recs += R.batch_records(b["x"], b["pid"], b["pt"], b["eta"], b["reco"], b["true_edge_index"], s["ks"],
                                max_radius=s["max_radius"], pt_thld=s["pt_thld"], max_eta=s["max_eta"],
                                max_edges=s["max_edges"])
    assert_records(recs, golden_records(name), name)
    assert_foms(R.foms(R.mean_rows(recs), s["targets"]), golden_foms(name), name)


@pytest.mark.parametrize("name", CASES)
def test_emulated_scanner_matches_golden(name):
    with emulated():
        scanner = scan(name)
        foms = scanner.get_foms()
    assert_records(scanner.results_raw, golden_records(name), name)
    assert_foms(foms, golden_foms(name), name)
    nan_cols = {str(c) for c in GOLD[f"{name}/nan_columns"]}
    res = scanner.get_results()
    assert {c for c in res.columns if np.isnan(res.table[c]).any()} == nan_cols


def canonical(labels):
    """Any component numbering -> the smallest index of the component."""
    labels = np.asarray(labels)
    first = np.full(labels.max() + 1, len(labels), dtype=np.int64)
    np.minimum.at(first, labels, np.arange(len(labels)))
    return first[labels]


@pytest.mark.parametrize("name", CASES)
def test_emulated_free_functions_match_golden(name):
    b, s = batches(name)[0], settings(name)
    ei = GOLD[f"{name}/first/edge_index"]
    d = data_of(b)
    d.edge_index = torch.from_numpy(ei)
    d.y = d.particle_id[d.edge_index[0]] == d.particle_id[d.edge_index[1]]
    n = len(b["pid"])
    with emulated():
        cc_all = GA.get_cc_labels(d.edge_index, n).numpy()
        cc_true = GA.get_cc_labels(d.edge_index[:, d.y], num_nodes=n).numpy()
        lsf = GA.get_largest_segment_fracs(d, pt_thld=s["pt_thld"], max_eta=s["max_eta"])
        ep = GA.get_efficiency_purity_edges(d, pt_thld=s["pt_thld"], max_eta=s["max_eta"])
    assert np.array_equal(cc_all, canonical(GOLD[f"{name}/first/cc_all"]))
    assert np.array_equal(cc_true, canonical(GOLD[f"{name}/first/cc_true"]))
    assert np.array_equal(np.sort(lsf), GOLD[f"{name}/first/lsf_sorted"])
    assert [ep["efficiency"], ep["purity"]] == GOLD[f"{name}/first/eff_pur"].tolist() and list(ep) == ["efficiency", "purity"]


def test_golden_separates_the_two_component_problems():
    """A particle whose two good segments are joined only through a masked-out hit of its own: on the
    masked hits the same-id components of all hits are coarser than the segment components."""
    b, s = batches("base")[1], settings("base")
    n = len(b["pid"])
    mask = R.good_node_mask(b["pid"], b["pt"], b["eta"], b["reco"], s["pt_thld"], s["max_eta"])
    nbr, cnt = R.neighbour_table(b["x"], max(s["ks"]), s["max_radius"])
    e = R.table_edges(nbr, cnt, 3)
    seg = R.cc_labels(e, n, same_pid=b["pid"], node_mask=mask)
    upper = R.cc_labels(e, n, same_pid=b["pid"])
    assert len(np.unique(upper[mask])) < len(np.unique(seg[mask]))


def random_graph(g, n, m, n_part, big_ids):
    pid = g.integers(0, n_part, n).astype(np.int64)
    if big_ids:
        pid = pid * (2 ** 40) - 2 ** 41   # (negative ids too)
    ei = g.integers(0, n, size=(2, m)).astype(np.int64)
    mask = g.random(n) < 0.7
    return pid, ei, mask


@pytest.mark.parametrize("n,m,big_ids", [(50, 30, False), (3000, 4000, True), (20000, 60000, True)])
def test_emulated_edge_list_components_match_restatement(n, m, big_ids):
    g = np.random.default_rng(n)
    pid, ei, mask = random_graph(g, n, m, max(2, n // 40), big_ids)
    # chains make deep trees: a path through all nodes in random order, same id
    if n == 3000:
        order = g.permutation(n)
        ei = np.concatenate([ei, np.stack([order[:-1], order[1:]])], axis=1)
    t = torch.from_numpy
    for use_pid in (False, True):
        for use_mask in (False, True):
            with emulated():
                got = GA.cc_labels(t(ei), n, same_pid=t(pid) if use_pid else None,
                                   node_mask=t(mask) if use_mask else None).numpy()
            want = R.cc_labels(ei, n, same_pid=pid if use_pid else None, node_mask=mask if use_mask else None)
            assert np.array_equal(got, want), (use_pid, use_mask)


def test_emulated_edge_list_out_of_range_is_refused():
    ei = torch.tensor([[0, 1, 7], [1, 2, 3]])
    with emulated(), pytest.raises(ValueError, match="outside"):
        GA.get_cc_labels(ei, 5)


def table_labels(lib, nbr, cnt, k_stride, k, pid, mask):
    n = len(cnt)
    labels = np.zeros(n, np.int64)
    bad = np.zeros(1, np.int64)
    ws = np.zeros(lib.gnntrk_cc_labels_workspace_bytes(n), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    m8 = None if mask is None else mask.astype(np.uint8)
    rc = lib.gnntrk_cc_labels(None, 0, p(nbr), p(cnt), k_stride, k, p(pid), p(m8), n, p(labels), p(bad), p(ws),
                              ws.size, None)
    assert rc == 0, lib.gnntrk_last_error()
    assert bad[0] == 0
    return labels


@pytest.mark.parametrize("n,kmax,big_ids", [(300, 5, False), (5000, 9, True)])
def test_emulated_table_components_and_counts_match_restatement(n, kmax, big_ids):
    g = np.random.default_rng(n + 1)
    pid, _, mask = random_graph(g, n, 1, max(2, n // 12), big_ids)
    nbr = g.integers(0, n, size=(n, kmax)).astype(np.int32)
    cnt = g.integers(0, kmax + 1, size=n).astype(np.int32)
    te = g.integers(0, n, size=(2, 2 * n)).astype(np.int64)
    ks = [3, 1, kmax, 2, 3]   # unsorted, with a repeat
    lib = emulator_lib()
    for k in (1, kmax):
        e = R.table_edges(nbr, cnt, k)
        for use_pid in (False, True):
            for use_mask in (False, True):
                got = table_labels(lib, nbr, cnt, kmax, k, pid if use_pid else None, mask if use_mask else None)
                want = R.cc_labels(e, n, same_pid=pid if use_pid else None, node_mask=mask if use_mask else None)
                assert np.array_equal(got, want), (k, use_pid, use_mask)
    t = torch.from_numpy
    with emulated():
        counts, labels = KS.kscan_counts(t(nbr.reshape(-1)), t(cnt), kmax, ks, t(pid), t(mask), t(te))
    want_c, want_l = R.scan_table(nbr, cnt, ks, pid, mask, te)
    assert np.array_equal(counts.numpy(), want_c)
    assert np.array_equal(labels.numpy(), want_l)


def test_new_entries_validate_on_the_host():
    lib = emulator_lib()
    buf = (ctypes.c_int64 * 64)()
    i32 = (ctypes.c_int32 * 64)()
    err = lambda: lib.gnntrk_last_error()   # noqa: E731
    assert lib.gnntrk_cc_labels_workspace_bytes(1000) >= 4000
    assert lib.gnntrk_cc_labels(buf, 0, None, None, 0, 0, None, None, 0, None, None, None, 0, None) == 0   # nothing to do
    assert lib.gnntrk_cc_labels(buf, 1, None, None, 0, 0, None, None, -1, buf, None, buf, 512, None) == 1
    assert lib.gnntrk_cc_labels(buf, -1, None, None, 0, 0, None, None, 4, buf, None, buf, 512, None) == 1
    assert lib.gnntrk_cc_labels(None, 0, i32, i32, 4, 0, None, None, 4, buf, None, buf, 512, None) == 1 and b"k = 0" in err()
    assert lib.gnntrk_cc_labels(None, 0, i32, i32, 4, 5, None, None, 4, buf, None, buf, 512, None) == 1
    assert lib.gnntrk_cc_labels(None, 0, None, i32, 4, 2, None, None, 4, buf, None, buf, 512, None) == 1 and b"NULL" in err()
    assert lib.gnntrk_cc_labels(buf, 1, None, None, 0, 0, None, None, 4, None, None, buf, 512, None) == 1 and b"NULL" in err()
    assert lib.gnntrk_cc_labels(buf, 1, None, None, 0, 0, None, None, 4, buf, None, buf, 8, None) == 1 and b"workspace" in err()
    assert lib.gnntrk_cc_labels(buf, 1, None, None, 0, 0, None, None, 1 << 30, buf, None, buf, 8, None) == 4

    ks = (ctypes.c_int32 * 3)(1, 2, 3)
    u8 = (ctypes.c_uint8 * 64)()
    need = lib.gnntrk_kscan_counts_workspace_bytes(4)
    ws = (ctypes.c_uint8 * need)()
    ok = lambda **kw: dict(dict(nbr=i32, cnt=i32, n=4, k_stride=3, ks=ks, n_ks=3, pid=buf, mask=u8, te=None, n_te=0,   # noqa: E731
                                out=buf, labels=buf, ws=ws, ws_bytes=need), **kw)
    call = lambda a: lib.gnntrk_kscan_counts(a["nbr"], a["cnt"], a["n"], a["k_stride"], a["ks"], a["n_ks"], a["pid"],   # noqa: E731
                                             a["mask"], a["te"], a["n_te"], a["out"], a["labels"], a["ws"],
                                             a["ws_bytes"], None)
    assert call(ok(n=0)) == 0
    assert call(ok(n=-1)) == 1
    assert call(ok(n_ks=0)) == 1 and call(ok(n_ks=65)) == 1
    assert call(ok(ks=None)) == 1 and b"NULL" in err()
    assert call(ok(ks=(ctypes.c_int32 * 3)(1, 0, 3))) == 1 and b"k = 0" in err()
    assert call(ok(k_stride=2)) == 1 and b"k = 3" in err()
    assert call(ok(nbr=None)) == 1 and call(ok(mask=None)) == 1 and call(ok(labels=None)) == 1 and b"NULL" in err()
    assert call(ok(out=None)) == 1
    assert call(ok(n_te=2)) == 1 and call(ok(n_te=-1)) == 1
    assert call(ok(ws_bytes=need - 1)) == 1 and b"workspace" in err()
    assert call(ok(n=1 << 30)) == 4


def rows_of(ks, f50, **cols):
    return [{"k": k, "frac50": f, "frac75": f / 2, "frac100": f / 4, "n_edges": 100 * k, "efficiency": 0.1 * k,
             "purity": 1 / k, **{c: v[i] for c, v in cols.items()}} for i, (k, f) in enumerate(zip(ks, f50))]


def test_kscan_results_two_three_and_nine_ks():
    # two points: a line
    r = KScanResults(rows_of([2, 6], [0.2, 0.6]), targets=(0.4, 0.7)).get_foms()
    assert r["k_at_segment50_40"] == pytest.approx(4.0, abs=1e-12)
    assert r["n_edges_frac_segment50_40"] == pytest.approx(400.0, abs=1e-9)
    assert np.isnan(r["k_at_segment50_70"]) and np.isnan(r["n_edges_frac_segment50_70"])   # above the maximum
    assert r["max_frac_segment50"] == 0.6 and r["k_at_max_frac_segment50"] == 6.0
    # three points: the parabola through them
    ks, f = [1, 2, 4], [0.1, 0.4, 0.8]
    res = KScanResults(rows_of(ks, f), targets=(0.5,))
    p = np.polyfit(ks, f, 2)
    k = res.get_foms()["k_at_segment50_50"]
    assert abs(np.polyval(p, k) - 0.5) < 1e-12 and 2 < k < 4
    # nine points of a cubic: a not-a-knot spline reproduces a cubic
    ks = list(range(1, 10))
    cubic = lambda k: 0.05 + 0.2 * k - 0.02 * k ** 2 + 0.0008 * k ** 3   # noqa: E731
    res = KScanResults(rows_of(ks, [cubic(k) for k in ks]), targets=(0.5, 0.1))
    foms = res.get_foms()
    assert abs(cubic(foms["k_at_segment50_50"]) - 0.5) < 1e-12
    assert list(foms)[:6] == ["n_edges_frac_segment50_50", "k_at_segment50_50", "frac75_at_segment50_50",
                              "frac100_at_segment50_50", "efficiency_at_segment50_50", "purity_at_segment50_50"]
    assert list(foms)[-7:] == ["max_frac_segment50", "n_edges_max_frac_segment50", "k_at_max_frac_segment50",
                               "frac75_at_max_frac_segment50", "frac100_at_max_frac_segment50",
                               "efficiency_at_max_frac_segment50", "purity_at_max_frac_segment50"]
    # a target below frac50(k_min): no crossing, the end point
    assert foms["k_at_segment50_10"] == 1.0 and foms["n_edges_frac_segment50_10"] == pytest.approx(100.0)
    # one k: NaN at every target, the max block from the row
    one = KScanResults(rows_of([3], [0.5]), targets=(0.4,)).get_foms()
    assert np.isnan(one["k_at_segment50_40"]) and one["max_frac_segment50"] == 0.5


def test_kscan_results_nan_column_and_first_maximum():
    ks = [1, 2, 3, 4]
    rows = rows_of(ks, [0.2, 0.7, 0.7, 0.6], max_fake_lhc_pt0_9=[0.1, float("nan"), 0.2, 0.3])
    res = KScanResults(rows, targets=(0.5,))
    at = res._eval_spline(1.5)
    assert np.isnan(at["max_fake_lhc_pt0_9"]) and np.isfinite(at["n_edges"])
    foms = res.get_foms()
    assert foms["k_at_max_frac_segment50"] == 2.0   # the first row attaining the maximum
    assert 1 < foms["k_at_segment50_50"] < 2


def test_scanner_bookkeeping():
    s = GraphConstructionKNNScanner(ks=[2, 1], subsample_pids=5)
    assert list(s.hparams) == ["ks", "targets", "max_radius", "pt_thld", "max_eta", "subsample_pids", "max_edges"]
    s._results = [{"k": 2, "frac50": 0.5, "v": float("nan")}, {"k": 1, "frac50": 0.25, "v": 1.0},
                  {"k": 2, "frac50": 1.0, "v": 3.0}]
    res = s.get_results()
    assert [r["k"] for r in res.rows] == [1, 2] and res.rows[1]["frac50"] == 0.75 and res.rows[1]["v"] == 3.0
    s.reset()
    assert s.results_raw == []
