"""Binned tracking metrics, the cluster table and DBSCANPerformanceDetails on the GPU: the reference's
golden values (G20), random events with 32 random windows against the numpy restatement, the scanner
over the three golden batches and ``TCModule.validation_step`` with it."""

import ctypes

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
import tracking_binned_ref as B
from gnn_tracking_amd import _capi, ops
from gnn_tracking_amd import cluster_metrics as CM
from gnn_tracking_amd.postprocessing import DBSCANPerformanceDetails
from gnn_tracking_amd.training import TCModule
from tracking_binned_cases import (BINNED, G20, MULTI, TABLES, assert_rows, assert_table, batch, golden_rows,
                                   golden_table, hit_record, random_event, random_windows, scan_batch)

pytestmark = pytest.mark.gpu

PT_EDGES, ETA_EDGES = G20["pt_edges"].tolist(), G20["eta_edges"].tolist()
MAX_ETA, PT_THLD = float(G20["max_eta"]), float(G20["pt_thld"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _capi.load().gnntrk_version() == 600
    return torch.device("cuda")


def records(names, dev):
    """The cases' hit records as device tensors and as numpy arrays."""
    on = [hit_record(batch(n), lambda a: torch.from_numpy(np.asarray(a)).to(dev)) for n in names]
    return on, [hit_record(batch(n)) for n in names]


@pytest.mark.parametrize("name", BINNED)
def test_binned_golden_cases(dev, name):
    for h, how in zip(records([name], dev), ("device", "numpy")):
        vp = CM.tracking_metrics_vs_pt(h, [None], PT_EDGES, max_eta=MAX_ETA)
        ve = CM.tracking_metrics_vs_eta(h, [None], ETA_EDGES, pt_thld=PT_THLD)
        assert_rows(vp, golden_rows(f"single/{name}/", "vs_pt"), f"{name} ({how})")
        assert_rows(ve, golden_rows(f"single/{name}/", "vs_eta"), f"{name} ({how})")


def test_multi_batch_golden(dev):
    for h, how in zip(records(MULTI, dev), ("device", "numpy")):
        vp = CM.tracking_metrics_vs_pt(h, [None] * 3, PT_EDGES, max_eta=MAX_ETA)
        ve = CM.tracking_metrics_vs_eta(h, [None] * 3, ETA_EDGES, pt_thld=PT_THLD)
        assert_rows(vp, golden_rows("multi/", "vs_pt"), f"multi ({how})")
        assert_rows(ve, golden_rows("multi/", "vs_eta"), f"multi ({how})")


@pytest.mark.parametrize("name", TABLES)
def test_table_golden_cases(dev, name):
    b = batch(name)
    t = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in b.items()}
    got = CM.tracking_metric_table(t["labels"], truth=t["pid"], pts=t["pt"], reconstructable=t["reco"], eta=t["eta"])
    assert_table(got, golden_table(f"table/{name}/"), name, dtypes=True)
    got_np = CM.tracking_metric_table(b["labels"], truth=b["pid"], pts=b["pt"], reconstructable=b["reco"],
                                      eta=b["eta"])
    assert_table(got_np, golden_table(f"table/{name}/"), name + " (numpy)", dtypes=True)


def windows_on_device(dev, labels, pid, pt, eta, reco, win, thld=3):
    lib = _capi.load()
    n_trials, n = labels.shape
    lab, p, a, e, r = (torch.from_numpy(x).to(dev) for x in (labels, pid, pt, eta, reco))
    nw = len(win)
    out = torch.full((nw + n_trials * nw * 4 + 1,), -1, dtype=torch.int64, device=dev)
    ws = ops._ws(lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, n_trials), lab)
    q = ops._p
    _capi.check(lib.gnntrk_tracking_metrics_windows(q(lab), n_trials, q(p), q(a), q(e), q(r), n,
                                                    win.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nw, thld,
                                                    q(out), q(ws), ws.numel(), ops._stream(lab)), lib)
    host = out.cpu().numpy()
    assert host[-1] == 0
    return host[:nw], host[nw:-1].reshape(n_trials, nw, 4)


# 3000 hits: several workgroups, contended tables.  150 000 hits x 4 trials = 600 000 label slots: the
# pair kernels' grid-stride loops wrap (256 CUs x 8 workgroups x 256 threads = 524 288).
@pytest.mark.parametrize("n", [3000, 150_000])
def test_random_event_windows_exact(dev, n):
    g = np.random.default_rng(n + 1)
    pid, pt, eta, reco = random_event(g, n, n // 12, True)
    labels = g.integers(-3, n // 8, size=(4, n)).astype(np.int64)
    win = random_windows(g)
    n_part, counts = windows_on_device(dev, labels, pid, pt, eta, reco, win)
    assert counts[:, :, 0].sum() > 0 and n_part.sum() > 0
    for t in range(4):
        want_part, want = B.window_counts(labels[t], pid, pt, eta, reco, win)
        assert np.array_equal(n_part, want_part), f"trial {t}"
        assert np.array_equal(counts[t], want), f"trial {t}"
    # the table of the first labelling
    got = CM.tracking_metric_table(labels[0], truth=pid, pts=pt, reconstructable=reco, eta=eta)
    assert_table(got, B.cluster_table(labels[0], pid, pt, eta, reco), f"table n={n}", dtypes=True,
                 exact_means=True)


def scan_data(i, dev):
    b = scan_batch(i)
    t = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    return G.Data(particle_id=t["pid"], pt=t["pt"], eta=t["eta"], reconstructable=t["reco"]), {"H": t["H"]}, b


def test_scanner_three_batches_match_golden(dev):
    scanner = DBSCANPerformanceDetails(eps=float(G20["scan/eps"]), min_samples=int(G20["scan/min_samples"]))
    assert scanner.hparams.eps == 0.2 and scanner.hparams.min_samples == 3
    for i in range(3):
        data, out, b = scan_data(i, dev)
        scanner(data, out | {"ec_hit_mask": torch.zeros(len(b["pid"]), dtype=torch.bool, device=dev)}, 0)
    h_dfs, c_dfs = scanner.get_results()
    assert len(h_dfs) == 3 and len(c_dfs) == 3 and scanner.get_foms() == {}   # (no reset on i_batch == 0)
    for i in range(3):
        assert list(h_dfs[i]) == ["c", "id", "reconstructable", "pt", "eta"]
        assert all(v.is_cuda for v in h_dfs[i].values())
        assert np.array_equal(h_dfs[i]["c"].cpu().numpy(), scan_batch(i)["labels"])
        assert_table(c_dfs[i], golden_table(f"scan/b{i}/table/"), f"scan b{i}", dtypes=True)
    assert_rows(CM.tracking_metrics_vs_pt(h_dfs, c_dfs, PT_EDGES, max_eta=MAX_ETA), golden_rows("scan/", "vs_pt"),
                "scan")
    assert_rows(CM.tracking_metrics_vs_eta(h_dfs, c_dfs, ETA_EDGES, pt_thld=PT_THLD), golden_rows("scan/", "vs_eta"),
                "scan")


def test_tc_validation_step_with_the_scanner(dev):
    from gnn_tracking_amd import synthetic

    torch.manual_seed(0)
    data = synthetic.make_event(5, 3000, 12000, dev)
    data.particle_id = (torch.arange(3000, device=dev) // 8) * 2 ** 40
    model = G.GraphTCN(14, 4, h_outdim=3, hidden_dim=40, L_ec=2, L_hc=2).to(dev)
    scanner = DBSCANPerformanceDetails(eps=0.3, min_samples=2)
    plain = TCModule(model, loss_fct=G.CondensationLossRG())
    module = TCModule(model, loss_fct=G.CondensationLossRG(), cluster_scanner=scanner)
    want = plain.validation_step(data, 0, last_batch=True)
    got = module.validation_step(data, 0, last_batch=True)
    assert list(got) == list(want)
    assert all(float(got[k]) == float(want[k]) for k in want)
    h_dfs, c_dfs = scanner.get_results()
    assert len(h_dfs) == 1 and int(h_dfs[0]["c"].shape[0]) == 3000 and list(c_dfs[0])[0] == "c"
    rows = CM.tracking_metrics_vs_pt(h_dfs, c_dfs, [0.0, 0.9, float("inf")])
    assert len(rows) == 2 and list(rows[0])[-2:] == ["pt_min", "pt_max"]
