"""Edge-classifier validation metrics on the MI355X (csrc/metrics.hip through gnn_tracking_amd.metrics):
the reference's golden values, a cfg3-size batch (32 synthetic events, 64 M edges) against host
bincounts and the float64 restatement, the EdgeOrdered fast path, and ECModule.validation_step."""

import numpy as np
import pytest
import torch

import ec_metrics_ref as R
import gnn_tracking_amd as G
from gnn_tracking_amd import metrics as M
from gnn_tracking_amd import _capi, ops
from gnn_tracking_amd.training import ECModule

pytestmark = pytest.mark.gpu

GOLD = np.load(__import__("pathlib").Path(__file__).resolve().parent / "golden" / "g16_ec_metrics.npz")
CASES = ("g1", "ties", "saturated", "nanscore", "nopos", "empty")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _capi.load().gnntrk_version() == 600
    return torch.device("cuda")


def golden(name):
    return dict(zip([str(k) for k in GOLD[f"{name}/keys"]], GOLD[f"{name}/values"].tolist()))


def assert_metrics(got: dict, want: dict, what: str, auc_tol=1e-12, tol=0.0):
    assert list(got) == list(want), f"{what}: keys {list(got)} vs {list(want)}"
    for k, v in want.items():
        tl = max(tol, auc_tol) if k.startswith("roc_auc") else tol
        assert R.same_value(float(got[k]), float(v), tl), f"{what}: {k} = {got[k]!r}, want {v!r}"


def same_dict(a: dict, b: dict) -> bool:
    return list(a) == list(b) and all(R.same_value(float(a[k]), float(b[k])) for k in a)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(dev, name):
    w, y, pt, ei = (torch.from_numpy(GOLD[f"{name}/{k}"]).to(dev) for k in ("w", "y", "pt", "edge_index"))
    gold = golden(name)
    assert_metrics(M.ec_validation_metrics(w, y, pt, ei), gold, name)
    # fp32 labels take the same path
    assert_metrics(M.ec_validation_metrics(w, y.float(), pt, ei), gold, name + " (fp32 labels)")
    full = M.get_roc_auc_scores(y, w, [None, 0.01, 0.001]) | M.get_maximized_bcs(output=w, y=y)
    assert_metrics(full, {k: v for k, v in gold.items() if "_pt" not in k}, name + " (no cut)")
    for th, row in zip(GOLD["bcs_thlds"], GOLD[f"{name}/bcs_values"]):
        got = M.BinaryClassificationStats(w, y, float(th)).get_all()
        assert [float(v) for v in got.values()] == row.tolist(), f"{name}: BinaryClassificationStats({th})"


def _cfg3_batch(dev):
    from gnn_tracking_amd import synthetic

    return G.collate([synthetic.make_event(300 + i, 150_000, 2_000_000, dev) for i in range(32)])


@pytest.mark.parametrize("dist", ["saturated", "uniform"])
def test_cfg3_batch_exact(dev, dist):
    """64 M edges: count tables equal host bincounts exactly, AUCs within 1e-12 of the float64
    restatement, all 44 keys."""
    batch = _cfg3_batch(dev)
    E = batch.edge_index.shape[1]
    assert E == 64_000_000
    gen = torch.Generator(device=dev).manual_seed(7)
    if dist == "uniform":
        w = torch.rand(E, generator=gen, device=dev)
    else:
        good = torch.rand(E, generator=gen, device=dev) < 0.95
        w = torch.where(good == batch.y, torch.tensor(0.999, device=dev), torch.tensor(0.001, device=dev))
    cuts = list(R.PT_THLDS)
    thr = torch.linspace(0.0, 1.0, 200)
    e = M._Edges(w, batch.y, batch.pt, batch.edge_index)
    counts = torch.empty(len(cuts) * 2 * 201, dtype=torch.int64, device=dev)
    M._launch_counts(e, cuts, thr.to(dev), counts)
    auc = torch.empty(len(cuts) * _capi.AUC_STRIDE, dtype=torch.int64, device=dev)
    M._launch_auc(e, cuts, [0.01, 0.001], auc)
    metrics = M.ec_validation_metrics(w, batch.y, batch.pt, batch.edge_index)
    assert len(metrics) == 44
    wn, yn = w.cpu().numpy(), batch.y.cpu().numpy()
    ptn, ein = batch.pt.cpu().numpy(), batch.edge_index.cpu().numpy()
    want = R.counts_table(wn, yn, ptn, ein, cuts, thr.numpy())
    assert np.array_equal(counts.cpu().numpy().reshape(want.shape), want), "count tables differ from np.bincount"
    auc = auc.cpu().numpy().reshape(len(cuts), -1)
    for c, cut in enumerate(cuts):
        m = R.cut_mask(ptn, ein, cut)
        ref = R.roc_aucs(yn[m], wn[m], [None, 0.01, 0.001])
        got = M._auc_from_row(auc[c], [0.01, 0.001])
        sfx = R.denote_pt("", cut)
        assert [metrics[f"roc_auc{sfx}"], metrics[f"roc_auc_0.01FPR{sfx}"], metrics[f"roc_auc_0.001FPR{sfx}"]] == got
        for a, b in zip(got, ref):
            assert abs(a - b) <= 1e-12, (dist, cut, got, ref)


@pytest.mark.parametrize("order", [False, True])
def test_edge_ordered_fast_path(dev, order):
    """ECForGraphTCN's CSR-held W: bit-identical to the plain tensor W.in_edge_index_order(), and W is
    never materialised (with and without the node renumbering, which moves pt into the new numbering)."""
    from gnn_tracking_amd import synthetic
    from gnn_tracking_amd.edge_order import EdgeOrdered

    ev = synthetic.make_event(11, 20_000, 300_000, dev)
    torch.manual_seed(0)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40).to(dev)
    ops.clear_graph_index_cache()
    with torch.no_grad(), G.node_order(1 if order else "off"):
        w = model(ev)["W"]
    assert isinstance(w, EdgeOrdered)
    assert (w.graph_index.node_perm is not None) == order
    fast = M.ec_validation_metrics(w, ev.y, ev.pt, ev.edge_index)
    assert w._coo is None, "the metrics materialised W"
    plain = M.ec_validation_metrics(w.in_edge_index_order().clone(), ev.y, ev.pt, ev.edge_index)
    assert same_dict(fast, plain), (fast, plain)
    ref = R.ec_metrics(w.in_edge_index_order().cpu().numpy(), ev.y.cpu().numpy(), ev.pt.cpu().numpy(),
                       ev.edge_index.cpu().numpy())
    assert_metrics(fast, ref, "fast path vs restatement")


@pytest.mark.parametrize("bf16", [False, True])
def test_validation_step_g1(dev, bf16):
    """ECModule.validation_step on the reference's test graph: the golden's 45 keys; values of the golden
    (fp32), of the restatement applied to the run's own W (bf16 storage)."""
    z = np.load(__import__("pathlib").Path(__file__).resolve().parent / "golden" / "g1_ec_testgraph.npz")
    torch.manual_seed(0)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=14, L_ec=1)
    model.load_state_dict({k: torch.from_numpy(z["p0/" + k]) for k in model.state_dict()})
    model = model.to(dev).eval()
    data = G.Data(**{k: torch.from_numpy(z[k]).to(dev) for k in ("x", "edge_index", "edge_attr", "y", "pt")})
    step = ECModule(model, loss_fct=G.EdgeWeightBCELoss(), bf16=bf16)
    got = step.validation_step(data, 0)
    want = {"total": float(GOLD["g1/total"]), **golden("g1")}
    assert list(got) == list(want) and len(got) == 45
    assert step.highlight_metric("max_mcc_pt0.9") and not step.highlight_metric("max_mcc")
    with torch.no_grad(), G.bf16_storage(bf16):
        w_own = torch.as_tensor(model(data)["W"]).cpu().numpy()
    own = R.ec_metrics(w_own, z["y"], z["pt"], z["edge_index"])
    assert_metrics({k: v for k, v in got.items() if k != "total"}, own, "validation_step vs restatement(own W)")
    if bf16:
        assert abs(got["total"] - want["total"]) <= 5e-3
    else:
        assert abs(got["total"] - want["total"]) <= 1e-5
        assert_metrics(got, want, "validation_step vs golden", tol=1e-5)
