"""The k-scan of the metric-learning validation on the device: every G18 case exactly, a 200 k-hit event
against the numpy restatement on the same neighbour table (labels and counts exact, computed twice), the
scanner over three batches, and ``MLModule.validation_step`` in fp32 and bf16 storage."""

import numpy as np
import pytest
import torch

import kscan_ref as R
from test_kscan_cpu import CASES, assert_foms, assert_records, golden_foms, golden_records, scan
from test_tracking_metrics_gpu import pileup_event
from gnn_tracking_amd import (Data, GraphConstructionFCNN, GraphConstructionHingeEmbeddingLoss,
                              GraphConstructionKNNScanner, _capi, bf16_storage, ops)
from gnn_tracking_amd import k_scanner as KS
from gnn_tracking_amd.graph_masks import get_good_node_mask
from gnn_tracking_amd.training import MLModule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_on_the_device(dev, name):
    scanner = scan(name, dev)
    assert_records(scanner.results_raw, golden_records(name), name)
    assert_foms(scanner.get_foms(), golden_foms(name), name)


def chain_event(seed, n, dim=8, n_particles=6000):
    """``pileup_event``'s hits with every particle laid out as a short chain instead of a blob: its hits
    are spread along a random direction through the particle's centre (step 0.03), so that small k joins
    neighbours along the chain only.  True edges: consecutive hits of a chain, both directions."""
    x, pid, pt, eta, reco = pileup_event(seed, n, dim=dim, n_particles=n_particles, sigma=0.01)
    g = np.random.default_rng(seed + 1)
    order = np.argsort(pid, kind="stable")
    sp = pid[order]
    start = np.flatnonzero(np.r_[True, sp[1:] != sp[:-1]])
    rank = np.arange(n) - np.repeat(start, np.diff(np.r_[start, n]))
    direction = g.normal(size=(n_particles + 1, dim))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    real = sp > 0
    x = x.copy()
    x[order[real]] += (0.03 * rank[real, None] * direction[sp[real] >> 40]).astype(np.float32)
    nxt = np.flatnonzero(real[:-1] & (sp[1:] == sp[:-1]))
    a, b = order[nxt], order[nxt + 1]
    te = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    return x, pid, pt, eta, reco, te


def data_on(dev, x, pid, pt, eta, reco, te):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return Data(x=t(x), particle_id=t(pid), pt=t(pt), eta=t(eta), reconstructable=t(reco), true_edge_index=t(te))


def neighbour_table(d, kmax):
    n = int(d.x.shape[0])
    nbr = torch.empty(n * kmax, dtype=torch.int32, device=d.x.device)
    cnt = torch.empty(n, dtype=torch.int32, device=d.x.device)
    ops._knn_search(_capi.load(), d.x, kmax, 1.0, None, nbr, cnt, ops._stream(d.x))
    return nbr, cnt


def test_200k_event_labels_and_counts_exact_and_repeatable(dev):
    ev = chain_event(18, 200_000)
    x, pid, pt, eta, reco, te = ev
    ks, kmax, n = list(range(1, 10)), 9, len(pid)
    d = data_on(dev, *ev)
    nbr, cnt = neighbour_table(d, kmax)
    mask = get_good_node_mask(d)
    c1, l1 = KS.kscan_counts(nbr, cnt, kmax, ks, d.particle_id, mask, d.true_edge_index)
    c2, l2 = KS.kscan_counts(nbr, cnt, kmax, ks, d.particle_id, mask, d.true_edge_index)
    assert torch.equal(c1, c2) and torch.equal(l1, l2), "the result depends on the order of the atomics"
    print("200k counts:\n", c1.cpu().numpy())
    assert np.array_equal(mask.cpu().numpy(), R.good_node_mask(pid, pt, eta, reco))
    want_c, want_l = R.scan_table(nbr.cpu().numpy().reshape(n, kmax), cnt.cpu().numpy(), ks, pid,
                                  mask.cpu().numpy(), te)
    assert np.array_equal(c1.cpu().numpy(), want_c)
    assert np.array_equal(l1.cpu().numpy(), want_l)
    assert want_c[:, 4].min() > 1000 and want_c[0, 5] < want_c[-1, 5]   # (a scan that has something to find)
    # the scanner's records of this batch come from the same counts
    scanner = GraphConstructionKNNScanner(ks=ks)
    scanner(d, 0)
    assert_records(scanner.results_raw, R.records(want_c, want_l, ks, pid, pt, eta, reco), "200k")


def test_scanner_three_batches_foms(dev):
    ks, targets = [1, 2, 3, 4, 6, 8], (0.5, 0.7, 0.8)
    scanner = GraphConstructionKNNScanner(ks=ks, targets=targets)
    recs = []
    for i in range(3):
        ev = chain_event(30 + i, 20_000, n_particles=600)
        x, pid, pt, eta, reco, te = ev
        d = data_on(dev, *ev)
        scanner(d, i)
        nbr, cnt = neighbour_table(d, max(ks))
        mask = R.good_node_mask(pid, pt, eta, reco)
        c, lab = R.scan_table(nbr.cpu().numpy().reshape(len(pid), max(ks)), cnt.cpu().numpy(), ks, pid, mask, te)
        recs += R.records(c, lab, ks, pid, pt, eta, reco)
    assert_records(scanner.results_raw, recs, "three batches")
    print("three batches frac50:", [r["frac50"] for r in R.mean_rows(recs)])
    # (both sides are this repository's own deterministic root finders on the same spline, built from
    #  identical rows: fp64 rounding of two spline solves, 1e-9 relative)
    assert_foms(scanner.get_foms(), R.foms(R.mean_rows(recs), targets), "three batches", rtol=1e-9)


@pytest.mark.parametrize("bf16", [False, True])
def test_ml_module_validation_step(dev, bf16):
    torch.manual_seed(5)
    model = GraphConstructionFCNN(in_dim=8, hidden_dim=64, out_dim=8, depth=3).to(dev)
    ks, targets = [1, 2, 3, 5], (0.5, 0.8)
    step = MLModule(model, loss_fct=GraphConstructionHingeEmbeddingLoss(max_num_neighbors=16),
                    gc_scanner=GraphConstructionKNNScanner(ks=ks, targets=targets), bf16=bf16)
    assert step.highlight_metric("n_edges_frac_segment50_95") and step.highlight_metric("max_frac_segment50")
    assert not step.highlight_metric("trk.lhc_pt0.9")
    by_hand = GraphConstructionKNNScanner(ks=ks, targets=targets)
    for i in range(2):
        d = data_on(dev, *chain_event(40 + i, 5000, n_particles=150))
        m = step.validation_step(d, i, last_batch=i == 1)
        with torch.no_grad(), bf16_storage(bf16):
            h = model(d)["H"]
        by_hand(d, i, latent=h)
        fom_keys = list(by_hand.get_foms())
        losses = [k for k in m if k not in fom_keys]
        assert "total" in losses and all(np.isfinite(float(m[k])) for k in losses)
        if i == 0:
            assert list(m) == losses   # the figures of merit come with the last batch only
    foms = by_hand.get_foms()
    assert list(m) == losses + list(foms)
    for k, v in foms.items():
        assert m[k] == v or (m[k] != m[k] and v != v), k
