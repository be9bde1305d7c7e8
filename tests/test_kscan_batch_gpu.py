"""The k-scan on a collated batch on the GPU: every case of tests/kscan_batch_cases.py against the single-event
restatement applied per event (exact: tables, labels, records, figures of merit), ``MLModule.validation_step`` on
``collate([...])``, and a batch above the pruned neighbour search's threshold."""

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
import kscan_batch_cases as C
import kscan_ref as R
from gnn_tracking_amd import (GraphConstructionFCNN, GraphConstructionHingeEmbeddingLoss, GraphConstructionKNNScanner,
                              _capi, ops)
from gnn_tracking_amd import k_scanner as KS
from gnn_tracking_amd.graph_masks import get_good_node_mask
from gnn_tracking_amd.training import MLModule
from test_kscan_gpu import chain_event

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


def test_random_tables_per_event():
    C.case_random_tables(DEVICE)


def test_cross_event_entries_are_bad_and_join_nothing():
    C.case_cross_event_entries(DEVICE)


def test_many_small_events():
    C.case_many_small_events(DEVICE)


def test_scanner_on_a_collated_batch():
    C.case_scanner_batch(DEVICE)


def test_scanner_one_event_is_todays_call():
    C.case_scanner_one_event(DEVICE)


def test_scanner_max_edges_stops_one_event(caplog):
    C.case_scanner_max_edges(DEVICE, caplog)


def test_scanner_skips_a_one_hit_event():
    C.case_scanner_small_event(DEVICE)


def test_scanner_refuses_a_true_edge_across_events():
    C.case_scanner_refuses_cross_event_true_edge(DEVICE)


def test_ml_validation_step_on_a_collated_batch():
    """the figures of merit of one step on ``collate([...])`` are those of single-event steps accumulated in the same
    scanner (the model works row by row: an event's latent rows are the same either way)"""
    torch.manual_seed(5)
    model = GraphConstructionFCNN(in_dim=8, hidden_dim=64, out_dim=8, depth=3).to(DEVICE)
    ks, targets = [1, 2, 3, 5], (0.5, 0.8)

    def module():
        return MLModule(model, loss_fct=GraphConstructionHingeEmbeddingLoss(max_num_neighbors=16),
                        gc_scanner=GraphConstructionKNNScanner(ks=ks, targets=targets))

    events = [C.data_of(raw, DEVICE) for raw in C.scan_events()]
    alone = module()
    for i, d in enumerate(events):
        want = alone.validation_step(d, i, last_batch=i == len(events) - 1)
    batched = module()
    got = batched.validation_step(G.collate(events), 0, last_batch=True)
    C.records_equal(batched.gc_scanner.results_raw, alone.gc_scanner.results_raw, "validation_step: records")
    assert len(batched.gc_scanner.results_raw) == len(events) * len(ks)
    foms = list(alone.gc_scanner.get_foms())
    assert foms and all(k in got for k in foms) and any(np.isfinite(float(want[k])) for k in foms)
    C.assert_same({k: got[k] for k in foms}, {k: want[k] for k in foms}, "validation_step: figures of merit")
    assert all(np.isfinite(float(v)) for k, v in got.items() if k not in foms)


def test_batch_above_the_pruned_search_threshold_exact_and_repeatable():
    """three events, 8 400 rows in 8 dimensions: the neighbour table of the batched (pruned) search, counts and labels of
    every event against the restatement on that event's slice of the table, computed twice"""
    sizes = (3000, 2900, 2500)
    assert sum(sizes) >= 8192
    raws = [chain_event(1820 + i, n, n_particles=n // 12) for i, n in enumerate(sizes)]
    data = G.collate([C.data_of(raw, DEVICE) for raw in raws])
    ks, kmax, n = list(range(1, 10)), 9, sum(sizes)
    nbr = torch.empty(n * kmax, dtype=torch.int32, device=DEVICE)
    cnt = torch.empty(n, dtype=torch.int32, device=DEVICE)
    ops._knn_search(_capi.load(), data.x, kmax, 1.0, data.ptr, nbr, cnt, ops._stream(data.x))
    mask = get_good_node_mask(data)
    args = (nbr, cnt, kmax, ks, data.particle_id, mask, data.true_edge_index)
    c1, l1 = KS.kscan_counts(*args, ptr=data.ptr)
    c2, l2 = KS.kscan_counts(*args, ptr=data.ptr)
    assert torch.equal(c1, c2) and torch.equal(l1, l2), "the result depends on the order of the atomics"
    nbr_h, cnt_h = nbr.cpu().numpy().reshape(n, kmax), cnt.cpu().numpy()
    want = C.scan_oracle(nbr_h, cnt_h, ks, data.particle_id.cpu().numpy(), mask.cpu().numpy().astype(bool),
                         data.true_edge_index.cpu().numpy(), sizes)
    print("pruned batch counts:\n", c1.cpu().numpy())
    assert (want[0][:, 0, R.COLUMNS.index("n50")] < want[0][:, -1, R.COLUMNS.index("n50")]).all()
    assert (want[0][:, :, C.N_PIDS] > 20).all()
    C.assert_events_equal((c1.cpu().numpy(), l1.cpu().numpy()), want, sizes, "pruned batch")
