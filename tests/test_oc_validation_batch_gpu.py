"""Validation of a collated batch on the GPU: every case of tests/oc_validation_batch_cases.py against the single-event
oracles applied per event (exact: graphs bit for bit, labels, counts), and ``TCModule.validation_step`` on
``collate([...])`` with the model and loss settings of tests/test_tc_batch_gpu.py."""

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
import neighbor_cases as N
import oc_validation_batch_cases as C
from gnn_tracking_amd import training
from gnn_tracking_amd.postprocessing import ClusterScanner, DBSCANHyperParamScannerFixed

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("flags", N.FLAGS)
@pytest.mark.parametrize("dim", C.RADIUS_WIDTHS)
def test_radius_graph_per_event_every_width(dim, flags):
    C.case_radius_events(DEVICE, dim, flags)


def test_radius_graph_per_event_chunk_edges():
    C.case_radius_chunk_edges(DEVICE)


def test_radius_graph_per_event_above_the_pruned_threshold():
    C.case_radius_big_events(DEVICE)


@pytest.mark.parametrize("flags", N.FLAGS)
def test_colliding_events_share_no_edge(flags):
    C.case_colliding_events(DEVICE, flags)


@pytest.mark.parametrize("flags", N.FLAGS)
def test_dbscan_labels_per_event(flags):
    C.case_dbscan_events(DEVICE, flags)


@pytest.mark.parametrize("flags", N.FLAGS)
def test_one_event_takes_todays_path(flags):
    C.case_one_event_is_todays_call(DEVICE, flags)


def test_tracking_metrics_per_event():
    C.case_metrics_events(DEVICE)


def test_label_beyond_its_event_is_refused():
    C.case_metrics_bad_label(DEVICE)


def test_majority_tie_inside_the_event():
    C.case_metrics_tie(DEVICE)


def test_tracking_metrics_one_event_is_todays_call():
    C.case_metrics_one_event(DEVICE)


def test_scanner_on_a_collated_batch():
    C.case_scanner_batch(DEVICE)


def test_performance_details_on_a_collated_batch():
    C.case_performance_details_batch(DEVICE)


class _Recorder(ClusterScanner):
    """hands every call on to ``scanner`` and keeps what it was called with"""

    def __init__(self, scanner):
        super().__init__()
        self.scanner, self.calls = scanner, []

    def __call__(self, data, out, i_batch):
        self.calls.append((data, out))
        self.scanner(data, out, i_batch)

    def get_foms(self):
        return self.scanner.get_foms()


def test_tc_validation_step_on_a_collated_batch():
    """the model and loss of tests/test_tc_batch_gpu.py (14 features: the 8 latent coordinates and 6 more): finite losses,
    and the figures of merit of a scanner fed the three events alone on the same ``out["H"]`` rows"""
    torch.manual_seed(0)
    events = []
    for i, raw in enumerate(C.scan_events()):
        g = np.random.default_rng(600 + i)
        extra = torch.from_numpy(g.uniform(0, 1.5, size=(raw["x"].shape[0], 6)).astype(np.float32))
        events.append(C.scan_data(dict(raw, x=torch.cat([raw["x"], extra], dim=1)), DEVICE))
    model = G.GraphTCN(14, 28, h_outdim=8, hidden_dim=40, L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=8).to(DEVICE)
    rec = _Recorder(DBSCANHyperParamScannerFixed(list(C.SCAN_TRIALS)))
    mod = training.TCModule(model, loss_fct=G.CondensationLossRG(lw_repulsive=1.0, lw_coward=0.1, lw_noise=0.1),
                            preproc=G.MLGraphConstruction(ml=None, embedding_slice=(0, 8), max_radius=1.0,
                                                          max_num_neighbors=16),
                            cluster_scanner=rec)
    metrics = mod.validation_step(G.collate(events), 0, last_batch=True)
    losses = {k: v for k, v in metrics.items() if not (k.startswith("trk.") or k.startswith("best_dbscan"))}
    assert losses and all(np.isfinite(float(v)) for v in losses.values())
    (data, out), = rec.calls
    assert len(rec.scanner._results) == 12 and tuple(torch.diff(data.ptr).tolist()) == C.SCAN_HITS
    alone = DBSCANHyperParamScannerFixed(list(C.SCAN_TRIALS))
    s = C.starts_of(C.SCAN_HITS)
    for i, (a, b) in enumerate(zip(s, s[1:])):
        d = G.Data(**{k: getattr(data, k)[a:b] for k in ("particle_id", "pt", "eta", "reconstructable")})
        alone(d, {"H": out["H"][a:b]}, i)
    C.records_equal(rec.scanner._results, alone._results, "validation_step on a collated batch")
    foms = {k: v for k, v in metrics.items() if k not in losses}
    assert len(foms) == 68
    C.foms_equal(foms, alone.get_foms(), "validation_step: figures of merit")
