"""Clustering scores, ``common_metrics`` and the hits-per-cluster histogram on the GPU: the reference's golden
values (G21), random events with every spectrum compared with ``==`` against the numpy restatement, a
labelling with half the hits in cluster -1, and the input forms of ``clustering_spectra``."""

import numpy as np
import pytest
import torch

import cluster_scores_ref as R
import gnn_tracking_amd as G
from cluster_scores_cases import (G21, NAMES, SCORE_KEYS, assert_hist, assert_scores, assert_spectra, case,
                                  golden_flat, golden_scores, random_case)
from gnn_tracking_amd import _capi
from gnn_tracking_amd import cluster_metrics as CM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _capi.load().gnntrk_version() == 600
    return torch.device("cuda")


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(dev, name):
    truth, predicted = case(name)
    t, p = torch.from_numpy(truth).to(dev), torch.from_numpy(predicted).to(dev)
    got = G.clustering_scores_trials(p, truth=t)
    assert len(got) == 1
    assert_scores(got[0], golden_scores(name), truth, predicted, name)
    # numpy inputs are copied to the device; the registry gives the same values one by one
    assert G.clustering_scores_trials(predicted, truth=truth) == got
    assert {k: G.common_metrics[k](truth=t, predicted=p, pts=None) for k in SCORE_KEYS} == got[0]
    hist = G.count_hits_per_cluster(p)
    assert_hist(hist, G21[f"{name}/hist"], name)
    flat = G.hits_per_cluster_count_to_flat_dict(hist)
    assert list(flat) == list(golden_flat(name)) and [float(v) for v in flat.values()] == list(golden_flat(name).values())


def test_common_metrics_trk_is_the_flattened_tracking_metrics(dev):
    truth, predicted = case("blobs")
    n = len(truth)
    g = np.random.default_rng(2)
    hits = dict(pts=g.random(n).astype(np.float32) * 2, reconstructable=np.ones(n, np.float32),
                eta=g.normal(0, 2, n).astype(np.float32), pt_thlds=[0.0, 0.9])
    assert list(G.common_metrics) == ["v_measure", "homogeneity", "completeness", "trk", "adjusted_rand",
                                      "fowlkes_mallows"]
    trk = G.common_metrics["trk"](truth=truth, predicted=predicted, **hits, something_else=1)
    want = G.flatten_track_metrics(G.tracking_metrics(truth=truth, predicted=predicted, **hits))
    assert list(trk) == list(want) and len(trk) == 16 and trk["n_particles"] > 0
    assert all(trk[k] == want[k] or (trk[k] != trk[k] and want[k] != want[k]) for k in want)


# 3000 hits: several workgroups, contended tables.  150 000 hits x 4 trials = 600 000 label slots: the hit
# kernel's grid-stride loop wraps (256 CUs x 8 workgroups x 256 threads = 524 288).
@pytest.mark.parametrize("n", [3000, 150_000])
def test_random_event_spectra_exact(dev, n):
    g = np.random.default_rng(n + 2)
    truth, labels = random_case(g, n, 4)
    got = CM.clustering_spectra(torch.from_numpy(labels).to(dev), torch.from_numpy(truth).to(dev))
    scores = CM.clustering_scores_trials(torch.from_numpy(labels).to(dev), truth=torch.from_numpy(truth).to(dev))
    assert len(got) == 4 and len(scores) == 4
    for t in range(4):
        assert_spectra(got[t], R.spectra(labels[t], truth), n, f"n = {n}, trial {t}")
        assert_scores(scores[t], R.scores(truth, labels[t]), truth, labels[t], f"n = {n}, trial {t}")
    assert all(np.array_equal(got[t]["classes"][0], got[0]["classes"][0]) for t in range(4))


def test_half_the_hits_in_the_noise_cluster(dev):
    """Cluster -1 holds 75 000 of 150 000 hits: a size beyond the histogram bins, and a hot slot."""
    n = 150_000
    g = np.random.default_rng(9)
    truth, labels = random_case(g, n, 2)
    labels[0, labels[0] == -1] = -2
    labels[0, g.permutation(n)[: n // 2]] = -1
    assert int((labels[0] == -1).sum()) == n // 2
    got = CM.clustering_spectra(torch.from_numpy(labels).to(dev), torch.from_numpy(truth).to(dev))
    assert got[0]["clusters"][0][-1] == 75_000 and got[0]["clusters"][1][-1] == 1
    for t in range(2):
        assert_spectra(got[t], R.spectra(labels[t], truth), n, f"trial {t}")
    scores = CM.clustering_scores_trials(torch.from_numpy(labels[0]).to(dev), truth=torch.from_numpy(truth).to(dev))
    assert_scores(scores[0], R.scores(truth, labels[0]), truth, labels[0], "half noise")
    hist = CM.count_hits_per_cluster(torch.from_numpy(labels[0]).to(dev))
    assert len(hist) == 75_000 and hist[-1] == 1
    assert_hist(hist, R.count_hits_per_cluster(labels[0]), "half noise")


def test_input_forms(dev):
    """[n] and [T, n] labels, device tensors and numpy arrays, with and without truth."""
    g = np.random.default_rng(4)
    n = 3000
    truth, labels = random_case(g, n, 3)
    lab_d, truth_d = torch.from_numpy(labels).to(dev), torch.from_numpy(truth).to(dev)
    many = CM.clustering_spectra(lab_d, truth_d)
    assert len(many) == 3
    for t in range(3):
        one = CM.clustering_spectra(lab_d[t], truth_d)
        assert len(one) == 1
        assert_spectra(one[0], many[t], n, f"[n] input, trial {t}")
    assert_spectra(CM.clustering_spectra(labels[1], truth)[0], many[1], n, "numpy input")
    alone = CM.clustering_spectra(lab_d)
    for t in range(3):
        assert_spectra(alone[t], R.spectra(labels[t]), n, f"no truth, trial {t}")
        assert alone[t]["classes"][0].size == 0 and alone[t]["cells"][0].size == 0
        assert np.array_equal(alone[t]["clusters"][0], many[t]["clusters"][0])
    # a strided view is made contiguous
    assert_spectra(CM.clustering_spectra(lab_d.t().contiguous().t()[2], truth_d)[0], many[2], n, "strided input")
