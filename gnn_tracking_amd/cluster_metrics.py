"""Tracking metrics of the object-condensation stage, computed on the device
(``metrics/cluster_metrics.py:76-259``, as ``postprocessing/dbscanscanner.py:146-187`` calls them once
per DBSCAN trial in ``TCModule``'s validation step).

The reference builds pandas frames per trial: ``value_counts`` of (cluster, particle), ``groupby``
means per particle, a merge, then masked sums per pt cut.  Here one C entry
(``gnntrk_tracking_metrics``, ``csrc/tracking_metrics.hip``) takes the labels of any number of trials
at once and returns integer counts - per cut the particles passing the hit mask, per trial and cut the
clusters passing the cluster mask and their perfect / double-majority / LHC matches.  The host reads
them in one copy and finishes with the reference's own divisions (``zero_division_gives_nan``: x / 0
is NaN).

Semantics are the reference's with pandas 2 / numpy 2 (``include/gnntrk.h``), with one fixed rule where
the reference has none: when two particles have the same number of hits in a cluster, the smallest
particle id is the cluster's majority particle (pandas leaves the choice to an unstable sort).  Cut
and ``max_eta`` comparisons are in fp32, as numpy 2 compares float32 columns with Python scalars.
"""

from __future__ import annotations

import ctypes as C
from typing import Iterable, TypedDict

import numpy as np
import torch
from torch import Tensor

from . import _capi, ops
from .metrics import denote_pt

__all__ = ["TrackingMetrics", "tracking_metrics", "tracking_metrics_data", "tracking_metrics_trials",
           "flatten_track_metrics", "denote_pt"]


class TrackingMetrics(TypedDict):
    """``metrics/cluster_metrics.py:35-65``."""

    n_particles: int
    n_cleaned_clusters: int
    perfect: float
    double_majority: float
    lhc: float
    fake_perfect: float
    fake_double_majority: float
    fake_lhc: float


# (key order as the reference's: it differs from TrackingMetrics')
_tracking_metrics_nan_results: TrackingMetrics = {
    "n_particles": 0,
    "n_cleaned_clusters": 0,
    "perfect": float("nan"),
    "lhc": float("nan"),
    "double_majority": float("nan"),
    "fake_perfect": float("nan"),
    "fake_lhc": float("nan"),
    "fake_double_majority": float("nan"),
}


def flatten_track_metrics(custom_metrics_result: dict[float, dict[str, float]]) -> dict[str, float]:
    """``cluster_metrics.py:flatten_track_metrics``: ``{pt: {k: v}}`` -> ``{k_pt: v}``."""
    return {denote_pt(k, pt): v for pt, results in custom_metrics_result.items() for k, v in results.items()}


def _zdiv(a: float, b: float) -> float:
    """``utils/math.py:zero_division_gives_nan``."""
    return float("nan") if b == 0 else a / b


def _from_counts(n_particles: int, c: np.ndarray) -> TrackingMetrics:
    """``count_tracking_metrics`` (cluster_metrics.py:163-201) from the integer counts of one trial and
    cut: ``c`` = (clusters, perfect, double majority, lhc)."""
    n_clusters, n_pm, n_dm, n_lhc = (int(v) for v in c)
    return {
        "n_particles": n_particles,
        "n_cleaned_clusters": n_clusters,
        "perfect": _zdiv(n_pm, n_particles),
        "double_majority": _zdiv(n_dm, n_particles),
        "lhc": _zdiv(n_lhc, n_clusters),
        "fake_perfect": _zdiv(n_clusters - n_pm, n_clusters),
        "fake_double_majority": _zdiv(n_clusters - n_dm, n_clusters),
        "fake_lhc": _zdiv(n_clusters - n_lhc, n_clusters),
    }


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")


def _on(x, dtype, device) -> Tensor:
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    return x.detach().to(device=device, dtype=dtype).contiguous()


def _cut_plan(pt_thlds) -> tuple[list, list[float], list[int]]:
    """The reference's cuts in its order, the ascending distinct fp32 cuts the kernel takes, and for
    every reference cut its index among them."""
    pts = list(pt_thlds)
    f32 = [float(np.float32(p)) for p in pts]
    if any(v != v for v in f32):
        raise ValueError("tracking_metrics: NaN pt threshold")
    asc = sorted(set(f32))
    if len(asc) > _capi.METRICS_MAX_CUTS:
        raise ValueError(f"tracking_metrics: at most {_capi.METRICS_MAX_CUTS} distinct pt thresholds")
    return pts, asc, [asc.index(v) for v in f32]


def _counts(labels: Tensor, truth: Tensor, pts: Tensor, reconstructable: Tensor, eta: Tensor, cuts: list[float],
            predicted_count_thld: int, max_eta: float) -> Tensor:
    """One launch sequence for all trials of ``labels`` [T, n]: the device int64 output of
    ``gnntrk_tracking_metrics`` (n_cuts + T * n_cuts * 4 + 1 values)."""
    lib = _capi.load()
    _capi.require_device(labels, truth, pts, reconstructable, eta)
    n_trials, n = int(labels.shape[0]), int(labels.shape[1])
    if n_trials > _capi.TRACKING_MAX_TRIALS:
        raise ValueError(f"tracking_metrics: at most {_capi.TRACKING_MAX_TRIALS} trials per call")
    nc = len(cuts)
    out = torch.empty(nc + n_trials * nc * 4 + 1, dtype=torch.int64, device=labels.device)
    ws = ops._ws(lib.gnntrk_tracking_metrics_workspace_bytes(n, n_trials), labels)
    p = ops._p
    _capi.check(lib.gnntrk_tracking_metrics(p(labels), n_trials, p(truth), p(pts), p(eta), p(reconstructable), n,
                                            (C.c_float * nc)(*cuts), nc, float(max_eta), int(predicted_count_thld),
                                            p(out), p(ws), ws.numel(), ops._stream(labels)), lib)
    return out


def _results(host: np.ndarray, n_trials: int, pts: list, idx: list[int]) -> list[dict[float, TrackingMetrics]]:
    nc = (host.size - 1) // (1 + 4 * n_trials)
    if host[-1] != 0:
        raise ValueError(f"tracking_metrics: {int(host[-1])} labels are >= the number of hits")
    n_part = host[:nc]
    cnt = host[nc:nc + n_trials * nc * 4].reshape(n_trials, nc, 4)
    return [{pt: _from_counts(int(n_part[j]), cnt[t, j]) for pt, j in zip(pts, idx)} for t in range(n_trials)]


def _hits(truth, pts, reconstructable, eta, device):
    return (_on(truth, torch.int64, device), _on(pts, torch.float32, device),
            _on(reconstructable, torch.float32, device), _on(eta, torch.float32, device))


def tracking_metrics(*, truth, predicted, pts, reconstructable, eta, pt_thlds: Iterable[float],
                     predicted_count_thld=3, max_eta=4) -> dict[float, TrackingMetrics]:
    """``cluster_metrics.py:204-257``: same arguments, same result.  Inputs are device tensors, or
    numpy arrays / host tensors that are copied to the device; labels may be any integers (negative =
    noise)."""
    n = int(np.shape(truth)[0]) if not torch.is_tensor(truth) else int(truth.shape[0])
    if not (np.shape(predicted)[0] if not torch.is_tensor(predicted) else predicted.shape[0]) == n:
        raise ValueError("tracking_metrics: predicted and truth differ in length")
    pts_l, cuts, idx = _cut_plan(pt_thlds)
    if n == 0:
        return {pt: dict(_tracking_metrics_nan_results) for pt in pts_l}
    dev = _device_of(truth, predicted, pts, reconstructable, eta)
    lab = _on(predicted, torch.int64, dev)
    # (labels may be any integers: negatives -> -1, the rest -> dense ranks below n; no host sync)
    _, inv = torch.unique(lab, return_inverse=True)
    lab = torch.where(lab < 0, torch.full_like(lab, -1), inv).view(1, n)
    t, p, r, e = _hits(truth, pts, reconstructable, eta, dev)
    out = _counts(lab, t, p, r, e, cuts, predicted_count_thld, max_eta)
    return _results(out.cpu().numpy(), 1, pts_l, idx)[0]


def tracking_metrics_trials(labels, *, truth, pts, reconstructable, eta, pt_thlds: Iterable[float] = (0.0, 0.5, 0.9, 1.5),
                            predicted_count_thld=3, max_eta=4) -> list[dict[str, float]]:
    """The tracking metrics of many labellings of the same hits (``labels`` [n_trials, n], values in
    [-1, n) as DBSCAN gives them; any negative value is noise) from one C call and one host copy: per
    trial the flattened dict of ``flatten_track_metrics(tracking_metrics(...))``."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() != 2:
        raise ValueError("tracking_metrics_trials: labels must be [n_trials, n]")
    n_trials, n = int(labels.shape[0]), int(labels.shape[1])
    pts_l, cuts, idx = _cut_plan(pt_thlds)
    if n == 0 or n_trials == 0:
        return [flatten_track_metrics({pt: dict(_tracking_metrics_nan_results) for pt in pts_l})
                for _ in range(n_trials)]
    dev = _device_of(labels, truth, pts, reconstructable, eta)
    lab = _on(labels, torch.int64, dev)
    t, p, r, e = _hits(truth, pts, reconstructable, eta, dev)
    if int(t.shape[0]) != n:
        raise ValueError("tracking_metrics_trials: labels and truth differ in the number of hits")
    out = _counts(lab, t, p, r, e, cuts, predicted_count_thld, max_eta)
    return [flatten_track_metrics(m) for m in _results(out.cpu().numpy(), n_trials, pts_l, idx)]


def tracking_metrics_data(data, labels, pt_thlds: Iterable[float], predicted_count_thld=3,
                          max_eta=4) -> dict[float, TrackingMetrics]:
    """``cluster_metrics.py:260-288``: ``tracking_metrics`` of a ``Data`` object's hits."""
    return tracking_metrics(truth=data.particle_id, predicted=labels, pts=data.pt,
                            reconstructable=data.reconstructable, eta=data.eta, pt_thlds=pt_thlds,
                            max_eta=max_eta, predicted_count_thld=predicted_count_thld)
