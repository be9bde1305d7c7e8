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

The binned views of a study's end (``cluster_metrics.py:76-149, 292-384``) are here too, without
pandas: ``tracking_metric_table`` is ``tracking_metric_df`` as a dict of numpy columns
(``gnntrk_cluster_table``), ``tracking_metrics_vs_pt`` / ``tracking_metrics_vs_eta`` return one dict
per bin; their counts come from ``gnntrk_tracking_metrics_windows``, one call per batch and 32 bins.

The module's registry closes it (``cluster_metrics.py:400-456``): ``common_metrics`` with the reference's
six keys, ``count_hits_per_cluster`` and ``hits_per_cluster_count_to_flat_dict``.  The reference hands
host copies of one trial's labels to sklearn; here ``gnntrk_cluster_spectra``
(``csrc/cluster_scores.hip``) counts on the device, for all trials of a call, the *size spectra* of the
truth classes, the predicted clusters and the cells of their contingency table - the distinct sizes and
how many classes / clusters / cells have each, at most ``floor((sqrt(8n + 1) - 1) / 2)`` entries each - and
the host finishes v-measure, homogeneity, completeness, the adjusted Rand index and the Fowlkes-Mallows
index from those few hundred integers (``clustering_scores_trials``: one C call and one host copy for all
trials).  For these scores labels and truth ids are categories of any integer value, as for sklearn: the
noise label -1 is ONE cluster and truth id 0 an ordinary class, unlike in the tracking metrics.

A collated batch of several events is that many independent problems from one C call.  The rule, once for this module:
``ptr=`` is the [B + 1] row offsets of the events (``events.py`` derives and checks them); ``None`` or one event is
today's single-event call with today's return type, more than one event calls the ``_batched`` C entry and returns
per-event results (``[trial][event]``, or a list of tables).  The host functions below exist once and treat one event as
B = 1 of the batched layouts; the only thing ``ptr`` selects is the C entry.  Labels: the public single-event calls
accept any integers and rank them with ``torch.unique``; with ``ptr`` labels are local to their event, in ``[-1, n_e)``,
as ``DBSCANFastRescan(..., ptr=ptr)`` gives them.  ``tracking_metrics_vs_pt`` / ``_vs_eta`` count the hit records that
``DBSCANPerformanceDetails`` sliced from one batch (``HitRecord``) in one call per 32 bins.  ``common_metrics`` and
``count_hits_per_cluster`` stay one event per call.
"""

from __future__ import annotations

import ctypes as C
import itertools
import math
from typing import Callable, Iterable, TypedDict

import numpy as np
import torch
from torch import Tensor

from . import _capi, events, ops
from .metrics import denote_pt

__all__ = ["TrackingMetrics", "tracking_metrics", "tracking_metrics_data", "tracking_metrics_trials",
           "flatten_track_metrics", "denote_pt", "tracking_metric_table", "tracking_metrics_vs_pt",
           "tracking_metrics_vs_eta", "clustering_spectra", "clustering_scores_trials", "count_hits_per_cluster",
           "hits_per_cluster_count_to_flat_dict", "common_metrics"]


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


def _nanmean(v: np.ndarray) -> float:
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


def _nanstd(v: np.ndarray) -> float:   # (ddof = 1, as pandas)
    v = v[~np.isnan(v)]
    return float(v.std(ddof=1)) if v.size > 1 else float("nan")


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
            predicted_count_thld: int, max_eta: float, ptr: Tensor | None = None) -> Tensor:
    """One launch sequence for all trials of ``labels`` [T, n]: the device int64 output of
    ``gnntrk_tracking_metrics`` (n_cuts + T * n_cuts * 4 + 1 values); with the events' offsets ``ptr`` [B + 1] that of
    ``gnntrk_tracking_metrics_batched`` (B * n_cuts + T * B * n_cuts * 4 + 1 values)."""
    lib = _capi.load()
    _capi.require_device(labels, truth, pts, reconstructable, eta)
    n_trials, n = int(labels.shape[0]), int(labels.shape[1])
    if n_trials > _capi.TRACKING_MAX_TRIALS:
        raise ValueError(f"tracking_metrics: at most {_capi.TRACKING_MAX_TRIALS} trials per call")
    nc = len(cuts)
    n_ev = 1 if ptr is None else int(ptr.numel()) - 1
    out = torch.empty(n_ev * nc * (1 + n_trials * 4) + 1, dtype=torch.int64, device=labels.device)
    ws = ops._ws(lib.gnntrk_tracking_metrics_workspace_bytes(n, n_trials), labels)
    p = ops._p
    tail = ((C.c_float * nc)(*cuts), nc, float(max_eta), int(predicted_count_thld), p(out), p(ws), ws.numel(),
            ops._stream(labels))
    hits = (p(labels), n_trials, p(truth), p(pts), p(eta), p(reconstructable), n)
    if ptr is None:
        _capi.check(lib.gnntrk_tracking_metrics(*hits, *tail), lib)
    else:
        _capi.require_device(ptr)
        _capi.check(lib.gnntrk_tracking_metrics_batched(*hits, p(ptr), n_ev, *tail), lib)
    return out


def _count_arrays(host: np.ndarray, n_trials: int, n_ev: int, per_event: bool) -> tuple[np.ndarray, np.ndarray]:
    """The host copy of ``_counts``' output as (particles [B, n_cuts], cluster counts [T, B, n_cuts, 4]) - one event is
    B = 1 of the batched layout; refuses a bad-label count (the last value) that is not 0."""
    if host[-1] != 0:
        raise ValueError(f"tracking_metrics: {int(host[-1])} labels are >= the number of hits"
                         + (" of their event" if per_event else ""))
    nc = (host.size - 1) // (n_ev * (1 + 4 * n_trials))
    return host[:n_ev * nc].reshape(n_ev, nc), host[n_ev * nc:-1].reshape(n_trials, n_ev, nc, 4)


def _results(host: np.ndarray, n_trials: int, sizes: list[int], pts: list, idx: list[int], per_event: bool) -> list[list[dict]]:
    """``[trial][event] -> flatten_track_metrics(...)`` of ``_counts``' output for events of ``sizes`` hits; an event
    without hits gets the NaN results of ``n == 0``"""
    n_part, cnt = _count_arrays(host, n_trials, len(sizes), per_event)
    nan = flatten_track_metrics({pt: dict(_tracking_metrics_nan_results) for pt in pts})
    # (flatten_track_metrics with the flat names made once per call, not once per trial, event and value)
    cols = {pt: (j, {k: denote_pt(k, pt) for k in TrackingMetrics.__annotations__}) for pt, j in zip(pts, idx)}

    def flat(t, e):
        return {names[k]: v for j, names in cols.values() for k, v in _from_counts(int(n_part[e, j]), cnt[t, e, j]).items()}

    return [[flat(t, e) if sizes[e] else dict(nan) for e in range(len(sizes))] for t in range(n_trials)]


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
    lab = _dense_labels(_on(predicted, torch.int64, dev))[0].view(1, n)
    t, p, r, e = _hits(truth, pts, reconstructable, eta, dev)
    out = _counts(lab, t, p, r, e, cuts, predicted_count_thld, max_eta)
    n_part, cnt = _count_arrays(out.cpu().numpy(), 1, 1, False)
    return {pt: _from_counts(int(n_part[0, j]), cnt[0, 0, j]) for pt, j in zip(pts_l, idx)}


def _metrics_per_event(labels, *, truth, pts, reconstructable, eta, pt_thlds, predicted_count_thld, max_eta,
                       ptr) -> list[list[dict]]:
    """``tracking_metrics_trials`` as ``[trial][event] -> flat dict`` whatever ``ptr`` is: one event is B = 1"""
    who = "tracking_metrics_trials"
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() != 2:
        raise ValueError(f"{who}: labels must be [n_trials, n]")
    n_trials, n = int(labels.shape[0]), int(labels.shape[1])
    pts_l, cuts, idx = _cut_plan(pt_thlds)
    ptr = events.event_ptr(ptr=ptr)
    sizes = events.event_sizes(ptr, n, who) or [n]
    if n == 0 or n_trials == 0:
        nan = flatten_track_metrics({pt: dict(_tracking_metrics_nan_results) for pt in pts_l})
        return [[dict(nan) for _ in sizes] for _ in range(n_trials)]
    dev = _device_of(labels, truth, pts, reconstructable, eta)
    lab = _on(labels, torch.int64, dev)
    t, p, r, e = _hits(truth, pts, reconstructable, eta, dev)
    if int(t.shape[0]) != n:
        raise ValueError(f"{who}: labels and truth differ in the number of hits")
    out = _counts(lab, t, p, r, e, cuts, predicted_count_thld, max_eta, None if ptr is None else _on(ptr, torch.int64, dev))
    return _results(out.cpu().numpy(), n_trials, sizes, pts_l, idx, ptr is not None)


def tracking_metrics_trials(labels, *, truth, pts, reconstructable, eta, pt_thlds: Iterable[float] = (0.0, 0.5, 0.9, 1.5),
                            predicted_count_thld=3, max_eta=4, ptr=None):
    """The tracking metrics of many labellings of the same hits (``labels`` [n_trials, n], values in
    [-1, n) as DBSCAN gives them; any negative value is noise) from one C call and one host copy: per
    trial the flattened dict of ``flatten_track_metrics(tracking_metrics(...))``.

    ``ptr`` (the events of a collated batch, module docstring): particles are (event, id) pairs and labels local to the
    event, as ``DBSCANFastRescan(..., ptr=ptr)`` gives them; the result is ``[trial][event] -> flat dict``."""
    res = _metrics_per_event(labels, truth=truth, pts=pts, reconstructable=reconstructable, eta=eta, pt_thlds=pt_thlds,
                             predicted_count_thld=predicted_count_thld, max_eta=max_eta, ptr=ptr)
    return res if events.event_ptr(ptr=ptr) is not None else [r[0] for r in res]


def tracking_metrics_data(data, labels, pt_thlds: Iterable[float], predicted_count_thld=3,
                          max_eta=4) -> dict[float, TrackingMetrics]:
    """``cluster_metrics.py:260-288``: ``tracking_metrics`` of a ``Data`` object's hits."""
    return tracking_metrics(truth=data.particle_id, predicted=labels, pts=data.pt,
                            reconstructable=data.reconstructable, eta=data.eta, pt_thlds=pt_thlds,
                            max_eta=max_eta, predicted_count_thld=predicted_count_thld)


# ------------------------------------------------------------------ cluster table, binned metrics
TABLE_COLUMNS = ("maj_pid", "maj_hits", "cluster_size", "valid_cluster", "maj_reconstructable", "maj_eta", "maj_pt",
                 "maj_pid_hits", "maj_frac", "maj_pid_frac", "perfect_match", "double_majority", "lhc_match")


def _dense_labels(lab: Tensor) -> tuple[Tensor, Tensor]:
    """Labels of any integers -> (labels in [-1, n): negatives -1, the rest their rank; the ascending
    distinct labels).  No host sync."""
    uniq, inv = torch.unique(lab, return_inverse=True)
    return torch.where(lab < 0, torch.full_like(lab, -1), inv), uniq


def _table(lab: Tensor, uniq: Tensor | None, t: Tensor, p: Tensor, r: Tensor, e: Tensor, predicted_count_thld: int,
           ptr: Tensor | None = None, sizes: list[int] | None = None):
    """``gnntrk_cluster_table`` of dense labels [n] in [-1, n), its rows with a cluster selected on the device, one host
    copy; ``uniq``: the label value of every dense label (None: itself).  With the events' offsets ``ptr`` (device,
    [B + 1]) and ``sizes``: ``gnntrk_cluster_table_batched`` of local labels in [-1, n_e), still one C call and one host
    copy, and a list with every event's rows as it gives them alone (``c``: the local label)."""
    lib = _capi.load()
    _capi.require_device(lab, t, p, r, e, ptr)
    n = int(lab.shape[0])
    dev = lab.device
    ints = torch.empty((5, max(n, 1)), dtype=torch.int64, device=dev)   # size, maj_hits, maj_pid, maj_pid_hits | bad
    flts = torch.empty((3, max(n, 1)), dtype=torch.float32, device=dev)
    ws = ops._ws(lib.gnntrk_cluster_table_workspace_bytes(n), lab)
    q = ops._p
    hits = (q(lab), q(t), q(p), q(e), q(r), n)
    tail = (q(ints[0]), q(ints[1]), q(ints[2]), q(ints[3]), q(flts[0]), q(flts[1]), q(flts[2]), q(ints[4]), q(ws),
            ws.numel(), ops._stream(lab))
    if ptr is None:
        _capi.check(lib.gnntrk_cluster_table(*hits, *tail), lib)
    else:
        _capi.check(lib.gnntrk_cluster_table_batched(*hits, q(ptr), len(sizes), *tail), lib)
    # (cluster slots - a batch: ptr[e] + label - ascending, so grouped by event; there the slot rides along as the
    # label column and the local label is taken on the host, where the events' rows are)
    rows = torch.nonzero(ints[0, :n] > 0).view(-1)
    col = _table_rows(rows if uniq is None else uniq[rows], rows, ints, flts,
                      "the number of hits" + (" of their event" if ptr is not None else ""))
    if ptr is None:
        return _table_columns(col, predicted_count_thld)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    cut = np.searchsorted(col[0], starts)
    tables = []
    for k in range(len(sizes)):
        part = col[:, cut[k]:cut[k + 1]].copy()
        part[0] -= starts[k]
        tables.append(_table_columns(part, predicted_count_thld))
    return tables


def _table_rows(c: Tensor, rows: Tensor, ints: Tensor, flts: Tensor, limit: str) -> np.ndarray:
    """The selected rows of the dense columns on the host, one copy: [8, m] int64 - the label, four integer
    columns, three fp32 columns as their bits; refuses a bad-label count (``ints[4, 0]``) that is not 0."""
    packed = torch.cat([c.view(1, -1), ints[:4, rows], flts[:, rows].view(torch.int32).to(torch.int64)]).view(-1)
    host = torch.cat([packed, ints[4, :1]]).cpu().numpy()
    if host[-1] != 0:
        raise ValueError(f"tracking_metric_table: {int(host[-1])} labels are >= {limit}")
    return host[:-1].reshape(8, int(rows.shape[0]))


def _table_columns(col: np.ndarray, predicted_count_thld: int) -> dict[str, np.ndarray]:
    """``tracking_metric_df``'s columns from the [8, m] rows of ``_table_rows``."""
    size, maj_hits, maj_pid, pid_hits = col[1], col[2], col[3], col[4]
    mpt, meta, mreco = (col[5 + k].astype(np.int32).view(np.float32) for k in range(3))
    valid = size >= predicted_count_thld
    # (fp64 ratios; the reference's fillna(0) never applies: a cluster and its majority particle have hits)
    frac = maj_hits / size
    pid_frac = maj_hits / pid_hits
    return {
        "c": col[0].copy(), "maj_pid": maj_pid.copy(), "maj_hits": maj_hits.copy(), "cluster_size": size.copy(),
        "valid_cluster": valid, "maj_reconstructable": mreco, "maj_eta": meta, "maj_pt": mpt,
        "maj_pid_hits": pid_hits.copy(), "maj_frac": frac, "maj_pid_frac": pid_frac,
        "perfect_match": (pid_hits == maj_hits) & (frac > 0.99) & valid,
        "double_majority": (pid_frac > 0.5) & (frac > 0.5) & valid,
        "lhc_match": (frac > 0.75) & valid,
    }


def tracking_metric_table(labels, *, truth, pts, reconstructable, eta, predicted_count_thld=3, ptr=None):
    """``tracking_metric_df`` (cluster_metrics.py:76-149) of one labelling as a dict of numpy columns:
    the index ``c`` (ascending cluster labels) and the reference's 13 columns in its order and dtypes.
    Inputs as ``tracking_metrics`` takes them.  Differences from the reference: only clusters (labels
    >= 0) have rows - the reference also lists its negative labels, as rows that are never valid - and
    ties for the majority particle go to the smallest id.

    ``ptr`` (the events of a collated batch, module docstring): a list with one table per event, each what the event's
    rows alone give (``c``: the local label; an event without hits has a table of no rows), from one C call and one
    host copy."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() != 1:
        raise ValueError("tracking_metric_table: labels must be [n]")
    dev = _device_of(labels, truth, pts, reconstructable, eta)
    t, p, r, e = _hits(truth, pts, reconstructable, eta, dev)
    if int(t.shape[0]) != int(labels.shape[0]):
        raise ValueError("tracking_metric_table: labels and truth differ in the number of hits")
    ptr = events.event_ptr(ptr=ptr)
    if ptr is not None:
        sizes = events.event_sizes(ptr, int(labels.shape[0]), "tracking_metric_table")
        return _table(_on(labels, torch.int64, dev), None, t, p, r, e, predicted_count_thld, _on(ptr, torch.int64, dev), sizes)
    lab, uniq = _dense_labels(_on(labels, torch.int64, dev))
    return _table(lab, uniq, t, p, r, e, predicted_count_thld)


def _window_counts(h: dict, windows: np.ndarray, predicted_count_thld: int, ptr=None) -> tuple[np.ndarray, np.ndarray]:
    """A hit record and fp32 windows [n, 4] -> (n_particles [B, n], counts [B, n, 4]), B = 1 without ``ptr``: one
    ``gnntrk_tracking_metrics_windows`` call and one host copy per 32 windows.  With ``ptr`` (more than one event) the
    record is that of a whole collated batch and the calls are ``gnntrk_tracking_metrics_windows_batched``: still one per
    32 windows, for ALL events."""
    lib = _capi.load()
    dev = _device_of(h["c"], h["id"], h["pt"], h["reconstructable"], h["eta"])
    t, p, r, e = _hits(h["id"], h["pt"], h["reconstructable"], h["eta"], dev)
    lab = _on(h["c"], torch.int64, dev).view(-1)
    n = int(lab.shape[0])
    if int(t.shape[0]) != n:
        raise ValueError("tracking_metrics_vs: a hit record's columns differ in length")
    ptr = events.event_ptr(ptr=ptr)
    n_ev = len(events.event_sizes(ptr, n, "tracking_metrics_vs") or [n])
    n_part = np.zeros((n_ev, len(windows)), dtype=np.int64)
    counts = np.zeros((n_ev, len(windows), 4), dtype=np.int64)
    if n == 0:
        return n_part, counts
    q = ops._p
    if ptr is None:
        lab, _ = _dense_labels(lab)
        entry, seg = lib.gnntrk_tracking_metrics_windows, ()
    else:
        ptr = _on(ptr, torch.int64, dev)
        entry, seg = lib.gnntrk_tracking_metrics_windows_batched, (q(ptr), n_ev)
    _capi.require_device(lab, t, p, r, e, ptr)
    ws = ops._ws(lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, 1), lab)
    for lo in range(0, len(windows), _capi.TRACKING_MAX_WINDOWS):
        win = np.ascontiguousarray(windows[lo:lo + _capi.TRACKING_MAX_WINDOWS], dtype=np.float32)
        nw = len(win)
        out = torch.empty(n_ev * nw * 5 + 1, dtype=torch.int64, device=dev)
        _capi.check(entry(q(lab), 1, q(t), q(p), q(e), q(r), n, *seg, win.ctypes.data_as(C.POINTER(C.c_float)), nw,
                          int(predicted_count_thld), q(out), q(ws), ws.numel(), ops._stream(lab)), lib)
        host = out.cpu().numpy()
        if host[-1] != 0:
            raise ValueError(f"tracking_metrics_vs: {int(host[-1])} labels are >= the number of hits"
                             + (" of their event" if ptr is not None else ""))
        n_part[:, lo:lo + nw] = host[:n_ev * nw].reshape(n_ev, nw)
        counts[:, lo:lo + nw] = host[n_ev * nw:-1].reshape(n_ev, nw, 4)
    return n_part, counts


class HitRecord(dict):
    """The hit record of one event that ``DBSCANPerformanceDetails`` sliced from a collated batch: a dict with the
    five keys of every hit record.  ``origin`` - an attribute, not a key - remembers the batch (``EventBatch``) and
    the event's index in it, so that ``tracking_metrics_vs_pt`` / ``_vs_eta`` can count all events of the batch in
    one call."""

    origin = None   # (EventBatch, index of the event)


class EventBatch:
    """The hits of a collated batch behind its ``HitRecord``s: the whole columns (``record``: ``c`` holds labels local
    to the event), the events' offsets on the device and the per-event records that were handed out."""

    def __init__(self, record: dict, ptr: Tensor):
        self.record, self.ptr = record, ptr
        rows = ptr.tolist()
        self.sizes = [b - a for a, b in zip(rows, rows[1:])]
        self.records, self._views = [], []
        for k, (a, b) in enumerate(zip(rows, rows[1:])):
            rec = HitRecord({key: v[a:b] for key, v in record.items()})
            rec.origin = (self, k)
            self.records.append(rec)
            self._views.append(tuple(rec.values()))

    def holds(self, rec) -> bool:
        """whether ``rec`` still has the columns it was handed out with (a record whose columns were replaced is
        counted on its own)"""
        views = self._views[rec.origin[1]]
        return list(rec) == list(self.record) and all(v is w for v, w in zip(rec.values(), views))


def _per_record_counts(h_dfs: list, windows: np.ndarray, predicted_count_thld: int) -> list:
    """(n_particles, counts) of every hit record, in the records' order.  Records that ``DBSCANPerformanceDetails``
    sliced from one collated batch are counted together - ``_window_counts`` with the batch's ``ptr``, once per batch
    instead of once per event -, every other record on its own."""
    out: list = [None] * len(h_dfs)
    groups: dict[int, list[int]] = {}
    for i, h in enumerate(h_dfs):
        origin = getattr(h, "origin", None)
        if origin is not None and origin[0].holds(h):
            groups.setdefault(id(origin[0]), []).append(i)
    for members in groups.values():
        if len(members) < 2:
            continue
        batch = h_dfs[members[0]].origin[0]
        n_part, counts = _window_counts(batch.record, windows, predicted_count_thld, batch.ptr)
        for i in members:
            k = h_dfs[i].origin[1]
            out[i] = (n_part[k], counts[k])
    for i, h in enumerate(h_dfs):
        if out[i] is None:
            n_part, counts = _window_counts(h, windows, predicted_count_thld)
            out[i] = (n_part[0], counts[0])
    return out


def _binned(h_dfs, c_dfs, edges, window_of, names: tuple[str, str], predicted_count_thld: int) -> list[dict]:
    h_dfs, edges = list(h_dfs), list(edges)
    if len(list(c_dfs)) != len(h_dfs):
        raise ValueError("tracking_metrics_vs: h_dfs and c_dfs differ in length")
    bins = list(itertools.pairwise(edges))
    if not bins:
        return []
    # (edges rounded to fp32: numpy 2 compares float32 columns with Python scalars in fp32)
    windows = np.array([window_of(lo, hi) for lo, hi in bins], dtype=np.float32).reshape(len(bins), 4)
    per_batch = _per_record_counts(h_dfs, windows, predicted_count_thld)
    rows = []
    for j, (lo, hi) in enumerate(bins):
        ms = [_from_counts(int(n_part[j]), counts[j]) for n_part, counts in per_batch]
        keys = list(ms[0]) if ms else list(_from_counts(0, np.zeros(4, np.int64)))
        vals = {k: np.array([float(m[k]) for m in ms], dtype=np.float64) for k in keys}
        row = {k: _nanmean(v) for k, v in vals.items()}
        norm = math.sqrt(len(ms)) if ms else float("nan")
        row.update({k + "_err": _nanstd(v) / norm for k, v in vals.items()})
        row[names[0]], row[names[1]] = lo, hi
        rows.append(row)
    return rows


def tracking_metrics_vs_pt(h_dfs, c_dfs, pts, *, max_eta: float = 4.0, predicted_count_thld=3) -> list[dict[str, float]]:
    """``cluster_metrics.py:292-337``: the tracking metrics per pt slice ``[pts[i], pts[i + 1])``, one
    dict per slice with the eight ``TrackingMetrics`` keys (NaN-skipping mean over the batches), their
    ``_err`` (ddof = 1 std over the batches / sqrt(number of batches); NaN for one batch), ``pt_min``
    and ``pt_max``.  ``h_dfs``: per batch a hit record - a mapping with ``c`` (labels), ``id``,
    ``reconstructable``, ``pt``, ``eta`` as device tensors or arrays, as ``DBSCANPerformanceDetails``
    keeps them.  ``c_dfs`` is accepted for the reference's signature and checked for its length only:
    the clusters are rebuilt on the device with ``predicted_count_thld``.  As in the reference, eta is
    tested as ``eta < max_eta``, signed."""
    nan = float("nan")
    return _binned(h_dfs, c_dfs, pts, lambda lo, hi: (lo, hi, nan, max_eta), ("pt_min", "pt_max"),
                   predicted_count_thld)


def tracking_metrics_vs_eta(h_dfs, c_dfs, etas, pt_thld: float = 0.9, *, predicted_count_thld=3) -> list[dict[str, float]]:
    """``cluster_metrics.py:340-384``: the same per eta slice ``[etas[i], etas[i + 1])`` for
    ``pt >= pt_thld``, with ``eta_min`` and ``eta_max``."""
    nan = float("nan")
    return _binned(h_dfs, c_dfs, etas, lambda lo, hi: (pt_thld, nan, lo, hi), ("eta_min", "eta_max"),
                   predicted_count_thld)


# ------------------------------------------------------------------ clustering scores, common_metrics
SCORE_KEYS = ("v_measure", "homogeneity", "completeness", "adjusted_rand", "fowlkes_mallows")
_EMPTY = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))


def _spectrum(row: np.ndarray, cap: int) -> tuple[np.ndarray, np.ndarray]:
    d = int(row[0])
    if not 0 <= d <= cap:
        raise RuntimeError(f"clustering_spectra: a spectrum of {d} entries, at most {cap} are possible")
    pairs = row[1:1 + 2 * d].reshape(d, 2)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def _spectra(lab: Tensor, tru: Tensor | None, ptr: Tensor | None = None, sizes: list[int] | None = None) -> list[list[dict]]:
    """``gnntrk_cluster_spectra`` of ``lab`` [T, n] (1 <= T, 1 <= n), with the events' offsets ``ptr`` (device) and
    ``sizes`` ``gnntrk_cluster_spectra_batched``: one C call and one host copy, then ``[trial][event] -> spectra``.  The
    two entries differ in layout: one event's spectrum is a row of (size, multiplicity) pairs, a batch's one pooled list
    of (event, size, multiplicity) with its own capacity."""
    lib = _capi.load()
    _capi.require_device(lab, tru, ptr)
    n_trials, n = int(lab.shape[0]), int(lab.shape[1])
    if n_trials > _capi.TRACKING_MAX_TRIALS:
        raise ValueError(f"clustering_spectra: at most {_capi.TRACKING_MAX_TRIALS} trials per call")
    p = ops._p
    if ptr is None:
        entry, seg, width, cap = lib.gnntrk_cluster_spectra, (), 2, int(lib.gnntrk_cluster_spectra_capacity(n))
    else:
        entry, seg, width = lib.gnntrk_cluster_spectra_batched, (p(ptr), len(sizes)), 3
        cap = int(lib.gnntrk_cluster_spectra_batched_capacity(n, len(sizes)))
    out = torch.empty((1 + 2 * n_trials, 1 + width * cap), dtype=torch.int64, device=lab.device)
    ws = ops._ws(lib.gnntrk_cluster_spectra_workspace_bytes(n, n_trials), lab)
    _capi.check(entry(p(lab), n_trials, p(tru) if tru is not None else None, n, *seg, p(out), p(ws), ws.numel(),
                      ops._stream(lab)), lib)
    host = out.cpu().numpy()
    if ptr is None:
        def per_event(row: np.ndarray) -> list[tuple[np.ndarray, np.ndarray]]:
            return [_spectrum(row, cap)]
    else:
        n_ev = len(sizes)
        caps = [int(lib.gnntrk_cluster_spectra_capacity(m)) for m in sizes]

        def per_event(row: np.ndarray) -> list[tuple[np.ndarray, np.ndarray]]:
            d = int(row[0])
            if not 0 <= d <= cap:
                raise RuntimeError(f"clustering_spectra: spectra of {d} entries, at most {cap} are possible")
            triples = row[1:1 + 3 * d].reshape(d, 3)
            triples = triples[np.argsort(triples[:, 0], kind="stable")]
            cut = np.searchsorted(triples[:, 0], np.arange(n_ev + 1))
            # (the event's pairs behind their number: a row as gnntrk_cluster_spectra writes it, checked against D(n_e))
            return [_spectrum(np.concatenate([[cut[k + 1] - cut[k]], triples[cut[k]:cut[k + 1], 1:].reshape(-1)]), caps[k])
                    for k in range(n_ev)]

    classes = per_event(host[0])
    res = []
    for t in range(n_trials):
        clusters, cells = per_event(host[1 + 2 * t]), per_event(host[2 + 2 * t])
        res.append([{"classes": a, "clusters": b, "cells": c} for a, b, c in zip(classes, clusters, cells)])
    return res


def clustering_spectra(labels, truth=None, ptr=None):
    """The size spectra of ``labels`` ([n] or [n_trials, n]) against ``truth`` ([n], optional): one dict per
    trial with ``classes`` (truth classes; the same for every trial), ``clusters`` and ``cells`` (non-zero
    cells of the contingency table), each a pair of ascending int64 arrays ``(sizes, multiplicities)``.
    Labels and ids are categories of any integer value (-1 is one cluster).  Without ``truth``, ``classes``
    and ``cells`` are empty.  One C call and one host copy.

    ``ptr`` (the events of a collated batch, module docstring): a class is (event, truth id), a cluster (event, label),
    so equal labels or ids of two events stay apart; the result is ``[trial][event] -> dict``, each what the event's
    rows alone give (an event without hits: empty spectra)."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() == 1:
        labels = labels.view(1, -1)
    if labels.dim() != 2:
        raise ValueError("clustering_spectra: labels must be [n] or [n_trials, n]")
    n_trials, n = int(labels.shape[0]), int(labels.shape[1])
    if truth is not None and int(np.shape(truth)[0] if not torch.is_tensor(truth) else truth.shape[0]) != n:
        raise ValueError("clustering_spectra: labels and truth differ in the number of hits")
    ptr = events.event_ptr(ptr=ptr)
    sizes = events.event_sizes(ptr, n, "clustering_spectra")
    if n == 0 or n_trials == 0:
        empty = {"classes": _EMPTY, "clusters": _EMPTY, "cells": _EMPTY}
        return [dict(empty) if sizes is None else [dict(empty) for _ in sizes] for _ in range(n_trials)]
    dev = _device_of(labels, truth)
    lab = _on(labels, torch.int64, dev)
    tru = _on(truth, torch.int64, dev).view(-1) if truth is not None else None
    if sizes is not None:
        return _spectra(lab, tru, _on(ptr, torch.int64, dev), sizes)
    return [per_event[0] for per_event in _spectra(lab, tru)]


def _xlogx(s: tuple[np.ndarray, np.ndarray]) -> float:
    """X(s) = sum of m v ln v over a spectrum."""
    return math.fsum(int(m) * int(v) * math.log(int(v)) for v, m in zip(*s))


def _squares(s: tuple[np.ndarray, np.ndarray]) -> int:
    """Q(s) = sum of m v^2 over a spectrum, as a Python int."""
    return sum(int(m) * int(v) * int(v) for v, m in zip(*s))


def _scores_from_spectra(sp: dict[str, tuple[np.ndarray, np.ndarray]]) -> dict[str, float]:
    """sklearn's v_measure / homogeneity / completeness / adjusted_rand / fowlkes_mallows scores from the
    three spectra of one trial.  With X, Q as above and L = ln n: H(C) = L - X(a) / n, H(K) = L - X(b) / n,
    MI = (X(c) - X(a) - X(b)) / n + L (0 where either labelling has one group, as in sklearn); the pair
    counts are integers: tp = Q(c) - n, fp = Q(b) - Q(c), fn = Q(a) - Q(c), tn = n^2 - fp - fn - Q(c)."""
    a, b, c = sp["classes"], sp["clusters"], sp["cells"]
    n = sum(int(m) * int(v) for v, m in zip(*b))
    if n == 0:
        return dict(zip(SCORE_KEYS, (1.0, 1.0, 1.0, 1.0, 0.0)))
    one_class, one_cluster = int(a[1].sum()) == 1, int(b[1].sum()) == 1
    log_n = math.log(n)
    xa, xb, xc = _xlogx(a), _xlogx(b), _xlogx(c)
    h_c = 0.0 if one_class else log_n - xa / n
    h_k = 0.0 if one_cluster else log_n - xb / n
    mi = 0.0 if one_class or one_cluster else max(0.0, (xc - xa - xb) / n + log_n)
    hom = mi / h_c if h_c else 1.0
    com = mi / h_k if h_k else 1.0
    v = 0.0 if hom + com == 0.0 else 2 * hom * com / (hom + com)
    qa, qb, s = _squares(a), _squares(b), _squares(c)
    tp, fp, fn = s - n, qb - s, qa - s
    tn = n * n - fp - fn - s
    # (Python ints up to the one floating expression, which is sklearn's: the products pass 2^63)
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    tk, pk, qk = s - n, qb - n, qa - n
    fmi = math.sqrt(tk / pk) * math.sqrt(tk / qk) if tk != 0 else 0.0
    return dict(zip(SCORE_KEYS, (v, hom, com, ari, fmi)))


def clustering_scores_trials(labels, *, truth, ptr=None):
    """sklearn's clustering scores of many labellings of the same hits (``labels`` [n_trials, n] or [n]) from
    one C call and one host copy: per trial a dict with ``v_measure``, ``homogeneity``, ``completeness``,
    ``adjusted_rand`` and ``fowlkes_mallows``, as the reference's ``common_metrics`` give them one by one.
    The sibling of ``tracking_metrics_trials`` for a scanner that ranks DBSCAN trials by such a score.

    ``ptr`` (more than one event, as ``clustering_spectra`` takes it): ``[trial][event] -> dict``, each event scored
    on its own - without it a collated batch would be scored as one mixture, in which equal labels and truth ids of
    different events merge.  ``common_metrics`` and ``count_hits_per_cluster`` stay one event per call."""
    if truth is None:
        raise ValueError("clustering_scores_trials: truth is required")
    spectra = clustering_spectra(labels, truth, ptr)
    if spectra and isinstance(spectra[0], list):
        return [[_scores_from_spectra(sp) for sp in per_event] for per_event in spectra]
    return [_scores_from_spectra(sp) for sp in spectra]


def count_hits_per_cluster(predicted) -> np.ndarray:
    """``cluster_metrics.py:400-404``: ``out[v - 1]`` = the number of clusters with exactly ``v`` hits, for
    ``v`` = 1 ... the largest cluster size (every distinct label is a cluster, -1 included)."""
    if not torch.is_tensor(predicted):
        predicted = torch.as_tensor(np.asarray(predicted))
    if predicted.dim() != 1:
        raise ValueError("count_hits_per_cluster: predicted must be [n]")
    if int(predicted.shape[0]) == 0:   # (the reference fails on counts.max() of nothing)
        raise ValueError("count_hits_per_cluster: no hits")
    sizes, mult = clustering_spectra(predicted)[0]["clusters"]
    out = np.zeros(int(sizes[-1]), dtype=np.int64)
    out[sizes - 1] = mult
    return out


def hits_per_cluster_count_to_flat_dict(counts: np.ndarray, min_max=10) -> dict[str, float]:
    """``cluster_metrics.py:407-424``: the result of ``count_hits_per_cluster``, padded with zeros to at
    least ``min_max`` sizes, as cumulative fractions (keys ``hitcountgeq_0001`` ... enumerate the cumulative
    sums from the last one down, as the reference does)."""
    cumulative = np.cumsum(np.pad(counts, (0, max(0, min_max - len(counts))), "constant"))
    total = cumulative[-1]
    return {f"hitcountgeq_{i:04}": cumulative / total for i, cumulative in enumerate(reversed(cumulative), start=1)}


def _score_metric(key: str) -> Callable[..., float]:
    def metric(*, truth, predicted, **_ignored) -> float:
        return clustering_scores_trials(predicted, truth=truth)[0][key]

    metric.__name__ = metric.__qualname__ = f"{key}_score"
    metric.__doc__ = f"sklearn's ``{key}_score(truth, predicted)`` from the device's size spectra."
    return metric


def _trk_metric(*, truth, predicted, pts, reconstructable, eta, pt_thlds, predicted_count_thld=3, max_eta=4,
                **_ignored) -> dict[str, float]:
    return flatten_track_metrics(tracking_metrics(truth=truth, predicted=predicted, pts=pts,
                                                  reconstructable=reconstructable, eta=eta, pt_thlds=pt_thlds,
                                                  predicted_count_thld=predicted_count_thld, max_eta=max_eta))


#: ``cluster_metrics.py:440-456``: the metrics a ``ClusterMetricType`` consumer looks up by name, in the
#: reference's order.  Every value takes ``truth=`` and ``predicted=`` (``trk`` also the hit properties and
#: ``pt_thlds`` of ``tracking_metrics``) and ignores further keyword arguments.
common_metrics: dict[str, Callable] = {
    "v_measure": _score_metric("v_measure"),
    "homogeneity": _score_metric("homogeneity"),
    "completeness": _score_metric("completeness"),
    "trk": _trk_metric,
    "adjusted_rand": _score_metric("adjusted_rand"),
    "fowlkes_mallows": _score_metric("fowlkes_mallows"),
}
