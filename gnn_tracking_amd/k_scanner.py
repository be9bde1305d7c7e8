"""Finds the right k for the kNN graph construction (``graph_construction/k_scanner.py:31-285``): the
validation of the metric-learning stage, on the device.

``GraphConstructionKNNScanner`` has the reference's constructor, call signature, record keys and
figures of merit.  Per batch the reference runs, for every k, a neighbour search, two networkx
component walks and the pandas chain of ``tracking_metrics``.  Here a batch costs ONE neighbour search
at ``max(ks)`` (the graph of a smaller k is a prefix of every row of its table), one
``gnntrk_kscan_counts`` call (components and counts of all ks, ``csrc/kscan.hip``), one
``gnntrk_tracking_metrics`` call with ``n_trials = len(ks)`` for the upper bounds, and ONE host copy.
``KScanResults`` interpolates the per-k means with a not-a-knot cubic spline in numpy (no pandas, scipy
or networkx).

A collated batch of B > 1 events (``data.ptr`` / ``data.batch``, as ``events.event_ptr`` reads them) is B scans from
the same launch sequence: the search per event, ``gnntrk_kscan_counts_batched`` and ``gnntrk_tracking_metrics_batched``,
still one host copy, and one record per (event, k) - the records of the events fed one by one
(``GraphConstructionKNNScanner.per_event``).  One event is B = 1 of the same record loop, from the single-event entries.

What differs from the reference, all of it outside what its results pin down:

* ``subsample_pids`` exists there to make the host loop affordable.  It is accepted, a warning is given
  once, and all particles are evaluated - the quantity the subsample estimates.
* The k at which ``frac50`` meets a target: the reference runs L-BFGS-B from the mid-point of the k range
  on ``|frac50(k) - target|``.  Here the sign changes of ``frac50(k) - target`` are bracketed on a grid of
  2 001 points and bisected; with several crossings the one nearest the mid-point is taken (the reference's
  choice then depends on its optimiser's path: unpinned); without a crossing the minimiser of the
  objective on the grid, refined by a ternary search unless it is an end point.
* A ``frac50`` column that holds a NaN (no particle passes the cuts) gives NaN at every target; the
  ``max_frac_segment50`` block then comes from the last row.
"""

from __future__ import annotations

import ctypes as C
import logging
import math
import typing

import numpy as np
import torch
from torch import Tensor

from . import _capi, events, ops
from .cluster_metrics import _counts as _tracking_counts, _cut_plan, _hits, _results as _tracking_results, _zdiv
from .graph_analysis import efficiency_purity_from_counts
from .graph_masks import get_good_node_mask
from .hparams import HyperparametersMixin

__all__ = ["KScanResults", "GraphConstructionKNNScanner", "kscan_counts", "COUNT_COLUMNS"]

logger = logging.getLogger("gnn_tracking_amd")

# columns of gnntrk_kscan_counts' table (include/gnntrk.h)
COUNT_COLUMNS = ("n_edges", "n_masked", "n_true_masked", "n_true_edges_masked", "n_pids", "n50", "n75", "n100",
                 "n_bad")


class _NotAKnotSpline:
    """Cubic spline through (x_i, y_i[, c]) with scipy ``CubicSpline``'s default ends (not-a-knot): two
    points give the line, three the parabola through them."""

    def __init__(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
        n = len(x)
        if n < 2 or not np.all(np.diff(x) > 0):
            raise ValueError("spline: needs at least two strictly increasing abscissae")
        dx = np.diff(x)
        slope = np.diff(y, axis=0) / dx[:, None]
        if n == 2:
            s = np.vstack([slope[0], slope[0]])
        else:
            a = np.zeros((n, n))
            b = np.zeros_like(y)
            for i in range(1, n - 1):
                a[i, i - 1], a[i, i], a[i, i + 1] = dx[i], 2 * (dx[i - 1] + dx[i]), dx[i - 1]
                b[i] = 3 * (dx[i] * slope[i - 1] + dx[i - 1] * slope[i])
            if n == 3:
                a[0, 0], a[0, 1] = 1, 1
                a[2, 1], a[2, 2] = 1, 1
                b[0], b[2] = 2 * slope[0], 2 * slope[1]
            else:
                d = x[2] - x[0]
                a[0, 0], a[0, 1] = dx[1], d
                b[0] = ((dx[0] + 2 * d) * dx[1] * slope[0] + dx[0] ** 2 * slope[1]) / d
                d = x[-1] - x[-3]
                a[-1, -1], a[-1, -2] = dx[-2], d
                b[-1] = (dx[-1] ** 2 * slope[-2] + (2 * d + dx[-1]) * dx[-2] * slope[-1]) / d
            s = np.linalg.solve(a, b)
        t = (s[:-1] + s[1:] - 2 * slope) / dx[:, None]
        self.x = x
        self.c = np.stack([t / dx[:, None], (slope - s[:-1]) / dx[:, None] - t, s[:-1], y[:-1]])

    def __call__(self, k):
        k = np.asarray(k, dtype=np.float64)
        i = np.clip(np.searchsorted(self.x, k, side="right") - 1, 0, len(self.x) - 2)
        h = (k - self.x[i])[..., None]
        c = self.c[:, i]
        return ((c[0] * h + c[1]) * h + c[2]) * h + c[3]


class KScanResults:
    _extra_metrics = ("k", "frac75", "frac100", "efficiency", "purity")
    _grid = 2001

    def __init__(self, results: typing.Sequence[typing.Mapping[str, float]], targets: typing.Sequence[float]):
        """Holds the results of scanning over ks and interpolates them to get the figures of merit
        (k_scanner.py:31-148).

        Args:
            results: one row per k: ``{"k": k, "frac50": ..., "n_edges": ..., ...}`` (the reference's frame
                of per-k means); sorted by k here
            targets: the 50 %-segment fractions of interest
        """
        rows = sorted((dict(r) for r in results), key=lambda r: r["k"])
        self.rows = rows
        # (column order of the reference's frame: "k" is moved to the end)
        self.columns = [c for c in (rows[0] if rows else {}) if c != "k"] + ["k"]
        self.table = {c: np.array([float(r[c]) for r in rows], dtype=np.float64) for c in self.columns}
        self.targets = targets
        self._spl = None

    def __len__(self) -> int:
        return len(self.rows)

    def get_foms(self) -> dict[str, float]:
        """Figures of merit, keys and order as ``KScanResults.get_foms`` (k_scanner.py:50-65)."""
        foms = {}
        for t in self.targets:
            fat = self._get_foms_at_target(t)
            foms[f"n_edges_frac_segment50_{t * 100:.0f}"] = fat["n_edges"]
            for v in self._extra_metrics:
                foms[f"{v}_at_segment50_{t * 100:.0f}"] = fat[v]
        f50 = self.table["frac50"]
        # (first row attaining the maximum, NaN skipped; all NaN: the last row)
        idx = len(f50) - 1 if np.isnan(f50).all() else int(np.nanargmax(f50))
        fat = {c: float(self.table[c][idx]) for c in self.columns}
        foms["max_frac_segment50"] = fat["frac50"]
        foms["n_edges_max_frac_segment50"] = fat["n_edges"]
        for v in self._extra_metrics:
            foms[f"{v}_at_max_frac_segment50"] = fat[v]
        return foms

    @property
    def _spline(self):
        if self._spl is None:
            nan_cols = [c for c in self.columns if np.isnan(self.table[c]).any()]
            cols = [c for c in self.columns if c not in nan_cols]
            self._spl = (_NotAKnotSpline(self.table["k"], np.stack([self.table[c] for c in cols], axis=1)),
                         nan_cols, cols)
        return self._spl

    def _eval_spline(self, k: float) -> dict[str, float]:
        spline, nan_cols, cols = self._spline
        result = dict(zip(cols, spline(float(k)).tolist()))
        for c in nan_cols:
            result[c] = float("nan")
        return result

    def _frac50(self, k):
        spline, _, cols = self._spline
        return spline(k)[..., cols.index("frac50")]

    def _get_target_k(self, target: float) -> float:
        """k in [k_min, k_max] that minimises ``|frac50(k) - target|`` (module docstring)."""
        f50 = self.table["frac50"]
        if np.isnan(f50).any() or target > f50.max():
            return float("nan")
        ks = self.table["k"]
        lo, hi = float(ks.min()), float(ks.max())
        grid = np.linspace(lo, hi, self._grid)
        g = self._frac50(grid) - target
        mid = (lo + hi) / 2
        zero = np.flatnonzero(g == 0)
        cross = np.flatnonzero(g[:-1] * g[1:] < 0)
        cands = [(abs(grid[i] - mid), i, True) for i in zero] + \
                [(abs((grid[i] + grid[i + 1]) / 2 - mid), i, False) for i in cross]
        if cands:
            _, i, exact = min(cands)
            if exact:
                return float(grid[i])
            a, b, ga = float(grid[i]), float(grid[i + 1]), float(g[i])
            for _ in range(200):
                m = (a + b) / 2
                if m == a or m == b:
                    break
                gm = float(self._frac50(m) - target)
                if gm == 0:
                    return m
                if (gm < 0) == (ga < 0):
                    a, ga = m, gm
                else:
                    b = m
            return (a + b) / 2
        i = int(np.argmin(np.abs(g)))
        if i == 0 or i == len(grid) - 1:
            return float(grid[i])
        a, b = float(grid[i - 1]), float(grid[i + 1])
        for _ in range(200):
            m1, m2 = a + (b - a) / 3, b - (b - a) / 3
            if not a < m1 < m2 < b:
                break
            if abs(float(self._frac50(m1) - target)) <= abs(float(self._frac50(m2) - target)):
                b = m2
            else:
                a = m1
        return (a + b) / 2

    def _get_foms_at_target(self, target: float) -> dict[str, float]:
        nan_results = {c: float("nan") for c in self.columns}
        if len(self.rows) < 2:
            return nan_results
        k = self._get_target_k(target)
        if math.isnan(k):
            return nan_results
        return self._eval_spline(k)


_DEFAULT_KS = list(range(1, 10))


def _mean_skipna(values: list[float]) -> float:
    """pandas' ``groupby().mean()``: NaN skipped, Kahan summation, NaN for an empty group."""
    total, comp, n = 0.0, 0.0, 0
    for v in values:
        if v != v:
            continue
        n += 1
        y = v - comp
        t = total + y
        comp = t - total - y
        if comp != comp:   # (an infinite sum)
            comp = 0.0
        total = t
    return total / n if n else float("nan")


def kscan_counts(nbr: Tensor, cnt: Tensor, k_stride: int, ks: typing.Sequence[int], particle_id: Tensor,
                 node_mask: Tensor, true_edge_index: Tensor | None, ptr: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """``gnntrk_kscan_counts`` on one neighbour table (``nbr`` int32 ``[n * k_stride]``, ``cnt`` int32
    ``[n]`` of a search with ``k = k_stride``): the int64 table ``[len(ks), len(COUNT_COLUMNS)]`` and the
    int64 labels ``[len(ks), n]`` of the same-id components on all hits, both on the device; no host read.

    ``ptr`` (int64 ``[B + 1]`` row offsets of the events of a collated batch, more than one event; the table of a
    search per event): ``gnntrk_kscan_counts_batched`` - the table ``[B, len(ks), len(COUNT_COLUMNS)]`` of every
    event on its own and labels local to the event, as ``_tracking_counts(..., ptr=ptr)`` takes them."""
    _capi.require_device(nbr, cnt, particle_id, node_mask)
    lib = _capi.load()
    n = int(cnt.shape[0])
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= _capi.KSCAN_MAX_KS:
        raise ValueError(f"kscan_counts: {len(ks)} ks, expected 1..{_capi.KSCAN_MAX_KS}")
    if int(nbr.numel()) < n * int(k_stride) or nbr.dtype != torch.int32 or cnt.dtype != torch.int32:
        raise ValueError("kscan_counts: nbr / cnt must be the int32 table of a search with k = k_stride")
    dev = cnt.device
    pid = particle_id.detach().to(device=dev, dtype=torch.int64).contiguous()
    mask = node_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    if int(pid.shape[0]) != n or int(mask.shape[0]) != n:
        raise ValueError("kscan_counts: particle_id / node_mask and the neighbour table differ in the number of hits")
    te, m_te = None, 0
    if true_edge_index is not None and true_edge_index.numel():
        te = true_edge_index.detach().to(device=dev, dtype=torch.int64).contiguous()
        m_te = int(te.shape[1])
    n_ev = int(ptr.numel()) - 1 if ptr is not None and ptr.numel() > 2 else 0
    shape = (len(ks), _capi.KSCAN_COLUMNS)
    out = torch.empty((n_ev, *shape) if n_ev else shape, dtype=torch.int64, device=dev)
    labels = torch.empty((len(ks), n), dtype=torch.int64, device=dev)
    p = ops._p
    head = (p(nbr), p(cnt), n, int(k_stride), (C.c_int32 * len(ks))(*ks), len(ks), p(pid), p(mask), p(te), m_te)
    if n_ev:
        _capi.require_device(ptr)
        seg = ptr.detach().to(device=dev, dtype=torch.int64).contiguous()
        ws = ops._ws(lib.gnntrk_kscan_counts_batched_workspace_bytes(n, n_ev, len(ks)), cnt)
        _capi.check(lib.gnntrk_kscan_counts_batched(*head, p(seg), n_ev, p(out), p(labels), p(ws), ws.numel(),
                                                    ops._stream(cnt)), lib)
    else:
        ws = ops._ws(lib.gnntrk_kscan_counts_workspace_bytes(n), cnt)
        _capi.check(lib.gnntrk_kscan_counts(*head, p(out), p(labels), p(ws), ws.numel(), ops._stream(cnt)), lib)
    return out, labels


class GraphConstructionKNNScanner(HyperparametersMixin):
    # noinspection PyUnusedLocal
    def __init__(self, ks: list[int] = _DEFAULT_KS, *, targets=(0.8, 0.85, 0.88, 0.9, 0.93, 0.95, 0.97, 0.99),
                 max_radius=1.0, pt_thld=0.9, max_eta=4.0, subsample_pids: int | None = None,
                 max_edges=5_000_000):
        """Scan over different values of k to build a graph and calculate the figures of merit
        (k_scanner.py:151-285; same arguments).

        Args:
            ks: ks to scan; results are interpolated between them
            targets: targets for the 50 %-segment fraction: the k that gets closest to each is found and
                the number of edges (and the other columns) reported there
            max_radius: maximum length of edges of the kNN graph
            pt_thld: pt threshold of the good-node mask
            max_eta: eta cut of the good-node mask
            subsample_pids: accepted for compatibility; all particles are evaluated (module docstring)
            max_edges: the scan of a batch stops at the first k (in the given order) whose graph has more
                edges than this; on a collated batch (``per_event``) that of every event on its own
        """
        super().__init__()
        self.save_hyperparameters()
        self._results: list[dict[str, float]] = []
        self._warned_subsample = False

    @property
    def results_raw(self) -> list[dict[str, float]]:
        """Raw results for all graphs and all k: one record per (batch, event, k), in scan order."""
        return self._results

    def get_results(self) -> KScanResults:
        """Per-k means of the records (NaN skipped, as pandas' ``groupby("k").mean()``)."""
        by_k: dict[int, list[dict[str, float]]] = {}
        for r in self._results:
            by_k.setdefault(r["k"], []).append(r)
        rows = []
        for k in sorted(by_k):
            recs = by_k[k]
            rows.append({"k": k, **{c: _mean_skipna([float(r[c]) for r in recs]) for c in recs[0] if c != "k"}})
        return KScanResults(rows, targets=self.hparams.targets)

    def get_foms(self) -> dict[str, float]:
        """Figures of merit (``get_results().get_foms()``)."""
        return self.get_results().get_foms()

    def reset(self):
        """Reset the results; called on every batch with ``i_batch == 0``."""
        self._results = []

    #: a collated ``data`` of more than one event (``ptr`` / ``batch``): every event is its own scan - neighbours,
    #: components and true edges inside the event, particles as (event, id) pairs (ids repeat from event to event,
    #: and id 0 is noise in all of them) - and gets its own record per k: the records of the events fed one by one,
    #: from one launch sequence.  False: the reference's behaviour, which ignores ``batch`` (one point cloud).  A
    #: class attribute so that YAML configurations stay those of the reference.
    per_event = True

    def __call__(self, data, i_batch: int, *, progress=False, latent: Tensor | None = None) -> None:
        """Run on a batch: ``data.x`` (or ``latent``) is the space the graph is built in, every event of the
        batch on its own (``per_event``).  ``progress`` is accepted and ignored (there is no per-k loop to
        show)."""
        if i_batch == 0:
            self.reset()
        if self.hparams.subsample_pids is not None and not self._warned_subsample:
            self._warned_subsample = True
            logger.warning("GraphConstructionKNNScanner: subsample_pids is ignored, all particles are evaluated")
        x = (latent if latent is not None else data.x).detach()
        self._results.extend(self.evaluate(data, x))

    @staticmethod
    def _record(k: int, c: dict[str, int], upper: dict[str, float]) -> dict[str, float]:
        """one record (k_scanner.py:248-285) from a row of the counts table and the flattened upper bounds"""
        return {
            "k": k,
            "frac50": _zdiv(c["n50"], c["n_pids"]),
            "frac75": _zdiv(c["n75"], c["n_pids"]),
            "frac100": _zdiv(c["n100"], c["n_pids"]),
            "n_edges": c["n_edges"],
            **efficiency_purity_from_counts(c["n_true_masked"], c["n_true_edges_masked"], c["n_masked"]),
            **{"max_" + key: v for key, v in upper.items()},
        }

    def evaluate(self, data, x: Tensor) -> list[dict[str, float]]:
        """The records of one batch (k_scanner.py:248-285 for every k, and with ``per_event`` for every event):
        one search, one counts call, one tracking-metrics call, one host copy."""
        hp = self.hparams
        ks = [int(k) for k in hp.ks]
        if not ks:
            return []
        lib = _capi.load()
        _capi.require_device(x)
        x = ops._as_rows(x.float() if x.dtype != torch.float32 else x)
        n, dev = int(x.shape[0]), x.device
        ptr = events.event_ptr(data, who="GraphConstructionKNNScanner") if self.per_event else None
        if n < 2:
            if ptr is None:
                raise ValueError("GraphConstructionKNNScanner: needs at least two hits")
            return []   # (no event of the batch has a graph to scan)
        if ptr is not None:
            ptr = ptr.to(device=dev, dtype=torch.int64).contiguous()
        kmax = min(max(ks), n - 1)
        nbr = torch.empty(n * kmax, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        r = float(hp.max_radius) if hp.max_radius is not None else -1.0
        ops._knn_search(lib, x, kmax, r, ptr, nbr, cnt, ops._stream(x))
        mask = get_good_node_mask(data, pt_thld=hp.pt_thld, max_eta=hp.max_eta)
        counts, labels = kscan_counts(nbr, cnt, kmax, [min(k, kmax) for k in ks], data.particle_id, mask,
                                      getattr(data, "true_edge_index", None), ptr=ptr)
        pts, cuts, idx = _cut_plan([0.9])   # (hard-coded in the reference: k_scanner.py:243)
        hits = _hits(data.particle_id, data.pt, data.reconstructable, data.eta, dev)
        trk = _tracking_counts(labels, *hits, cuts, 3, 4, ptr=ptr)
        # the batch's one host copy (the events' sizes ride along); one event is B = 1 of the batched layouts
        host = torch.cat([counts.reshape(-1), trk] + ([ptr] if ptr is not None else [])).cpu().numpy()
        sizes = [n] if ptr is None else np.diff(host[counts.numel() + trk.numel():]).tolist()
        table = host[:counts.numel()].reshape(len(sizes), len(ks), len(COUNT_COLUMNS))
        upper = _tracking_results(host[counts.numel():counts.numel() + trk.numel()], len(ks), sizes, pts, idx,
                                  ptr is not None)
        for e, n_e in enumerate(sizes):
            n_bad = int(table[e, 0, COUNT_COLUMNS.index("n_bad")])   # (the same in every row of the event)
            if n_bad:
                where = f"are outside [0, {n})" if ptr is None else f"of event {e} are outside its {n_e} hits"
                raise ValueError(f"GraphConstructionKNNScanner: {n_bad} neighbour or true-edge indices {where}")
        records = []
        for e, n_e in enumerate(sizes):
            if n_e < 2:   # (an event of a batch that alone has no graph to scan)
                continue
            for i, k in enumerate(ks):
                c = dict(zip(COUNT_COLUMNS, (int(v) for v in table[e, i])))
                if c["n_edges"] > hp.max_edges:
                    logger.warning(f"Not scanning k>={k}{'' if ptr is None else f' in event {e}'} because max edges "
                                   f"exceeded ({c['n_edges']} > {hp.max_edges})")
                    break
                records.append(self._record(k, c, upper[i][e]))
        return records
