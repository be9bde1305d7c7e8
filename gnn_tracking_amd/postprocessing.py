"""DBSCAN post-processing on the device.

Reference: postprocessing/fastrescanner.py:6-66 (``DBSCANFastRescan``: one radius graph at
``max_eps``, then ``cluster(eps, min_pts)`` for many hyperparameters, as the DBSCAN
hyperparameter scanners of postprocessing/dbscanscanner.py:146-187 call it).  Same
constructor, same ``cluster`` signature, same labels (cluster numbering, border points,
noise = -1); the graph and the clustering stay on the GPU, ``cluster`` hands back a numpy
array like the reference (``cluster_device`` the device tensor).

The DBSCAN hyperparameter scanners of the object-condensation validation
(postprocessing/clusterscanner.py, dbscanscanner.py:29-187) are here too: per batch one radius graph,
every trial's labels into one device buffer, and the tracking metrics of all trials from one C call
(``cluster_metrics.tracking_metrics_trials``) and one host copy.  ``DBSCANPerformanceDetails``
(dbscanscanner.py:215-264) keeps per batch the hit record on the device and the cluster table, the
inputs of ``cluster_metrics.tracking_metrics_vs_pt`` / ``_vs_eta``.

A collated batch of several events (``batch`` / ``ptr``, turned into row offsets and checked by ``events.py``) is that
many independent problems in one launch sequence: the radius graph has no edge between events, cluster labels are local
to the event (noise -1, the clusters of an event numbered from 0, so ``labels[ptr[e]:ptr[e + 1]]`` is what the event
alone gives), the tracking metrics come per event, and the scanners append one record per (event, trial) - exactly the
results of the events fed one by one (``DBSCANHyperParamScanner.per_event``).  One event - no offsets, or offsets of one
event - takes the single-event C entries.
"""

from __future__ import annotations

import math
import os
from abc import ABC, abstractmethod
from typing import Any

import numpy as np
import torch
from torch import Tensor

from . import _capi, events, ops
from .cluster_metrics import _nanmean, _nanstd
from .hparams import HyperparametersMixin


#: bit 0: pruned radius graph below its size threshold too; bit 1: brute force only (tests, measurements)
RADIUS_FLAGS = int(os.environ.get("GNNTRK_RADIUS_FLAGS", "0"))


class DBSCANFastRescan:
    def __init__(self, x, max_eps: float = 1.0, *, batch=None, ptr=None, n_jobs: int | None = None, device=None):
        """Args as fastrescanner.py:7-24 (``n_jobs`` is accepted and ignored).  ``x``: the
        cluster coordinates ``[N, D]``, D <= 32 - a device tensor, or a numpy array /
        host tensor that is copied to ``device`` (default ``cuda:0``).

        ``batch`` (sorted event id per hit) or ``ptr`` (``[B + 1]`` row offsets) of a collated batch: with more than
        one event every event is clustered on its own, in the same launches - no neighbourhood crosses an event,
        ``cluster_device`` / ``cluster`` return labels local to the event (noise -1, clusters from 0 in every event)
        and ``cluster_ptr`` (int64 ``[B + 1]`` on the device: the number of clusters of the events before each, then
        the total) is set by each call."""
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x))
        if not x.is_cuda and device is None and torch.cuda.is_available():
            device = torch.device("cuda", 0)
        if device is not None:
            x = x.to(device)
        _capi.require_device(x)
        if x.dim() != 2:
            raise ValueError("DBSCANFastRescan: x must be [N, D]")
        self.x = ops._as_rows(x.detach().to(torch.float32))
        self._max_eps = float(max_eps)
        self._n_jobs = n_jobs
        self._ptr = None
        self.cluster_ptr: Tensor | None = None
        seg = events.event_ptr(batch=batch, ptr=ptr, who="DBSCANFastRescan")
        if seg is not None:
            events.event_sizes(seg, int(x.shape[0]), "DBSCANFastRescan",
                               "the events' offsets must ascend from 0 to the number of points")
            self._ptr = seg.to(device=self.x.device, dtype=torch.int64).contiguous()
        self._reset_graph(self._max_eps)

    def _reset_graph(self, max_eps: float) -> None:
        """The radius-neighbourhood graph (fastrescanner.py:25-39): CSR offsets, neighbour
        ids and fp64 distances."""
        lib = _capi.load()
        x = self.x
        n, dim = int(x.shape[0]), int(x.shape[1])
        st = ops._stream(x)
        cnt = torch.empty(max(n, 1), dtype=torch.int32, device=x.device)
        self._off = torch.empty(n + 1, dtype=torch.int64, device=x.device)
        # (the library prunes the N^2 walk with the sorted chunks it builds in ws_p; same output)
        nb = int(lib.gnntrk_radius_points_workspace_bytes(n, dim))
        ws_p = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
        head = (ops._p(x), n, dim, ops._row_stride(x), float(max_eps))
        if self._ptr is None:
            count, fill = lib.gnntrk_radius_count_ws, lib.gnntrk_radius_fill_ws
        else:   # (every event its own graph: the same entries with the events' offsets)
            count, fill = lib.gnntrk_radius_count_batched_ws, lib.gnntrk_radius_fill_batched_ws
            head += (ops._p(self._ptr), int(self._ptr.numel()) - 1)
        _capi.check(count(*head, ops._p(cnt), ops._p(self._off), ops._p(ws_p), nb, RADIUS_FLAGS, st), lib)
        m = int(self._off[n].item())
        self._nbr = torch.empty(max(m, 1), dtype=torch.int32, device=x.device)
        self._dist = torch.empty(max(m, 1), dtype=torch.float64, device=x.device)
        ne = int(lib.gnntrk_radius_edges_workspace_bytes(m)) if nb else 0
        ws_e = torch.empty(ne, dtype=torch.uint8, device=x.device) if ne else None
        _capi.check(fill(*head, ops._p(self._off), m, ops._p(self._nbr), ops._p(self._dist), ops._p(ws_p), nb,
                         ops._p(ws_e), ne, RADIUS_FLAGS, st), lib)
        self._n_edges = m
        self._max_eps = float(max_eps)

    def cluster_device(self, eps: float = 1.0, min_pts: int = 1) -> Tensor:
        """Labels as an int64 device tensor (several events: local to the event, and ``cluster_ptr`` is set)."""
        if eps > self._max_eps:
            self._reset_graph(eps)
        lib = _capi.load()
        x = self.x
        n = int(x.shape[0])
        dev = x.device
        st = ops._stream(x)
        core = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        root = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        changed = torch.ones(1, dtype=torch.int32, device=dev)
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        args = (ops._p(self._off), ops._p(self._nbr), ops._p(self._dist), n, float(eps))
        _capi.check(lib.gnntrk_dbscan_init(args[0], args[2], n, float(eps), int(min_pts), ops._p(core),
                                           ops._p(root), st), lib)
        # a few rounds per host check (compact clusters need one or two), more per check for
        # long chains; n rounds always suffice (the lowest index moves at least one hop per round)
        rounds, done = 4, 0
        while True:
            _capi.check(lib.gnntrk_dbscan_propagate(*args, ops._p(core), ops._p(root), rounds, ops._p(changed), st),
                        lib)
            done += rounds
            if int(changed.item()) == 0:
                break
            if done > n + 8:
                raise RuntimeError("DBSCAN label propagation did not converge")
            rounds = min(2 * rounds, 64)
        ws = torch.empty(max(int(lib.gnntrk_dbscan_workspace_bytes(n)), 256), dtype=torch.uint8, device=dev)
        if self._ptr is None:   # (as _reset_graph: the same entry with the events' offsets)
            entry, seg, n_clusters = lib.gnntrk_dbscan_labels, (), torch.empty(1, dtype=torch.int64, device=dev)
        else:
            n_ev = int(self._ptr.numel()) - 1
            entry, seg = lib.gnntrk_dbscan_labels_batched, (ops._p(self._ptr), n_ev)
            n_clusters = self.cluster_ptr = torch.empty(n_ev + 1, dtype=torch.int64, device=dev)
        _capi.check(entry(*args, ops._p(core), ops._p(root), *seg, ops._p(labels), ops._p(n_clusters), ops._p(ws),
                          ws.numel(), st), lib)
        return labels

    def cluster(self, eps: float = 1.0, min_pts: int = 1) -> np.ndarray:
        """fastrescanner.py:41-66: DBSCAN labels (``np.intp``), noise = -1."""
        return self.cluster_device(eps, min_pts).cpu().numpy().astype(np.intp)


def dbscan(x, eps: float, min_samples: int, device=None) -> np.ndarray:
    """``sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(x)`` on the device."""
    return DBSCANFastRescan(x, max_eps=eps, device=device).cluster(eps, min_samples)


# ------------------------------------------------------------------ cluster scanners
class ClusterScanner(HyperparametersMixin, ABC):
    """``postprocessing/clusterscanner.py:9-31``: base class of the validation-time scanners."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    @abstractmethod
    def __call__(self, data, out: dict[str, Tensor], i_batch: int) -> None:
        pass

    def reset(self) -> None:
        pass

    def get_foms(self) -> dict[str, Any]:
        return {}


class CombinedClusterScanner(ClusterScanner):
    """``clusterscanner.py:34-54``: several scanners as one."""

    def __init__(self, scanners: list[ClusterScanner]):
        super().__init__()
        self._scanners = scanners

    def __call__(self, *args, **kwargs):
        for scanner in self._scanners:
            scanner(*args, **kwargs)

    def reset(self) -> None:
        for scanner in self._scanners:
            scanner.reset()

    def get_foms(self) -> dict[str, Any]:
        foms = {}
        for scanner in self._scanners:
            foms |= scanner.get_foms()
        return foms


class OCScanResults:
    """``dbscanscanner.py:29-73`` without pandas.  ``records``: one dict per (batch, trial) with
    ``i_batch``, ``eps``, ``min_samples`` and the flattened tracking metrics.  Grouped by (eps,
    min_samples) in ascending order, every other column (``i_batch`` included, as in the reference)
    gets its NaN-skipping mean and a ``_std`` column: the ddof = 1 std over the group's rows divided
    by the square root of the number of GROUPS - the reference's expression, kept as it is."""

    def __init__(self, records: list[dict[str, float]]):
        self._parameters = ["eps", "min_samples"]
        self._records = list(records)
        cols: dict[str, None] = {}
        for r in self._records:
            cols.update(dict.fromkeys(r))
        self._cols = [c for c in cols if c not in self._parameters]
        groups: dict[tuple, list[dict]] = {}
        for r in self._records:
            groups.setdefault((r["eps"], r["min_samples"]), []).append(r)
        norm = math.sqrt(len(groups))
        self._rows = []
        for key in sorted(groups):
            rows = groups[key]
            vals = {c: np.array([float(r.get(c, float("nan"))) for r in rows], dtype=np.float64) for c in self._cols}
            row = {"eps": key[0], "min_samples": key[1]}
            row.update({c: _nanmean(v) for c, v in vals.items()})
            row.update({c + "_std": _nanstd(v) / norm for c, v in vals.items()})
            self._rows.append(row)

    @property
    def records(self) -> list[dict[str, float]]:
        return self._records

    @property
    def mean_rows(self) -> list[dict[str, float]]:
        """Mean and std grouped by hyperparameters (the reference's ``df_mean``, one dict per row)."""
        return self._rows

    def get_foms(self, guide="double_majority_pt0.9") -> dict[str, float]:
        """Figures of merit of the (eps, min_samples) with the largest mean ``guide`` (first one on
        ties, NaN skipped): every mean and std column with the prefix ``trk.``, then
        ``best_dbscan_eps`` and ``best_dbscan_min_samples`` (floats, as the reference's row)."""
        fom_cols = [c for c in self._rows[0] if c not in self._parameters] if self._rows else []
        assert guide in fom_cols
        g = np.array([r[guide] for r in self._rows], dtype=np.float64)
        if np.isnan(g).all():
            raise ValueError(f"OCScanResults: {guide} is NaN for every parameter set")
        best = self._rows[int(np.nanargmax(g))]
        foms = {f"trk.{c}": float(best[c]) for c in fom_cols}
        for param in self._parameters:
            foms[f"best_dbscan_{param}"] = float(best[param])
        return foms

    def get_n_best_trials(self, n: int, guide="double_majority_pt0.9") -> list[dict[str, float]]:
        g = np.array([r[guide] for r in self._rows], dtype=np.float64)
        order = sorted(range(len(g)), key=lambda i: (np.isnan(g[i]), -g[i] if not np.isnan(g[i]) else 0.0))
        return [{p: self._rows[i][p] for p in self._parameters} for i in order[:n]]


class DBSCANHyperParamScanner(ClusterScanner):
    #: data of more than one event (``batch`` / ``ptr``): every event is its own problem (its own radius graph,
    #: cluster numbers and particles - ids repeat from event to event, and id 0 is noise in all of them) and gets its
    #: own record per trial - the records of the events fed one by one, from one launch sequence.  False: the
    #: reference's behaviour, which ignores ``batch`` (one DBSCAN over the hits of all events: hits of different
    #: events that share a latent position are clustered together).  A class attribute so that YAML configurations
    #: stay those of the reference.
    per_event = True

    def __init__(self, *, eps_range=(0, 1), min_samples_range=(1, 4), n_trials=10, keep_best=0,
                 n_jobs: int | None = None, guide: str = "double_majority_pt0.9", pt_thlds=(0.0, 0.5, 0.9, 1.5),
                 max_eta: float = 4.0):
        """``dbscanscanner.py:76-187``: random (eps, min_samples) DBSCAN trials per batch, tracking metrics
        per trial, figures of merit of the best trial over the epoch.  Same arguments (``n_jobs`` is
        accepted and ignored).  Per batch: one ``DBSCANFastRescan`` on ``out["H"]`` where it lies, all
        trials' labels into one device buffer, one metrics call and one host copy."""
        super().__init__()
        self.save_hyperparameters()
        # (the reference's backwards compatibility: a "trk." prefix of the guide is dropped)
        self.hparams.guide = self.hparams.guide.removeprefix("trk.")
        self._results: list[dict[str, float]] = []
        self._rng = np.random.default_rng()
        self._trials: list[dict[str, float]] = []
        self.reset()

    def get_results(self) -> OCScanResults:
        return OCScanResults(self._results)

    def get_foms(self) -> dict[str, float]:
        return self.get_results().get_foms()

    def _get_best_trials(self) -> list[dict[str, float]]:
        if not self._results:
            return []
        return self.get_results().get_n_best_trials(self.hparams.keep_best)

    def _reset_trials(self) -> None:
        # As the reference (dbscanscanner.py:133-142), kept for parity rather than fixed: the best
        # trials only shorten the random draw, which then replaces them.
        self._trials = self._get_best_trials()
        size_random = self.hparams.n_trials - len(self._trials)
        eps = self._rng.uniform(*self.hparams.eps_range, size=size_random)
        min_samples = self._rng.integers(self.hparams.min_samples_range[0], self.hparams.min_samples_range[1] + 1,
                                         size=size_random)
        self._trials = [{"eps": e, "min_samples": n} for e, n in zip(eps, min_samples)]

    def reset(self):
        """Reset the results; called on every batch with ``i_batch == 0``."""
        self._reset_trials()
        self._best_trials = []
        self._results = []

    def __call__(self, data, out: dict[str, Tensor], i_batch: int, *, progress=False):
        from .cluster_metrics import _metrics_per_event

        ec_hit_mask = out.get("ec_hit_mask")
        if ec_hit_mask is not None and not bool(ec_hit_mask.all()):
            raise NotImplementedError("Handling of orphan node pruning not implemented")
        if i_batch == 0:
            self.reset()
        if not self._trials:
            return
        ptr = events.event_ptr(data, who="DBSCANHyperParamScanner") if self.per_event else None
        scanner = DBSCANFastRescan(out["H"].detach(), max_eps=max(v["eps"] for v in self._trials), ptr=ptr,
                                   n_jobs=self.hparams.n_jobs)
        n = int(scanner.x.shape[0])
        labels = torch.empty((len(self._trials), n), dtype=torch.int64, device=scanner.x.device)
        for k, trial in enumerate(self._trials):
            labels[k] = scanner.cluster_device(eps=trial["eps"], min_pts=trial["min_samples"])
        metrics = _metrics_per_event(labels, truth=data.particle_id, pts=data.pt, eta=data.eta,
                                     reconstructable=data.reconstructable, pt_thlds=self.hparams.pt_thlds,
                                     predicted_count_thld=3, max_eta=self.hparams.max_eta, ptr=ptr)
        for e in range(len(metrics[0])):       # (records grouped by event: as the events fed one by one)
            for trial, per_event in zip(self._trials, metrics):
                self._results.append({"i_batch": i_batch, "eps": trial["eps"], "min_samples": trial["min_samples"],
                                      **per_event[e]})


class DBSCANHyperParamScannerFixed(DBSCANHyperParamScanner):
    def __init__(self, trials: list[dict[str, float]], *, n_jobs: int | None = None, pt_thlds=(0.0, 0.5, 0.9, 1.5),
                 max_eta: float = 4.0):
        """``dbscanscanner.py:190-214``: the given trials on every batch."""
        super().__init__(n_jobs=n_jobs, pt_thlds=pt_thlds, max_eta=max_eta)
        self._trials = trials

    def _reset_trials(self) -> None:
        pass


class DBSCANPerformanceDetails(DBSCANHyperParamScanner):
    def __init__(self, eps: float, min_samples: int):
        """``dbscanscanner.py:215-264``: the detailed performance of fixed DBSCAN parameters.  Per batch
        the device DBSCAN of ``out["H"]``, then the hit record (``c``, ``id``, ``reconstructable``,
        ``pt``, ``eta`` as device tensors) and the cluster table
        (``cluster_metrics.tracking_metric_table``: numpy columns) are kept; see ``get_results``.  As
        the reference, it neither resets on ``i_batch == 0`` nor looks at ``ec_hit_mask``.  Data of several events
        (``per_event``): one DBSCAN and one cluster-table call for all of them, then one hit record
        (``cluster_metrics.HitRecord``: a dict with the same five keys that remembers its batch, so that the binned
        metrics count the events of a batch in one call) and one cluster table per event."""
        super().__init__()
        self.save_hyperparameters()
        self._h_dfs: list[dict[str, Tensor]] = []
        self._c_dfs: list[dict[str, np.ndarray]] = []

    def __call__(self, data, out: dict[str, Tensor], i_batch: int) -> None:
        from . import cluster_metrics as CM

        ptr = events.event_ptr(data, who="DBSCANPerformanceDetails") if self.per_event else None
        fr = DBSCANFastRescan(out["H"].detach(), max_eps=self.hparams.eps, ptr=ptr)
        labels = fr.cluster_device(eps=self.hparams.eps, min_pts=self.hparams.min_samples)
        dev = labels.device
        pid, pt, reco, eta = CM._hits(data.particle_id, data.pt, data.reconstructable, data.eta, dev)
        record = {"c": labels, "id": pid, "reconstructable": reco, "pt": pt, "eta": eta}
        # (DBSCAN's labels are in [-1, n) - several events: in [-1, n_e) - already: no ranking pass)
        if ptr is None:
            self._h_dfs.append(record)
            self._c_dfs.append(CM._table(labels, None, pid, pt, reco, eta, 3))
            return
        # several events: one DBSCAN and one table call for all, then per event its slice of the hits (a record that
        # remembers the batch: tracking_metrics_vs_pt / _vs_eta count the events of a batch in one call) and its table
        batch = CM.EventBatch(record, ptr.to(device=dev, dtype=torch.int64).contiguous())
        self._h_dfs.extend(batch.records)
        self._c_dfs.extend(CM._table(labels, None, pid, pt, reco, eta, 3, batch.ptr, batch.sizes))

    def get_results(self) -> tuple[list[dict[str, Tensor]], list[dict[str, np.ndarray]]]:
        """(h_dfs, c_dfs): per batch the hit record and the cluster table, as
        ``tracking_metrics_vs_pt`` / ``tracking_metrics_vs_eta`` take them."""
        return self._h_dfs, self._c_dfs

    def get_foms(self) -> dict[str, float]:
        return {}
