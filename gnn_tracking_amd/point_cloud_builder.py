"""Point cloud builder on the device (``preprocessing/point_cloud_builder.py``): the tables of a TrackML event (hits,
cells, particles, truth) and the detector table to the sector point clouds that ``GraphBuilder`` and
``MLGraphConstruction`` read.

The reference is a chain of pandas merges and group-bys and, per sector, a Python loop over particle ids.  Here the
joins, the per-hit cell reduction, the feature rows, the per-particle counts, the sector predicate of every (hit,
sector), the stable fill of all clouds and the pair expansion of the truth edges are flat passes of
``csrc/point_cloud.hip``.  ``build`` makes ONE host read per event: the sizes and every counter.

Contract:

* Joins are by ``hit_id`` and ``particle_id``, never by position; the clouds keep the order of the hit table.  Where the
  reference would misalign silently or fail, ``build`` raises ``ValueError`` after the host read: duplicate ``hit_id``
  or ``particle_id``, several truth rows of one hit, a hit on a layer without cells, a kept hit on a module the
  detector table lacks, a ``volume_id`` / ``layer_id`` outside [0, 64).
* Features are evaluated in float64, divided by ``feature_scale`` in float64 and rounded once to float32.
* Noise hits (particle id 0) have ``pt`` 0 and ``eta`` NaN, as the reference's concatenation leaves them.
* Sector membership is decided with float64 ``+ - *`` on constants computed with numpy on the host: it is the
  reference's bit for bit.  ``sector`` is the reference's, not its comment's: the reference divides a particle's hits in
  the wedge by the length of the particle's ROW of its per-particle table (1), so a particle with id > 0 carries
  ``sector == s`` in every cloud ``s`` whose plain wedge holds at least one of its hits, and ``majority_contained`` is
  counted with the same denominator.
* The directory loop ``process()`` is ``data_transformer.build_point_clouds``, the ``.pt`` writer ``io.GraphWriter``; the
  ``.pickle`` detector cache is not part of this package.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

from . import _capi, ops
from .data import Data
from .hparams import HyperparametersMixin

__all__ = ["PointCloudBuilder", "DEFAULT_FEATURES", "load_detector", "get_truth_edge_index", "read_event"]

DEFAULT_FEATURES = ("r", "phi", "z", "eta_rz", "u", "v", "charge_frac", "leta", "lphi", "lx", "ly", "lz", "geta", "gphi")
#: the order of the feature codes of ``gnntrk_point_cloud_select``
FEATURE_CODES = ("x", "y", "z", "r", "phi", "eta_rz", "u", "v", "charge_frac", "cell_count", "cell_val", "leta", "lphi",
                 "lx", "ly", "lz", "geta", "gphi", "V7", "V8", "V9", "V12", "V13", "V14", "V16", "V17", "V18")
_PIXEL_LAYERS = tuple(sorted([(8, 2), (8, 4), (8, 6), (8, 8)] + [(7, l) for l in range(2, 16, 2)]
                             + [(9, l) for l in range(2, 16, 2)]))
_MAX_IDS = 64            # GNNTRK_PC_MAX_IDS
_HEAD, _SEC_COUNTS = 12, 6
_TABLES = {"hits": ("hit_id", "x", "y", "z", "volume_id", "layer_id", "module_id"),
           "cells": ("hit_id", "ch0", "ch1", "value"),
           "particles": ("particle_id", "px", "py", "pz", "q", "vx", "vy"),
           "truth": ("hit_id", "particle_id")}
_DETECTOR = ("volume_id", "layer_id", "module_id", "rot_xu", "rot_xv", "rot_xw", "rot_yu", "rot_yv", "rot_yw", "rot_zu",
             "rot_zv", "rot_zw", "module_t", "pitch_u", "pitch_v")
_ERRORS = ((1, "duplicate hit_ids in the hit table"), (2, "hits on a layer without cells"),
           (3, "kept hits on a module that the detector table lacks"),
           (4, "hits with a volume_id or layer_id outside [0, 64)"), (5, "further truth rows of one hit"),
           (6, "duplicate particle_ids in the particle table"))


def _default_device() -> torch.device:
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def load_detector(table) -> dict:
    """The per-module table of the detector, host only.  ``table`` maps the column names of ``detectors.csv`` to arrays
    (a pandas frame works).  Returns ``rows`` float64 [modules, 12] (the 3 x 3 rotation row-major, ``module_t``,
    ``pitch_u``, ``pitch_v``), ``index`` int32 [volumes, layers, modules] (row of a module, -1 where there is none) and
    ``dims``.  Unlike the reference's three dense arrays (65 MB of rotations) this is 12 doubles per module."""
    cols = {k: np.asarray(table[k]) for k in _DETECTOR}
    vlm = np.stack([cols[k].astype(np.int64) for k in _DETECTOR[:3]], axis=1)
    if vlm.size and vlm.min() < 0:
        raise ValueError("load_detector: negative volume_id, layer_id or module_id")
    rows = np.ascontiguousarray(np.stack([cols[k].astype(np.float64) for k in _DETECTOR[3:]], axis=1))
    dims = (vlm.max(axis=0) + 1) if len(vlm) else np.zeros(3, np.int64)
    index = np.full(tuple(int(d) for d in dims), -1, np.int32)
    index[vlm[:, 0], vlm[:, 1], vlm[:, 2]] = np.arange(len(vlm), dtype=np.int32)   # (a repeated module: its last row)
    return {"rows": rows, "index": index, "dims": np.asarray(dims, np.int32)}


def read_event(prefix) -> dict:
    """Host-only reader of ``prefix-{hits,cells,particles,truth}.csv.gz`` (plain ``.csv`` too): a dict of the four
    tables, each a dict of numpy columns, the input of ``PointCloudBuilder.build``.  pandas where importable,
    ``numpy.genfromtxt`` otherwise.  Not on the hot path.  Float parsing may differ from the reference's (pandas'
    default C parser) by one float64 ulp."""
    out = {}
    for name in _TABLES:
        path = Path(f"{prefix}-{name}.csv.gz")
        if not path.exists():
            path = Path(f"{prefix}-{name}.csv")
        try:
            import pandas as pd
        except ImportError:
            rec = np.atleast_1d(np.genfromtxt(path, delimiter=",", names=True, dtype=None, encoding="utf-8"))
            out[name] = {k: np.ascontiguousarray(rec[k]) for k in rec.dtype.names}
        else:
            frame = pd.read_csv(path, header=0, index_col=False)
            out[name] = {k: frame[k].to_numpy() for k in frame.columns}
    return out


def _device_of(arrays) -> torch.device:
    for a in arrays:
        if torch.is_tensor(a):
            return a.device
    return _default_device()


def _col(a, dtype, dev) -> Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return t.detach().to(device=dev, dtype=dtype).contiguous()


def _stack(table, names, dtype, dev) -> Tensor:
    return torch.stack([_col(table[k], dtype, dev) for k in names], dim=1).contiguous()


def _truth_edges(lib, pid: Tensor, seg_ptr: Tensor, n_edges: int | None, global_ids: bool):
    """(edge_index flat int64 [2 * E], edge_ptr int64 [segments + 1]); ``n_edges=None``: counted first (a host read)"""
    n, n_seg, dev = int(pid.numel()), int(seg_ptr.numel()) - 1, pid.device
    p, stream = ops._p, ops._stream(pid)
    ws = ops._ws(lib.gnntrk_truth_edges_workspace_bytes(n), pid)
    if n_edges is None:
        counts = torch.empty(n_seg, dtype=torch.int64, device=dev)
        _capi.check(lib.gnntrk_truth_edges_count(p(pid) if n else None, n, p(seg_ptr), n_seg, p(counts), p(ws), ws.numel(),
                                                 stream), lib)
        n_edges = int(counts.sum().cpu())
    ei = torch.empty(2 * n_edges, dtype=torch.int64, device=dev)
    edge_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
    _capi.check(lib.gnntrk_truth_edges_fill(p(pid) if n else None, n, p(seg_ptr), n_seg, n_edges, int(global_ids),
                                            p(ei) if n_edges else None, p(edge_ptr), p(ws), ws.numel(), stream), lib)
    return ei, edge_ptr


def get_truth_edge_index(particle_id) -> Tensor:
    """``[2, E]`` int64 on the device: every pair ``i < j`` of hits with the same non-zero particle id, in
    lexicographic ``(i, j)`` order (the order the reference's merge, sort and ``drop_duplicates`` leave).  One
    direction only.  One host read (the number of pairs)."""
    pid = _col(particle_id, torch.int64, _device_of([particle_id]))
    _capi.require_device(pid)
    if pid.dim() != 1:
        raise ValueError(f"get_truth_edge_index: particle_id must have one dimension, got {tuple(pid.shape)}")
    seg_ptr = torch.tensor([0, pid.numel()], dtype=torch.int64, device=pid.device)
    return _truth_edges(_capi.load(), pid, seg_ptr, None, True)[0].view(2, -1)


class PointCloudBuilder(HyperparametersMixin):
    def __init__(self, *, detector: dict, n_sectors: int, pixel_only: bool = True, sector_di: float = 0.0001,
                 sector_ds: float = 1.1, measurement_mode: bool = False, thld: float = 0.5, remove_noise: bool = False,
                 feature_names: tuple = DEFAULT_FEATURES, feature_scale: tuple | None = None,
                 add_true_edges: bool = False):
        """Build point clouds: the tables of an event to ``Data`` objects without edges (or with the truth edges).

        Args:
            detector: what ``load_detector`` returned
            n_sectors: total number of sectors
            pixel_only: keep the hits of the 18 pixel layers only (otherwise every (volume, layer) of the event)
            sector_di: the intercept offset of the extended sector
            sector_ds: the slope factor of the extended sector
            measurement_mode: keep a record per (event, sector) in ``measurements``
            thld: pt threshold of ``majority_contained``
            remove_noise: drop the hits with particle id 0
            feature_names: names of the columns of ``x``
            feature_scale: their divisors (default: 1 each)
            add_true_edges: ``edge_index`` holds the truth edges of the cloud
        """
        self.save_hyperparameters(ignore=["detector"])
        self.n_sectors = int(n_sectors)
        if self.n_sectors < 1:
            raise ValueError("PointCloudBuilder: n_sectors must be >= 1")
        self.pixel_only, self.sector_di, self.sector_ds = bool(pixel_only), float(sector_di), float(sector_ds)
        self.measurement_mode, self.thld, self.remove_noise = bool(measurement_mode), float(thld), bool(remove_noise)
        self.feature_names = list(feature_names)
        self.feature_scale = [1.0] * len(self.feature_names) if feature_scale is None else [float(v) for v in feature_scale]
        if len(self.feature_names) != len(self.feature_scale):
            raise ValueError("PointCloudBuilder: feature_names and feature_scale differ in length")
        unknown = [f for f in self.feature_names if f not in FEATURE_CODES]
        if unknown or not self.feature_names:
            raise ValueError(f"PointCloudBuilder: unknown or no features {unknown}; known: {FEATURE_CODES}")
        self.add_true_edges = bool(add_true_edges)
        self.stats: dict[int, dict[str, int]] = {}
        self.measurements: list[dict] = []
        self._detector = {k: np.asarray(detector[k]) for k in ("rows", "index", "dims")}
        self._on_device: dict = {}

    # ------------------------------------------------------------------------------------------------ host tables
    def _detector_on(self, dev):
        if dev not in self._on_device:
            d = self._detector
            self._on_device[dev] = (torch.from_numpy(np.ascontiguousarray(d["index"], np.int32).reshape(-1)).to(dev),
                                    torch.from_numpy(np.ascontiguousarray(d["rows"], np.float64)).to(dev))
        return self._on_device[dev]

    def _layer_map(self, vlm: Tensor) -> Tensor:
        """int32 [64 * 64] on the device: (volume_id, layer_id) -> layer; no host read"""
        dev = vlm.device
        if self.pixel_only:
            m = np.full((_MAX_IDS, _MAX_IDS), -1, np.int32)
            for i, (v, l) in enumerate(_PIXEL_LAYERS):
                m[v, l] = i
            return torch.from_numpy(m.reshape(-1)).to(dev)
        v, l = vlm[:, 0].long(), vlm[:, 1].long()
        ok = (v >= 0) & (v < _MAX_IDS) & (l >= 0) & (l < _MAX_IDS)      # (the others are counted by the kernel)
        present = torch.zeros(_MAX_IDS * _MAX_IDS, dtype=torch.int32, device=dev)
        present[torch.where(ok, v * _MAX_IDS + l, 0)] = 1
        if vlm.numel():
            present[0] = ((v == 0) & (l == 0)).any().to(torch.int32)
        return torch.where(present > 0, torch.cumsum(present, 0, dtype=torch.int32) - 1,
                           torch.full_like(present, -1)).contiguous()

    def _sector_constants(self):
        """cos and sin of 2 s theta and slope = arctan(theta), with numpy as the reference computes them"""
        theta = np.pi / self.n_sectors
        cs = np.array([[np.cos(2 * s * theta), np.sin(2 * s * theta)] for s in range(self.n_sectors)], np.float64)
        return cs, float(np.arctan(theta))

    # ----------------------------------------------------------------------------------------------------- public
    def build(self, tables: dict, evtid: int = -1, *, collated: bool = False):
        """The point clouds of one event: a list of ``n_sectors`` ``Data`` (``x`` float32, ``edge_index``, ``y`` (empty),
        ``layer``, ``particle_id``, ``pt``, ``reconstructable``, ``sector``, ``eta``, ``n_hits``, ``n_layers_hit``, on the
        device), or with ``collated=True`` the same clouds as one batch, equal to ``collate(list)`` field by field.

        ``tables`` maps ``hits`` / ``cells`` / ``particles`` / ``truth`` to dicts of columns (numpy arrays or tensors;
        ``read_event`` returns this).  ``stats[evtid]`` and, with ``measurement_mode``, one record per sector in
        ``measurements`` are filled from the one host read."""
        for name, need in _TABLES.items():
            missing = [k for k in need if k not in tables[name] and not (name == "particles" and k in ("q", "vx", "vy"))]
            if missing:
                raise ValueError(f"PointCloudBuilder: table '{name}' lacks the columns {missing}")
        hits, cells, parts, truth = (tables[k] for k in ("hits", "cells", "particles", "truth"))
        dev = _device_of([hits["hit_id"], cells["hit_id"]])
        i64, i32, f64 = torch.int64, torch.int32, torch.float64
        hit_id, xyz = _col(hits["hit_id"], i64, dev), _stack(hits, ("x", "y", "z"), f64, dev)
        vlm = _stack(hits, ("volume_id", "layer_id", "module_id"), i32, dev)
        cell_hit, cell_ch = _col(cells["hit_id"], i64, dev), _stack(cells, ("ch0", "ch1"), i32, dev)
        cell_val = _col(cells["value"], f64, dev)
        part_id, part_p = _col(parts["particle_id"], i64, dev), _stack(parts, ("px", "py", "pz"), f64, dev)
        truth_hit, truth_pid = _col(truth["hit_id"], i64, dev), _col(truth["particle_id"], i64, dev)
        _capi.require_device(hit_id, cell_hit, part_id, truth_hit)
        H, Cn, P, T = int(hit_id.numel()), int(cell_hit.numel()), int(part_id.numel()), int(truth_hit.numel())
        if cell_val.numel() != Cn or truth_pid.numel() != T:
            raise ValueError("PointCloudBuilder: the columns of a table differ in length")
        lib, S, F = _capi.load(), self.n_sectors, len(self.feature_names)
        p, stream = ops._p, ops._stream(hit_id)
        addr = lambda t: p(t) if t.numel() else None   # noqa: E731
        det_index, det_rows = self._detector_on(dev)
        dims = (C.c_int32 * 3)(*[int(d) for d in self._detector["dims"]])
        codes = (C.c_int32 * F)(*[FEATURE_CODES.index(f) for f in self.feature_names])
        scale = (C.c_double * F)(*self.feature_scale)
        layer_map = self._layer_map(vlm)

        # ---- the kept hits of the event (columns with room for every hit) and the rows of all clouds
        x = torch.empty((H, F), dtype=torch.float32, device=dev)
        cols = torch.empty((6, H), dtype=i64, device=dev)
        pt_eta = torch.empty((2, H), dtype=torch.float32, device=dev)
        uv = torch.empty((H, 2), dtype=f64, device=dev)
        slot = torch.empty(H, dtype=i32, device=dev)
        head = torch.zeros(_HEAD + 2 + S * _SEC_COUNTS, dtype=i64, device=dev)
        sec_head, counts = head[_HEAD:_HEAD + 2], head[_HEAD + 2:]
        ws = ops._ws(lib.gnntrk_point_cloud_select_workspace_bytes(H, Cn, P), hit_id)
        _capi.check(lib.gnntrk_point_cloud_select(
            addr(hit_id), addr(xyz), addr(vlm), H, addr(cell_hit), addr(cell_ch), addr(cell_val), Cn, addr(part_id),
            addr(part_p), P, addr(truth_hit), addr(truth_pid), T, p(layer_map), addr(det_index), dims, addr(det_rows),
            int(det_rows.shape[0]), codes, scale, F, int(self.remove_noise), addr(x), addr(cols), addr(pt_eta), addr(uv),
            addr(slot), p(head), p(ws), ws.numel(), stream), lib)
        cs, slope = self._sector_constants()
        sector_cs = torch.from_numpy(cs).to(dev)
        sws = ops._ws(lib.gnntrk_point_cloud_sectors_workspace_bytes(H, P, S), hit_id)
        _capi.check(lib.gnntrk_point_cloud_sectors(
            addr(uv), addr(slot), p(head), H, addr(part_p), P, S, p(sector_cs), slope,
            self.sector_ds, self.sector_di, self.thld, p(counts), p(sec_head), p(sws), sws.numel(), stream), lib)
        host = head.cpu().numpy()                                            # the one host read
        for k, what in _ERRORS:
            if host[k]:
                raise ValueError(f"PointCloudBuilder: {int(host[k])} {what}")
        n_rows, n_pairs = int(host[_HEAD]), int(host[_HEAD + 1])
        sec = host[_HEAD + 2:].reshape(S, _SEC_COUNTS)

        # ---- the clouds, one after the other
        x_out = torch.empty((n_rows, F), dtype=torch.float32, device=dev)
        cols_out = torch.empty((6, n_rows), dtype=i64, device=dev)
        pte_out = torch.empty((2, n_rows), dtype=torch.float32, device=dev)
        _capi.check(lib.gnntrk_point_cloud_gather(
            addr(x), addr(cols), addr(pt_eta), addr(slot), H, F, P, S, n_rows, addr(x_out), addr(cols_out), addr(pte_out),
            p(sws), sws.numel(), stream), lib)
        offs = np.concatenate([[0], np.cumsum(sec[:, 1])]).astype(np.int64)
        assert offs[-1] == n_rows
        ptr = torch.from_numpy(offs).to(dev)
        if self.add_true_edges:
            ei, edge_ptr = _truth_edges(lib, cols_out[1], ptr, n_pairs, collated)
            e_offs = np.concatenate([[0], np.cumsum(sec[:, 5])]).astype(np.int64)
        else:
            ei, e_offs = torch.zeros(0, dtype=i64, device=dev), np.zeros(S + 1, np.int64)

        self.stats[evtid] = {"n_hits": int(host[0]), "n_particles": int(host[7]), "n_noise": int(host[8]),
                             "n_sector_hits": int(sec[:, 1].sum()), "n_sector_particles": int(sec[:, 2].sum())}
        if self.measurement_mode and S > 1:
            self.measurements.extend(_record(row) for row in sec)

        def cloud(a, b, edge_index):
            return Data(x=x_out[a:b], edge_index=edge_index, y=torch.zeros(0, dtype=torch.float32, device=dev),
                        layer=cols_out[0, a:b], particle_id=cols_out[1, a:b], pt=pte_out[0, a:b],
                        reconstructable=cols_out[2, a:b], sector=cols_out[5, a:b], eta=pte_out[1, a:b],
                        n_hits=cols_out[3, a:b], n_layers_hit=cols_out[4, a:b])

        if collated:
            out = cloud(0, n_rows, ei.view(2, -1))
            out.batch = torch.bucketize(torch.arange(n_rows, device=dev), ptr[1:], right=True)
            out.ptr = ptr
            return out
        return [cloud(int(offs[s]), int(offs[s + 1]), ei[2 * e_offs[s]:2 * e_offs[s + 1]].view(2, -1)) for s in range(S)]

    def get_measurements(self) -> dict:
        """mean and ``_err`` (standard deviation, ddof = 1) of every key of the measurement records"""
        out = {}
        if not self.measurements:
            return out
        with np.errstate(all="ignore"):
            for var in self.measurements[0]:
                v = np.array([float(r[var]) for r in self.measurements], dtype=np.float64)
                out[var] = v.mean()
                out[var + "_err"] = v.std(ddof=1) if len(v) > 1 else np.float64("nan")
        return out


def _record(row) -> dict:
    """the reference's measurement record of a sector from its row of integer counts, finished in float64"""
    n_hits, n_ext, n_unique, num, den = (int(v) for v in row[:5])
    return {"n_hits": n_hits, "n_hits_ext": n_ext, "n_hits_ratio": n_ext / n_hits if n_hits > 0 else 0,
            "n_unique_pids": n_unique, "majority_contained": num / den if den != 0 else 0}
