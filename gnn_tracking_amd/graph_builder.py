"""Geometric graph builder on the device (``graph_construction/graph_builder.py``): point clouds to the graphs that the
edge classifier is trained on.  ``graph_construction.py`` is the ML graph construction (kNN in a learned space); this
module is the reference's ``GraphBuilder``, which connects the hits of neighbouring detector layers that pass cuts on
the phi slope, z0, dR and the intersecting-line cut.

The reference cross-joins the hits of two layers in pandas for each of 23 layer pairs.  Here a candidate pair is one
lane's work in ``csrc/graph_builder.hip`` (``gnntrk_graph_builder_count`` / ``_fill`` / ``_truth``): a counting pass, a
scan, and a filling pass that writes the surviving edges in the reference's order.  ``build_edges`` makes ONE host
read (the number of edges, needed to allocate the outputs); a measurement record is made from counts that stay on the
device until ``measurements`` is looked at.

Contract:

* Order: layer pairs in the order of the reference's list (``add_two_hop``: the extra pairs appended ascending, where
  the reference has Python's set order); inside a pair hit 1 ascending in hit index, then hit 2 ascending.
* Precision: every cut is decided in float64 from the float32 columns of ``x`` (the reference: float32).  The decisions
  agree with the reference's wherever a pair is not within float32 rounding of a cut; ``edge_attr`` is the float64 value
  rounded once.
* A collated batch (``ptr`` or ``batch``): pairs inside an event only, edges event-major with global node ids;
  ``build(collate(clouds))`` equals ``collate([build(c) for c in clouds])`` field by field.
* Layers must lie in ``[0, 64)``.  Strip layers have no pairs (``pixel_only=False`` gives an empty list, as in the
  reference).  The directory loop ``process()`` is ``data_transformer.build_graphs``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import Tensor

from . import _capi, events, ops
from .data import Data
from .hparams import HyperparametersMixin

__all__ = ["GraphBuilder", "get_two_hop_tuples", "DEFAULT_FEATURES"]

DEFAULT_FEATURES = ("r", "phi", "z", "eta_rz", "u", "v", "charge_frac", "leta", "lphi", "lx", "ly", "lz", "geta", "gphi")
_PIXEL_PAIRS = ((7, 8), (8, 9), (9, 10),                              # barrel-barrel
                (7, 6), (8, 6), (9, 6), (10, 6),                      # barrel-LEC
                (7, 11), (8, 11), (9, 11), (10, 11),                  # barrel-REC
                (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6),       # LEC-LEC
                (11, 12), (12, 13), (13, 14), (14, 15), (15, 16), (16, 17))   # REC-REC
#: r of barrel layers 0 and 1 (layers 7, 8): the intersecting-line cut of their pairs with an innermost endcap layer
_INTERSECT_RADIUS = {7: 71.56298065185547, 8: 115.37811279296875}
_PT_THLDS = (0, 0.1, 0.5, 0.9, 1.0)
_N_COUNTS = 14   # GNNTRK_GB_COUNTS: edges, true, true with pt > thld x 5, relabelled, n_truth_edges x 5, bad layers


def get_two_hop_tuples(tuples) -> set[tuple[int, int]]:
    """Given a list of tuples ``(a, b)``, the set of tuples ``(x, y)`` where ``(x, t)`` and ``(t, y)`` are in the list."""
    return {(a, d) for a, b in tuples for c, d in tuples if b == c}


class GraphBuilder(HyperparametersMixin):
    def __init__(self, *, pixel_only=True, phi_slope_max=0.005, z0_max=200, dR_max=1.7, remove_intersecting=True,
                 directed=False, measurement_mode=False, edge_augmentation: str | None = None):
        """Build graphs out of point clouds.

        Args:
            pixel_only: only consider the pixel detector (otherwise: no layer pairs, as in the reference)
            phi_slope_max, z0_max, dR_max: the cuts
            remove_intersecting: remove "ambiguous" edges (Fig. 3 of arXiv:2103.16701) and mark the remaining
                barrel-to-endcap edges of a particle but those of its outermost barrel layer as incorrect
            directed: build directed edges (no doubling)
            measurement_mode: append a measurement record per built event to ``measurements``
            edge_augmentation: ``"add_two_hop"`` adds next-neighbour layer pairs; needs ``remove_intersecting=False``
        """
        self.save_hyperparameters()
        self.pixel_only = pixel_only
        self.phi_slope_max, self.z0_max, self.dR_max = phi_slope_max, z0_max, dR_max
        #: name / meaning of the node features
        self.feature_names = DEFAULT_FEATURES
        #: scaling of the node features
        self.feature_scale = np.array([1000.0, np.pi, 1000.0, 1, 1 / 1000.0, 1 / 1000.0]
                                      + [1.0] * (len(DEFAULT_FEATURES) - 6))
        self.directed = directed
        self.measurement_mode = measurement_mode
        self._measurements: list[dict] = []
        self._pending: list[Tensor] = []     # counts of built batches that no one has looked at yet
        self._remove_intersecting = remove_intersecting
        self._edge_augmentation = edge_augmentation
        if edge_augmentation and remove_intersecting:
            raise ValueError("Edge autmentation currently requires remove_intersecting==False")
        self._layer_pairs()   # (an unknown augmentation is refused here, not at the first build)

    # ------------------------------------------------------------------------------------------ the pair table
    def _layer_pairs(self) -> list[tuple[int, int]]:
        pairs = list(_PIXEL_PAIRS) if self.pixel_only else []
        if self._edge_augmentation is None:
            pass
        elif self._edge_augmentation == "add_two_hop":
            pairs.extend(sorted(get_two_hop_tuples(pairs)))
        else:
            raise ValueError(f"Invalid augmentation mode: {self._edge_augmentation}")
        return pairs

    def _tables(self):
        pairs = self._layer_pairs()
        flat = [l for p in pairs for l in p]
        radius = [_INTERSECT_RADIUS.get(l1, 0.0) if l2 in (6, 11) else 0.0 for l1, l2 in pairs]
        cuts = [float(self.phi_slope_max), float(self.z0_max), float(self.dR_max), float(bool(self._remove_intersecting))]
        return ((C.c_int32 * max(len(flat), 1))(*flat), (C.c_double * max(len(radius), 1))(*radius), len(pairs),
                (C.c_double * 4)(*cuts))

    # --------------------------------------------------------------------------------------------- the device part
    @staticmethod
    def _columns(pc, who: str | None = "GraphBuilder"):
        """the checked columns of a point cloud and the offsets of its events; ``who=None`` leaves the order of a
        ``batch`` unread and returns it as a flag on the device (last element) for the caller's own host read"""
        x, layer, pid, pt = pc.x, pc.layer, pc.particle_id, pc.pt
        _capi.require_device(x, layer, pid, pt)
        if x.dim() != 2 or x.shape[1] < 3 or x.dtype != torch.float32:
            raise ValueError(f"GraphBuilder: x must be float32 [n, >= 3] (r, phi, z, ...), got {x.dtype} {tuple(x.shape)}")
        x = x.detach()
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < 3):
            x = x.contiguous()
        n, dev = int(x.shape[0]), x.device
        cols = [layer.detach().to(device=dev, dtype=torch.int64).contiguous(),
                pid.detach().to(device=dev, dtype=torch.int64).contiguous(),
                pt.detach().to(device=dev, dtype=torch.float32).contiguous()]
        if any(tuple(c.shape) != (n,) for c in cols):
            raise ValueError(f"GraphBuilder: layer, particle_id and pt must have shape ({n},)")
        ptr = events.event_ptr(pc, who=who)
        seg_ptr = (torch.tensor([0, n], dtype=torch.int64, device=dev) if ptr is None
                   else ptr.detach().to(device=dev, dtype=torch.int64).contiguous())
        batch = getattr(pc, "batch", None)
        if who is None and getattr(pc, "ptr", None) is None and batch is not None and batch.numel() > 1:
            unsorted = events.unsorted(batch).to(device=dev, dtype=torch.int64).reshape(1)
        else:
            unsorted = torch.zeros(1, dtype=torch.int64, device=dev)
        return x, *cols, seg_ptr, unsorted

    def _truth(self, lib, ei, y, edge_pt, layer, pid, pt, seg_ptr, relabel: bool) -> Tensor:
        """``gnntrk_graph_builder_truth``: relabels ``y`` in place, returns the counts int64 [events, 14] on the device"""
        n, n_ev, m = int(layer.shape[0]), int(seg_ptr.numel()) - 1, 0 if ei is None else int(ei.shape[1])
        counts = torch.empty((n_ev, _N_COUNTS), dtype=torch.int64, device=layer.device)
        ws = ops._ws(lib.gnntrk_graph_builder_truth_workspace_bytes(n), layer)
        p = ops._p
        addr = lambda t: p(t) if t is not None and t.numel() else None   # noqa: E731
        _capi.check(lib.gnntrk_graph_builder_truth(addr(ei) if m else None, m, addr(y), addr(edge_pt), addr(layer),
                                                   addr(pid), addr(pt), n, p(seg_ptr), n_ev, int(relabel), p(counts), p(ws),
                                                   ws.numel(), ops._stream(layer)), lib)
        return counts

    def _edges(self, pc, want_counts: bool):
        """(edge_index [2, E], edge_attr [4, E], y [E], edge_pt [E], edge_ptr [events + 1], counts or None)"""
        x, layer, pid, pt, seg_ptr, unsorted = self._columns(pc, who=None)
        lib = _capi.load()
        n, dev, n_ev = int(x.shape[0]), x.device, int(seg_ptr.numel()) - 1
        pairs, radius, n_pairs, cuts = self._tables()
        p, stream = ops._p, ops._stream(x)
        x_stride = int(x.stride(0)) if n > 1 else int(x.shape[1])
        head = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = None
        if n > 0 and n_pairs > 0:
            ws = ops._ws(lib.gnntrk_graph_builder_count_workspace_bytes(n, n_ev, pairs, n_pairs), x)
            _capi.check(lib.gnntrk_graph_builder_count(p(x), x_stride, p(layer), n, p(seg_ptr), n_ev, pairs, radius,
                                                       n_pairs, cuts, p(head), p(ws), ws.numel(), stream), lib)
        host = torch.cat([head, unsorted, seg_ptr]).cpu().numpy()             # the one host read
        (m, n_bad, bad_order), offs = host[:3].tolist(), host[3:]
        if bad_order:
            raise ValueError("GraphBuilder: `batch` must be sorted (PyG convention)")
        if offs[0] != 0 or offs[-1] != n or (np.diff(offs) < 0).any():
            raise ValueError("GraphBuilder: ptr must ascend from 0 to the number of hits")
        if n_bad:
            raise ValueError(f"GraphBuilder: {n_bad} hits lie on a layer outside [0, 64)")
        ei = torch.empty((2, m), dtype=torch.int64, device=dev)
        ea = torch.empty((4, m), dtype=torch.float32, device=dev)
        y = torch.empty(m, dtype=torch.float32, device=dev)
        edge_pt = torch.empty(m, dtype=torch.float32, device=dev)
        edge_ptr = torch.zeros(n_ev + 1, dtype=torch.int64, device=dev)
        if ws is not None:
            addr = lambda t: p(t) if m else None   # noqa: E731
            _capi.check(lib.gnntrk_graph_builder_fill(p(x), x_stride, p(layer), p(pid), p(pt), n, p(seg_ptr), n_ev, pairs,
                                                      radius, n_pairs, cuts, m, addr(ei), addr(ea), addr(y), addr(edge_pt),
                                                      p(edge_ptr), p(ws), ws.numel(), stream), lib)
        counts = None
        if want_counts or (self._remove_intersecting and m):
            counts = self._truth(lib, ei, y, edge_pt, layer, pid, pt, seg_ptr, bool(self._remove_intersecting))
        return ei, ea, y, edge_pt, edge_ptr, counts

    # ------------------------------------------------------------------------------------------------- public
    def build_edges(self, point_cloud) -> tuple[Tensor, Tensor, Tensor, Tensor]:
        """Build edges between the hits of ``point_cloud`` (``x`` float32 with r, phi, z in its first columns, ``layer``,
        ``particle_id``, ``pt``; one event or a collated batch).

        Returns:
            ``edge_index`` int64 [2, E], ``edge_attr`` float32 [4, E] (dr / 1000, dphi / pi, dz / 1000, dR), ``y`` float32
            [E] (same particle with id > 0, corrected with ``remove_intersecting``), ``edge_pt`` float32 [E] (pt of the first
            hit): the reference's quantities before the undirected doubling, on the device
        """
        return self._edges(point_cloud, False)[:4]

    def build(self, point_cloud, evtid: int = -1, s: int = -1) -> Data:
        """``build_edges`` and ``to_pyg_data``: the graph of one event, or of every event of a collated batch (then
        with ``batch`` and ``ptr``, as ``collate`` of the events' graphs).  With ``measurement_mode`` a record per event
        goes to ``measurements``."""
        ei, ea, y, _, edge_ptr, counts = self._edges(point_cloud, self.measurement_mode)
        if self.measurement_mode:
            self._pending.append(counts)
        pc, dev = point_cloud, ei.device
        n_ev = int(edge_ptr.numel()) - 1
        scale = torch.from_numpy(self.feature_scale).to(dev)
        if not self.directed:
            ei, ea, y = _double(ei, ea, y, edge_ptr)
        data = Data(x=(pc.x.detach().clone() / scale).float(), edge_index=ei, edge_attr=ea.T, pt=pc.pt.clone().float(),
                    particle_id=pc.particle_id.clone().long(), y=y, reconstructable=pc.reconstructable.clone().long(),
                    sector=pc.sector.clone().long(), evtid=torch.full((n_ev,), int(evtid), dtype=torch.int64, device=dev),
                    s=torch.full((n_ev,), int(s), dtype=torch.int64, device=dev), eta=pc.eta.clone().float(),
                    layer=pc.layer.clone().long())
        if n_ev > 1:
            n = int(pc.x.shape[0])
            ptr = events.event_ptr(pc, who=None).to(dev)
            data.batch = torch.bucketize(torch.arange(n, device=dev), ptr[1:], right=True)
            data.ptr = ptr
        return data

    def get_n_truth_edges(self, point_cloud):
        """``{0: n, 0.1: n, 0.5: n, 0.9: n, 1.0: n}``: per particle with id > 0 the products of its hit counts on
        consecutive occupied layers (ascending layer number), summed over the particles whose first hit has pt above the
        threshold.  A collated batch gives a list with one dict per event.  One host copy."""
        _, layer, pid, pt, seg_ptr, _ = self._columns(point_cloud)
        counts = self._truth(_capi.load(), None, None, None, layer, pid, pt, seg_ptr, False).cpu().numpy()
        if counts[:, 13].any():
            raise ValueError(f"GraphBuilder: {int(counts[:, 13].sum())} hits lie on a layer outside [0, 64)")
        out = [{t: int(row[8 + k]) for k, t in enumerate(_PT_THLDS)} for row in counts]
        return out[0] if len(out) == 1 else out

    def count_edges(self, point_cloud) -> dict[str, np.ndarray]:
        """The integer counts of ``build_edges(point_cloud)``, int64 arrays with one entry per event: ``n_edges``,
        ``n_true_edges``, ``n_true_edges_pt`` [events, 5] (true edges with ``edge_pt`` above each threshold),
        ``n_corrected`` (edges that ``correct_truth_labels`` relabelled) and ``n_truth_edges`` [events, 5]."""
        counts = self._edges(point_cloud, True)[5].cpu().numpy()
        return {"n_edges": counts[:, 0], "n_true_edges": counts[:, 1], "n_true_edges_pt": counts[:, 2:7],
                "n_corrected": counts[:, 7], "n_truth_edges": counts[:, 8:13]}

    @property
    def measurements(self) -> list[dict]:
        """the measurement records, one per built event (the counts of builds that were not looked at yet are copied
        from the device here)"""
        pending, self._pending = self._pending, []
        for counts in pending:
            self._measurements.extend(_record(row) for row in counts.cpu().numpy())
        return self._measurements

    def get_measurements(self) -> dict:
        """mean and ``_err`` (standard deviation, ddof = 1) of every key of the measurement records"""
        records = self.measurements
        out = {}
        if not records:
            return out
        with np.errstate(all="ignore"):
            for var in records[0]:
                v = np.array([float(r[var]) for r in records], dtype=np.float64)
                out[var] = v.mean()
                out[var + "_err"] = v.std(ddof=1) if len(v) > 1 else np.float64("nan")
        return out


def _record(row) -> dict:
    """the reference's measurement record of one event from its row of counts; a zero denominator gives numpy's
    inf / nan"""
    n_edges, n_true = int(row[0]), np.float64(row[1])
    n_truth = {t: int(row[8 + k]) for k, t in enumerate(_PT_THLDS)}
    with np.errstate(all="ignore"):
        return {"n_edges": n_edges, "n_true_edges": n_true, "n_false_edges": n_edges - n_true,
                **{f"n_truth_edge_{t}": v for t, v in n_truth.items()},
                "edge_purity": n_true / np.float64(n_edges),
                **{f"edge_efficiency_{t}": np.float64(row[2 + k]) / np.float64(n_truth[t])
                   for k, t in enumerate(_PT_THLDS)}}


def _double(ei: Tensor, ea: Tensor, y: Tensor, edge_ptr: Tensor):
    """``to_pyg_data``'s undirected doubling, event by event: [row|col ; col|row], the first three attributes negated
    in the second half, y repeated.  No host read: the events' edge offsets stay on the device."""
    negate = torch.tensor([[-1.0], [-1.0], [-1.0], [1.0]], device=ea.device)
    if edge_ptr.numel() == 2:
        return torch.cat([ei, ei.flip(0)], dim=1), torch.cat([ea, negate * ea], dim=1), torch.cat([y, y])
    m = int(ei.shape[1])
    j = torch.arange(m, device=ei.device)
    event = torch.bucketize(j, edge_ptr[1:], right=True)
    first = j + edge_ptr[event]                                   # 2 * offset of the event + place in the event
    second = first + (edge_ptr[event + 1] - edge_ptr[event])
    ei2 = torch.empty((2, 2 * m), dtype=ei.dtype, device=ei.device)
    ea2 = torch.empty((4, 2 * m), dtype=ea.dtype, device=ea.device)
    y2 = torch.empty(2 * m, dtype=y.dtype, device=y.device)
    ei2[:, first], ei2[:, second] = ei, ei.flip(0)
    ea2[:, first], ea2[:, second] = ea, negate * ea
    y2[first], y2[second] = y, y
    return ei2, ea2, y2
