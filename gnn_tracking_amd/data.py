"""Minimal graph container + collate with the part of the PyG ``Data`` /
``DataLoader`` behaviour the reference's hot path relies on.

The modules of this package accept ANY object exposing ``.x / .edge_index /
.edge_attr / ...`` (a real ``torch_geometric.data.Data`` works unchanged); this class
exists so the package, its tests and the bench run without PyG installed.
"""

from __future__ import annotations

import copy
from typing import Iterable

import torch
from torch import Tensor


class Data:
    """Attribute bag.  Node-level attributes have ``num_nodes`` rows, edge-level ones
    (``edge_attr``, ``y``, names starting with ``edge_``) have ``num_edges`` rows."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def keys(self) -> list[str]:
        return [k for k in self.__dict__ if not k.startswith("_")]

    def __getitem__(self, k):
        return getattr(self, k)

    def __setitem__(self, k, v):
        setattr(self, k, v)

    def __contains__(self, k) -> bool:
        return k in self.__dict__

    def __getattr__(self, k):
        # PyG declares these as properties that are None when the attribute was never set
        # (training/tc.py:61 reads ``data.batch`` of a graph built by MLGraphConstruction)
        if k in ("batch", "pos", "edge_weight", "edge_attr", "y", "x", "edge_index"):
            return None
        raise AttributeError(k)

    @property
    def num_nodes(self) -> int:
        return int(self.x.shape[0])

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.shape[1])

    @property
    def num_node_features(self) -> int:
        return int(self.x.shape[1])

    @property
    def num_edge_features(self) -> int:
        return int(self.edge_attr.shape[1])

    def _map(self, fn):
        out = copy.copy(self)
        for k in self.keys():
            v = getattr(self, k)
            if torch.is_tensor(v):
                setattr(out, k, fn(v))
        return out

    def to(self, device, **kw):
        return self._map(lambda t: t.to(device, **kw))

    def cpu(self):
        return self.to("cpu")

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def detach(self):
        return self._map(lambda t: t.detach())

    # -- PyG ``Data.edge_subgraph`` / ``Data.subgraph`` as the reference uses them
    # (models/track_condensation_networks.py:252,259): every edge-level attribute is
    # filtered by the edge mask; ``subgraph`` keeps a node subset, filters node-level
    # attributes, drops edges touching removed nodes and relabels ``edge_index``.
    def edge_subgraph(self, mask: Tensor) -> "Data":
        out = copy.copy(self)
        for k in self.keys():
            v = getattr(self, k)
            if k == "edge_index":
                out.edge_index = v[:, mask]
            elif self.is_edge_attr(k):
                setattr(out, k, v[mask])
        return out

    def subgraph(self, subset: Tensor) -> "Data":
        n = self.num_nodes
        dev = self.edge_index.device
        if subset.dtype == torch.bool:
            node_mask = subset
        else:
            node_mask = torch.zeros(n, dtype=torch.bool, device=dev)
            node_mask[subset] = True
        relabel = torch.full((n,), -1, dtype=torch.long, device=dev)
        relabel[node_mask] = torch.arange(int(node_mask.sum()), device=dev)
        ei = self.edge_index
        emask = node_mask[ei[0]] & node_mask[ei[1]]
        out = copy.copy(self)
        for k in self.keys():
            v = getattr(self, k)
            if k == "edge_index":
                out.edge_index = relabel[ei[:, emask]]
            elif self.is_edge_attr(k):
                setattr(out, k, v[emask])
            elif self.is_node_attr(k):
                setattr(out, k, v[node_mask])
        return out

    def is_edge_attr(self, key: str) -> bool:
        if key == "edge_index" or "index" in key:
            return False
        v = getattr(self, key)
        return (torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == self.num_edges
                and (key.startswith("edge_") or key in ("y", "ec_edge_embedding", "ec_score")))

    def is_node_attr(self, key: str) -> bool:
        v = getattr(self, key)
        return (torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == self.num_nodes
                and "index" not in key and not self.is_edge_attr(key))


def collate(graphs: Iterable[Data]) -> Data:
    """Concatenate graphs into one disjoint graph the way PyG's ``Batch`` does:
    node-/edge-level tensors are concatenated along dim 0, every attribute whose name
    contains ``index`` is concatenated along dim -1 after adding the cumulative node
    count, and ``batch`` (graph id per node) / ``ptr`` (node offsets) are added."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("collate: empty list")
    out = Data()
    offs = [0]
    for g in graphs:
        offs.append(offs[-1] + g.num_nodes)
    for k in graphs[0].keys():
        vals = [getattr(g, k) for g in graphs]
        if not torch.is_tensor(vals[0]):
            setattr(out, k, vals)
        elif "index" in k:
            # (offset while copying: one read and one write of every id instead of a shifted temporary and its copy)
            cat = torch.empty(*vals[0].shape[:-1], sum(int(v.shape[-1]) for v in vals), dtype=vals[0].dtype,
                              device=vals[0].device)
            a = 0
            for v, o in zip(vals, offs):
                if v.shape[:-1] != vals[0].shape[:-1] or v.dtype != vals[0].dtype:   # (what torch.cat would refuse)
                    raise RuntimeError(f"collate: '{k}' of the events disagrees in shape / dtype: {tuple(vals[0].shape)} "
                                       f"{vals[0].dtype} against {tuple(v.shape)} {v.dtype}")
                torch.add(v, o, out=cat[..., a:a + v.shape[-1]])
                a += int(v.shape[-1])
            setattr(out, k, cat)
        elif vals[0].dim() == 0:
            setattr(out, k, torch.stack(vals))
        else:
            setattr(out, k, torch.cat(vals, dim=0))
    dev = graphs[0].x.device
    out.batch = torch.cat([torch.full((g.num_nodes,), i, dtype=torch.long, device=dev)
                           for i, g in enumerate(graphs)])
    out.ptr = torch.tensor(offs, dtype=torch.long, device=dev)
    return out


class EventLayout:
    """Where the events of a collated batch lie in its fields, from ONE host read: ``n_events``, ``node_ptr`` (B + 1 row
    offsets), ``edge_ptr`` (for every ``*index*`` field its B + 1 offsets along the last dimension) and ``kinds``, which
    names for every field but ``batch`` / ``ptr`` how it is divided among the events:

    ==========  ============================================================================================
    ``index``   the name contains ``index``: split along the last dimension by the event of the first row, the
                ids made event-local
    ``edge``    ``Data.is_edge_attr`` (the edge-level NAME rule and ``num_edges`` rows): the edge ranges of
                ``edge_index``
    ``node``    a tensor with ``num_nodes`` rows: split by the node offsets
    ``event``   a tensor with B rows (``evtid`` and ``s`` as ``GraphBuilder.build`` writes them): row ``b`` as a
                one-element slice
    ``list``    a list or tuple of length B: element ``b``
    ``copy``    anything else: handed to every event as it is
    ==========  ============================================================================================

    The order above is the precedence: the edge-level name rule comes first, then the node row count, then the
    per-event count - a ``y`` of a batch with as many edges as hits is edge-level, a node-level field of a batch
    with as many hits as events is node-level.  The edges of every index field must lie inside one event and be
    event-contiguous in event order, as ``collate`` leaves them: ``ValueError`` otherwise, as the other entries
    that take a collated batch raise it."""

    def __init__(self, batch, who: str = "uncollate"):
        from . import events

        x = batch.x
        if not torch.is_tensor(x):
            raise ValueError(f"{who}: the batch has no node features `x`")
        n, dev = int(x.shape[0]), x.device
        ptr, ids = getattr(batch, "ptr", None), getattr(batch, "batch", None)
        flags = []
        if ptr is not None:
            ptr = torch.as_tensor(ptr).to(device=dev, dtype=torch.int64).reshape(-1)
        elif ids is not None and ids.numel() > 0:
            ptr = events.offsets_of(ids.to(dev))
            flags.append(events.unsorted(ids.to(dev)).reshape(1).long())
        else:
            ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        if ptr.numel() < 2:
            raise ValueError(f"{who}: ptr must hold at least two offsets")
        B = int(ptr.numel()) - 1
        self.index_fields = [k for k in batch.keys() if "index" in k and torch.is_tensor(getattr(batch, k))]
        parts = [ptr, *flags]
        for k in self.index_fields:
            v = getattr(batch, k)
            m = int(v.shape[-1]) if v.dim() else 0
            if v.dim() == 0 or m == 0:
                parts += [torch.zeros(3 + B + 1, dtype=torch.int64, device=dev)]
                continue
            rows = v.to(dev).reshape(-1, m).long()
            ev = torch.bucketize(rows, ptr[1:].contiguous(), right=True)
            first = ev[0]
            counts = torch.bincount(first.clamp(max=B - 1), minlength=B)
            offs = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            offs[1:] = torch.cumsum(counts, 0)
            parts += [torch.stack([((rows < 0) | (rows >= n)).any(), (ev != first).any(),
                                   (first[1:] < first[:-1]).any()]).long(), offs]
        host = torch.cat(parts).cpu().tolist()                                   # the one host read
        node_ptr, at = host[:B + 1], B + 1
        if flags:
            if host[at]:
                raise ValueError(f"{who}: `batch` must be sorted (PyG convention)")
            at += 1
        if node_ptr[0] != 0 or node_ptr[-1] != n or any(b < a for a, b in zip(node_ptr, node_ptr[1:])):
            raise ValueError(f"{who}: ptr must ascend from 0 to the number of hits")
        self.edge_ptr = {}
        for k in self.index_fields:
            bad_range, cross, order = host[at:at + 3]
            if bad_range:
                raise ValueError(f"{who}: '{k}' contains node ids outside [0, {n})")
            if cross:
                raise ValueError(f"{who}: '{k}' has an edge between two events")
            if order:
                raise ValueError(f"{who}: the edges of '{k}' are not in event order (collate leaves them event-contiguous)")
            self.edge_ptr[k] = host[at + 3:at + 3 + B + 1]
            at += 3 + B + 1
        self.n_events, self.node_ptr, self.n_nodes = B, node_ptr, n
        has_edges = torch.is_tensor(getattr(batch, "edge_index", None))
        self.kinds = {}
        for k in batch.keys():
            if k in ("batch", "ptr"):
                continue
            v = getattr(batch, k)
            if torch.is_tensor(v):
                if k in self.edge_ptr:
                    kind = "index"
                elif has_edges and Data.is_edge_attr(batch, k):
                    kind = "edge"
                elif v.dim() >= 1 and v.shape[0] == n:
                    kind = "node"
                elif v.dim() >= 1 and v.shape[0] == B:
                    kind = "event"
                else:
                    kind = "copy"
            else:
                kind = "list" if isinstance(v, (list, tuple)) and len(v) == B else "copy"
            self.kinds[k] = kind

    def bounds(self, k: str, b: int) -> tuple[int, int]:
        """the range of event ``b`` in field ``k`` (of its last dimension for an index field, of its rows otherwise)"""
        kind = self.kinds[k]
        if kind == "index":
            return self.edge_ptr[k][b], self.edge_ptr[k][b + 1]
        if kind == "edge":
            return self.edge_ptr["edge_index"][b], self.edge_ptr["edge_index"][b + 1]
        if kind == "node":
            return self.node_ptr[b], self.node_ptr[b + 1]
        return b, b + 1


def uncollate(batch, layout: EventLayout | None = None) -> list[Data]:
    """The inverse of ``collate``: the events of a collated batch as a list of ``Data`` (``uncollate(collate(gs))``
    equals ``gs`` field by field, bit for bit).  ``EventLayout`` documents how every field is divided and in which
    order the rules apply; the events come from ``ptr``, or from ``batch`` where there is no ``ptr``, and a batch with
    neither is one event.  ``batch`` and ``ptr`` are dropped.  Node-, edge- and event-level tensors are views of the
    batch's, the index fields are new tensors (event-local ids).  One host read (none with the batch's ``layout``)."""
    lay = EventLayout(batch, "uncollate") if layout is None else layout
    out = [Data() for _ in range(lay.n_events)]
    for k, kind in lay.kinds.items():
        v = getattr(batch, k)
        for b, d in enumerate(out):
            if kind in ("copy", "list"):
                setattr(d, k, v[b] if kind == "list" else v)
                continue
            lo, hi = lay.bounds(k, b)
            setattr(d, k, v[..., lo:hi] - lay.node_ptr[b] if kind == "index" else v[lo:hi])
    return out
