"""Graph analysis of the metric-learning validation on the device (``analysis/graphs.py:281-343``,
``metrics/graph_construction.py:8-31``): connected-component labels, the largest-segment fraction of
every particle and the edge efficiency / purity of a built graph.

The reference copies the edges to the host, builds a networkx graph and walks its components in
Python.  Here the components are a lock-free union-find (``gnntrk_cc_labels``, ``csrc/kscan.hip``)
and everything else is an integer count (``gnntrk_kscan_counts`` for the k-scan,
``k_scanner.GraphConstructionKNNScanner``).  Differences that are not contract in the reference:

* ``get_cc_labels`` labels a component by its SMALLEST node index (networkx: by discovery order).  The
  partition is the same; the labels are unique and repeatable.
* ``get_largest_segment_fracs`` returns the fractions ordered by the particle's first masked hit (the
  reference: the insertion order of a Python dict filled while walking networkx's components, then a
  ``set`` difference).  Only the multiset of fractions is contract; every use in the reference is a
  mean of a comparison.
* ``get_track_graph_info_from_data`` ranks the segments of a particle by size and, among segments of ONE size,
  by their smallest hit index (the reference: a stable sort over the iteration order of networkx's sets, which
  is no contract).  ``distance_largest_segments`` is measured between the first two segments of that order, so
  it can differ from the reference's where the second-largest segment is not unique.

The track-graph statistics (``analysis/graphs.py:49-278``: ``get_track_graph_info_from_data``,
``summarize_track_graph_info``, ``get_orphan_counts``, ``get_basic_counts``,
``get_all_graph_construction_stats``) take one event or a ``collate([...])`` batch, every event its own problem
and a particle the pair (event, particle id).  The reference walks networkx once per particle and runs one
shortest-path search per pair of hits of its two largest segments; here the table is two ``gnntrk_cc_labels``
calls, integer counting and one breadth-first search per split particle (``csrc/track_graph.hip``), and comes
back in one host copy.

The EC threshold scan (``analysis/edge_classification.py:24-112``: ``get_all_ec_stats``, ``collect_all_ec_stats``) is
``ec_threshold_scan``: the binary-classification counts and the summary of the track-graph table for ALL thresholds of
a list from one pass over the edges and two union-find forests that grow from the largest threshold to the smallest
(``csrc/ec_scan.hip``), with one host read and one host copy per scan.
"""

from __future__ import annotations

import types
import typing

import numpy as np
import torch
from torch import Tensor

from . import _capi, events, ops
from .edge_order import as_tensor
from .graph_masks import get_good_node_mask
from .metrics import _thresholds_from_counts, bcs_from_counts

__all__ = ["get_cc_labels", "get_largest_segment_fracs", "get_efficiency_purity_edges", "TrackGraphInfo",
           "OrphanCount", "get_track_graph_info_from_data", "summarize_track_graph_info", "get_orphan_counts",
           "get_basic_counts", "get_all_graph_construction_stats", "ec_threshold_scan", "get_all_ec_stats",
           "collect_all_ec_stats"]


def cc_labels(edge_index: Tensor, num_nodes: int, *, same_pid: Tensor | None = None,
              node_mask: Tensor | None = None, check: bool = True) -> Tensor:
    """Int64 labels ``[num_nodes]`` of the connected components of the undirected graph ``edge_index``
    (``[2, M]``): the smallest node index of every component.  ``same_pid`` (int64 ``[num_nodes]``): keep
    an edge only if its ends carry the same value; ``node_mask`` (bool ``[num_nodes]``): keep an edge only
    if both ends pass - both evaluated in the kernel.  ``check``: read the number of edges with an end
    outside ``[0, num_nodes)`` back (one host read) and raise if there are any."""
    _capi.require_device(edge_index)
    lib = _capi.load()
    n = int(num_nodes)
    ei = edge_index.detach().to(torch.int64).contiguous()
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError(f"cc_labels: edge_index must be [2, M], got {tuple(ei.shape)}")
    dev = ei.device
    pid = None if same_pid is None else same_pid.detach().to(device=dev, dtype=torch.int64).contiguous()
    mask = None if node_mask is None else node_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    for name, t in (("same_pid", pid), ("node_mask", mask)):
        if t is not None and (t.dim() != 1 or int(t.shape[0]) != n):
            raise ValueError(f"cc_labels: {name} has shape {tuple(t.shape)}, expected ({n},)")
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = ops._ws(lib.gnntrk_cc_labels_workspace_bytes(n), ei)
    p = ops._p
    _capi.check(lib.gnntrk_cc_labels(p(ei), int(ei.shape[1]), None, None, 0, 0, p(pid), p(mask), n, p(labels), p(bad),
                                     p(ws), ws.numel(), ops._stream(ei)), lib)
    if check and int(bad.item()):
        raise ValueError(f"cc_labels: {int(bad.item())} edges have an end outside [0, {n})")
    return labels


def get_cc_labels(edge_index: Tensor, num_nodes: int) -> Tensor:
    """``analysis/graphs.py:331-343``: labels for the connected components of a graph, on the device of
    ``edge_index``.  A component's label is its smallest node index (see the module docstring)."""
    return cc_labels(edge_index, num_nodes)


def _segment_counts(data, pt_thld: float, max_eta: float):
    """(mask, labels of the masked same-id components, particle ids) of ``data`` on the device."""
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    pid = data.particle_id.to(torch.int64)
    n = int(pid.shape[0])
    y = getattr(data, "y", None)
    ei = data.edge_index
    if y is not None:   # (the reference strips every edge that is not flagged true: edge_index[:, data.y])
        ei = ei[:, y.bool()]
    # every component has to be single-id (graphs.py:319 reads the id of one of its hits): as in the
    # k-scan, where y = pid[e0] == pid[e1], the id filter is applied in the kernel as well
    labels = cc_labels(ei, n, same_pid=pid, node_mask=mask)
    return mask, labels, pid


def get_largest_segment_fracs(data, *, pt_thld=0.9, n_particles_sampled=None, max_eta=4) -> np.ndarray:
    """``analysis/graphs.py:281-328``: for every particle with hits in the good-node mask, the fraction
    of its masked hits that lie in its largest segment (connected component of the ``data.y`` edges whose
    both ends are masked).  ``data.y`` must flag same-particle edges only, as the k-scan's does.  Returns
    a float64 numpy array; its ORDER is by the particle's first masked hit (the reference's order is an
    implementation detail of dict / set iteration).  ``n_particles_sampled`` draws that many particles at
    random, as the reference does, after the exact computation (it exists there to shorten a host loop)."""
    mask, labels, pid = _segment_counts(data, float(pt_thld), float(max_eta))
    if not bool(mask.any()):
        return np.array([], dtype=np.float64)
    pm, lm = pid[mask], labels[mask]
    upid, pinv, pcount = torch.unique(pm, return_inverse=True, return_counts=True)
    _, linv, lcount = torch.unique(lm, return_inverse=True, return_counts=True)
    largest = torch.zeros_like(pcount).scatter_reduce(0, pinv, lcount[linv], reduce="amax")
    first = torch.full_like(pcount, pm.numel()).scatter_reduce(
        0, pinv, torch.arange(pm.numel(), device=pm.device), reduce="amin")
    order = torch.argsort(first)
    fr = (largest.double() / pcount.double())[order].cpu().numpy()
    if n_particles_sampled is not None:
        fr = fr[torch.randperm(len(fr)).numpy()[:n_particles_sampled]]
    return fr


def efficiency_purity_from_counts(n_true_masked: int, n_true_edges_masked: int, n_masked: int) -> dict[str, float]:
    """The two divisions of ``metrics/graph_construction.py:23-24`` as torch evaluates them: both int64
    counts cast to float32, the quotient in float32 (0 / 0 = nan, x / 0 = inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        num = np.float32(n_true_masked)
        eff = num / np.float32(2 * int(n_true_edges_masked))
        pur = num / np.float32(n_masked)
    return {"efficiency": float(eff), "purity": float(pur)}


def get_efficiency_purity_edges(data, pt_thld: float = 0.9, max_eta: float = 4.0) -> dict[str, float]:
    """``metrics/graph_construction.py:8-31``: efficiency and purity of ``data.edge_index`` (labels
    ``data.y``) against ``data.true_edge_index``; only edges with at least one end in the good-node mask
    count.  Masked sums on the device, one host copy of three integers."""
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    ei, te = data.edge_index, data.true_edge_index
    edge_mask = mask[ei[0]] | mask[ei[1]]
    counts = torch.stack([(data.y.bool() & edge_mask).sum(), (mask[te[0]] & mask[te[1]]).sum(), edge_mask.sum()])
    return efficiency_purity_from_counts(*(int(v) for v in counts.tolist()))


# ------------------------------------------------------------------------------------ track-graph statistics
class TrackGraphInfo(typing.NamedTuple):
    """Information about how well connected the hits of a track are in the graph (``analysis/graphs.py:49-72``).

    "Component" means connected component of the graph, "segment" a connected component of the subgraph that
    holds only the hits of the track.

    Attributes:
        pid: the particle id of the track
        n_hits: the number of hits of the track
        n_segments: the number of segments of the track
        n_hits_largest_segment: the number of hits in the largest segment of the track
        distance_largest_segments: the shortest path length between the two largest segments
        n_hits_largest_component: the largest number of hits of the track in one component
    """

    pid: int
    n_hits: int
    n_segments: int
    n_hits_largest_segment: int
    distance_largest_segments: int
    n_hits_largest_component: int


# columns of gnntrk_track_graph_table's rows (include/gnntrk.h)
_TABLE_COLUMNS = ("event", "pid", "n_hits", "n_segments", "n_hits_largest_segment", "n_hits_largest_component",
                  "distance_largest_segments", "segment_a", "segment_b")


def track_graph_table(edge_index: Tensor, particle_id: Tensor, node_mask: Tensor, ptr: Tensor | None = None, *,
                      lds_hits: int | None = None) -> dict[str, np.ndarray]:
    """The table of ``get_track_graph_info_from_data`` for the graph ``edge_index`` (``[2, M]``) on the hits
    ``particle_id`` / ``node_mask`` (``[n]``), ``ptr`` the row offsets of the events of a collated batch (``None``: one
    event): two ``gnntrk_cc_labels`` calls, ``gnntrk_track_graph_adjacency``, ``gnntrk_track_graph_table`` and
    ``gnntrk_track_graph_distance`` on one stream, then ONE host copy.  The only host read before it is the bad-edge
    count of ``cc_labels``.  ``lds_hits``: the search keeps its bitmaps in LDS for events of at most that many hits
    (``gnntrk_track_graph_distance_ex``; tests send small events down the workspace path with it)."""
    _capi.require_device(edge_index, particle_id, node_mask, ptr)
    lib = _capi.load()
    ei = edge_index.detach().to(torch.int64).contiguous()
    dev = ei.device
    pid = particle_id.detach().to(device=dev, dtype=torch.int64).contiguous()
    mask = node_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    n, m = int(pid.shape[0]), int(ei.shape[1])
    if ei.dim() != 2 or ei.shape[0] != 2 or pid.dim() != 1 or tuple(mask.shape) != (n,):
        raise ValueError(f"track_graph_table: edge_index {tuple(ei.shape)}, particle_id {tuple(pid.shape)}, node_mask "
                         f"{tuple(mask.shape)}: expected [2, M], [n], [n]")
    if n == 0:
        return {c: np.zeros(0, dtype=np.float64 if c == "distance_largest_segments" else np.int64)
                for c in _TABLE_COLUMNS}
    if m == 0:   # (an empty tensor has no address to hand over: the self loop (0, 0) joins nothing)
        ei, m = torch.zeros((2, 1), dtype=torch.int64, device=dev), 1
    seg_ptr = (torch.tensor([0, n], dtype=torch.int64, device=dev) if ptr is None
               else ptr.detach().to(device=dev, dtype=torch.int64).contiguous())
    n_ev = int(seg_ptr.numel()) - 1
    segments = cc_labels(ei, n, same_pid=pid)            # (raises on an end outside [0, n): its one host read)
    components = cc_labels(ei, n, check=False)
    p, stream = ops._p, ops._stream(ei)
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbrs = torch.empty(max(2 * m, 1), dtype=torch.int32, device=dev)
    table = torch.empty((n, len(_TABLE_COLUMNS)), dtype=torch.int64, device=dev)
    search = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    head = torch.empty(4, dtype=torch.int64, device=dev)   # rows, searches | edges out of range, edges across events
    ws = ops._ws(lib.gnntrk_track_graph_adjacency_workspace_bytes(n), ei)
    _capi.check(lib.gnntrk_track_graph_adjacency(p(ei), m, n, p(seg_ptr), n_ev, p(rowptr), p(nbrs), p(head[2:]), p(ws),
                                                 ws.numel(), stream), lib)
    ws = ops._ws(lib.gnntrk_track_graph_table_workspace_bytes(n), ei)
    _capi.check(lib.gnntrk_track_graph_table(p(segments), p(components), p(pid), p(mask), n, p(seg_ptr), n_ev, p(table),
                                             p(search), p(head), p(ws), ws.numel(), stream), lib)
    cap = int(lds_hits) if lds_hits is not None else 0
    ws = ops._ws(lib.gnntrk_track_graph_distance_workspace_bytes(n, cap), ei)
    args = (p(table), p(search), p(head), p(segments), p(rowptr), p(nbrs), n, p(seg_ptr), n_ev)
    if lds_hits is None:
        _capi.check(lib.gnntrk_track_graph_distance(*args, p(ws), ws.numel(), stream), lib)
    else:
        _capi.check(lib.gnntrk_track_graph_distance_ex(*args, cap, p(ws), ws.numel(), stream), lib)
    host = torch.cat([head, seg_ptr, table.reshape(-1)]).cpu().numpy()        # the one host copy
    (n_rows, _, n_range, n_cross), offs = host[:4].tolist(), host[4:5 + n_ev]
    if offs[0] != 0 or offs[-1] != n or (np.diff(offs) < 0).any():
        raise ValueError("track_graph_table: ptr must ascend from 0 to the number of hits")
    if n_range or n_cross:
        raise ValueError(f"track_graph_table: {n_range} edges have an end outside [0, {n}), the ends of {n_cross} edges "
                         "lie in two events")
    rows = host[5 + n_ev:].reshape(n, len(_TABLE_COLUMNS))[:n_rows]
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]                         # by (event, pid)
    cols = {c: np.ascontiguousarray(rows[:, i]) for i, c in enumerate(_TABLE_COLUMNS)}
    dist = cols["distance_largest_segments"]
    assert (dist >= -1).all(), "a row of the search list was not searched"
    cols["distance_largest_segments"] = np.where(dist < 0, np.inf, dist.astype(np.float64))
    return cols


def get_track_graph_info_from_data(data, *, w: Tensor | None = None, pt_thld=0.9, threshold: float | None = None,
                                   max_eta: float = 4.0) -> dict[str, np.ndarray]:
    """``analysis/graphs.py:143-192``: the ``TrackGraphInfo`` of every particle that has a hit in the good-node mask,
    as a dict of numpy columns (the project's stand-in for a DataFrame): ``pid``, ``n_hits``, ``n_segments``,
    ``n_hits_largest_segment`` and ``n_hits_largest_component`` int64, ``distance_largest_segments`` float64 (0 for
    an unsplit particle, ``inf`` without a path) and ``event`` int64 (0 without a batch); rows ascend by
    ``(event, pid)``.  ``data`` is one event or a collated batch (``events.event_ptr``): a particle is the pair
    (event, id), and an edge whose ends lie in two events is refused.

    ``w``: edge weights; an edge is kept iff ``w > threshold`` (``gnntrk_threshold_compact``; a NaN weight drops the
    edge, where the reference asserts).  ``n_hits`` counts all hits of the id, masked or not; the graph is undirected.
    The ranking of segments of one size: module docstring."""
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    ei = data.edge_index
    if w is not None:
        if threshold is None:
            raise ValueError("get_track_graph_info_from_data: `w` needs a `threshold`")
        _capi.require_device(w, ei)
        lib = _capi.load()
        wf = w.detach().reshape(-1).to(torch.float32).contiguous()
        m = int(wf.shape[0])
        if m != int(ei.shape[1]):
            raise ValueError(f"get_track_graph_info_from_data: {m} weights for {int(ei.shape[1])} edges")
        keep = torch.empty(m, dtype=torch.uint8, device=wf.device)
        idx = torch.empty(max(m, 1), dtype=torch.int32, device=wf.device)
        n_kept = torch.empty(1, dtype=torch.int64, device=wf.device)
        ws = ops._ws(lib.gnntrk_compact_workspace_bytes(m), wf)
        _capi.check(lib.gnntrk_threshold_compact(ops._p(wf), m, float(threshold), ops._p(keep), ops._p(idx),
                                                 ops._p(n_kept), ops._p(ws), ws.numel(), ops._stream(wf)), lib)
        # a dropped edge becomes the self loop (0, 0), which joins nothing: the number of kept edges stays on the device
        ei = ei.to(torch.int64) * keep.to(torch.int64)
    ptr = events.event_ptr(data, who="get_track_graph_info_from_data")
    cols = track_graph_table(ei, data.particle_id, mask, None if ptr is None else ptr.to(ei.device))
    return {c: cols[c] for c in (*TrackGraphInfo._fields, "event")}


_SUMMARY_KEYS = ("frac_segment100", "frac_component100", "frac_segment50", "frac_component50", "frac_segment75",
                 "frac_component75", "n_segments", "frac_hits_largest_segment", "frac_hits_largest_component")


def summarize_track_graph_info(tgi: dict, per_event: bool = False, n_events: int | None = None):
    """``analysis/graphs.py:195-217``: the nine figures of a table of ``get_track_graph_info_from_data`` (the
    fractions of particles whose largest segment / component holds all, >= 75 %, >= 50 % of their hits, and three
    means), evaluated in float64 as pandas does; an empty table gives NaN.  ``per_event``: a list with one such dict
    per event ``0 .. n_events - 1`` (default: up to the last event that has a row) of the ``event`` column."""
    if per_event:
        ev = np.asarray(tgi["event"])
        n_events = (int(ev.max()) + 1 if ev.size else 0) if n_events is None else int(n_events)
        return [summarize_track_graph_info({k: np.asarray(v)[ev == e] for k, v in tgi.items()}) for e in range(n_events)]
    n_hits = np.asarray(tgi["n_hits"], dtype=np.float64)
    n = len(n_hits)
    if n == 0:
        return dict.fromkeys(_SUMMARY_KEYS, float("nan"))
    seg = np.asarray(tgi["n_hits_largest_segment"], dtype=np.float64) / n_hits
    comp = np.asarray(tgi["n_hits_largest_component"], dtype=np.float64) / n_hits
    return {
        "frac_segment100": int((seg == 1).sum()) / n,
        "frac_component100": int((comp == 1).sum()) / n,
        "frac_segment50": int((seg >= 0.50).sum()) / n,
        "frac_component50": int((comp >= 0.50).sum()) / n,
        "frac_segment75": int((seg >= 0.75).sum()) / n,
        "frac_component75": int((comp >= 0.75).sum()) / n,
        "n_segments": float(np.mean(np.asarray(tgi["n_segments"], dtype=np.float64))),
        "frac_hits_largest_segment": float(seg.mean()),
        "frac_hits_largest_component": float(comp.mean()),
    }


class OrphanCount(typing.NamedTuple):
    """Stats about the number of orphan nodes in a graph (``analysis/graphs.py:220-232``).

    Attributes:
        n_orphan_correct: number of orphan nodes that are bad nodes (low pt or noise)
        n_orphan_incorrect: number of orphan nodes that are good nodes
        n_orphan_total: total number of orphan nodes
    """

    n_orphan_correct: int
    n_orphan_incorrect: int
    n_orphan_total: int


def get_orphan_counts(data, *, pt_thld=0.9, max_eta: float = 4.0) -> OrphanCount:
    """``analysis/graphs.py:235-247``: the hits without an incident edge, split by the good-node mask (over all
    events of a batch).  DEVIATION: the reference clears entries of a mask that it has just zeroed
    (``orphan_mask[connected_nodes] = False`` on ``zeros_like``), so it returns zeros for every graph; this is the
    documented meaning of ``OrphanCount``.  The hit flags are ``gnntrk_connected_nodes``'."""
    from .graph_cut import connected_nodes

    n = int(data.particle_id.shape[0])
    hit, _, _ = connected_nodes(data.edge_index, n)
    good = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    orphan = ~hit
    counts = torch.stack([(orphan & ~good).sum(), (orphan & good).sum(), orphan.sum()]).tolist()
    return OrphanCount(*(int(v) for v in counts))


def get_basic_counts(data, *, pt_thld: float = 0.9, max_eta: float = 4.0) -> dict[str, int]:
    """``analysis/graphs.py:250-265``: basic counts of edges and nodes, the reference's arithmetic as written
    (``n_true_edges_thld`` counts the edges with ``y == 0`` whose first end is a good hit), as Python ints.  On a
    collated batch a track is the pair (event, particle id)."""
    good = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    pid, ei, y = data.particle_id, data.edge_index, data.y
    n = int(pid.shape[0])
    ptr = events.event_ptr(data, who="get_basic_counts")
    if ptr is None:
        n_tracks = pid.unique().numel()
    else:
        event = torch.bucketize(torch.arange(n, device=pid.device), ptr.to(pid.device)[1:], right=True)
        n_tracks = torch.unique(torch.stack([event, pid.long()], dim=1), dim=0).shape[0]
    good_edges = (y == 0) & (good[ei[0].long()] > 0)
    sums = torch.stack([(pid <= 0).sum(), good.sum(), y.sum(), good_edges.sum()]).tolist()
    return {
        "n_hits": n,
        "n_hits_noise": int(sums[0]),
        "n_hits_thld": int(sums[1]),
        "n_edges": int(ei.shape[1]),
        "n_tracks": int(n_tracks),
        "n_true_edges": int(sums[2]),
        "n_true_edges_thld": int(sums[3]),
    }


def get_all_graph_construction_stats(data, pt_thld=0.9, max_eta: float = 4.0) -> dict[str, float]:
    """``analysis/graphs.py:268-278``: orphan counts, the summary of the track-graph table (which, as in the
    reference, is built with the default ``max_eta``) and the basic counts of one batch."""
    return {
        **get_orphan_counts(data, pt_thld=pt_thld, max_eta=max_eta)._asdict(),
        **summarize_track_graph_info(get_track_graph_info_from_data(data, pt_thld=pt_thld)),
        **get_basic_counts(data, pt_thld=pt_thld, max_eta=max_eta),
    }


# ------------------------------------------------------------------------------------------ EC threshold scan
def _scan_records(thresholds, inverse, counts, orphans, summaries):
    """the records of one event (or of all events together) in the caller's order: ``counts`` int64
    [2 mask classes][2 labels][n_thr + 1], ``summaries`` one dict per ascending threshold"""
    rates = []
    for c in (counts[0] + counts[1], counts[1]):           # all edges | both ends in the good-node mask
        tp, fp, P, N = _thresholds_from_counts(c)
        rates.append([bcs_from_counts(int(a), int(b), P, N) for a, b in zip(tp.tolist(), fp.tolist())])
    orphan = OrphanCount(*(int(v) for v in orphans))._asdict()
    return [{"threshold": t, **rates[0][j], **{f"{k}_thld": v for k, v in rates[1][j].items()}, **orphan, **summaries[j]}
            for t, j in zip(thresholds, inverse)]


def ec_threshold_scan(data, w, thresholds, *, pt_thld=0.9, max_eta=4.0, per_event=False):
    """``get_all_ec_stats`` (``analysis/edge_classification.py:24-64``) for every entry of ``thresholds``: a list
    with one record per entry, in the given order (unsorted input and duplicates are fine; at most 256 different
    float32 values).  A record holds ``threshold`` (the caller's value), the twelve keys of
    ``BinaryClassificationStats.get_all()`` over all edges, the same with the suffix ``_thld`` over the edges whose both
    ends are in the good-node mask, the three ``OrphanCount`` fields of the uncut graph and the nine keys of
    ``summarize_track_graph_info`` of the graph cut at the threshold.  It equals the composition of those functions
    bit for bit:

    * an edge is in the graph of ``t`` iff ``w > t`` in float32 (a NaN weight: in none), and is predicted true iff
      ``not (w < t)`` (a NaN score: always) - an edge with ``w == t`` counts as predicted true and is NOT in the graph;
    * a label is positive iff ``int(y) == 1``; segments unite same-id edges, components all edges; ``n_hits`` counts all
      hits of the id; a particle is selected iff one of its hits is in the good-node mask;
    * ``get_orphan_counts`` as documented there (the reference returns zeros).

    ``distance_largest_segments`` is NOT computed: no key of the summary reads it, and it is what the single-threshold
    table spends most of its time on.  ``data`` is one event or a ``collate([...])`` batch (``events.event_ptr``), a
    particle the pair (event, id); ``per_event=True`` returns one such list per event, with the classification and
    orphan counts of that event's edges and hits.  An edge with an end outside ``[0, n)`` or with its ends in two
    events raises ``ValueError`` before any record is built.  ``w`` may be an ``edge_order.EdgeOrdered``.

    The graphs of the thresholds are nested, so every edge is united once per scan (``gnntrk_ec_scan_prepare`` /
    ``gnntrk_ec_scan_steps``); the host reads four counters to size the output and copies everything back once."""
    st = _scan_prepare(data, w, thresholds, pt_thld, max_eta, per_event)
    if st.n_thr == 0:
        return [[] for _ in range(st.n_ev)] if per_event else []
    _scan_steps(st)
    return _scan_finish(st)


def _scan_prepare(data, w, thresholds, pt_thld, max_eta, per_event):
    """the checks of ``ec_threshold_scan``, ``gnntrk_ec_scan_prepare`` and the scan's one host read"""
    st = types.SimpleNamespace(per_event=bool(per_event))
    st.given = [float(t) for t in thresholds]
    thr32 = np.asarray(st.given, dtype=np.float32)
    if np.isnan(thr32).any():
        raise ValueError("ec_threshold_scan: a threshold is NaN")
    uniq, st.inverse = np.unique(thr32, return_inverse=True)
    st.n_thr = n_thr = len(uniq)
    if n_thr > _capi.EC_SCAN_MAX_THR:
        raise ValueError(f"ec_threshold_scan: {n_thr} different thresholds, at most {_capi.EC_SCAN_MAX_THR} per scan")
    wt = as_tensor(w).detach().reshape(-1)
    ei, y = data.edge_index, data.y.detach().reshape(-1)
    _capi.require_device(wt, ei, y, data.particle_id)
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    st.lib = lib = _capi.load()
    st.ei = ei = ei.detach().to(torch.int64).contiguous()
    dev = ei.device
    wf = wt.to(device=dev, dtype=torch.float32).contiguous()
    st.pid = pid = data.particle_id.detach().to(device=dev, dtype=torch.int64).contiguous()
    mask = mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    st.n, st.m = n, m = int(pid.shape[0]), int(ei.shape[1])
    if ei.dim() != 2 or ei.shape[0] != 2 or tuple(mask.shape) != (n,):
        raise ValueError(f"ec_threshold_scan: edge_index {tuple(ei.shape)}, {n} hits: expected [2, M]")
    if int(wf.shape[0]) != m or int(y.shape[0]) != m:
        raise ValueError(f"ec_threshold_scan: {int(wf.shape[0])} weights and {int(y.shape[0])} labels for {m} edges")
    if y.dtype in (torch.bool, torch.uint8):       # (the y_kind of metrics._Edges)
        y, y_kind = y.contiguous().view(torch.uint8), 0
    elif y.dtype == torch.float32:
        y, y_kind = y.contiguous(), 1
    else:
        y, y_kind = (y.int() == 1).view(torch.uint8), 0
    y = y.to(dev)
    ptr = events.event_ptr(data, who="ec_threshold_scan")
    seg_ptr = (torch.tensor([0, n], dtype=torch.int64, device=dev) if ptr is None
               else ptr.detach().to(device=dev, dtype=torch.int64).contiguous())
    st.n_ev = n_ev = int(seg_ptr.numel()) - 1
    st.n_out = n_out = n_ev if per_event else 1
    if n_thr == 0:
        return st
    if n == 0 and m > 0:
        raise ValueError(f"ec_threshold_scan: {m} edges have an end outside [0, 0), the ends of 0 edges lie in two events")
    nb = n_thr + 1
    thr = torch.from_numpy(uniq).to(dev)
    head = torch.empty(4, dtype=torch.int64, device=dev)
    st.particles = torch.empty((max(n, 1), 3), dtype=torch.int64, device=dev)
    st.tail = torch.empty(n_out * (4 * nb + 3), dtype=torch.int64, device=dev)   # bcs | orphans
    bcs, orphans = st.tail[:n_out * 4 * nb], st.tail[n_out * 4 * nb:]
    st.ws = ws = ops._ws(lib.gnntrk_ec_scan_prepare_workspace_bytes(n, m, n_thr), ei)
    p, st.stream = ops._p, ops._stream(ei)
    _capi.check(lib.gnntrk_ec_scan_prepare(_addr(ei), m, _addr(wf), _addr(y), y_kind, _addr(pid), _addr(mask), n,
                                           p(seg_ptr), n_ev, p(thr), n_thr, int(st.per_event), p(head), p(st.particles),
                                           p(bcs), p(orphans), p(ws), ws.numel(), st.stream), lib)
    first = torch.cat([head, seg_ptr]).cpu().numpy()                          # the one host read
    (st.n_rows, _, n_range, n_cross), offs = first[:4].tolist(), first[4:]
    if offs[0] != 0 or offs[-1] != n or (np.diff(offs) < 0).any():
        raise ValueError("ec_threshold_scan: ptr must ascend from 0 to the number of hits")
    if n_range or n_cross:
        raise ValueError(f"ec_threshold_scan: {n_range} edges have an end outside [0, {n}), the ends of {n_cross} edges "
                         "lie in two events")
    return st


def _addr(t: Tensor):
    return ops._p(t) if t.numel() else None   # (an empty tensor has no address to hand over)


def _scan_steps(st) -> None:
    """``gnntrk_ec_scan_steps`` into a buffer sized by the particles that ``_scan_prepare`` read back"""
    n_steps = st.n_thr * st.n_rows * 3
    st.steps = torch.empty(n_steps + (n_steps & 1), dtype=torch.int32, device=st.ei.device)   # (even: copied as int64)
    _capi.check(st.lib.gnntrk_ec_scan_steps(_addr(st.ei), st.m, _addr(st.pid), st.n, st.n_thr, st.n_rows, _addr(st.steps),
                                            ops._p(st.ws), st.ws.numel(), st.stream), st.lib)


def _scan_finish(st):
    """the one host copy and the records"""
    n_rows, n_out, n_thr, nb = st.n_rows, st.n_out, st.n_thr, st.n_thr + 1
    host = torch.cat([st.particles[:n_rows].reshape(-1), st.tail, st.steps.view(torch.int64)]).cpu().numpy()
    rows = host[:3 * n_rows].reshape(n_rows, 3)
    counts = host[3 * n_rows:3 * n_rows + n_out * 4 * nb].reshape(n_out, 2, 2, nb)
    orph = host[3 * n_rows + n_out * 4 * nb:3 * n_rows + n_out * (4 * nb + 3)].reshape(n_out, 3)
    steps = host[3 * n_rows + n_out * (4 * nb + 3):].view(np.int32)[:n_thr * n_rows * 3].reshape(n_thr, n_rows, 3)
    order = np.lexsort((rows[:, 1], rows[:, 0]))                              # by (event, pid), as track_graph_table
    rows, steps = rows[order], steps[:, order].astype(np.int64)

    def summaries(sel):
        return [summarize_track_graph_info({"n_hits": rows[sel, 2], "n_segments": steps[j, sel, 0],
                                            "n_hits_largest_segment": steps[j, sel, 1],
                                            "n_hits_largest_component": steps[j, sel, 2]}) for j in range(n_thr)]

    if not st.per_event:
        return _scan_records(st.given, st.inverse, counts[0], orph[0], summaries(slice(None)))
    return [_scan_records(st.given, st.inverse, counts[e], orph[e], summaries(rows[:, 0] == e)) for e in range(st.n_ev)]


def get_all_ec_stats(threshold: float, w, data, *, pt_thld=0.9, max_eta=4) -> dict[str, float]:
    """``analysis/edge_classification.py:24-64``: edge-classification and graph-construction performance of one batch
    at one threshold - ``ec_threshold_scan`` with a single threshold (see there for the keys and the semantics)."""
    return ec_threshold_scan(data, w, [threshold], pt_thld=pt_thld, max_eta=max_eta)[0]


def collect_all_ec_stats(model, data_loader, thresholds, n_batches: int | None = None, max_workers=6,
                         pt_thld=0.9) -> dict[str, np.ndarray]:
    """``analysis/edge_classification.py:67-112``: ``get_all_ec_stats`` at every threshold for the first ``n_batches``
    batches of ``data_loader`` (``w = model(data)["W"]`` under ``model.eval()`` and ``torch.no_grad()``, one
    ``ec_threshold_scan`` per batch), then per threshold the mean over the batches of every key and
    ``f"{key}_err" = np.std(values) / sqrt(number of batches)``.  Returns a dict of columns of length
    ``len(thresholds)`` (the project's stand-in for a DataFrame).  ``max_workers`` is accepted for the reference's
    signature and ignored: there is no host loop over thresholds to spread."""
    thresholds = list(thresholds)
    model.eval()
    r = []
    with torch.no_grad():
        for idx, data in enumerate(data_loader):
            r.append(ec_threshold_scan(data, model(data)["W"], thresholds, pt_thld=pt_thld))
            if n_batches is not None and idx >= n_batches - 1:
                break
    if not r or not thresholds:
        return {}
    n = len(r)
    cols: dict[str, list] = {}
    for i in range(len(thresholds)):
        batched = {k: np.array([records[i][k] for records in r]) for k in r[0][0]}
        for k, batch in batched.items():
            cols.setdefault(k, []).append(np.mean(batch))
        for k, batch in batched.items():
            cols.setdefault(f"{k}_err", []).append(np.std(batch) / np.sqrt(n))
    return {k: np.array(v) for k, v in cols.items()}
