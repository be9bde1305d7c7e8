"""Restatement of the track-graph statistics of ``analysis/graphs.py:49-278`` in networkx / numpy, for the tests of
``gnn_tracking_amd.graph_analysis`` (no torch, no product code).  It follows the reference function by function with
one pinned difference: segments of ONE size rank by their smallest hit index (the reference: by the iteration order of
networkx's sets).  ``tie_distances`` gives the distances of every ranking the reference's stable sort could produce, which
is what ``tests/test_track_graph_cpu.py`` holds the reference's own numbers against (``tests/golden/track_graph_info.npz``).

A batch is given by the sizes of its events: every event is its own graph, a particle the pair (event, id)."""

from __future__ import annotations

import collections
import math

import networkx as nx
import numpy as np

COLUMNS = ("pid", "n_hits", "n_segments", "n_hits_largest_segment", "distance_largest_segments",
           "n_hits_largest_component", "event")
SUMMARY_KEYS = ("frac_segment100", "frac_component100", "frac_segment50", "frac_component50", "frac_segment75",
                "frac_component75", "n_segments", "frac_hits_largest_segment", "frac_hits_largest_component")


def graph_of(edge_index, n):
    """the undirected graph on all n hits (``to_networkx(..., to_undirected=True)``)"""
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(np.asarray(edge_index).T.tolist())
    return g


def set_distance(g, sources, targets):
    """fewest edges on a path of g from a node of ``sources`` to a node of ``targets`` (``shortest_path_length_multi``):
    a breadth-first search from all sources at once; ``inf`` without a path"""
    targets = set(targets) - set(sources)
    seen = set(sources)
    frontier, level = list(seen), 0
    while frontier:
        level += 1
        nxt = []
        for v in frontier:
            for u in g.adj[v]:
                if u in seen:
                    continue
                if u in targets:
                    return level
                seen.add(u)
                nxt.append(u)
        frontier = nxt
    return math.inf


def segments_of(g, hits):
    """the segments of a particle, largest first, segments of one size by their smallest hit"""
    return sorted((sorted(c) for c in nx.connected_components(g.subgraph(hits))), key=lambda s: (-len(s), s[0]))


def particle_info(g, component_of, pid_of_hit, pid):
    """``get_track_graph_info`` (graphs.py:86-140) as a dict, plus the segments"""
    hits = np.flatnonzero(pid_of_hit == pid).tolist()
    segments = segments_of(g, hits)
    per_component = collections.Counter(component_of[h] for h in hits)
    distance = 0.0 if len(segments) == 1 else float(set_distance(g, segments[0], segments[1]))
    return dict(pid=pid, n_hits=len(hits), n_segments=len(segments), n_hits_largest_segment=len(segments[0]),
                distance_largest_segments=distance, n_hits_largest_component=max(per_component.values())), segments


def tie_distances(g, segments):
    """the distances between (first, second) for every order of the segments that a stable sort by size alone could
    give: the first is any segment of the largest size, the second any other segment of the largest size if there
    is one, else any segment of the second-largest size"""
    if len(segments) == 1:
        return {0.0}
    top = [s for s in segments if len(s) == len(segments[0])]
    if len(top) > 1:
        pairs = [(a, b) for i, a in enumerate(top) for b in top[i + 1:]]
    else:
        pairs = [(top[0], s) for s in segments[1:] if len(s) == len(segments[1])]
    return {float(set_distance(g, a, b)) for a, b in pairs}


def event_table(edge_index, pid, mask):
    """rows (dicts, ascending pid) and segments per row of ONE event"""
    pid = np.asarray(pid, dtype=np.int64)
    g = graph_of(edge_index, len(pid))
    component_of = {v: i for i, c in enumerate(nx.connected_components(g)) for v in c}
    rows, segs = [], []
    for p in sorted(set(pid[np.asarray(mask, dtype=bool)].tolist())):
        row, s = particle_info(g, component_of, pid, p)
        rows.append(row)
        segs.append(s)
    return g, rows, segs


def table(edge_index, pid, mask, sizes=None):
    """``get_track_graph_info_from_data`` as a dict of numpy columns, rows by (event, pid); ``sizes``: the hits per
    event of a batch (edges must stay inside an event)"""
    edge_index, pid, mask = np.asarray(edge_index, dtype=np.int64).reshape(2, -1), np.asarray(pid), np.asarray(mask)
    sizes = [len(pid)] if sizes is None else list(sizes)
    starts = [0, *np.cumsum(sizes).tolist()]
    rows = []
    for e, (a, b) in enumerate(zip(starts, starts[1:])):
        mine = (edge_index[0] >= a) & (edge_index[0] < b)
        assert ((edge_index[1][mine] >= a) & (edge_index[1][mine] < b)).all(), "an edge leaves its event"
        _, ev_rows, _ = event_table(edge_index[:, mine] - a, pid[a:b], mask[a:b])
        rows += [dict(r, event=e) for r in ev_rows]
    return {c: np.array([r[c] for r in rows], dtype=np.float64 if c == "distance_largest_segments" else np.int64)
            for c in COLUMNS}


def summarize(tgi):
    """``summarize_track_graph_info`` (graphs.py:195-217), particle by particle in Python floats"""
    n = len(tgi["n_hits"])
    seg = [int(a) / int(b) for a, b in zip(tgi["n_hits_largest_segment"], tgi["n_hits"])]
    comp = [int(a) / int(b) for a, b in zip(tgi["n_hits_largest_component"], tgi["n_hits"])]
    return {
        "frac_segment100": sum(f == 1 for f in seg) / n,
        "frac_component100": sum(f == 1 for f in comp) / n,
        "frac_segment50": sum(f >= 0.5 for f in seg) / n,
        "frac_component50": sum(f >= 0.5 for f in comp) / n,
        "frac_segment75": sum(f >= 0.75 for f in seg) / n,
        "frac_component75": sum(f >= 0.75 for f in comp) / n,
        "n_segments": math.fsum(int(v) for v in tgi["n_segments"]) / n,
        "frac_hits_largest_segment": math.fsum(seg) / n,
        "frac_hits_largest_component": math.fsum(comp) / n,
    }


def orphan_counts(edge_index, n, good):
    """the documented meaning of ``OrphanCount`` (graphs.py:220-247): hits without an incident edge, by the good mask"""
    orphan = np.ones(n, dtype=bool)
    orphan[np.asarray(edge_index).reshape(-1)] = False
    good = np.asarray(good, dtype=bool)
    return dict(n_orphan_correct=int((orphan & ~good).sum()), n_orphan_incorrect=int((orphan & good).sum()),
                n_orphan_total=int(orphan.sum()))


def basic_counts(edge_index, y, pid, good, sizes=None):
    """``get_basic_counts`` (graphs.py:250-265) as written; a track of a batch is the pair (event, id)"""
    edge_index, pid, good, y = np.asarray(edge_index), np.asarray(pid), np.asarray(good, dtype=bool), np.asarray(y)
    event = np.repeat(np.arange(len(sizes)), sizes) if sizes is not None else np.zeros(len(pid), dtype=np.int64)
    return {
        "n_hits": len(pid),
        "n_hits_noise": int((pid <= 0).sum()),
        "n_hits_thld": int(good.sum()),
        "n_edges": int(edge_index.shape[1]),
        "n_tracks": len(set(zip(event.tolist(), pid.tolist()))),
        "n_true_edges": int(y.sum()),
        "n_true_edges_thld": int(((y == 0) & good[edge_index[0]]).sum()),
    }
