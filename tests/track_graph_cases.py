"""The track-graph statistics (``gnn_tracking_amd.graph_analysis``: ``get_track_graph_info_from_data`` and what is
built on it; ``csrc/track_graph.hip``), shared by the emulator tests (tests/test_track_graph_emul.py) and the GPU tests
(tests/test_track_graph_gpu.py).  The oracle is ``track_graph_ref`` (networkx), which tests/test_track_graph_cpu.py pins
to the reference's own numbers.  Every comparison of a table is exact, ``inf`` included; the only tolerance in this
file is the 1e-12 (relative) of the three means of a summary: a float64 mean of a few hundred values in [0, 1]
carries at most n * eps of rounding, whatever the order of the additions.  Each case asserts on the oracle's own output
that the situation it exists for occurs."""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import gnn_tracking_amd as G
import track_graph_ref as R
from batch_util import ptr_of, starts_of
from gnn_tracking_amd import graph_analysis as GA

#: an empty event, a one-hit event, a two-hit event, event edges inside a wave (rows 5, 75, 139) and inside a block (396)
EVENTS = (5, 0, 70, 64, 257, 1, 2)
#: the same ids in every event: 0 (noise), small ones, ids beyond 2^31 and a negative one
IDS = (0, 1, 2, 3, 2 ** 40 + 1, 2 ** 40 + 2, -2 ** 41)
MEANS = ("n_segments", "frac_hits_largest_segment", "frac_hits_largest_component")


# ------------------------------------------------------------------------------------------------- plumbing
def data_of(edge_index, pid, good, device, sizes=None):
    """a ``Data`` whose good-node mask is ``good & (pid > 0)``: pt on either side of the threshold"""
    pid = np.asarray(pid, dtype=np.int64)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n = len(pid)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    inside = (ei >= 0).all(0) & (ei < n).all(0)
    y = np.zeros(ei.shape[1], dtype=bool)
    y[inside] = (pid[ei[0, inside]] == pid[ei[1, inside]]) & (pid[ei[0, inside]] > 0)
    data = G.Data(edge_index=t(ei), particle_id=t(pid), pt=t(np.where(good, 2.0, 0.5).astype(np.float32)),
                  eta=t(np.zeros(n, dtype=np.float32)), reconstructable=t(np.ones(n, dtype=np.float32)), y=t(y),
                  x=t(np.zeros((n, 1), dtype=np.float32)))
    if sizes is not None:
        data.ptr = ptr_of(sizes, device)
    return data


def mask_of(pid, good):
    return np.asarray(good, dtype=bool) & (np.asarray(pid) > 0)


def assert_table(got, want, what):
    assert tuple(got) == R.COLUMNS, f"{what}: columns {tuple(got)}"
    for c in R.COLUMNS:
        assert got[c].dtype == want[c].dtype, f"{what}: {c} is {got[c].dtype}"
        assert np.array_equal(got[c], want[c]), f"{what}: {c}\n{got[c]}\nwant\n{want[c]}"


def check(device, edge_index, pid, good=None, sizes=None, what="", **kw):
    """device against restatement; returns the restatement's table"""
    good = np.ones(len(pid), dtype=bool) if good is None else good
    want = R.table(edge_index, pid, mask_of(pid, good), sizes)
    got = G.get_track_graph_info_from_data(data_of(edge_index, pid, good, device, sizes), **kw)
    assert_table(got, want, what)
    return want


def row_of(table, pid, event=0):
    (i,) = np.flatnonzero((table["pid"] == pid) & (table["event"] == event))
    return {c: table[c][i] for c in R.COLUMNS}


def chain(*hits):
    """the edges of a path through ``hits``"""
    return [(a, b) for a, b in zip(hits, hits[1:])]


def edges_of(pairs):
    return np.array(pairs, dtype=np.int64).reshape(-1, 2).T


# -------------------------------------------------------------------------------- case 1: event boundaries and ids
def random_event(g, n, n_random=0.4, keep=0.7):
    pid = g.choice(np.array(IDS, dtype=np.int64), n)
    if n >= len(IDS):
        pid[:len(IDS)] = IDS
    edges = [g.integers(0, max(n, 1), size=(2, int(n_random * n) if n > 1 else 0))]
    for p in IDS:
        hits = np.flatnonzero(pid == p)
        c = np.stack([hits[:-1], hits[1:]])
        edges.append(c[:, g.random(c.shape[1]) < keep])
    return np.concatenate(edges, axis=1).astype(np.int64), pid, g.random(n) < 0.7


@functools.lru_cache(maxsize=None)
def batch_case():
    g = np.random.default_rng(2601)
    evs = [random_event(g, n) for n in EVENTS]
    s = starts_of(EVENTS)
    ei = np.concatenate([e[0] + a for e, a in zip(evs, s)], axis=1)
    pid, good = np.concatenate([e[1] for e in evs]), np.concatenate([e[2] for e in evs])
    return evs, ei, pid, good, R.table(ei, pid, mask_of(pid, good), EVENTS)


def case_event_boundaries_and_ids(device):
    _, ei, pid, good, want = batch_case()
    s = starts_of(EVENTS)
    assert 0 in EVENTS and 1 in EVENTS and any(a % 64 for a in s[1:-1]) and s[-1] > 256
    assert (want["pid"] > 0).all() and len(set(want["event"].tolist())) >= 4 and 1 not in want["event"]
    big = [set(want["pid"][want["event"] == e].tolist()) for e in (2, 3, 4)]
    assert all(ids == {1, 2, 3, 2 ** 40 + 1, 2 ** 40 + 2} for ids in big), "the ids do not repeat from event to event"
    d = want["distance_largest_segments"]
    assert np.isinf(d).any() and (d == 0).any() and ((d >= 2) & np.isfinite(d)).sum() >= 5
    assert (want["n_hits_largest_component"] > want["n_hits_largest_segment"]).any()
    # (one graph over all rows would count a particle once, not once per event)
    assert len(R.table(ei, pid, mask_of(pid, good))["pid"]) < len(want["pid"])
    data = data_of(ei, pid, good, device, EVENTS)
    got = G.get_track_graph_info_from_data(data)
    assert_table(got, want, "event boundaries and ids")
    assert_table(G.get_track_graph_info_from_data(data), got, "the same call again")
    by_batch = data_of(ei, pid, good, device)
    by_batch.batch = torch.repeat_interleave(torch.arange(len(EVENTS), device=device), data.ptr.diff())
    assert_table(G.get_track_graph_info_from_data(by_batch), want, "events given by `batch`")


def case_collation(device):
    """the collated batch equals the events fed one by one, row for row"""
    evs, ei, pid, good, want = batch_case()
    singles = [data_of(*e, device) for e in evs]
    got = G.get_track_graph_info_from_data(G.collate(singles))
    assert_table(got, want, "collate([...])")
    rows = 0
    for e, d in enumerate(singles):
        alone = G.get_track_graph_info_from_data(d)
        assert (alone["event"] == 0).all()
        mine = got["event"] == e
        for c in R.COLUMNS[:-1]:
            assert np.array_equal(alone[c], got[c][mine]), f"event {e} alone: {c}"
        rows += len(alone["pid"])
    assert rows == len(got["pid"]) > 10


# ------------------------------------------------------------------------------------- case 2: bitmap word edges
def word_edge_event(n):
    """particle 1: the segment {0, 1} and, two edges away through the noise hit 2, the LAST hit of the event"""
    pid = np.zeros(n, dtype=np.int64)
    pid[[0, 1, n - 1]] = 1
    return edges_of(chain(0, 1, 2, n - 1)), pid


def case_bitmap_word_edges(device):
    sizes = (63, 64, 65)
    evs = [word_edge_event(n) for n in sizes]
    for n, (ei, pid) in zip(sizes, evs):
        r = row_of(check(device, ei, pid, what=f"{n} hits"), 1)
        assert r["n_segments"] == 2 and r["distance_largest_segments"] == 2 and r["n_hits_largest_component"] == 3
    s = starts_of(sizes)
    want = check(device, np.concatenate([e[0] + a for e, a in zip(evs, s)], axis=1), np.concatenate([e[1] for e in evs]),
                 sizes=sizes, what="63 | 64 | 65 hits")
    assert want["distance_largest_segments"].tolist() == [2, 2, 2]


# ------------------------------------------------------------------------- cases 3, 4: many levels, wide frontier
def chain_graph(length=300):
    """particle 1: {0, 1} and {length + 2, length + 3}, joined by a chain of ``length`` noise hits"""
    pid = np.zeros(length + 4, dtype=np.int64)
    pid[[0, 1, length + 2, length + 3]] = 1
    return edges_of(chain(*range(length + 4))), pid


def hub_graph(degree=600):
    """particle 1: {0, 1} - hub 2 - ``degree`` leaves, the last of which touches {degree + 3, degree + 4}"""
    pid = np.zeros(degree + 5, dtype=np.int64)
    pid[[0, 1, degree + 3, degree + 4]] = 1
    leaves = range(3, degree + 3)
    return edges_of(chain(0, 1, 2) + [(2, v) for v in leaves] + chain(degree + 2, degree + 3, degree + 4)), pid


def case_many_levels(device):
    ei, pid = chain_graph()
    r = row_of(check(device, ei, pid, what="chain"), 1)
    assert r["distance_largest_segments"] == 301 > 256 and r["n_hits_largest_component"] == 4


def case_wide_frontier(device):
    ei, pid = hub_graph()
    assert np.bincount(ei.reshape(-1)).max() == 601 > 2 * 256
    r = row_of(check(device, ei, pid, what="hub"), 1)
    assert r["distance_largest_segments"] == 3 and r["n_segments"] == 2


def case_workspace_path(device):
    """the chain and the hub with LDS bitmaps for at most 128 hits: the bitmaps of the workspace, the same table"""
    for name, (ei, pid) in (("chain", chain_graph()), ("hub", hub_graph())):
        n = len(pid)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
        assert n > 128 and G._capi.load().gnntrk_track_graph_distance_workspace_bytes(n, 128) > 0
        args = (t(ei), t(pid), t(pid > 0))
        lds, ws = GA.track_graph_table(*args), GA.track_graph_table(*args, lds_hits=128)
        want = R.table(ei, pid, pid > 0)
        assert math.isfinite(want["distance_largest_segments"][0]) and want["distance_largest_segments"][0] >= 3
        for c in R.COLUMNS:
            assert np.array_equal(lds[c], want[c]) and np.array_equal(ws[c], want[c]), f"{name}: {c}"
        assert np.array_equal(lds["segment_b"], ws["segment_b"])


# ------------------------------------------------------------------------- cases 5-9: small hand-built situations
def case_path_contents(device):
    """particle 1: A = {0, 1, 2}, B = {3, 4}, C = {5}; the only way from A to B runs through the noise hit 6, hit 7 of
    particle 2, the third segment C and the noise hit 8"""
    pid = np.array([1, 1, 1, 1, 1, 1, 0, 2, 0], dtype=np.int64)
    ei = edges_of(chain(0, 1, 2) + chain(3, 4) + chain(2, 6, 7, 5, 8, 3))
    want = check(device, ei, pid, what="path contents")
    r = row_of(want, 1)
    assert r["n_segments"] == 3 and r["n_hits_largest_segment"] == 3 and r["distance_largest_segments"] == 5
    assert r["n_hits_largest_component"] == 6 and row_of(want, 2)["distance_largest_segments"] == 0


def case_no_path(device):
    pid = np.array([1, 1, 1, 0, 0], dtype=np.int64)
    want = check(device, edges_of(chain(0, 1) + chain(2, 3, 4)), pid, what="no path")
    r = row_of(want, 1)
    assert np.isinf(r["distance_largest_segments"]) and r["n_hits_largest_component"] == 2 and r["n_segments"] == 2


def case_unsplit(device):
    pid = np.array([1, 2, 2, 2, 0, 3], dtype=np.int64)
    want = check(device, edges_of(chain(1, 2, 3, 4)), pid, what="unsplit")
    assert want["n_segments"].tolist() == [1, 1, 1] and not want["distance_largest_segments"].any()
    assert np.array_equal(want["n_hits_largest_component"], want["n_hits"]) and want["n_hits"].tolist() == [1, 3, 1]


def case_ties(device):
    """particle 1: three segments of two hits, {0, 1} - {2, 3} four edges apart, {0, 1} - {4, 5} two; particle 2:
    {10..13}, {14} three edges away and {15} two.  The smallest hit index decides: 4 and 3."""
    pid = np.zeros(19, dtype=np.int64)
    pid[:6], pid[10:16] = 1, 2
    ei = edges_of(chain(0, 1) + chain(2, 3) + chain(4, 5) + chain(1, 6, 7, 8, 2) + chain(0, 9, 4)
                  + chain(10, 11, 12, 13) + chain(13, 16, 17, 14) + chain(10, 18, 15))
    g, rows, segs = R.event_table(ei, pid, pid > 0)
    assert [len(s) for s in segs[0]] == [2, 2, 2] and [len(s) for s in segs[1]] == [4, 1, 1]
    assert R.tie_distances(g, segs[0]) == {4.0, 2.0, 7.0} and R.tie_distances(g, segs[1]) == {3.0, 2.0}
    want = check(device, ei, pid, what="ties")
    assert want["distance_largest_segments"].tolist() == [4, 3]


def case_masking(device):
    """particle 1 has a hit outside the mask, particle 2 no hit inside it"""
    pid = np.array([1, 1, 1, 2, 2], dtype=np.int64)
    good = np.array([True, False, True, False, False])
    want = check(device, edges_of(chain(0, 1) + chain(3, 4)), pid, good, what="masking")
    assert want["pid"].tolist() == [1] and want["n_hits"].tolist() == [3] and want["n_segments"].tolist() == [2]


# ------------------------------------------------------------------------------------------- cases 10-12: edges
def case_edge_forms(device):
    """self loops, duplicate edges and both directions change nothing"""
    evs, *_ = batch_case()
    ei, pid, good = evs[4]
    more = np.concatenate([ei, ei[::-1], ei[:, :40], np.tile(np.arange(0, len(pid), 3), (2, 1))], axis=1)
    assert (more[0] == more[1]).sum() >= 80
    want = check(device, more, pid, good, what="edge forms")
    assert_table(want, R.table(ei, pid, mask_of(pid, good)), "the oracle on the plain edges")
    assert (want["n_segments"] > 1).sum() >= 3


def raises(fn, *needles):
    try:
        fn()
    except ValueError as e:
        assert all(s in str(e) for s in needles), str(e)
    else:
        raise AssertionError(f"no ValueError with {needles}")


def case_bad_edges(device):
    _, ei, pid, good, _ = batch_case()
    n, s = len(pid), starts_of(EVENTS)
    for end in (n, -1):
        bad = ei.copy()
        bad[1, 7] = end
        raises(lambda: G.get_track_graph_info_from_data(data_of(bad, pid, good, device, EVENTS)), "1 edges", "outside")
    cross = ei.copy()
    first = int(np.flatnonzero(cross[0] >= s[4])[0])
    cross[1, first] = s[2] + 3        # (from event 4 into event 2)
    raises(lambda: G.get_track_graph_info_from_data(data_of(cross, pid, good, device, EVENTS)), "1 edges lie in two events")


def case_w_and_threshold(device):
    evs, *_ = batch_case()
    ei, pid, good = evs[4]
    m = ei.shape[1]
    w = np.random.default_rng(2602).choice(np.array([0.25, 0.5, 0.75], dtype=np.float32), m)
    wt = torch.from_numpy(w).to(device)
    assert (w == 0.5).sum() > 20 and (w > 0.5).sum() > 20
    want = check(device, ei[:, w > 0.5], pid, good, what="the oracle's cut graph")
    data = data_of(ei, pid, good, device)
    assert_table(G.get_track_graph_info_from_data(data, w=wt, threshold=0.5), want, "w > threshold")
    uncut = R.table(ei, pid, mask_of(pid, good))
    assert any(not np.array_equal(uncut[c], want[c]) for c in R.COLUMNS), "the cut changes nothing"
    for thr in (0.0, -1.0):
        assert_table(G.get_track_graph_info_from_data(data, w=wt, threshold=thr), uncut, f"threshold {thr}")
    raises(lambda: G.get_track_graph_info_from_data(data, w=wt), "threshold")


# ------------------------------------------------------------------------------------ case 13: counts and summary
def assert_summary(got, want, what):
    assert tuple(got) == R.SUMMARY_KEYS == tuple(want), f"{what}: keys {tuple(got)}"
    for k in R.SUMMARY_KEYS:
        if k in MEANS:
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), f"{what}: {k} = {got[k]!r}, want {want[k]!r}"
        else:
            assert got[k] == want[k], f"{what}: {k} = {got[k]!r}, want {want[k]!r}"


def case_counts_and_summary(device):
    _, ei, pid, good, table = batch_case()
    mask = mask_of(pid, good)
    data = data_of(ei, pid, good, device, EVENTS)
    y = data.y.cpu().numpy()
    want_orphans = R.orphan_counts(ei, len(pid), mask)
    assert want_orphans["n_orphan_correct"] > 0 and want_orphans["n_orphan_incorrect"] > 0
    got_orphans = G.get_orphan_counts(data)
    assert isinstance(got_orphans, G.OrphanCount) and got_orphans._asdict() == want_orphans
    want_basic = R.basic_counts(ei, y, pid, mask, EVENTS)
    assert want_basic["n_tracks"] > len(IDS) and want_basic["n_true_edges_thld"] > 0 and want_basic["n_hits_noise"] > 0
    got_basic = G.get_basic_counts(data)
    assert got_basic == want_basic and list(got_basic) == list(want_basic)
    assert all(type(v) is int for v in got_basic.values())
    tgi = G.get_track_graph_info_from_data(data)
    want_summary = R.summarize(table)
    assert 0 < want_summary["frac_segment100"] < want_summary["frac_segment50"] < 1
    assert want_summary["frac_component75"] > want_summary["frac_segment75"]
    assert_summary(G.summarize_track_graph_info(tgi), want_summary, "summary")
    per_event = G.summarize_track_graph_info(tgi, per_event=True, n_events=len(EVENTS))
    assert len(per_event) == len(EVENTS) and math.isnan(per_event[1]["n_segments"])
    for e in (0, 2, 3, 4):
        assert_summary(per_event[e], R.summarize({c: v[table["event"] == e] for c, v in table.items()}), f"event {e}")
    stats = G.get_all_graph_construction_stats(data)
    assert list(stats) == [*want_orphans, *R.SUMMARY_KEYS, *want_basic]
    assert_summary({k: stats[k] for k in R.SUMMARY_KEYS}, want_summary, "all stats")
    assert {k: stats[k] for k in (*want_orphans, *want_basic)} == {**want_orphans, **want_basic}
    # one event without `ptr`: the same functions
    evs, *_ = batch_case()
    one = data_of(*evs[4], device)
    assert G.get_basic_counts(one) == R.basic_counts(evs[4][0], one.y.cpu().numpy(), evs[4][1], mask_of(*evs[4][1:]))


CASES = (case_event_boundaries_and_ids, case_collation, case_bitmap_word_edges, case_many_levels, case_wide_frontier,
         case_workspace_path, case_path_contents, case_no_path, case_unsplit, case_ties, case_masking, case_edge_forms,
         case_bad_edges, case_w_and_threshold, case_counts_and_summary)
