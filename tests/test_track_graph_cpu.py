"""The restatement ``tests/track_graph_ref.py`` against the reference's own numbers
(``tests/golden/track_graph_info.npz``, written by tools/make_track_graph_golden.py from ``get_track_graph_info`` and
``summarize_track_graph_info`` of analysis/graphs.py on six random graphs), and the host-only parts of
``gnn_tracking_amd.graph_analysis``.  No GPU, no emulator.

The restatement ranks segments of one size by their smallest hit, the reference by networkx's set order, so the two
may measure ``distance_largest_segments`` between different segments where the second-largest is not unique.
What is pinned: the four integer columns and the summaries are equal for every particle; the reference's distance is
one of the distances of the admissible rankings (``tie_distances``) for EVERY particle; it equals the restatement's for
at least 75 % of them (on this fixture: 294 particles, 274 split; the figures are printed)."""

import functools
import math
import pathlib

import numpy as np
import pytest

import gnn_tracking_amd as G
import track_graph_ref as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "track_graph_info.npz"
SEEDS = range(6)
FIELDS = ("pid", "n_hits", "n_segments", "n_hits_largest_segment", "distance_largest_segments",
          "n_hits_largest_component")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def restated(seed):
    z = golden()
    ei, pid = z[f"g{seed}_edge_index"], z[f"g{seed}_pid"]
    g, rows, segs = R.event_table(ei, pid, pid > 0)
    return g, rows, segs, R.table(ei, pid, pid > 0)


def test_fixture_shape():
    z = golden()
    assert GOLDEN.stat().st_size < 256 * 1024
    for s in SEEDS:
        assert z[f"g{s}_pid"].shape == (600,) and z[f"g{s}_edge_index"].shape[0] == 2
        assert z[f"g{s}_rows"].shape[1] == len(FIELDS) and z[f"g{s}_summary"].shape == (len(R.SUMMARY_KEYS),)
    assert G.TrackGraphInfo._fields == FIELDS


@pytest.mark.parametrize("seed", SEEDS)
def test_integer_columns_and_summaries_equal_the_reference(seed):
    ref = golden()[f"g{seed}_rows"]
    _, _, _, table = restated(seed)
    assert len(ref) == len(table["pid"]) > 40
    for i, c in enumerate(FIELDS):
        if c != "distance_largest_segments":
            assert np.array_equal(ref[:, i], table[c]), c
    # (split or not is never a matter of ties; with a path or not can be: tied segments may lie in different components)
    assert np.array_equal(ref[:, 4] == 0, table["distance_largest_segments"] == 0)
    want = dict(zip(R.SUMMARY_KEYS, golden()[f"g{seed}_summary"].tolist()))
    for got in (R.summarize(table), G.summarize_track_graph_info(table)):
        assert tuple(got) == R.SUMMARY_KEYS
        for k, v in want.items():
            if k.startswith("frac_segment") or k.startswith("frac_component"):
                assert got[k] == v, k
            else:   # a float64 mean of < 100 values in [0, 50]: n * eps relative, whatever the order of the additions
                assert abs(got[k] - v) <= 1e-12 * abs(v), k


def test_reference_distances_are_admissible_and_mostly_the_tie_rules():
    n = split = ambiguous = equal = 0
    for seed in SEEDS:
        ref = golden()[f"g{seed}_rows"][:, 4]
        g, rows, segs, table = restated(seed)
        for r, s, mine in zip(ref.tolist(), segs, table["distance_largest_segments"].tolist()):
            admissible = R.tie_distances(g, s)
            assert r in admissible and mine in admissible, (seed, r, mine, admissible)
            assert len(s) == 1 or r >= 2
            n += 1
            split += len(s) > 1
            ambiguous += len(admissible) > 1
            equal += r == mine
    print(f"{n} particles, {split} split, {ambiguous} ambiguous, reference == smallest-index rule on {equal}")
    assert n == 294 and split > 200 and 0 < ambiguous < n
    assert equal >= 0.75 * n


def test_summary_of_hand_made_tables():
    tgi = {"pid": np.array([1, 2, 3, 4]), "n_hits": np.array([4, 4, 2, 1]), "n_segments": np.array([1, 2, 2, 1]),
           "n_hits_largest_segment": np.array([4, 3, 1, 1]), "n_hits_largest_component": np.array([4, 4, 1, 1]),
           "distance_largest_segments": np.array([0, 2, math.inf, 0]), "event": np.array([0, 0, 1, 3])}
    s = G.summarize_track_graph_info(tgi)
    assert s == {"frac_segment100": 0.5, "frac_component100": 0.75, "frac_segment50": 1.0, "frac_component50": 1.0,
                 "frac_segment75": 0.75, "frac_component75": 0.75, "n_segments": 1.5,
                 "frac_hits_largest_segment": 0.8125, "frac_hits_largest_component": 0.875}
    per = G.summarize_track_graph_info(tgi, per_event=True)
    assert len(per) == 4 and per[0]["frac_segment100"] == 0.5 and per[1]["frac_segment50"] == 1.0
    assert all(math.isnan(v) for v in per[2].values()) and per[3]["n_segments"] == 1.0
    assert len(G.summarize_track_graph_info(tgi, per_event=True, n_events=6)) == 6
    empty = G.summarize_track_graph_info({k: v[:0] for k, v in tgi.items()})
    assert tuple(empty) == R.SUMMARY_KEYS and all(math.isnan(v) for v in empty.values())


def test_named_tuples_are_the_references():
    assert G.OrphanCount._fields == ("n_orphan_correct", "n_orphan_incorrect", "n_orphan_total")
    assert G.TrackGraphInfo(1, 2, 3, 4, 5, 6)._asdict() == dict(zip(FIELDS, range(1, 7)))
