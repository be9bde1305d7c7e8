#!/usr/bin/env python3
"""Golden vectors of the track-graph statistics, FROM THE REFERENCE ITSELF: ``tests/golden/track_graph_info.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``) with networkx and
pandas, never on a GPU machine.  It installs the stand-ins of ``oracle/_ref_standins.py`` for the third-party packages
the reference imports, then calls the reference's own ``get_track_graph_info`` (analysis/graphs.py:86-140) for every
particle id > 0 of six random graphs on an ``nx.Graph`` that holds all hits, and ``summarize_track_graph_info``
(graphs.py:195-217) on the records.

Graphs (seeds 0..5): 600 hits with ids drawn from 0..49 (0 is noise), 700 random edges, plus the chain edges between
consecutive hits of one id, each kept with probability 0.75 - most particles are split into a few segments, many
of which are joined again through other particles' hits.

The file holds, per graph g: ``g_edge_index`` int64 [2, M], ``g_pid`` int64 [600], the reference's rows
``g_rows`` float64 [n_particles, 6] in the order of ``TrackGraphInfo`` (inf: no path) and ``g_summary`` float64 [9]
in the order of the reference's dict.

Usage:  python tools/make_track_graph_golden.py --ref PATH
"""

from __future__ import annotations

import argparse
import pathlib
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "track_graph_info.npz"
SEEDS = tuple(range(6))
N_HITS, N_IDS, N_RANDOM_EDGES, KEEP = 600, 50, 700, 0.75
FIELDS = ("pid", "n_hits", "n_segments", "n_hits_largest_segment", "distance_largest_segments",
          "n_hits_largest_component")
SUMMARY_KEYS = ("frac_segment100", "frac_component100", "frac_segment50", "frac_component50", "frac_segment75",
                "frac_component75", "n_segments", "frac_hits_largest_segment", "frac_hits_largest_component")


def graph(seed):
    g = np.random.default_rng(seed)
    pid = g.integers(0, N_IDS, size=N_HITS).astype(np.int64)
    edges = [g.integers(0, N_HITS, size=(2, N_RANDOM_EDGES))]
    for p in range(1, N_IDS):
        hits = np.flatnonzero(pid == p)
        chain = np.stack([hits[:-1], hits[1:]])
        edges.append(chain[:, g.random(chain.shape[1]) < KEEP])
    return np.concatenate(edges, axis=1).astype(np.int64), pid


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", required=True, type=pathlib.Path, help="checkout of the reference")
    args = ap.parse_args()
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(args.ref / "src"))
    import _ref_standins

    _ref_standins.install()
    import networkx as nx
    import pandas as pd
    from gnn_tracking.analysis.graphs import TrackGraphInfo, get_track_graph_info, summarize_track_graph_info

    assert TrackGraphInfo._fields == FIELDS
    arrs, n_rows, n_split = {}, 0, 0
    for seed in SEEDS:
        edge_index, pid = graph(seed)
        gx = nx.Graph()
        gx.add_nodes_from(range(N_HITS))
        gx.add_edges_from(edge_index.T.tolist())
        records = [get_track_graph_info(gx, pid, int(p))._asdict() for p in np.unique(pid[pid > 0])]
        summary = summarize_track_graph_info(pd.DataFrame.from_records(records))
        assert tuple(summary) == SUMMARY_KEYS
        rows = np.array([[float(r[f]) for f in FIELDS] for r in records], dtype=np.float64)
        n_rows += len(rows)
        n_split += int((rows[:, 2] > 1).sum())
        arrs[f"g{seed}_edge_index"] = edge_index
        arrs[f"g{seed}_pid"] = pid
        arrs[f"g{seed}_rows"] = rows
        arrs[f"g{seed}_summary"] = np.array([float(summary[k]) for k in SUMMARY_KEYS], dtype=np.float64)
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **arrs)
    print(f"{OUT}: {len(SEEDS)} graphs, {n_rows} particles, {n_split} of them split, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
