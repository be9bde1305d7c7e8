#!/usr/bin/env python3
"""Golden vectors of the EC threshold scan, FROM THE REFERENCE ITSELF: ``tests/golden/g22_ec_scan.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``) with networkx, pandas,
matplotlib and tqdm, never on a GPU machine.  It installs the stand-ins of ``oracle/_ref_standins.py`` for the third-party
packages the reference imports, adds the one that is missing there - ``torch_geometric.utils.convert.to_networkx``: an
``nx.Graph`` with ``num_nodes`` nodes and the undirected edges of ``edge_index`` - and calls the reference's own
``get_all_ec_stats`` (analysis/edge_classification.py:24-64) at every threshold.

Graphs: the first three of tools/make_track_graph_golden.py (600 hits, ids 0..49, random and chain edges).  Hits are good
with probability 0.7 (pt 2.0 against 0.5; eta 0, reconstructable).  Labels: both ends carry the same id > 0.  Weights,
seeded: true edges ~ Beta(5, 2), false ~ Beta(2, 5); three weights of either label are set EQUAL to each of the thresholds
0.3 and 0.7.  With chains of a dozen hits no particle keeps every edge above 0.9, so the same-id edges of ONE selected
particle per graph that is whole in the uncut graph are set to 0.95: a case is accepted only if, at every threshold, at
least one particle is split and at least one is whole (checked below on the reference's own table).  Thresholds
(0.1, 0.3, 0.5, 0.7, 0.9): all > 0, the reference asserts at <= 0.

The file holds ``thresholds`` float64 [5], ``keys`` (the keys of a record, in the reference's order) and per graph g:
``g_edge_index`` int64 [2, M], ``g_pid`` int64 [600], ``g_pt`` float32 [600], ``g_w`` float32 [M], ``g_y`` bool [M] and
``g_records`` float64 [5, len(keys)].

Usage:  python tools/make_golden_ec_scan.py --ref PATH
"""

from __future__ import annotations

import argparse
import importlib.util
import pathlib
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "g22_ec_scan.npz"
SEEDS = (0, 1, 2)
THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.9)
PINNED, N_PINNED, P_GOOD, WHOLE_W = (0.3, 0.7), 3, 0.7, 0.95


def track_graph_tool():
    spec = importlib.util.spec_from_file_location("make_track_graph_golden", REPO / "tools" / "make_track_graph_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def install_to_networkx():
    import networkx as nx

    def to_networkx(data, to_undirected=False, **_kw):
        assert to_undirected
        g = nx.Graph()
        g.add_nodes_from(range(data.num_nodes))
        g.add_edges_from(data.edge_index.t().tolist())
        return g

    convert = types.ModuleType("torch_geometric.utils.convert")
    convert.to_networkx = to_networkx
    sys.modules["torch_geometric.utils.convert"] = convert
    utils = sys.modules["torch_geometric.utils"]
    utils.convert = convert
    sys.modules["torch_geometric"].utils = utils
    sys.modules["torch_geometric.data"].DataLoader = sys.modules["torch_geometric.loader"].DataLoader


def inputs(seed, graph):
    edge_index, pid = graph(seed)
    g = np.random.default_rng(2200 + seed)
    pt = np.where(g.random(len(pid)) < P_GOOD, 2.0, 0.5).astype(np.float32)
    y = (pid[edge_index[0]] == pid[edge_index[1]]) & (pid[edge_index[0]] > 0)
    w = np.where(y, g.beta(5, 2, size=len(y)), g.beta(2, 5, size=len(y))).astype(np.float32)
    for t in PINNED:
        for lab in (True, False):
            w[g.choice(np.flatnonzero(y == lab), N_PINNED, replace=False)] = np.float32(t)
    return edge_index, pid, pt, w, y


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", required=True, type=pathlib.Path, help="checkout of the reference")
    args = ap.parse_args()
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(args.ref / "src"))
    import _ref_standins

    _ref_standins.install()
    install_to_networkx()
    import torch
    from gnn_tracking.analysis.edge_classification import get_all_ec_stats
    from gnn_tracking.analysis.graphs import get_track_graph_info_from_data

    graph = track_graph_tool().graph
    arrs = {"thresholds": np.array(THRESHOLDS, dtype=np.float64)}
    keys = None
    for seed in SEEDS:
        edge_index, pid, pt, w, y = inputs(seed, graph)

        def data_of(w):
            n = len(pid)
            return _ref_standins.Data(x=torch.zeros(n, 1), edge_index=torch.from_numpy(edge_index),
                                      particle_id=torch.from_numpy(pid), pt=torch.from_numpy(pt), eta=torch.zeros(n),
                                      reconstructable=torch.ones(n), y=torch.from_numpy(y)), torch.from_numpy(w)

        data, _ = data_of(w)
        uncut = get_track_graph_info_from_data(data)
        whole = uncut.pid[(uncut.n_segments == 1) & (uncut.n_hits > 2)]
        assert len(whole), f"graph {seed}: no selected particle is whole in the uncut graph"
        w[y & (pid[edge_index[0]] == int(whole.iloc[0]))] = np.float32(WHOLE_W)
        data, wt = data_of(w)
        records = []
        for t in THRESHOLDS:
            tgi = get_track_graph_info_from_data(data, w=wt, threshold=t)
            n_whole, n_split = int((tgi.n_segments == 1).sum()), int((tgi.n_segments > 1).sum())
            assert n_whole >= 1 and n_split >= 1, f"graph {seed}, threshold {t}: {n_whole} whole, {n_split} split"
            assert int((w == np.float32(t)).sum()) == (2 * N_PINNED if t in PINNED else 0)
            records.append(get_all_ec_stats(t, wt, data))
            print(f"graph {seed}  t = {t}: {n_whole} whole, {n_split} split, TPR {records[-1]['TPR']:.3f}, "
                  f"n_segments {records[-1]['n_segments']:.3f}")
        keys = keys or tuple(records[0])
        assert all(tuple(r) == keys for r in records)
        arrs[f"g{seed}_edge_index"], arrs[f"g{seed}_pid"], arrs[f"g{seed}_pt"] = edge_index, pid, pt
        arrs[f"g{seed}_w"], arrs[f"g{seed}_y"] = w, y
        arrs[f"g{seed}_records"] = np.array([[float(r[k]) for k in keys] for r in records], dtype=np.float64)
    arrs["keys"] = np.array(keys)
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **arrs)
    print(f"{OUT}: {len(SEEDS)} graphs, {len(THRESHOLDS)} thresholds, {len(keys)} keys, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
