"""Validation of a collated batch of events, shared by the emulator tests (tests/test_oc_validation_batch_emul.py) and
the GPU tests (tests/test_oc_validation_batch_gpu.py): the per-event radius graph and cluster numbering
(csrc/dbscan.hip), the per-event tracking metrics (csrc/tracking_metrics.hip) and the scanners of
``postprocessing`` on ``collate([...])``.

A batch of B events is B independent problems, so the oracles are the single-event ones applied to every event's rows:
``ref_cpu.radius_neighbors_blocked`` / ``dbscan_labels`` (through ``neighbor_cases.radius_ref`` / ``labels_ref``) and
``tracking_metrics_ref``.  Every comparison is exact: offsets, neighbour ids, fp64 distances bit for bit, labels,
counts and the floats derived from them.  There is no tolerance in this file.  Each case asserts on the oracle's output
that what it is there for occurs."""

from __future__ import annotations

import functools
from functools import partial

import numpy as np
import torch

import gnn_tracking_amd as G
import neighbor_cases as N
import tracking_metrics_ref as R
from batch_util import assert_same, counted_calls, one_event_ptrs, starts_of
from batch_util import records_equal as _records_equal
from gnn_tracking_amd import cluster_metrics as CM
from gnn_tracking_amd import postprocessing, synthetic
from gnn_tracking_amd.postprocessing import (DBSCANFastRescan, DBSCANHyperParamScannerFixed, DBSCANPerformanceDetails)

#: an empty event, a one-hit event, a 256-query block that spans four events, an event edge inside a block
RADIUS_EVENTS = (5, 0, 70, 64, 257, 1)
#: D = 2, 4, 8 and 32 (17 dimensions: brute force under either flag)
RADIUS_WIDTHS = (2, 3, 8, 17)
#: every 64-point chunk edge of the sorted order falls inside or between events
CHUNK_EVENTS = (63, 65, 1, 130)
BIG_EVENTS = N.BIG_EVENTS
CUTS = (0.0, 0.5, 0.9, 1.5)
METRIC_EVENTS = (40, 0, 300, 257)
SCAN_HITS = (1500, 1100, 700)
SCAN_TRIALS = ({"eps": 0.15, "min_samples": 2}, {"eps": 0.2, "min_samples": 3}, {"eps": 0.25, "min_samples": 2},
               {"eps": 0.3, "min_samples": 4})


def rescanner(device, x, max_eps, flags, sizes):
    with N.radius_flags(flags):
        return DBSCANFastRescan(x.to(device), max_eps=max_eps, ptr=N.seg_ptr_of(sizes).to(device), device=device)


def events_of(x, sizes):
    """the non-empty events as (first row, rows of the event)"""
    s = starts_of(sizes)
    return [(a, x[a:b]) for a, b in zip(s, s[1:]) if b > a]


def graph_ref(x, sizes, r):
    """the single-event oracle graphs, concatenated: neighbour ids shifted by the event's first row"""
    off, nbr, dist = [np.zeros(1, dtype=np.int64)], [], []
    s = starts_of(sizes)
    for a, b in zip(s, s[1:]):
        if b == a:
            continue
        o, nb, d = N.radius_ref(x[a:b], r)
        off.append(o[1:] + off[-1][-1])
        nbr.append(nb.astype(np.int64) + a)
        dist.append(d)
    return np.concatenate(off), np.concatenate(nbr), np.concatenate(dist)


def check_graph(fr, x, sizes, r, tag):
    off, nbr, dist = graph_ref(x, sizes, r)
    m = len(nbr)
    assert fr._n_edges == m, f"{tag}: {fr._n_edges} edges, the per-event oracle has {m}"
    assert np.array_equal(fr._off.cpu().numpy(), off), f"{tag}: offsets"
    assert np.array_equal(fr._nbr.cpu().numpy()[:m].astype(np.int64), nbr), f"{tag}: neighbours"
    assert np.array_equal(fr._dist.cpu().numpy()[:m], dist), f"{tag}: distances (fp64, bit for bit)"
    return off, nbr


def labels_ref(x, sizes, max_eps, eps, min_pts):
    """per event the oracle's labels of the event alone (local numbering), and the prefix sums of the cluster counts"""
    s = starts_of(sizes)
    labs, counts = [], []
    for a, b in zip(s, s[1:]):
        lab = N.labels_ref(x[a:b], max_eps, eps, min_pts) if b > a else np.zeros(0, dtype=np.intp)
        labs.append(lab)
        counts.append(int(lab.max()) + 1 if lab.size else 0)
    return labs, np.array([0, *np.cumsum(counts)], dtype=np.int64)


def check_labels(fr, x, sizes, max_eps, eps, min_pts, tag, flags):
    with N.radius_flags(flags):      # (a rescan beyond max_eps builds the graph again)
        got = fr.cluster(eps, min_pts)
    labs, cptr = labels_ref(x, sizes, max_eps, eps, min_pts)
    s = starts_of(sizes)
    assert got.dtype == np.intp and got.shape == (s[-1],)
    for e, (a, b) in enumerate(zip(s, s[1:])):
        assert np.array_equal(got[a:b], labs[e]), f"{tag}: labels of event {e}, eps={eps} min_pts={min_pts}"
    assert fr.cluster_ptr.dtype == torch.int64
    assert np.array_equal(fr.cluster_ptr.cpu().numpy(), cptr), f"{tag}: cluster_ptr eps={eps} min_pts={min_pts}"
    return labs


# ------------------------------------------------------------------------------------------ radius graph per event
def case_radius_events(device, dim, flags):
    """``radius_kernel<D, .., true>`` at D = 2, 4, 8, 32 and ``radius_pruned_kernel<D, .., true>`` at D = 4, 8"""
    sizes = RADIUS_EVENTS
    assert 0 in sizes and 1 in sizes and sum(sizes[:4]) < 256 < sum(sizes[:5])
    x = N.cloud(sum(sizes), dim, "val_events")
    r = 1.3 * N.cluster_radius(dim)
    fr = rescanner(device, x, r, flags, sizes)
    off, nbr = check_graph(fr, x, sizes, r, f"per-event radius graph dim={dim} flags={flags}")
    assert int(np.diff(off).max()) > 3 and int(np.diff(off).min()) == 1
    # (the inputs would show a mixture: the graph over all rows has edges between events)
    full = N.radius_ref(x, r)
    assert len(full[1]) > len(nbr), "no pair of hits of different events inside the radius"


def case_radius_chunk_edges(device):
    sizes = CHUNK_EVENTS
    edges = set(range(64, sum(sizes), 64))
    s = starts_of(sizes)
    assert 64 not in s and 128 in s and any(a < 192 < b for a, b in zip(s, s[1:])), (s, edges)
    for dim in (3, 12):
        x = N.cloud(sum(sizes), dim, "val_chunks")
        r = 1.3 * N.cluster_radius(dim)
        fr = rescanner(device, x, r, N.PRUNED, sizes)
        check_graph(fr, x, sizes, r, f"per-event pruned graph over chunk edges, dim={dim}")
        check_labels(fr, x, sizes, r, 0.8 * r, 3, f"chunk edges dim={dim}", N.PRUNED)


def case_radius_big_events(device):
    """above ``kRadiusPrunedMinRows`` by the total n, no flag: the pruned form, events that start, end and straddle the
    64-chunk turns of the box loop"""
    sizes = BIG_EVENTS
    n = sum(sizes)
    ends = starts_of(sizes)[1:]
    assert n >= 4096 and ends[0] < 4096 < ends[1] and ends[1] < 8192 < ends[2] and sizes[3] == 1
    x = N.cloud(n, 3, "events")
    r = 0.05
    fr = rescanner(device, x, r, 0, sizes)
    off, _ = check_graph(fr, x, sizes, r, "per-event radius graph over three turns of the box loop")
    assert int(np.diff(off).max()) > 3
    labs = check_labels(fr, x, sizes, r, 0.04, 3, "big events", 0)
    assert all(lab.max() >= 1 and lab.min() == -1 for lab in (labs[0], labs[2], labs[4])) and labs[3].tolist() == [-1]


def case_colliding_events(device, flags):
    """the same 300 points as two events: no list reaches into the other event, although every hit has its twin at
    distance 0 there - the graph over the mixture has twice the edges"""
    c = N.cloud(300, 3, "val_collide")
    x = torch.cat([c, c])
    sizes = (300, 300)
    r = 1.3 * N.cluster_radius(3)
    fr = rescanner(device, x, r, flags, sizes)
    off, nbr = check_graph(fr, x, sizes, r, f"colliding events flags={flags}")
    rows = np.repeat(np.arange(600), np.diff(off))
    assert np.array_equal(rows < 300, nbr < 300), "a neighbour of another event"
    with N.radius_flags(flags):
        mixed = DBSCANFastRescan(x.to(device), max_eps=r, device=device)
    assert mixed._n_edges == 2 * fr._n_edges
    labs = check_labels(fr, x, sizes, r, r, 3, f"colliding events flags={flags}", flags)
    assert np.array_equal(labs[0], labs[1]) and labs[0].max() >= 1


# ------------------------------------------------------------------------------------------------- DBSCAN labels
@functools.lru_cache(maxsize=None)
def dbscan_events():
    """four of ``neighbor_cases.DBSCAN_SHAPES``' point sets in 4 dimensions (narrower ones padded with zeros, which add
    exactly 0 to a distance), scaled to the radius of the cloud: the ``all_core`` / ``all_noise`` cloud, a zig-zag
    chain of 300 points (more than 32 pointer hops), the ``duplicates`` clumps, and ``shared_border``"""
    r, _ = N._trials(4)
    cloud = N.cloud(300, 4, "shapes")
    n = 300
    order = np.empty(n, dtype=np.int64)
    i = np.arange(n)
    order[n // 2 + np.where(i % 2 == 1, -((i + 1) // 2), i // 2)] = i
    chain = np.zeros((n, 4), dtype=np.float32)
    chain[:, :2] = (N._chain(order) * np.float32(r)).numpy()
    g = np.random.default_rng(N._seed("val_duplicates"))
    dup = np.zeros((150, 4), dtype=np.float32)
    dup[:, :3] = np.repeat(g.uniform(-1, 1, size=(7, 3)), (1, 2, 3, 10, 64, 65, 5), axis=0)[g.permutation(150)]
    pos = [1.2, 1.3, 1.4, 1.5, 0.0, 0.1, 0.2, 0.3, 0.75, 9.0]
    border = np.zeros((10, 4), dtype=np.float32)
    border[:, 0] = np.array(pos, dtype=np.float32) * np.float32(r / 0.5)
    parts = (cloud.numpy(), chain, dup, border)
    return torch.from_numpy(np.concatenate(parts)), tuple(len(p) for p in parts), r


def case_dbscan_events(device, flags):
    x, sizes, r = dbscan_events()
    longest = int(np.diff(N.radius_ref(x[:300], r)[0]).max())
    assert longest < 64
    fr = rescanner(device, x, r, flags, sizes)
    tag = f"DBSCAN per event, flags={flags}"
    check_graph(fr, x, sizes, r, tag)
    labs = check_labels(fr, x, sizes, r, r, longest + 1, tag, flags)
    assert (labs[0] == -1).all() and labs[2].max() == 1 and (labs[1] == -1).all(), "the first event is all noise"
    labs = check_labels(fr, x, sizes, r, r, 1, tag, flags)
    assert all(lab.min() == 0 for lab in labs) and not labs[1].any(), "every hit is core; the chain is one cluster"
    labs = check_labels(fr, x, sizes, r, 0.5 * r, 2, tag, flags)
    assert labs[0].max() >= 1 and labs[0].min() == -1
    check_labels(fr, x, sizes, r, 1.7 * r, 3, tag, flags)      # eps > max_eps: the batched graph is built again
    check_graph(fr, x, sizes, 1.7 * r, tag + " (rebuilt)")
    labs = check_labels(fr, x, sizes, 1.7 * r, r, 4, tag, flags)
    assert labs[3].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, -1], "shared_border, as the event alone"


def case_one_event_is_todays_call(device, flags):
    """one event in ``batch`` and ``batch=None``: today's path and today's tensors; an unsorted ``batch`` is refused"""
    x = N.cloud(300, 4, "shapes")
    r, trials = N._trials(4)
    with N.radius_flags(flags):
        plain = DBSCANFastRescan(x.to(device), max_eps=r, device=device)
        for kw in (dict(batch=torch.zeros(300, dtype=torch.long, device=device)), dict(batch=None),
                   dict(ptr=torch.tensor([0, 300], device=device))):
            fr = DBSCANFastRescan(x.to(device), max_eps=r, device=device, **kw)
            assert fr._ptr is None and fr._n_edges == plain._n_edges
            for a, b in ((fr._off, plain._off), (fr._nbr, plain._nbr), (fr._dist, plain._dist)):
                assert torch.equal(a, b)
            for eps, mp in trials:
                assert torch.equal(fr.cluster_device(eps, mp), plain.cluster_device(eps, mp))
            assert fr.cluster_ptr is None
    N.check_graph(plain, x, r, "one event")
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor((100, 200)))
    batch[3], batch[150] = 1, 0
    try:
        DBSCANFastRescan(x.to(device), max_eps=r, batch=batch.to(device), device=device)
    except ValueError as e:
        assert "sorted" in str(e)
    else:
        raise AssertionError("an unsorted batch vector was not refused")


# -------------------------------------------------------------------------------------- tracking metrics per event
BIG_IDS = (2 ** 60 + 1, 2 ** 60 + 2, 2 ** 60 - 5)


@functools.lru_cache(maxsize=None)
def metric_events():
    """hits of ``METRIC_EVENTS`` with the same particle ids in every event (0 and ids near 2^60 among them), NaNs in
    pt / eta / reconstructable, no particle passing the hit mask in the first event; three labellings with local
    labels, label 0 in every event, the third event all noise in the second trial"""
    sizes = METRIC_EVENTS
    n = sum(sizes)
    g = np.random.default_rng(N._seed("val_metrics"))
    ids = np.array([0, *range(1, 12), *BIG_IDS], dtype=np.int64)
    pid = g.choice(ids, n)
    pt = g.choice(np.array([0.3, 0.5, 0.9, 0.95, 1.5, 2.0, np.nan], np.float32), n)
    eta = g.choice(np.array([0.1, -3.9, 4.0, -4.0, 2.5, np.nan], np.float32), n)
    reco = g.choice(np.array([0, 1, np.nan], np.float32), n, p=[0.2, 0.75, 0.05])
    reco[:sizes[0]] = 0
    s = starts_of(sizes)
    labels = np.full((3, n), -1, dtype=np.int64)
    for t in range(3):
        for a, b in zip(s, s[1:]):
            if b > a:
                pid[a:a + len(ids)] = ids       # (every id in every event)
                labels[t, a:b] = g.integers(-2, min(b - a, 6 + 10 * t), size=b - a)
                labels[t, a] = 0
    labels[1, s[2]:s[3]] = -1
    return pid, pt, eta, reco, labels


def case_metrics_events(device):
    sizes = METRIC_EVENTS
    pid, pt, eta, reco, labels = metric_events()
    s = starts_of(sizes)
    for a, b in zip(s, s[1:]):
        if b > a:
            assert set(BIG_IDS + (0,)) <= set(pid[a:b].tolist()) and (labels[(0, 2), a] == 0).all()
    assert R.tracking_counts(labels[0, :40], pid[:40], pt[:40], eta[:40], reco[:40], CUTS)[0].tolist() == [0, 0, 0, 0]
    hits = dict(truth=torch.from_numpy(pid).to(device), pts=torch.from_numpy(pt).to(device),
                eta=torch.from_numpy(eta).to(device), reconstructable=torch.from_numpy(reco).to(device))
    got = CM.tracking_metrics_trials(torch.from_numpy(labels).to(device), pt_thlds=CUTS, ptr=N.seg_ptr_of(sizes).to(device),
                                     **hits)
    empty = CM.tracking_metrics_trials(torch.zeros((1, 0), dtype=torch.int64), truth=pid[:0], pts=pt[:0], eta=eta[:0],
                                       reconstructable=reco[:0], pt_thlds=CUTS)[0]
    assert len(got) == 3 and all(len(g) == len(sizes) for g in got)
    differ = 0
    for t in range(3):
        for e, (a, b) in enumerate(zip(s, s[1:])):
            want = R.tracking_metrics_flat(labels[t, a:b], pid[a:b], pt[a:b], eta[a:b], reco[a:b], CUTS)
            if b == a:
                assert list(got[t][e]) == list(empty)
            assert_same(got[t][e], want, f"trial {t} event {e}", ordered=b > a)
            if e == 2:
                assert (want["n_cleaned_clusters"] == 0) == (t == 1), "all noise in the second trial only"
        # (the inputs would show a mixture: the unbatched call on the same rows counts particles across events)
        mixed = R.tracking_metrics_flat(labels[t], pid, pt, eta, reco, CUTS)
        differ += mixed["n_particles"] != sum(g["n_particles"] for g in got[t])
    assert differ == 3


def case_metrics_bad_label(device):
    """a label equal to the event's number of hits is refused; the unbatched call takes the same value (it is < n)"""
    sizes = METRIC_EVENTS
    pid, pt, eta, reco, labels = metric_events()
    bad = labels.copy()
    bad[2, 7] = sizes[0]
    hits = dict(truth=torch.from_numpy(pid).to(device), pts=torch.from_numpy(pt).to(device),
                eta=torch.from_numpy(eta).to(device), reconstructable=torch.from_numpy(reco).to(device))
    try:
        CM.tracking_metrics_trials(torch.from_numpy(bad).to(device), pt_thlds=CUTS, ptr=N.seg_ptr_of(sizes).to(device), **hits)
    except ValueError as e:
        assert "1 labels are >=" in str(e)
    else:
        raise AssertionError("a label beyond its event's hits was not refused")
    got = CM.tracking_metrics_trials(torch.from_numpy(bad).to(device), pt_thlds=CUTS, **hits)
    assert_same(got[2], R.tracking_metrics_flat(bad[2], pid, pt, eta, reco, CUTS), "the same labels without events")


def case_metrics_tie(device):
    """event 0: cluster 0 holds two hits each of the ids 7 (pt 2.0) and 9 (pt 0.5) - the tie goes to 7, the cluster counts
    at the 0.9 cut; event 1: its cluster 0 holds six hits of id 3 (pt 0.5), which a mixture would make the majority"""
    pid = np.array([7, 7, 9, 9, 9] + [3] * 6 + [7], dtype=np.int64)
    lab = np.array([[0, 0, 0, 0, -1] + [0] * 6 + [-1]], dtype=np.int64)
    pt = np.where(pid == 7, np.float32(2.0), np.float32(0.5)).astype(np.float32)
    eta, reco = np.zeros(12, np.float32), np.ones(12, np.float32)
    sizes = (5, 7)
    got = CM.tracking_metrics_trials(torch.from_numpy(lab).to(device), truth=torch.from_numpy(pid).to(device),
                                     pts=torch.from_numpy(pt).to(device), eta=torch.from_numpy(eta).to(device),
                                     reconstructable=torch.from_numpy(reco).to(device), pt_thlds=(0.0, 0.9),
                                     ptr=N.seg_ptr_of(sizes).to(device))[0]
    assert got[0]["n_cleaned_clusters_pt0.9"] == 1 and got[1]["n_cleaned_clusters_pt0.9"] == 0
    assert got[1]["n_cleaned_clusters"] == 1 and got[1]["perfect"] == 1 / 2
    for e, (a, b) in enumerate(((0, 5), (5, 12))):
        assert_same(got[e], R.tracking_metrics_flat(lab[0, a:b], pid[a:b], pt[a:b], eta[a:b], reco[a:b], (0.0, 0.9)),
                    f"tie, event {e}")
    assert R.tracking_metrics_flat(lab[0], pid, pt, eta, reco, (0.0, 0.9))["n_cleaned_clusters_pt0.9"] == 0


def case_metrics_one_event(device):
    """``ptr=None`` and ``ptr=[0, n]``: today's return types and values, from the single-event entry alone"""
    pid, pt, eta, reco, labels = metric_events()
    s = starts_of(METRIC_EVENTS)
    rows = slice(s[2], s[3])
    n, lab = METRIC_EVENTS[2], labels[(0, 2), rows]
    assert n == 300 and lab.max() < n and (lab >= 0).any()
    hits = dict(truth=torch.from_numpy(pid[rows]).to(device), pts=torch.from_numpy(pt[rows]).to(device),
                eta=torch.from_numpy(eta[rows]).to(device), reconstructable=torch.from_numpy(reco[rows]).to(device))
    entries = ("gnntrk_tracking_metrics", "gnntrk_tracking_metrics_batched")
    first = None
    for ptr in one_event_ptrs(n):
        with counted_calls(entries) as calls:
            got = CM.tracking_metrics_trials(torch.from_numpy(lab).to(device), pt_thlds=CUTS, **hits,
                                             **({} if ptr is None else {"ptr": ptr}))
        assert calls == {entries[0]: 1, entries[1]: 0}, calls
        assert isinstance(got, list) and len(got) == 2
        first = got if first is None else first
        for t in range(2):
            assert isinstance(got[t], dict) and [type(v) for v in got[t].values()] == [type(v) for v in first[t].values()]
            assert_same(got[t], first[t], f"one event, trial {t}: ptr={ptr!r} against ptr=None")
            assert_same(got[t], R.tracking_metrics_flat(lab[t], pid[rows], pt[rows], eta[rows], reco[rows], CUTS),
                        f"one event, trial {t}")


# --------------------------------------------------------------------------------------------- scanners end to end
@functools.lru_cache(maxsize=None)
def scan_events():
    """three events of the cfg5 generator at a tenth of its size, as tests/test_tc_batch_gpu.py builds them: the 8 latent
    coordinates are ``H``; ids of 2000 particles, so that they repeat inside and across events"""
    out = []
    for i, n in enumerate(SCAN_HITS):
        ev = synthetic.make_pileup_event(600 + i, 20_000, 8, n_particles=2000, n_clusters=600)
        out.append({k: ev[k][:n].contiguous() for k in ("x", "particle_id", "pt", "eta", "reconstructable")})
    return tuple(out)


def scan_data(raw, device):
    return G.Data(x=raw["x"].to(device), edge_index=torch.zeros(2, 0, dtype=torch.long, device=device),
                  **{k: raw[k].to(device) for k in ("particle_id", "pt", "eta", "reconstructable")})


records_equal = partial(_records_equal, skip=("i_batch",))


def foms_equal(got, want, what, skip=("trk.i_batch", "trk.i_batch_std")):
    assert list(got) == list(want), what
    for k, v in want.items():
        if k not in skip:
            assert got[k] == v or (got[k] != got[k] and v != v), f"{what}: {k} = {got[k]!r}, want {v!r}"


def case_scanner_batch(device):
    events = [scan_data(raw, device) for raw in scan_events()]
    alone = DBSCANHyperParamScannerFixed(list(SCAN_TRIALS))
    for i, d in enumerate(events):
        alone(d, {"H": d.x}, i)
    assert len(alone._results) == 12 and any(r["n_cleaned_clusters"] > 0 for r in alone._results)
    data = G.collate(events)
    batched = DBSCANHyperParamScannerFixed(list(SCAN_TRIALS))
    assert batched.per_event
    batched(data, {"H": data.x}, 0)
    records_equal(batched._results, alone._results, "scanner on a collated batch")
    assert [list(r) for r in batched._results] == [list(r) for r in alone._results], "no new column"
    foms_equal(batched.get_foms(), alone.get_foms(), "figures of merit")
    # the reference's behaviour, which ignores `batch`: one record per trial, today's call on the mixture
    mixture = DBSCANHyperParamScannerFixed(list(SCAN_TRIALS))
    mixture.per_event = False
    mixture(data, {"H": data.x}, 0)
    plain = G.Data(**{k: getattr(data, k) for k in ("x", "particle_id", "pt", "eta", "reconstructable")})
    today = DBSCANHyperParamScannerFixed(list(SCAN_TRIALS))
    today(plain, {"H": plain.x}, 0)
    assert len(mixture._results) == 4
    records_equal(mixture._results, today._results, "per_event = False")
    assert any(m["n_particles"] != sum(r["n_particles"] for r in batched._results[k::4])
               for k, m in enumerate(mixture._results)), "the mixture counts particles across events"


def case_performance_details_batch(device):
    events = [scan_data(raw, device) for raw in scan_events()]
    alone = DBSCANPerformanceDetails(eps=0.25, min_samples=2)
    for i, d in enumerate(events):
        alone(d, {"H": d.x}, i)
    data = G.collate(events)
    batched = DBSCANPerformanceDetails(eps=0.25, min_samples=2)
    batched(data, {"H": data.x}, 0)
    (h_got, c_got), (h_want, c_want) = batched.get_results(), alone.get_results()
    assert len(h_got) == len(c_got) == 3
    for e in range(3):
        assert list(h_got[e]) == list(h_want[e]) and list(c_got[e]) == list(c_want[e])
        for k in h_want[e]:
            g, w = h_got[e][k].cpu().numpy(), h_want[e][k].cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f"hit record {e}: {k}"
        assert len(c_want[e]["c"]) > 10
        for k in c_want[e]:
            g, w = c_got[e][k], c_want[e][k]
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f"cluster table {e}: {k}"
