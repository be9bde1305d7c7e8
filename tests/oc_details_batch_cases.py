"""The binned tracking metrics, the cluster table and the clustering scores of a collated batch of events, shared by the
emulator tests (tests/test_oc_details_batch_emul.py) and the GPU tests (tests/test_oc_details_batch_gpu.py):
``gnntrk_tracking_metrics_windows_batched`` / ``gnntrk_cluster_table_batched`` (csrc/tracking_metrics.hip),
``gnntrk_cluster_spectra_batched`` (csrc/cluster_scores.hip) and what ``cluster_metrics`` / ``postprocessing`` build on
them.

A batch of B events is B independent problems, so the oracles are the single-event ones applied to every event's rows:
``tracking_binned_ref.window_counts`` / ``cluster_table`` / ``vs_pt`` / ``vs_eta`` and ``cluster_scores_ref.spectra``.
Everything is integer counting and every comparison is exact; floats that the host derives from the counts are compared
with ``==`` (or both NaN) against the package's own single-event call on the event's rows.  There is no tolerance in this
file.  Each case asserts on the oracle's output that what it is there for occurs."""

from __future__ import annotations

import functools
import itertools
import math

import numpy as np
import torch

import batch_util
import cluster_scores_cases as S
import cluster_scores_ref as SR
import gnn_tracking_amd as G
import neighbor_cases as N
import oc_validation_batch_cases as V
import tracking_binned_cases as T
import tracking_binned_ref as B
from batch_util import one_event_ptrs, ptr_of, starts_of
from gnn_tracking_amd import _capi
from gnn_tracking_amd import cluster_metrics as CM
from gnn_tracking_amd.postprocessing import DBSCANPerformanceDetails

#: an empty event, a one-hit event, and no 256-slot block that lies inside one event: all three span an event edge
EVENTS = (40, 0, 300, 257, 1)
#: the second and third 256-slot block lie inside the second event (the LDS path of the clusters kernel), the fourth spans
#: the last edge
INNER_EVENTS = (200, 700, 90)
BIG_IDS = V.BIG_IDS
IDS = np.array([0, *range(1, 12), *BIG_IDS], dtype=np.int64)
#: EVENTS, then an event with a cluster, a class and a cell of more than 2048 hits, two identical events, and a second
#: event with a cluster of the same large size
SPECTRA_EVENTS = EVENTS + (2500, 120, 120, 2300)
BIG = 2100
TABLE_KEYS = ("c",) + T.TABLE_COLUMNS


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@functools.lru_cache(maxsize=None)
def hits_of(sizes, n_trials=2):
    """hits of ``sizes`` with NaNs in pt / eta / reconstructable; every id of ``IDS`` (0 and ids near 2^60 among them) in
    every event that has room for them, the one-hit event holds one of them; local labels with label 0 in every event"""
    n = sum(sizes)
    g = np.random.default_rng(N._seed(f"details{sizes}"))
    pid = g.choice(IDS, n)
    _, pt, eta, reco = T.random_event(g, n, 4, False)
    s = starts_of(sizes)
    labels = np.full((n_trials, n), -1, dtype=np.int64)
    for t in range(n_trials):
        for a, b in zip(s, s[1:]):
            if b - a >= len(IDS):
                pid[a:a + len(IDS)] = IDS
            if b > a:
                labels[t, a:b] = g.integers(-2, min(b - a, 12 + 20 * t), size=b - a)
    # most hits of a particle share a cluster (its index among the ids, where the event has that many labels), so that
    # there are double-majority and LHC matches; particle 1 keeps a cluster to itself in the first trial (perfect matches)
    rank = np.searchsorted(np.sort(IDS), pid)
    for t in range(n_trials):
        for a, b in zip(s, s[1:]):
            keep = (g.random(b - a) < 0.85 - 0.2 * t) & (rank[a:b] < b - a)
            labels[t, a:b] = np.where(keep, rank[a:b], labels[t, a:b])
            if b > a:
                labels[t, a] = 0
    one = np.searchsorted(np.sort(IDS), 1)
    labels[0] = np.where(pid == 1, np.where(one < np.repeat(np.diff(s), np.diff(s)), one, -1),
                         np.where(labels[0] == one, -1, labels[0]))
    for a, b in zip(s, s[1:]):
        if b > a:
            labels[0, a] = 0
    return pid, pt, eta, reco, labels


@functools.lru_cache(maxsize=None)
def windows40():
    """the 32 overlapping windows with NaN bounds of ``random_windows`` and 8 of a second draw: two chunks of the entry"""
    g = np.random.default_rng(N._seed("details_windows"))
    return np.concatenate([T.random_windows(g), T.random_windows(g)[:8]])


def same_float(a, b):
    return a == b or (a != a and b != b)


def assert_columns_equal(got: dict, want: dict, what: str):
    """dtype and every value (NaN equals NaN) of the same columns in the same order"""
    assert list(got) == list(want), f"{what}: columns {list(got)}"
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f"{what}: {k}"


def hit_kwargs(pid, pt, eta, reco, device, rows=slice(None)):
    return dict(truth=dev(pid[rows], device), pts=dev(pt[rows], device), eta=dev(eta[rows], device),
                reconstructable=dev(reco[rows], device))


def record_of(labels, pid, pt, eta, reco, device, rows=slice(None)):
    return T.hit_record(dict(labels=labels[rows], pid=pid[rows], pt=pt[rows], eta=eta[rows], reco=reco[rows]),
                        lambda a: dev(a, device))


# ---------------------------------------------------------------------------------------- 1. windows and table per event
def case_windows_and_table(device, sizes=EVENTS):
    pid, pt, eta, reco, labels = hits_of(sizes)
    s = starts_of(sizes)
    n = s[-1]
    blocks = [(c0, min(c0 + 256, n) - 1) for c0 in range(0, n, 256)]
    inside = [any(a <= c0 and c1 < b for a, b in zip(s, s[1:])) for c0, c1 in blocks]
    if sizes == EVENTS:
        assert 0 in sizes and 1 in sizes and not any(inside), "every 256-slot block spans an event edge"
        assert all(np.isnan(v).any() for v in (pt, eta, reco))
    else:
        assert any(inside) and not all(inside), "blocks inside one event and a block over an edge"
    for a, b in zip(s, s[1:]):
        if b - a >= len(IDS):
            assert set(IDS.tolist()) <= set(pid[a:b].tolist())
        if b > a:
            assert (labels[:, a] == 0).all() and pid[a] in IDS
    win = windows40()
    assert len(win) > 32 and np.isnan(win).any()
    ptr = ptr_of(sizes, device)
    for t in range(labels.shape[0]):
        tables = CM.tracking_metric_table(dev(labels[t], device), ptr=ptr, **hit_kwargs(pid, pt, eta, reco, device))
        n_part, counts = CM._window_counts(record_of(labels[t], pid, pt, eta, reco, device), win, 3, ptr=ptr)
        assert isinstance(tables, list) and len(tables) == len(sizes)
        assert n_part.shape == (len(sizes), len(win)) and counts.shape == (len(sizes), len(win), 4)
        for e, (a, b) in enumerate(zip(s, s[1:])):
            rows = slice(a, b)
            what = f"trial {t} event {e} of {sizes}"
            want = B.cluster_table(labels[t, rows], pid[rows], pt[rows], eta[rows], reco[rows])
            T.assert_table(tables[e], want, what, dtypes=True, exact_means=True)
            alone = CM.tracking_metric_table(dev(labels[t, rows], device), **hit_kwargs(pid, pt, eta, reco, device, rows))
            assert_columns_equal(tables[e], alone, what + " (the package's single-event table)")
            if b == a:
                assert all(len(tables[e][k]) == 0 for k in TABLE_KEYS)
            want_part, want_counts = B.window_counts(labels[t, rows], pid[rows], pt[rows], eta[rows], reco[rows], win)
            assert np.array_equal(n_part[e], want_part), f"{what}: n_particles per window"
            assert np.array_equal(counts[e], want_counts), f"{what}: cluster counts per window"
        assert (counts.sum(axis=(0, 1)) > 0).all() and n_part.sum() > 0, "clusters and matches of every kind"
        # (the inputs would show a mixture: the unbatched count over the same rows joins the particles of the events)
        mixed_part, _ = B.window_counts(labels[t], pid, pt, eta, reco, win)
        assert (mixed_part != n_part.sum(axis=0)).any(), "no particle id shared between events inside a window"
        assert len(B.cluster_table(labels[t], pid, pt, eta, reco)["c"]) < sum(len(tb["c"]) for tb in tables)


# ------------------------------------------------------------------------------------- 2. majority tie inside the event
def case_tie(device):
    """the 12 hits of ``oc_validation_batch_cases.case_metrics_tie``: in event 0 cluster 0 holds two hits each of the ids 7
    (pt 2.0) and 9 (pt 0.5) - the tie goes to 7, so the cluster lies in the window pt >= 0.9; in event 1 cluster 0 holds
    six hits of id 3 (pt 0.5), which a mixture would make the majority"""
    pid = np.array([7, 7, 9, 9, 9] + [3] * 6 + [7], dtype=np.int64)
    lab = np.array([0, 0, 0, 0, -1] + [0] * 6 + [-1], dtype=np.int64)
    pt = np.where(pid == 7, np.float32(2.0), np.float32(0.5)).astype(np.float32)
    eta, reco = np.zeros(12, np.float32), np.ones(12, np.float32)
    sizes = (5, 7)
    ptr = ptr_of(sizes, device)
    tables = CM.tracking_metric_table(dev(lab, device), ptr=ptr, **hit_kwargs(pid, pt, eta, reco, device))
    assert tables[0]["maj_pid"].tolist() == [7] and tables[0]["maj_hits"].tolist() == [2]
    assert tables[1]["maj_pid"].tolist() == [3] and tables[1]["c"].tolist() == [0]
    win = np.array([[0.9, np.nan, np.nan, np.nan]], dtype=np.float32)
    n_part, counts = CM._window_counts(record_of(lab, pid, pt, eta, reco, device), win, 3, ptr=ptr)
    assert counts[:, 0, 0].tolist() == [1, 0] and n_part[:, 0].tolist() == [1, 1]
    for e, (a, b) in enumerate(((0, 5), (5, 12))):
        rows = slice(a, b)
        T.assert_table(tables[e], B.cluster_table(lab[rows], pid[rows], pt[rows], eta[rows], reco[rows]), f"tie, event {e}",
                       dtypes=True, exact_means=True)
        want_part, want_counts = B.window_counts(lab[rows], pid[rows], pt[rows], eta[rows], reco[rows], win)
        assert np.array_equal(n_part[e], want_part) and np.array_equal(counts[e], want_counts)
    mixed = B.cluster_table(lab, pid, pt, eta, reco)
    assert mixed["maj_pid"].tolist() == [3] and B.window_counts(lab, pid, pt, eta, reco, win)[1][0, 0] == 0


# ----------------------------------------------------------------------------------------------------- 3. bad label
def case_bad_label(device):
    """a label equal to its event's number of hits is refused by the table and by the windows"""
    sizes = EVENTS
    pid, pt, eta, reco, labels = hits_of(sizes)
    bad = labels[0].copy()
    bad[7] = sizes[0]
    assert bad[7] < sum(sizes), "the unbatched entries take this value"
    ptr = ptr_of(sizes, device)
    calls = (lambda: CM.tracking_metric_table(dev(bad, device), ptr=ptr, **hit_kwargs(pid, pt, eta, reco, device)),
             lambda: CM._window_counts(record_of(bad, pid, pt, eta, reco, device), windows40()[:3], 3, ptr=ptr))
    for call in calls:
        try:
            call()
        except ValueError as e:
            assert "1 labels are >=" in str(e)
        else:
            raise AssertionError("a label beyond its event's hits was not refused")
    CM.tracking_metric_table(dev(bad, device), **hit_kwargs(pid, pt, eta, reco, device))


# -------------------------------------------------------------------------------------------------------- 4. spectra
@functools.lru_cache(maxsize=None)
def spectra_hits():
    """truth ids and three labellings of ``SPECTRA_EVENTS``: random ones as ``cluster_scores_cases.random_case`` draws them
    (ids of any size, labels from -3 up: negative labels are clusters), the same ids and labels in every event; in the two
    large events a cluster of ``BIG`` hits, in the first also a class of ``BIG`` hits that shares 2080 hits with it; the two
    events of 120 hits identical"""
    sizes = SPECTRA_EVENTS
    s = starts_of(sizes)
    g = np.random.default_rng(N._seed("details_spectra"))
    truth, labels = S.random_case(g, s[-1], 3)
    truth %= 2 ** 40 * 5          # (few ids, negative ones and 0 among them: every one repeats from event to event)
    truth -= 2 ** 41
    labels %= 9
    labels -= 3
    a = s[5]
    labels[:, a:a + BIG] = 7
    truth[a + 20:a + 20 + BIG] = 3 * 2 ** 40
    truth[s[7]:s[8]] = truth[s[6]:s[7]]
    labels[:, s[7]:s[8]] = labels[:, s[6]:s[7]]
    a = s[8]
    labels[:2, a:a + BIG] = 7
    return truth, labels


def capacity_ref(n, n_seg):
    d = lambda x: (math.isqrt(8 * x + 1) - 1) // 2     # noqa: E731
    return n_seg * (d(-(-n // n_seg)) + 1) if n > 0 else 0


def case_spectra(device):
    sizes = SPECTRA_EVENTS
    truth, labels = spectra_hits()
    s = starts_of(sizes)
    n = s[-1]
    lib = _capi.load()
    cap = int(lib.gnntrk_cluster_spectra_batched_capacity(n, len(sizes)))
    assert cap == capacity_ref(n, len(sizes))
    ptr = ptr_of(sizes, device)
    got = CM.clustering_spectra(dev(labels, device), dev(truth, device), ptr)
    scores = CM.clustering_scores_trials(dev(labels, device), truth=dev(truth, device), ptr=ptr)
    no_truth = CM.clustering_spectra(dev(labels, device), ptr=ptr)
    empty = CM.clustering_spectra(np.zeros(0, np.int64), np.zeros(0, np.int64))[0]
    empty_scores = CM.clustering_scores_trials(np.zeros(0, np.int64), truth=np.zeros(0, np.int64))[0]
    assert len(got) == len(scores) == len(no_truth) == 3 and all(len(g) == len(sizes) for g in got + scores + no_truth)
    entries = np.zeros(3, dtype=np.int64)     # per kind of spectrum the entries of all events together, at most
    assert (truth < 0).any() and (truth == 0).any() and (labels < 0).any()
    for t in range(3):
        total = np.zeros(3, dtype=np.int64)
        for e, (a, b) in enumerate(zip(s, s[1:])):
            what = f"spectra of trial {t} event {e}"
            if b == a:
                assert all(len(v[0]) == 0 for v in got[t][e].values()) and list(got[t][e]) == list(empty)
                assert scores[t][e] == empty_scores
                continue
            want = SR.spectra(labels[t, a:b], truth[a:b])
            S.assert_spectra(got[t][e], want, b - a, what)
            S.assert_spectra(no_truth[t][e], SR.spectra(labels[t, a:b]), b - a, what + " without truth")
            total += [len(want[k][0]) for k in ("classes", "clusters", "cells")]
            alone = CM.clustering_scores_trials(dev(labels[t:t + 1, a:b], device), truth=dev(truth[a:b], device))[0]
            assert list(scores[t][e]) == list(alone) and all(same_float(scores[t][e][k], alone[k]) for k in alone), what
        entries = np.maximum(entries, total)
        # d of every pooled list: each of its triples went to exactly one event
        d = [sum(len(g[k][0]) for g in got[t]) for k in ("classes", "clusters", "cells")]
        assert d == total.tolist() and 0 < max(d) <= cap, (d, cap)
        # the large-size table: a cluster of BIG hits in both large events of the first two trials (the same (size) in two
        # events: two entries), a class of BIG hits and a cell of more than 2048 in the first
        first, last = SR.spectra(labels[t, s[5]:s[6]], truth[s[5]:s[6]]), SR.spectra(labels[t, s[8]:], truth[s[8]:])
        assert first["clusters"][0][-1] == BIG and first["classes"][0][-1] == BIG and first["cells"][0][-1] == BIG - 20
        assert (last["clusters"][0][-1] == BIG) == (t < 2)
        # negative labels are ordinary clusters, in more than one event
        assert sum(int((labels[t, a:b] < 0).any()) for a, b in zip(s, s[1:])) >= 2
        # two events with identical labels and identical truth ids: a mixture would merge them
        a, b, c = s[6], s[7], s[8]
        assert np.array_equal(labels[t, a:b], labels[t, b:c]) and np.array_equal(truth[a:b], truth[b:c])
        assert got[t][6].keys() == got[t][7].keys()
        for k in got[t][6]:
            assert np.array_equal(got[t][6][k][0], got[t][7][k][0]) and np.array_equal(got[t][6][k][1], got[t][7][k][1])
        both = SR.spectra(labels[t, a:c], truth[a:c])
        assert np.array_equal(both["clusters"][0], 2 * got[t][6]["clusters"][0]), "the mixture has clusters of twice the size"
    # capacity is not why this passes: the host refuses a list beyond cap instead of clipping it, and the entries the
    # oracle counts are all there - more of them than ONE event of n hits could have, so the single-event bound would
    # not do for the largest list if the events had as many hits as the first large one
    assert entries.max() <= cap, (entries, cap)
    assert entries.max() > int(lib.gnntrk_cluster_spectra_capacity(sizes[5])), (entries, sizes[5])
    # (the whole batch as one event has other spectra: equal ids and labels of different events merge)
    mixed = SR.spectra(labels[0], truth)
    assert len(mixed["classes"][0]) < entries[0]


def case_capacity(lib):
    """``cap`` bounds the sum of D(n_e): exhaustively for up to 4 events of up to 24 hits, and the formula's values"""
    d = lambda x: (math.isqrt(8 * x + 1) - 1) // 2     # noqa: E731
    caps = {(n, b): int(lib.gnntrk_cluster_spectra_batched_capacity(n, b)) for n in range(0, 97) for b in range(1, 5)}
    assert all(v == capacity_ref(n, b) for (n, b), v in caps.items())
    assert all(int(lib.gnntrk_cluster_spectra_batched_capacity(n, 1)) == int(lib.gnntrk_cluster_spectra_capacity(n)) + 1
               for n in (1, 2, 3, 5999, 6000, 150_000))
    assert lib.gnntrk_cluster_spectra_batched_capacity(0, 3) == 0 and lib.gnntrk_cluster_spectra_batched_capacity(-1, 3) == 0
    assert int(lib.gnntrk_cluster_spectra_batched_capacity(192_000, 32)) == capacity_ref(192_000, 32) == 32 * 110
    worst = 0
    for k in (2, 3, 4):
        for part in itertools.product(range(21), repeat=k):
            need = sum(d(x) for x in part)
            assert need <= caps[(sum(part), k)], part
            worst = max(worst, need)
    assert worst == 4 * d(20)


# ------------------------------------------------------------------------------------- 5. one event is today's call
def case_one_event(device):
    """``ptr=[0, n]`` and ``ptr=None``: today's return types and values"""
    pid, pt, eta, reco, labels = hits_of((300,))
    truth, _ = S.random_case(np.random.default_rng(5), 300, 1)
    n = 300
    for ptr in one_event_ptrs(n):
        kw = {} if ptr is None else {"ptr": ptr}
        table = CM.tracking_metric_table(dev(labels[0], device), **hit_kwargs(pid, pt, eta, reco, device), **kw)
        assert isinstance(table, dict)
        T.assert_table(table, B.cluster_table(labels[0], pid, pt, eta, reco), "one event", dtypes=True, exact_means=True)
        sp = CM.clustering_spectra(dev(labels, device), dev(truth, device), **kw)
        sc = CM.clustering_scores_trials(dev(labels, device), truth=dev(truth, device), **kw)
        assert len(sp) == len(sc) == labels.shape[0]
        for t in range(labels.shape[0]):
            assert isinstance(sp[t], dict) and isinstance(sc[t], dict) and list(sc[t]) == list(CM.SCORE_KEYS)
            S.assert_spectra(sp[t], SR.spectra(labels[t], truth), n, f"one event, trial {t}")
            assert sc[t] == CM._scores_from_spectra(SR.spectra(labels[t], truth))


# -------------------------------------------------------------------------------------------- 6. scanner end to end
COUNTED = ("gnntrk_cluster_table", "gnntrk_cluster_table_batched", "gnntrk_tracking_metrics_windows",
           "gnntrk_tracking_metrics_windows_batched")


def counted_calls():
    """the table and windows entries: {entry: number of calls}"""
    return batch_util.counted_calls(COUNTED)


def rows_identical(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w) and all(same_float(g[k], w[k]) for k in w), f"{what}: row {j}"


def case_scanner(device):
    events = [V.scan_data(raw, device) for raw in V.scan_events()]
    pt_edges = np.linspace(0.0, 4.0, 41).tolist()          # 40 bins: two chunks of 32 windows
    eta_edges = np.linspace(-4.0, 4.0, 9).tolist()
    chunks = math.ceil(40 / 32) + 1                        # windows calls per record: vs_pt, then the 8 eta bins
    alone = DBSCANPerformanceDetails(eps=0.25, min_samples=2)
    with counted_calls() as calls:
        for i, d in enumerate(events):
            alone(d, {"H": d.x}, i)
        h_want, c_want = alone.get_results()
        vp_want = CM.tracking_metrics_vs_pt(h_want, c_want, pt_edges)
        ve_want = CM.tracking_metrics_vs_eta(h_want, c_want, eta_edges)
    assert calls == {COUNTED[0]: 3, COUNTED[1]: 0, COUNTED[2]: 3 * chunks, COUNTED[3]: 0}, calls
    data = G.collate(events)
    batched = DBSCANPerformanceDetails(eps=0.25, min_samples=2)
    with counted_calls() as calls:
        batched(data, {"H": data.x}, 0)
        h_got, c_got = batched.get_results()
        vp_got = CM.tracking_metrics_vs_pt(h_got, c_got, pt_edges)
        ve_got = CM.tracking_metrics_vs_eta(h_got, c_got, eta_edges)
    # one table call for the batch, and one windows call per 32 bins - not three times as many
    assert calls == {COUNTED[0]: 0, COUNTED[1]: 1, COUNTED[2]: 0, COUNTED[3]: chunks}, calls
    assert len(h_got) == len(c_got) == 3
    for e in range(3):
        assert isinstance(h_got[e], dict) and list(h_got[e]) == list(h_want[e]) == ["c", "id", "reconstructable", "pt", "eta"]
        assert "origin" not in h_got[e] and h_got[e].origin[1] == e
        for k in h_want[e]:
            g, w = h_got[e][k].cpu().numpy(), h_want[e][k].cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f"hit record {e}: {k}"
        assert len(c_want[e]["c"]) > 10
        assert_columns_equal(c_got[e], c_want[e], f"cluster table {e}")
    rows_identical(vp_got, vp_want, "tracking_metrics_vs_pt")
    rows_identical(ve_got, ve_want, "tracking_metrics_vs_eta")
    assert any(r["n_cleaned_clusters"] > 0 for r in vp_want) and any(r["n_cleaned_clusters"] > 0 for r in ve_want)
    # the records against the restatement, event by event (one batch: every value ==)
    for e, h in enumerate(h_got):
        o = dict(labels=h["c"].cpu().numpy(), pid=h["id"].cpu().numpy(), pt=h["pt"].cpu().numpy(),
                 eta=h["eta"].cpu().numpy(), reco=h["reconstructable"].cpu().numpy())
        assert len(o["pid"]) == V.SCAN_HITS[e]
        T.assert_rows(CM.tracking_metrics_vs_pt([h], [None], pt_edges), B.vs_pt([o], pt_edges), f"vs_pt of event {e}")
        T.assert_rows(CM.tracking_metrics_vs_eta([h], [None], eta_edges), B.vs_eta([o], eta_edges), f"vs_eta of event {e}")
    # records of a batch mixed with records from elsewhere keep their order
    mixed_order = [h_got[2], dict(h_want[0]), h_got[0], h_got[1]]
    with counted_calls() as calls:
        vp_mixed = CM.tracking_metrics_vs_pt(mixed_order, [None] * 4, pt_edges)
    assert calls[COUNTED[3]] == math.ceil(40 / 32) and calls[COUNTED[2]] == math.ceil(40 / 32)
    rows_identical(vp_mixed, CM.tracking_metrics_vs_pt([h_want[2], h_want[0], h_want[0], h_want[1]], [None] * 4, pt_edges),
                   "records of a batch among others")


# ------------------------------------------------------------------------------------- 7. host-side validation
def case_host_validation(lib):
    """NULL ``seg_ptr``, ``n_seg = 0``, a small workspace and a NULL output are refused before any launch"""
    import ctypes

    n = 16
    seg = (ctypes.c_int64 * 3)(0, 6, n)
    lab = (ctypes.c_int64 * (2 * n))()
    ids = (ctypes.c_int64 * n)()
    f = (ctypes.c_float * n)()
    win = (ctypes.c_float * 8)()
    out = (ctypes.c_int64 * (2 * 2 * (1 + 2 * 4) + 1))()
    need = lib.gnntrk_tracking_metrics_windows_workspace_bytes(n, 2)
    ws = (ctypes.c_uint8 * need)()

    def windows(sp=seg, n_seg=2, wb=need, o=out):
        return lib.gnntrk_tracking_metrics_windows_batched(lab, 2, ids, f, f, f, n, sp, n_seg, win, 2, 3, o, ws, wb, None)

    assert windows(sp=None) == 1 and b"seg_ptr" in lib.gnntrk_last_error()
    assert windows(n_seg=0) == 1 and b"n_seg" in lib.gnntrk_last_error()
    assert windows(wb=need - 1) == 1 and b"workspace" in lib.gnntrk_last_error()
    assert windows(o=None) == 1 and b"NULL" in lib.gnntrk_last_error()
    assert windows() == 0 and out[len(out) - 1] == 0
    cols = [(ctypes.c_int64 * n)() for _ in range(4)]
    fcols = [(ctypes.c_float * n)() for _ in range(3)]
    bad = (ctypes.c_int64 * 1)(-1)
    need_t = lib.gnntrk_cluster_table_workspace_bytes(n)
    ws_t = (ctypes.c_uint8 * need_t)()

    def table(sp=seg, n_seg=2, wb=need_t, nb=bad, c0=cols[0]):
        return lib.gnntrk_cluster_table_batched(lab, ids, f, f, f, n, sp, n_seg, c0, *cols[1:], *fcols, nb, ws_t, wb, None)

    assert table(sp=None) == 1 and b"seg_ptr" in lib.gnntrk_last_error()
    assert table(n_seg=0) == 1 and b"n_seg" in lib.gnntrk_last_error()
    assert table(wb=need_t - 1) == 1 and b"workspace" in lib.gnntrk_last_error()
    assert table(nb=None) == 1 and b"NULL" in lib.gnntrk_last_error()
    assert table(c0=None) == 1 and b"NULL" in lib.gnntrk_last_error()
    # labels 0 everywhere: one cluster per event, of the event's hits, in its first row
    assert table() == 0 and bad[0] == 0 and [cols[0][i] for i in (0, 1, 6, 7)] == [6, 0, 10, 0]
    cap = lib.gnntrk_cluster_spectra_batched_capacity(n, 2)
    sp_out = (ctypes.c_int64 * (5 * (1 + 3 * cap)))()
    need_s = lib.gnntrk_cluster_spectra_workspace_bytes(n, 2)
    ws_s = (ctypes.c_uint8 * need_s)()

    def spectra(sp=seg, n_seg=2, wb=need_s, o=sp_out):
        return lib.gnntrk_cluster_spectra_batched(lab, 2, ids, n, sp, n_seg, o, ws_s, wb, None)

    assert spectra(sp=None) == 1 and b"seg_ptr" in lib.gnntrk_last_error()
    assert spectra(n_seg=0) == 1 and b"n_seg" in lib.gnntrk_last_error()
    assert spectra(wb=need_s - 1) == 1 and b"workspace" in lib.gnntrk_last_error()
    assert spectra(o=None) == 1 and b"NULL" in lib.gnntrk_last_error()
    assert spectra() == 0
    for k in range(5):      # one class, one cluster, one cell per event: (event, size, 1) for sizes 6 and 10
        row = list(sp_out[k * (1 + 3 * cap):(k + 1) * (1 + 3 * cap)])
        assert row[0] == 2 and sorted(zip(row[1:7:3], row[2:7:3], row[3:7:3])) == [(0, 6, 1), (1, 10, 1)]
