"""The k-scan on a collated batch of events, shared by the emulator tests (tests/test_kscan_batch_emul.py) and the GPU
tests (tests/test_kscan_batch_gpu.py): ``gnntrk_kscan_counts_batched`` (csrc/kscan.hip) through
``k_scanner.kscan_counts(..., ptr=...)`` and ``GraphConstructionKNNScanner`` on ``collate([...])``.

A batch of B events is B independent scans, so the oracle is the single-event one applied to every event's rows:
``kscan_ref.scan_table`` / ``batch_records`` and, inside the latter, ``tracking_metrics_ref``.  Every comparison is
exact: the integer tables, the labels and the floats derived from the counts.  There is no tolerance in this file.
Each case asserts on the oracle's own output that what it is there for occurs."""

from __future__ import annotations

import functools
import logging

import numpy as np
import torch

import gnn_tracking_amd as G
import kscan_ref as R
from batch_util import assert_same, counted_calls, one_event_ptrs, ptr_of, records_equal, starts_of
from gnn_tracking_amd import GraphConstructionKNNScanner
from gnn_tracking_amd import k_scanner as KS
from test_kscan_gpu import chain_event

#: an empty event, a one-hit event, a two-hit event, a 256-thread block that spans four events, event edges inside a
#: wave (rows 5, 75, 139) and inside a block (row 396)
TABLE_EVENTS = (5, 0, 70, 64, 257, 1, 2)
KMAX = 5
TABLE_KS = [3, 1, KMAX, 2, 3]       # unsorted, with a repeat, kmax larger than n_s - 1 of the small events
#: the same ids in every event: 0 (noise), small ones, ids beyond 2^31 and a negative one
IDS = (0, 1, 2, 3, 2 ** 40 + 1, 2 ** 40 + 2, -2 ** 41)
UNMASKED_EVENT = 3
SCAN_HITS = (300, 257, 40)
N_BAD = R.COLUMNS.index("n_bad")
N_PIDS = R.COLUMNS.index("n_pids")


def random_tables(sizes, kmax, seed, unmasked=None):
    """per event: neighbour entries drawn inside the event, cnt in 0..kmax, ids of ``IDS`` (every id in every event
    that has room for them), a mask (none of the hits of event ``unmasked``) and 2 n_s true edges inside the event"""
    g = np.random.default_rng(seed)
    s = starts_of(sizes)
    n = s[-1]
    nbr = np.zeros((n, kmax), dtype=np.int32)
    cnt = g.integers(0, kmax + 1, size=n).astype(np.int32)
    pid = g.choice(np.array(IDS, dtype=np.int64), n)
    mask = g.random(n) < 0.7
    te = []
    for e, (a, b) in enumerate(zip(s, s[1:])):
        if b == a:
            continue
        nbr[a:b] = g.integers(a, b, size=(b - a, kmax))
        if b - a >= len(IDS):
            pid[a:a + len(IDS)] = IDS
        if e == unmasked:
            mask[a:b] = False
        te.append(g.integers(a, b, size=(2, 2 * (b - a))))
    return nbr, cnt, pid, mask, np.concatenate(te, axis=1).astype(np.int64)


def scan_device(device, nbr, cnt, ks, pid, mask, te, sizes):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    counts, labels = KS.kscan_counts(t(nbr.reshape(-1)), t(cnt), nbr.shape[1], ks, t(pid), t(mask), t(te),
                                     ptr=ptr_of(sizes, device))
    assert counts.shape == (len(sizes), len(ks), len(R.COLUMNS)) and labels.shape == (len(ks), len(cnt))
    return counts.cpu().numpy(), labels.cpu().numpy()


def scan_oracle(nbr, cnt, ks, pid, mask, te, sizes):
    """``kscan_ref.scan_table`` of every event's rows alone (indices shifted to the event); an empty event: zeros"""
    s = starts_of(sizes)
    counts = np.zeros((len(sizes), len(ks), len(R.COLUMNS)), dtype=np.int64)
    labels = np.zeros((len(ks), s[-1]), dtype=np.int64)
    for e, (a, b) in enumerate(zip(s, s[1:])):
        if b == a:
            continue
        mine = (te[0] >= a) & (te[0] < b)
        assert ((te[1][mine] >= a) & (te[1][mine] < b)).all()
        counts[e], labels[:, a:b] = R.scan_table(nbr[a:b] - a, cnt[a:b], ks, pid[a:b], mask[a:b], te[:, mine] - a)
    return counts, labels


def assert_events_equal(got, want, sizes, what):
    (gc, gl), (wc, wl) = got, want
    s = starts_of(sizes)
    for e, (a, b) in enumerate(zip(s, s[1:])):
        assert np.array_equal(gc[e], wc[e]), f"{what}: counts of event {e}\n{gc[e]}\nwant\n{wc[e]}"
        assert np.array_equal(gl[:, a:b], wl[:, a:b]), f"{what}: labels of event {e}"


# ------------------------------------------------------------------------------------------- case 1: random tables
@functools.lru_cache(maxsize=None)
def table_case():
    args = random_tables(TABLE_EVENTS, KMAX, 1801, unmasked=UNMASKED_EVENT)
    return args, scan_oracle(args[0], args[1], TABLE_KS, *args[2:], TABLE_EVENTS)


def case_random_tables(device):
    sizes = TABLE_EVENTS
    (nbr, cnt, pid, mask, te), (want_c, want_l) = table_case()
    s = starts_of(sizes)
    assert 0 in sizes and 1 in sizes and 2 in sizes and sum(sizes[:4]) < 256 < sum(sizes[:5]) and s[-1] > 256
    assert any(a % 64 for a in s[1:-1]), "no event edge inside a wave"
    big = [set(pid[a:b].tolist()) for a, b in zip(s, s[1:]) if b - a >= len(IDS)]
    assert len(big) >= 3 and all(set(IDS) <= ids for ids in big), "the ids do not repeat from event to event"
    assert (want_c[UNMASKED_EVENT, :, N_PIDS] == 0).all() and (want_c[4, :, N_PIDS] > 0).all()
    assert not want_c[1].any() and not want_c[:, :, N_BAD].any()
    assert all((want_l[:, a:b] < b - a).all() for a, b in zip(s, s[1:])) and (want_l[:, s[4]:s[5]] > 0).any()
    # (the inputs would show a mixture: one scan over all rows counts a particle once, not once per event)
    mixed, _ = R.scan_table(nbr, cnt, TABLE_KS, pid, mask, te)
    assert (mixed[:, N_PIDS] < want_c[:, :, N_PIDS].sum(0)).all()
    got = scan_device(device, nbr, cnt, TABLE_KS, pid, mask, te, sizes)
    assert_events_equal(got, (want_c, want_l), sizes, "random tables")
    again = scan_device(device, nbr, cnt, TABLE_KS, pid, mask, te, sizes)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


# --------------------------------------------------------------------------------------- case 2: cross-event input
def case_cross_event_entries(device):
    """the last valid neighbour entry of a few queries and an end of a few true edges point into another event, at a
    hit with the query's / the other end's particle id: a scan without events would unite the two.  Expected: the
    scan of the input without these entries (cnt one lower, the true edges dropped), and these entries in n_bad of the
    event of the query / of the true edge's first end."""
    sizes = TABLE_EVENTS
    (nbr, cnt, pid, mask, te), _ = table_case()
    nbr, cnt_cut, te = nbr.copy(), cnt.copy(), te.copy()
    s = starts_of(sizes)
    event_of = np.repeat(np.arange(len(sizes)), sizes)
    bad = np.zeros(len(sizes), dtype=np.int64)
    g = np.random.default_rng(1802)

    def twin(q):
        """a hit of another event with q's particle id"""
        pool = np.flatnonzero((pid == pid[q]) & (event_of != event_of[q]))
        assert pool.size
        return int(g.choice(pool))

    queries = [int(g.choice(np.flatnonzero((event_of == e) & (cnt > 0)))) for e in (0, 2, 2, 4, 6)]
    assert len(set(queries)) == len(queries)
    for q in queries:
        nbr[q, cnt[q] - 1] = twin(q)
        cnt_cut[q] -= 1
        bad[event_of[q]] += 1
    edges = g.choice(te.shape[1], 4, replace=False)
    for i, t in enumerate(edges):
        end = 0 if i == 0 else 1                       # (one edge's first end moves, the others' second)
        te[end, t] = twin(int(te[1 - end, t]))
        bad[event_of[te[0, t]]] += 1
    assert bad.sum() == 9 and (bad > 0).sum() >= 3 and bad[1] == 0
    keep = np.ones(te.shape[1], dtype=bool)
    keep[edges] = False
    want_c, want_l = scan_oracle(nbr, cnt_cut, TABLE_KS, pid, mask, te[:, keep], sizes)
    want_c[:, :, N_BAD] = bad[:, None]
    got = scan_device(device, nbr, cnt, TABLE_KS, pid, mask, te, sizes)
    assert_events_equal(got, (want_c, want_l), sizes, "cross-event entries")
    assert all((got[1][:, a:b] >= 0).all() and (got[1][:, a:b] < max(b - a, 1)).all() for a, b in zip(s, s[1:]))


# ------------------------------------------------------------------------------------- case 3: many small events
def case_many_small_events(device):
    g = np.random.default_rng(1803)
    sizes = tuple(g.integers(3, 10, size=70).tolist())
    s = starts_of(sizes)
    ks = [2, 1, 4]
    nbr, cnt, pid, mask, te = random_tables(sizes, 4, 1804)
    per_wave = [len({int(e) for e in np.repeat(np.arange(70), sizes)[a:a + 64]}) for a in range(0, s[-1], 64)]
    assert len(sizes) > 256 // 64 and min(per_wave) >= 2 and s[-1] > 256
    want = scan_oracle(nbr, cnt, ks, pid, mask, te, sizes)
    assert (want[0][:, -1, N_PIDS] > 0).sum() > 60 and len({tuple(c.ravel()) for c in want[0]}) > 60
    got = scan_device(device, nbr, cnt, ks, pid, mask, te, sizes)
    assert_events_equal(got, want, sizes, "many small events")


# ------------------------------------------------------------------------------------------ case 5: the scanner
FIELDS = ("x", "particle_id", "pt", "eta", "reconstructable", "true_edge_index")


@functools.lru_cache(maxsize=None)
def scan_events():
    """three events of ``test_kscan_gpu.chain_event`` (particles as short chains in 8 dimensions, 10 % noise hits with
    id 0, true edges along the chains); the particle ids 2^40 .. 20 * 2^40 occur in every event"""
    return tuple(chain_event(1810 + i, n, n_particles=20) for i, n in enumerate(SCAN_HITS))


def data_of(raw, device):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    return G.Data(**{k: t(v) for k, v in zip(FIELDS, raw)})


@functools.lru_cache(maxsize=None)
def scan_oracle_records(max_edges=5_000_000):
    return tuple(tuple(R.batch_records(*raw, list(range(1, 10)), max_edges=max_edges)) for raw in scan_events())


def one_by_one(events, **kw):
    alone = GraphConstructionKNNScanner(**kw)
    for i, d in enumerate(events):
        alone(d, i)
    return alone


def case_scanner_batch(device):
    raws = scan_events()
    assert all(set(raws[0][1].tolist()) & set(r[1].tolist()) - {0} for r in raws[1:]) and all(0 in r[1] for r in raws)
    events = [data_of(raw, device) for raw in raws]
    data = G.collate(events)
    oracle = scan_oracle_records()
    assert [len(r) for r in oracle] == [9, 9, 9] and sum(r[-1]["frac50"] > r[0]["frac50"] for r in oracle) >= 2
    assert all(r["max_n_particles_pt0.9"] > 0 for recs in oracle for r in recs)
    alone = one_by_one(events)
    batched = GraphConstructionKNNScanner()
    assert batched.per_event
    batched(data, 0)
    records_equal(batched.results_raw, alone.results_raw, "scanner on a collated batch")
    records_equal(batched.results_raw, [r for recs in oracle for r in recs], "scanner against the restatement")
    assert [r["k"] for r in batched.results_raw] == 3 * list(range(1, 10))
    assert_same(batched.get_foms(), alone.get_foms(), "figures of merit")
    # the reference's behaviour, which ignores `batch`: one record per k, today's call on the mixture
    mixture = GraphConstructionKNNScanner()
    mixture.per_event = False
    mixture(data, 0)
    today = GraphConstructionKNNScanner()
    today(G.Data(**{k: getattr(data, k) for k in FIELDS}), 0)
    assert len(mixture.results_raw) == 9
    records_equal(mixture.results_raw, today.results_raw, "per_event = False")
    assert any(m["max_n_particles_pt0.9"] != sum(r["max_n_particles_pt0.9"] for r in batched.results_raw[k::9])
               for k, m in enumerate(mixture.results_raw)), "the mixture counts particles across events"
    single = GraphConstructionKNNScanner()
    single(G.collate(events[:1]), 0)
    records_equal(single.results_raw, alone.results_raw[:9], "a one-event batch")


def case_scanner_one_event(device):
    """a ``Data`` without ``ptr`` and with a one-event ``ptr``: today's records, from the single-event entries alone"""
    raw = scan_events()[0]
    n, ks = SCAN_HITS[0], [1, 2, 3]
    assert n == 300
    want = R.batch_records(*raw, ks, max_edges=5_000_000)
    assert len(want) == 3 and want[-1]["frac50"] > want[0]["frac50"]
    entries = ("gnntrk_kscan_counts", "gnntrk_kscan_counts_batched", "gnntrk_tracking_metrics",
               "gnntrk_tracking_metrics_batched")
    first = None
    for ptr in one_event_ptrs(n):
        data = data_of(raw, device)
        if ptr is not None:
            data.ptr = ptr
        scanner = GraphConstructionKNNScanner(ks=ks)
        with counted_calls(entries) as calls:
            scanner(data, 0)
        assert calls == dict(zip(entries, (1, 0, 1, 0))), calls
        got = scanner.results_raw
        first = got if first is None else first
        records_equal(got, first, f"one event: ptr={ptr!r} against no ptr")
        assert [[type(v) for v in r.values()] for r in got] == [[type(v) for v in r.values()] for r in first]
        records_equal(got, want, "one event against the restatement")


def case_scanner_max_edges(device, caplog):
    """``max_edges`` between the largest graphs of the two larger events: the first event stops early, alone"""
    oracle = scan_oracle_records()
    top = sorted(max(r["n_edges"] for r in recs) for recs in oracle)
    assert top[1] < top[2] and top[2] == oracle[0][-1]["n_edges"]
    max_edges = top[1]
    want = scan_oracle_records(max_edges)
    assert len(want[0]) < 9 and len(want[1]) == len(want[2]) == 9
    events = [data_of(raw, device) for raw in scan_events()]
    alone = one_by_one(events, max_edges=max_edges)
    batched = GraphConstructionKNNScanner(max_edges=max_edges)
    with caplog.at_level(logging.WARNING, logger="gnn_tracking_amd"):
        caplog.clear()
        batched(G.collate(events), 0)
    assert [r.getMessage() for r in caplog.records if "max edges" in r.getMessage()] == \
        [f"Not scanning k>={len(want[0]) + 1} in event 0 because max edges exceeded "
         f"({oracle[0][len(want[0])]['n_edges']} > {max_edges})"]
    records_equal(batched.results_raw, alone.results_raw, "max_edges per event")
    records_equal(batched.results_raw, [r for recs in want for r in recs], "max_edges per event, restatement")
    assert_same(batched.get_foms(), alone.get_foms(), "figures of merit with max_edges")


def case_scanner_small_event(device):
    """an event of one hit between two others: no record of its own (alone it is refused), the others untouched"""
    raws = scan_events()
    events = [data_of(raws[0], device), data_of(tuple(a[:1] for a in raws[1][:5]) + (np.zeros((2, 0), np.int64),), device),
              data_of(raws[2], device)]
    try:
        GraphConstructionKNNScanner()(events[1], 0)
    except ValueError as e:
        assert "at least two hits" in str(e)
    else:
        raise AssertionError("a one-hit event alone was not refused")
    batched = GraphConstructionKNNScanner()
    batched(G.collate(events), 0)
    oracle = scan_oracle_records()
    records_equal(batched.results_raw, [*oracle[0], *oracle[2]], "a one-hit event in the batch")


def case_scanner_refuses_cross_event_true_edge(device):
    events = [data_of(raw, device) for raw in scan_events()]
    data = G.collate(events)
    data.true_edge_index[1, 0] = SCAN_HITS[0] + 3        # (its first end is a hit of event 0)
    assert int(data.true_edge_index[0, 0]) < SCAN_HITS[0]
    try:
        GraphConstructionKNNScanner()(data, 0)
    except ValueError as e:
        assert "1 neighbour or true-edge indices of event 0" in str(e)
    else:
        raise AssertionError("a true edge across two events was not refused")
