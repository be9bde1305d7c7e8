"""Condensation losses on a collated batch of events (``_CondensationLoss.per_event``, csrc/oc.hip ``*_batched``),
shared by tests/test_oc_batch_emul.py (CPU emulator) and tests/test_oc_batch_gpu.py.

The reference of a batch is the blocked fp64 oracle of tests/oc_cases.py run on every event ALONE (``oc_cases.reference``:
computed once per (event, loss, weights) and shared with the single-event tests): the terms averaged over the events,
the gradients divided by the number of events and concatenated, Tiger's ``n_rep`` summed.  Events come from
``oc_cases.make_event`` and its relatives, so its conditions 1 to 4 hold for every event alone - and a hit never meets a
condensation point of another event, so they hold for the batch.

Bars (oc_cases): terms and total 1e-5 relative (exact 0 where the reference is 0); the gradient rows of every event
1e-4 of the largest entry of that event's oracle gradient, all finite; ``n_rep`` exact.  ``neighbor_cap`` is "off"
except in the neighbour-cap case."""

from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch

import oc_cases as C
import ref_cpu as O
from gnn_tracking_amd import ops
from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger, _CondensationLoss

#: 1: event starts inside 256-hit blocks, 64-hit waves and the 128-hit staging chunk; 21 hits: norm_att = 1e-9
TILE_HITS = (255, 257, 21, 129, 256, 64, 65)
#: 2: point ranges that straddle the 128-point LDS chunk at unaligned offsets
CHUNK_KS = (127, 129, 1, 128, 65)
CHUNK_WIDTHS = (3, 8)
#: 4: one width per padded class of the dense kernels
WIDTHS = (1, 2, 4, 8, 16, 17, 32)
ODD_IN_BATCH = ("huge_ids", "negative_ids", "beta_ties", "unmasked_particles")


# ---------------------------------------------------------------------------------------------- runs, checks
@contextlib.contextmanager
def _settings(cap="off", per_event=True):
    old = C.losses_oc.SPATIAL, CondensationLossRG.neighbor_cap, getattr(_CondensationLoss, "per_event", True)
    C.losses_oc.SPATIAL, CondensationLossRG.neighbor_cap, _CondensationLoss.per_event = "off", cap, per_event
    try:
        yield
    finally:
        C.losses_oc.SPATIAL, CondensationLossRG.neighbor_cap, _CondensationLoss.per_event = old


def _cat(events, name):
    return torch.cat([getattr(e, name) for e in events])


def _batch_of(events):
    return torch.repeat_interleave(torch.arange(len(events)), torch.tensor([e.n for e in events]))


def run_batch(device, events, mode, *, term=None, weights=None, batch="events", keep=None, cap="off", per_event=True,
              **loss_kw):
    """forward and backward of the loss on the concatenated events.  ``batch``: "events" (the event number of every
    hit), None, or a tensor.  ``keep`` (bool per hit): the model's ``ec_hit_mask`` - beta and x have the kept rows,
    the data attributes all of them (the radius-graph loss wants ``eta`` sliced by its caller, as in the reference)."""
    if isinstance(batch, str):
        batch = _batch_of(events)
    sel = slice(None) if keep is None else keep
    b = _cat(events, "beta")[sel].to(device, copy=True).requires_grad_(True)
    x = _cat(events, "x")[sel].to(device, copy=True).requires_grad_(True)
    eta = _cat(events, "eta")
    if keep is not None and mode == "rg":
        eta = eta[keep]
    kw = dict(beta=b, x=x, particle_id=_cat(events, "pid").to(device), reconstructable=_cat(events, "reco").to(device),
              pt=_cat(events, "pt").to(device), eta=eta.to(device))
    if batch is not None:
        kw["batch"] = batch.to(device)
    if keep is not None:
        kw["ec_hit_mask"] = keep.to(device)
    with _settings(cap, per_event):
        ret = C.LOSSES[mode](**(C.WEIGHTS if weights is None else weights), **loss_kw)(**kw)
        (ret.loss if term is None else ret.loss_dct[term]).backward()
    res = {t: float(ret.loss_dct[t].detach()) for t in C.TERMS}
    res.update(total=float(ret.loss.detach()), grad_x=x.grad.detach().cpu(), grad_beta=b.grad.detach().cpu(),
               n_rep=int(ret.extra_metrics["n_rep"]) if mode == "tiger" else None)
    return res


def _mean_of(ods, weights=(1.0, 2.0, 0.25, 0.5)):
    """the per-event results (oracle or single-event runs) as the reference of their batch"""
    n = len(ods)
    want = {t: sum(od[t] for od in ods) / n for t in C.TERMS}
    want["total"] = sum(w * want[t] for w, t in zip(weights, C.TERMS))
    want["grads"] = [(od["grad_x"] / n, od["grad_beta"] / n) for od in ods]
    want["n_rep"] = sum(od["n_rep"] or 0 for od in ods)
    return want


def check_batch(res, want, mode, what, terms=C.TERMS, total=True):
    for t in terms:
        C._check_term(res[t], want[t], f"{what} {t}")
    if total:
        C._check_term(res["total"], want["total"], f"{what} total")
    at = 0
    for e, (gx, gb) in enumerate(want["grads"]):
        n = gx.shape[0]
        C._check_grad(res["grad_x"][at:at + n], gx, f"{what} event {e} grad_x")
        C._check_grad(res["grad_beta"][at:at + n], gb, f"{what} event {e} grad_beta")
        at += n
    assert at == res["grad_x"].shape[0] == res["grad_beta"].shape[0], what
    if mode == "tiger":
        assert res["n_rep"] == want["n_rep"], f"{what}: n_rep {res['n_rep']}, the events alone have {want['n_rep']}"


def _against_oracle(device, events, mode, what, **kw):
    res = run_batch(device, events, mode, **kw)
    check_batch(res, _mean_of([C.reference(ev, mode) for ev in events]), mode, f"{what} {mode}")
    return res


# ---------------------------------------------------------------------------------------------- cases
def case_tile_edges(device, mode, reverse):
    """1: events that align with no tile"""
    events = [C.n_edge_event(n) for n in (TILE_HITS[::-1] if reverse else TILE_HITS)]
    _against_oracle(device, events, mode, "tile edges" + (" reversed" if reverse else ""))


def case_chunk_edges(device, mode, dim):
    """2: K = 127, 129, 1, 128, 65 in one batch"""
    _against_oracle(device, [C.k_edge_event(k, dim) for k in CHUNK_KS], mode, f"chunk edges width {dim}")


def _slice_oracle(events, mode, weights=(1.0, 2.0, 0.25, 0.5)):
    """the fp64 oracle on the concatenated hits as ONE event (what ignoring ``batch`` computes)"""
    pid = _cat(events, "pid")
    return O.condensation_loss_chunked(beta=_cat(events, "beta"), x=_cat(events, "x"), particle_id=pid,
                                       mask=_cat(events, "mask"), mode=mode, weights=weights)


@functools.lru_cache(maxsize=None)
def _shared_id_events():
    """two different events; every id of the second is one of the first's (50 of its 60)"""
    a, b = C.make_event(300, 60, 3), C.make_event(280, 50, 3)
    ids_a, ids_b = torch.unique(a.pid[a.pid > 0]), torch.unique(b.pid[b.pid > 0])
    assert ids_a.numel() == 60 and ids_b.numel() == 50
    pid = b.pid.clone()
    for old, new in zip(ids_b.tolist(), ids_a[:50].tolist()):   # (one to one: the event's particles stay what they are)
        pid[b.pid == old] = new
    arrays = {"beta": b.beta.numpy(), "x": b.x.numpy(), "pt": b.pt.numpy(), "eta": b.eta.numpy(), "reco": b.reco.numpy(),
              "pid": pid.numpy()}
    b2 = C.Event(arrays, 50)
    shared = np.intersect1d(ids_a.numpy(), np.unique(b2.pid.numpy()))
    assert shared.size >= 30
    return a, b2


def case_colliding_ids(device, mode, kind):
    """3: particle ids that repeat from event to event ("copies": one event three times, all ids and coordinates
    coincide; "shared": two events, the ids of one among the other's).  The oracle on the mixture gives other terms:
    the case cannot pass on a path that ignores ``batch``."""
    events = [C.make_event(300, 60, 3)] * 3 if kind == "copies" else list(_shared_id_events())
    want = _mean_of([C.reference(ev, mode) for ev in events])
    mixed = _slice_oracle(events, mode)
    far = max(abs(mixed[t] - want[t]) / abs(want[t]) for t in ("attractive", "repulsive"))
    assert far > 1e-2, f"the mixture's terms are the per-event means to {far:.1e}: the case shows nothing"
    res = run_batch(device, events, mode)
    check_batch(res, want, mode, f"colliding ids ({kind}) {mode}")
    if kind == "copies":
        single = C.reference(events[0], mode)
        for t in C.TERMS:
            C._check_term(res[t], single[t], f"copies {mode} {t} against the single event")


def case_width(device, mode, dim):
    """4: one width per padded class, two events"""
    _against_oracle(device, [C.make_event(700, 140, dim), C.make_event(300, 60, dim)], mode, f"width {dim}")


def case_term_gradient(device, mode, term):
    """5: ``loss_dct[term].backward()`` on a three-event batch"""
    events = [C.make_event(700, 140, 5), C.make_event(300, 60, 5), C.make_event(257, 50, 5)]
    w = C._one_hot(term)
    res = run_batch(device, events, mode, term=term)
    want = _mean_of([C.reference(ev, mode, w) for ev in events], w)
    check_batch(res, want, mode, f"d {term} {mode}", terms=(term,), total=False)


def _sliced(ev, keep):
    """the event without the dropped hits (what the loss sees of it)"""
    k = keep.numpy()
    a = {"beta": ev.beta.numpy()[k], "x": ev.x.numpy()[k], "pt": ev.pt.numpy()[k], "eta": ev.eta.numpy()[k],
         "reco": ev.reco.numpy()[k], "pid": ev.pid.numpy()[k]}
    uniq = torch.unique(ev.pid[keep & ev.mask])
    return C.Event(a, int(uniq.numel()), min_rep=0)


@functools.lru_cache(maxsize=None)
def _masked_events():
    events = (C.make_event(700, 140, 3), C.make_event(300, 60, 3), C.make_event(257, 20, 3))
    g = np.random.default_rng(6)
    keeps = [torch.from_numpy(g.uniform(size=ev.n) >= 0.2) for ev in events]
    for ev, keep in zip(events, keeps):
        assert bool((keep & ev.mask).any()) and int((~keep).sum()) > ev.n // 8
    return events, keeps, tuple(_sliced(ev, keep) for ev, keep in zip(events, keeps))


def case_ec_hit_mask(device, mode):
    """6: about a fifth of the hits dropped by ``ec_hit_mask``; the oracle runs on the sliced events"""
    events, keeps, sliced = _masked_events()
    res = run_batch(device, list(events), mode, keep=torch.cat(keeps))
    check_batch(res, _mean_of([C.reference(ev, mode) for ev in sliced]), mode, f"ec_hit_mask {mode}")


def case_kth_neighbor(device):
    """7: ``ops.knn_kth_neighbor(seg_ptr=...)`` is, event by event, the event's own answer (integers)"""
    events = [C.make_event(90, 20, 3), C.make_event(257, 20, 3), C.make_event(64, 20, 3)]
    x = _cat(events, "x").to(device)
    ptr = [0, 90, 347, 411]
    seg_ptr = torch.tensor(ptr, dtype=torch.int64, device=device)
    for radius in (None, 1.0):
        for k in (4, 63, 64, 89, 90, 100, 256, 300):   # below, at and above the neighbours an event can have
            got = ops.knn_kth_neighbor(x, k, radius, seg_ptr=seg_ptr).cpu()
            for ev, lo, hi in zip(events, ptr[:-1], ptr[1:]):
                alone = ops.knn_kth_neighbor(ev.x.to(device), k, radius).cpu()
                mine = got[lo:hi]
                assert torch.equal(torch.where(mine >= 0, mine - lo, mine), alone), f"k {k} radius {radius} event at {lo}"
            if k == 4 and radius is None:
                assert bool((got >= 0).all())


def case_neighbor_cap(device):
    """7: ``neighbor_cap = "nearest"`` at ``max_num_neighbors = 4`` on a three-event batch against the mean of the
    single-event runs of the same product path (the blocked oracle has no cap)"""
    events = [C.make_event(300, 60, 3), C.make_event(257, 20, 3), C.make_event(129, 20, 3)]
    alone = [run_batch(device, [ev], "rg", batch=None, cap="nearest", max_num_neighbors=4) for ev in events]
    free = [run_batch(device, [ev], "rg", batch=None) for ev in events]
    assert any(a["repulsive"] != f["repulsive"] for a, f in zip(alone, free)), "the cap binds in no event"
    res = run_batch(device, events, "rg", cap="nearest", max_num_neighbors=4)
    check_batch(res, _mean_of([dict(a, grad_x=a["grad_x"].double(), grad_beta=a["grad_beta"].double()) for a in alone]),
                "rg", "neighbour cap")


def case_no_change(device, mode):
    """8: ``batch=None``, an all-zero ``batch`` and ``per_event = False`` with a multi-event batch return, bit for bit,
    what the call without ``batch`` returns"""
    ev = C.make_event(300, 60, 3)
    plain = C.run(device, ev, mode, "off")
    C._same_bits(run_batch(device, [ev], mode, batch=None), plain, f"{mode} batch=None")
    C._same_bits(run_batch(device, [ev], mode, batch=torch.zeros(ev.n, dtype=torch.long)), plain, f"{mode} all-zero batch")
    events = list(_shared_id_events())
    mixed = run_batch(device, events, mode, batch=None)
    C._same_bits(run_batch(device, events, mode, per_event=False), mixed, f"{mode} per_event=False")


def case_refusals(device):
    """9"""
    import pytest

    events = [C.make_event(300, 60, 3), C.make_event(257, 20, 3)]
    batch = _batch_of(events)
    for mode in C.LOSSES:
        with pytest.raises(ValueError, match="sorted"):
            run_batch(device, events, mode, batch=batch.flip(0))
        with pytest.raises(ValueError, match="entries"):
            run_batch(device, events, mode, batch=batch[:-1])
        # an event without a hit of interest: the second one with every pt below the threshold
        b = events[1]
        dull = C.Event({"beta": b.beta.numpy(), "x": b.x.numpy(), "pt": np.full(b.n, 0.5, np.float32), "eta": b.eta.numpy(),
                        "reco": b.reco.numpy(), "pid": b.pid.numpy()}, 0)
        with pytest.raises(AssertionError, match=r"No hits left after masking \(event 1\)"):
            run_batch(device, [events[0], dull], mode)
    with pytest.raises(ValueError, match="max_n_rep"):
        run_batch(device, events, "tiger", max_n_rep=10)


def case_odd_events(device, mode):
    """10: odd events and a plain one in one batch (width 4; negative ids are Tiger's noise only)"""
    names = [n for n in ODD_IN_BATCH if not (n == "negative_ids" and mode == "rg")]
    _against_oracle(device, [C.odd_event(n) for n in names] + [C.make_event(300, 60, 4)], mode, "odd events")
