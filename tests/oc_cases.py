"""Condensation-loss cases shared by the emulator tests (tests/test_oc_emul.py) and the GPU tests
(tests/test_oc_gpu.py): ``CondensationLossRG`` / ``CondensationLossTiger`` (csrc/oc.hip) against the blocked fp64
oracle (oracle/ref_cpu.py: ``condensation_loss_chunked``, pinned on the reference's own values by
tests/test_oracle_golden.py) at every padded width of the dense and of the spatial passes, at the tile edges in the
number of condensation points K and of hits N, in the second condensation-point batch, term by term, and on odd
events (which shape reaches which instantiation).

Bars (the project's, as parity_cases.case_cfg5_condensation):
  * each of the four terms and the weighted total: relative error <= 1e-5; where the oracle's term is exactly 0 the
    kernel's is exactly 0;
  * grad_x, grad_beta: max |difference| <= 1e-4 of the oracle gradient's largest entry (an oracle gradient that is
    exactly 0 everywhere: exact zeros), every entry finite;
  * Tiger's ``n_rep`` equals the oracle's exactly.
Nothing is compared with another kernel path, except where a case says "bit for bit".

Events come from a seeded numpy generator (``make_event``) that enforces, on the fp64 side alone:
  1. coordinates, beta, pt, eta, reconstructable are fp32 values and the oracle gets those same values;
  2. no (hit, condensation point) pair of different particles - for either loss's points - has a distance d with
     |d - 1| < 1e-5 (such a hit is moved 1e-3 along the line to the point, and everything is checked again): the
     repulsive gradient jumps at the radius, and one fp32 flip of ``d2 < 1`` would be a legitimate difference beyond
     the gradient bar (and beyond ``n_rep`` equality);
  3. no two hits of different particles coincide (Tiger's sqrt has no gradient at 0);
  4. (checked on the oracle's own output, ``reference``) K is the intended value, the attractive term is non-zero
     and there are at least ``min_rep`` repulsive pairs (200 unless the case says otherwise): the spread of the
     cluster centres is the largest of 64 * 0.8^i at which this holds; a particle's hits are its centre + 0.15 *
     a normal draw;
  5. about a tenth of the hits are noise (id 0) and about a tenth fail the pt or the eta cut (never all hits of a
     particle), so the two losses pick different condensation points;
and, for Tiger's arg-max of q = atanh(beta)^2 + q_min (fp32 in the reference): the two largest q of a particle are
different fp32 numbers or come from equal betas - the kernels take the arg-max of beta itself, the same hit unless
two different betas round to one q."""

from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch

from gnn_tracking_amd import losses_oc
from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger
import ref_cpu as O

TOL_TERM = 1e-5
TOL_GRAD = 1e-4
WEIGHTS = dict(lw_repulsive=2.0, lw_noise=0.5, lw_coward=0.25)
TERMS = ("attractive", "repulsive", "coward", "noise")
LOSSES = {"rg": CondensationLossRG, "tiger": CondensationLossTiger}
PATHS = ("off", "on")   # losses_oc.SPATIAL: the dense N x K passes, the sorted-chunk passes

#: A / B: both ends of each padded width class (2, 4, 8, 16, 32; the spatial passes pad to 4, 8, 16)
DENSE_WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
SPATIAL_WIDTHS = (1, 4, 5, 8, 9, 16)
FALLBACK_WIDTHS = (17, 32)
#: C: around the 128-point LDS chunk, the 256-thread blocks of the point kernels, the 4 x 64 rounds of the hit pass
K_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 300)
K_EDGE_WIDTHS = (3, 8)
#: D: around the block of 256 hits, the chunk of 64 sorted hits, the 128-hit staging chunk, 32 slices of 128 hits
N_EDGES = (21, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097)
#: F: (hits, width, K)
TERM_SHAPES = ((700, 5, 140), (257, 20, 50))
ODD_EVENTS = ("singletons", "one_particle", "huge_ids", "negative_ids", "beta_ties", "unmasked_particles", "far_outlier",
              "long_own_run", "no_noise")


# ---------------------------------------------------------------------------------------------- events
class Event:
    """fp32 tensors on the CPU (``particle_id``: int64) and what ``reference`` asserts about the oracle's view"""

    def __init__(self, a: dict, k: int, min_rep: int = 200, need_att: bool = True, norm_att_fp64: bool = False):
        self.beta, self.x = torch.from_numpy(a["beta"]), torch.from_numpy(a["x"])
        self.pt, self.eta, self.reco = torch.from_numpy(a["pt"]), torch.from_numpy(a["eta"]), torch.from_numpy(a["reco"])
        self.pid = torch.from_numpy(a["pid"])
        for t in (self.beta, self.x, self.pt, self.eta, self.reco):
            assert t.dtype == torch.float32     # condition 1
        assert self.pid.dtype == torch.int64
        self.mask = O.good_node_mask(self.pt, self.pid, self.reco, self.eta)
        self.k, self.min_rep, self.need_att, self.norm_att_fp64 = k, min_rep, need_att, norm_att_fp64
        self.n, self.dim = int(self.x.shape[0]), int(self.x.shape[1])


def _mask(a):
    return (a["pt"] > 0.9) & (a["pid"] > 0) & (a["reco"] > 0) & (np.abs(a["eta"]) < 4.0)


def _points(a, mode):
    """hit index of each loss's condensation point per particle of interest (ascending id), ties to the lowest index;
    asserts the arg-max condition of the module docstring"""
    pid, mask = a["pid"], _mask(a)
    of_interest = np.unique(pid[mask])
    if mode == "rg":
        cand, score = np.nonzero(mask)[0], a["beta"]
    else:
        cand = np.nonzero(np.isin(pid, of_interest))[0]
        score = (torch.arctanh(torch.from_numpy(a["beta"])) ** 2 + 0.01).numpy()   # fp32, as the oracle
    order = cand[np.lexsort((cand, -score[cand].astype(np.float64), pid[cand]))]
    first = np.nonzero(np.r_[True, pid[order][1:] != pid[order][:-1]])[0]
    if mode == "tiger":
        second = first + 1
        ok = second < order.size
        ok[ok] &= pid[order[second[ok]]] == pid[order[first[ok]]]
        top, nxt = order[first[ok]], order[second[ok]]
        assert np.all((score[top] != score[nxt]) | (a["beta"][top] == a["beta"][nxt])), "two betas of a particle round to one largest q"
    return order[first]


def _blocks(x64, pts, rows=2048):
    """fp64 distances hits x points, block of hits by block"""
    xk = x64[pts]
    k2 = (xk ** 2).sum(1)
    for s in range(0, x64.shape[0], rows):
        xj = x64[s:s + rows]
        yield s, np.sqrt(np.maximum((xj ** 2).sum(1)[:, None] + k2[None, :] - 2.0 * xj @ xk.T, 0.0))


def _count_rep(a, mode="rg"):
    pts = _points(a, mode)
    x64, pid = a["x"].astype(np.float64), a["pid"]
    return sum(int(((d < 1.0) & (pid[s:s + d.shape[0], None] != pid[pts][None, :])).sum()) for s, d in _blocks(x64, pts))


def _on_the_radius(x64, pid, hits, pts, rows=1024):
    """(hit, point) pairs of different particles with |d - 1| < 1e-5, among ``hits`` x ``pts`` (hit indices)"""
    out = []
    xk = x64[pts]
    k2 = (xk ** 2).sum(1)
    for s in range(0, hits.size, rows):
        h = hits[s:s + rows]
        d2 = (x64[h] ** 2).sum(1)[:, None] + k2[None, :] - 2.0 * x64[h] @ xk.T
        for j, k in zip(*np.nonzero(np.abs(d2 - 1.0) < 3e-5)):   # (|d - 1| < 1e-5 is inside |d2 - 1| < 2.1e-5)
            if pid[h[j]] != pid[pts[k]] and abs(np.linalg.norm(x64[h[j]] - x64[pts[k]]) - 1.0) < 1e-5:
                out.append((int(h[j]), int(pts[k])))
    return out


def _off_the_radius(a):
    """condition 2, for the condensation points of both losses.  After the first pass over all pairs only what a
    move can have changed is looked at again: the moved hits against all points and, where a moved hit is a point,
    all hits against it - until nothing is left."""
    pid, every = a["pid"], np.arange(a["pid"].size)
    moved = None
    for _ in range(50):
        pts = np.union1d(_points(a, "rg"), _points(a, "tiger"))
        x64 = a["x"].astype(np.float64)
        if moved is None:
            found = _on_the_radius(x64, pid, every, pts)
        else:
            found = _on_the_radius(x64, pid, moved, pts) + _on_the_radius(x64, pid, every, np.intersect1d(pts, moved))
        if not found:
            return
        for j, c in found:
            x64 = a["x"].astype(np.float64)
            d = np.linalg.norm(x64[c] - x64[j])
            a["x"][j] = (x64[j] + (x64[c] - x64[j]) / d * 1e-3).astype(np.float32)
        moved = np.unique([j for j, _ in found])
    raise AssertionError("hits stay on the radius of a condensation point")


def _no_coincident_hits(a):
    """condition 3"""
    _, inv = np.unique(a["x"], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    same_x = inv[order][1:] == inv[order][:-1]
    assert np.all(a["pid"][order][1:][same_x] == a["pid"][order][:-1][same_x]), "hits of different particles coincide"


def _draw(seed, n, k, dim, n_noise=None, spread=None, min_rep=200):
    """arrays of a clustered event: ``k`` particles of interest (ids in random order, hits interleaved), every one
    with a hit that passes the cuts (``keeper``); ``spread`` None: condition 4's search"""
    g = np.random.default_rng(seed)
    n_noise = max(1, n // 10) if n_noise is None else n_noise
    n_noise = min(n_noise, n - k)
    n_part = n - n_noise
    extras = n_part - k
    owner = np.r_[np.arange(k), g.choice(k, size=extras, replace=extras > k)]
    keeper = np.r_[np.ones(k, bool), np.zeros(extras, bool)]
    ids = g.choice(np.arange(1, 10 * k + 10), size=k, replace=False).astype(np.int64)
    a = {"pid": np.r_[ids[owner], np.zeros(n_noise, np.int64)], "keeper": np.r_[keeper, np.zeros(n_noise, bool)]}
    a["beta"] = g.uniform(0.05, 0.95, size=n).astype(np.float32)
    a["pt"] = g.uniform(1.0, 3.0, size=n).astype(np.float32)
    a["eta"] = g.uniform(-3.5, 3.5, size=n).astype(np.float32)
    a["reco"] = np.ones(n, np.float32)
    # about a tenth of the hits fail a cut: never a keeper; noise hits fail through their id
    free = np.nonzero(~a["keeper"][:n_part])[0]
    cut = g.choice(free, size=min(free.size // 2, max(n // 10, 1)), replace=False)
    a["pt"][cut[::2]] = g.uniform(0.1, 0.89, size=cut[::2].size).astype(np.float32)
    a["eta"][cut[1::2]] = (g.choice([-1.0, 1.0], size=cut[1::2].size) * g.uniform(4.1, 5.0, size=cut[1::2].size)).astype(np.float32)
    centre = g.standard_normal((k + n_noise, dim))
    scatter = 0.15 * g.standard_normal((n, dim))
    where = np.r_[owner, k + np.arange(n_noise)]
    perm = g.permutation(n)

    def placed(s):
        b = {key: v[perm] for key, v in a.items()}
        b["x"] = (s * centre[where] + scatter)[perm].astype(np.float32)
        return b

    if spread is not None:
        return placed(spread)
    for i in range(60):
        b = placed(64.0 * 0.8 ** i)
        if min(_count_rep(b, "rg"), _count_rep(b, "tiger")) >= min_rep:
            return b
    raise AssertionError(f"no spread gives {min_rep} repulsive pairs (n {n}, k {k}, width {dim})")


def _finish(a, k, **kw):
    _off_the_radius(a)
    _no_coincident_hits(a)
    return Event(a, k, **kw)


@functools.lru_cache(maxsize=None)
def make_event(n, k, dim, seed=0, n_noise=None, spread=None, min_rep=200, need_att=True, norm_att_fp64=False):
    return _finish(_draw(1000 * dim + 7 * n + k + seed, n, k, dim, n_noise, spread, min_rep), k, min_rep=min_rep,
                   need_att=need_att, norm_att_fp64=norm_att_fp64)


def k_edge_event(k, dim):
    """case C; at K = 1 only noise hits are repelled and ``norm_rep`` is the bare 1e-9 (the oracle's too): no pair count"""
    return make_event(1000 if k >= 256 else 600, k, dim, min_rep=0 if k == 1 else 200)


def n_edge_event(n):
    """case D: width 3, K = 20.  21 hits with 20 particles of interest and a noise hit (without one the noise term is
    0/0) leave every particle ONE hit: no attractive pair exists, n_oi == K and ``norm_att`` is the bare 1e-9."""
    own = n == 21
    return make_event(n, 20, 3, need_att=not own, norm_att_fp64=own)


def batch2_event():
    """case E: 16 520 particles of interest (280 with two hits) and 500 noise hits, normal draws times 6"""
    ev = make_event(17_300, 16_520, 3, n_noise=500, spread=6.0, min_rep=50_000)
    assert ev.k > 16_384 and int((torch.bincount(torch.unique(ev.pid[ev.pid > 0], return_inverse=True)[1]) == 2).sum()) == 280
    return ev


@functools.lru_cache(maxsize=None)
def odd_event(name):
    """case G: width 4, about 300 hits; conditions 1 to 3 hold for every one of them"""
    seed = 50 + ODD_EVENTS.index(name)
    g = np.random.default_rng(seed)
    kw = {}
    if name == "singletons":
        # every hit of interest is its own particle: n_oi == K, norm_att = 1e-9, attractive exactly 0; the other
        # hits of the drawn particles become particles of their own that fail the pt cut
        a, k = _draw(seed, 300, 240, 4), 240
        rest = np.nonzero(~a["keeper"] & (a["pid"] > 0))[0]
        a["pid"][rest] = 10_000 + np.arange(rest.size)
        a["pt"][rest] = 0.5
        kw = dict(need_att=False, norm_att_fp64=True)
    elif name == "one_particle":
        # one particle of interest among noise: K = 1, no point of another particle, norm_rep = 1e-9
        a, k = _draw(seed, 300, 1, 4, n_noise=288, spread=1.0), 1
        kw = dict(min_rep=0)
    elif name == "huge_ids":
        # ids at and above 2^40 next to small ones (the selection sorts 64-bit keys)
        a, k = _draw(seed, 300, 40, 4), 40
        ids = np.unique(a["pid"][a["pid"] > 0])
        big = np.r_[1 << 40, (1 << 40) + 1, (1 << 62) + 5, (1 << 63) - 1, (1 << 40) + g.choice(1 << 30, size=16, replace=False) + 2]
        for old, new in zip(g.permutation(ids)[:big.size], big):
            a["pid"][a["pid"] == old] = new
    elif name == "negative_ids":
        # (Tiger) negative ids are noise through !(pid > 0) and never of interest
        a, k = _draw(seed, 300, 40, 4), 40
        noise = np.nonzero(a["pid"] == 0)[0]
        a["pid"][noise[:12]] = np.r_[-1, -1, -7, -(1 << 40), -(1 << 62), -3, -3, -3, -2, -9, -(1 << 40), -5]
    elif name == "beta_ties":
        # equal largest betas inside a particle: the lowest hit index is the condensation point
        a, k = _draw(seed, 300, 40, 4), 40
        m, tied = _mask(a), 0
        for p in np.unique(a["pid"][a["pid"] > 0]):
            hits = np.nonzero((a["pid"] == p) & m)[0]
            if hits.size >= 3:
                pick = g.choice(hits, size=2 + (tied % 2), replace=False)
                a["beta"][pick] = np.float32(0.955 + 0.001 * (tied % 7))
                tied += 1
        assert tied >= 10
        for mode in ("rg", "tiger"):
            pts = _points(a, mode)
            assert sum(int(((a["pid"] == a["pid"][c]) & (a["beta"] == a["beta"][c])).sum() > 1) for c in pts) >= 10
            assert all(c == np.nonzero((a["pid"] == a["pid"][c]) & (a["beta"] == a["beta"][c]))[0][0] for c in pts)
    elif name == "unmasked_particles":
        # particles none of whose hits passes the cuts (no condensation point: gid = -1 rows) and particles with one
        # passing hit among failing ones (RG: that hit is the point and nothing is attracted; Tiger: all hits are)
        a, k = _draw(seed, 300, 40, 4), 36
        ids = g.permutation(np.unique(a["pid"][a["pid"] > 0]))
        for p in ids[:4]:
            a["pt"][a["pid"] == p] = 0.5
        for p in ids[4:10]:
            a["eta"][(a["pid"] == p) & ~a["keeper"]] = 4.5
    elif name == "far_outlier":
        # a cluster at distance 1e4 that holds no condensation point: its box is culled for every point, its rows of
        # grad_x are exact zeros (ODD_CHECKS)
        a, k = _draw(seed, 280, 40, 4), 40
        far = {"pid": np.r_[np.zeros(15, np.int64), np.full(5, 7_000_000, np.int64)], "keeper": np.zeros(20, bool),
               "beta": g.uniform(0.05, 0.95, size=20).astype(np.float32), "pt": np.r_[np.full(15, 2.0), np.full(5, 0.5)].astype(np.float32),
               "eta": np.zeros(20, np.float32), "reco": np.ones(20, np.float32),
               "x": (np.r_[1e4, 0, 0, 0] + 0.15 * g.standard_normal((20, 4))).astype(np.float32)}
        a = {key: np.concatenate([a[key], far[key]]) for key in a}
    elif name == "long_own_run":
        # 200 hits of one particle within 1e-3 of its condensation point: a long own-particle run in the by-gid order
        a, k = _draw(seed, 100, 15, 4), 15
        c = np.nonzero(a["keeper"])[0][3]
        a["beta"][c] = np.float32(0.97)   # (the point of its particle for both losses)
        run = {"pid": np.full(200, a["pid"][c]), "keeper": np.zeros(200, bool), "beta": g.uniform(0.05, 0.9, size=200).astype(np.float32),
               "pt": np.where(np.arange(200) % 9 == 0, 0.5, 2.0).astype(np.float32), "eta": np.zeros(200, np.float32),
               "reco": np.ones(200, np.float32), "x": (a["x"][c] + 1e-3 * g.uniform(-0.5, 0.5, size=(200, 4))).astype(np.float32)}
        a = {key: np.concatenate([a[key], run[key]]) for key in a}
    elif name == "no_noise":
        # no hit with id 0: the noise term is 0/0 in the reference as well
        a, k = _draw(seed, 300, 40, 4, n_noise=0), 40
        assert not np.any(a["pid"] <= 0)
    else:
        raise KeyError(name)
    return _finish(a, k, **kw)


# ---------------------------------------------------------------------------------------------- oracle, runs, checks
@functools.lru_cache(maxsize=None)
def reference(ev: Event, mode: str, weights=(1.0, 2.0, 0.25, 0.5), chunk: int = 4096):
    """the fp64 oracle on the event's own fp32 values; ``weights``: attractive, repulsive, coward, noise.  Computed
    once per (event, loss, weights) and shared; condition 4 is asserted on what it reports."""
    od = O.condensation_loss_chunked(beta=ev.beta, x=ev.x, particle_id=ev.pid, mask=ev.mask, mode=mode, weights=weights,
                                     chunk=chunk, norm_att_fp64=ev.norm_att_fp64)
    assert od["K"] == ev.k, f"K is {od['K']}, the case wants {ev.k}"
    assert od["n_rep"] >= ev.min_rep, f"{od['n_rep']} repulsive pairs, the case wants {ev.min_rep}"
    assert (od["attractive"] != 0) == ev.need_att, f"attractive term {od['attractive']}"
    return od


def _one_hot(term):
    return tuple(1.0 if t == term else 0.0 for t in TERMS)


@contextlib.contextmanager
def _settings(spatial):
    old = losses_oc.SPATIAL, CondensationLossRG.neighbor_cap
    losses_oc.SPATIAL, CondensationLossRG.neighbor_cap = spatial, "off"
    try:
        yield
    finally:
        losses_oc.SPATIAL, CondensationLossRG.neighbor_cap = old


def run(device, ev: Event, mode: str, spatial: str, term=None, weights=None, dtype=torch.float32, x=None):
    """forward and backward (of the weighted total, or of ``loss_dct[term]`` alone) on ``device``"""
    b = ev.beta.to(device=device, dtype=dtype, copy=True).requires_grad_(True)   # (fresh leaves: the event stays as it is)
    x = ev.x.to(device=device, dtype=dtype, copy=True).requires_grad_(True) if x is None else x
    with _settings(spatial):
        ret = LOSSES[mode](**(WEIGHTS if weights is None else weights))(
            beta=b, x=x, particle_id=ev.pid.to(device), reconstructable=ev.reco.to(device), pt=ev.pt.to(device), eta=ev.eta.to(device))
        (ret.loss if term is None else ret.loss_dct[term]).backward()
    res = {t: float(ret.loss_dct[t].detach()) for t in TERMS}
    res.update(total=float(ret.loss.detach()), grad_x=x.grad.detach().cpu(), grad_beta=b.grad.detach().cpu(),
               n_rep=int(ret.extra_metrics["n_rep"]) if mode == "tiger" else None)
    return res


def _check_term(got, want, what):
    if want == 0:
        assert got == 0, f"{what}: {got!r}, the oracle has exactly 0"
        return
    rel = abs(got - want) / abs(want)
    print(f"{what}: rel {rel:.2e}")
    assert rel <= TOL_TERM, f"{what}: {got!r} vs {want!r}, rel err {rel:.2e} > {TOL_TERM:.0e}"


def _check_grad(got, want, what):
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    scale = float(want.abs().max())
    if scale == 0:
        assert bool((got == 0).all()), f"{what}: the oracle's gradient is exactly 0, largest entry here {float(got.abs().max()):.3e}"
        return
    err = float((got.double() - want).abs().max()) / scale
    print(f"{what}: {err:.2e} of the largest entry")
    if err > TOL_GRAD:
        row = int((got.double() - want).abs().reshape(got.shape[0], -1).max(1).values.argmax())
        raise AssertionError(f"{what}: {err:.2e} of the largest entry > {TOL_GRAD:.0e} (row {row}: {got[row].tolist()} vs {want[row].tolist()})")


def check(res, od, mode, what, terms=TERMS, total=True):
    for t in terms:
        _check_term(res[t], od[t], f"{what} {t}")
    if total:
        _check_term(res["total"], od["total"], f"{what} total")
    _check_grad(res["grad_x"], od["grad_x"], f"{what} grad_x")
    _check_grad(res["grad_beta"], od["grad_beta"], f"{what} grad_beta")
    if mode == "tiger":
        assert res["n_rep"] == od["n_rep"], f"{what}: n_rep {res['n_rep']}, the oracle counts {od['n_rep']}"


def _same_bits(ra, rb, what):
    for key in TERMS + ("total",):
        assert np.float32(ra[key]).tobytes() == np.float32(rb[key]).tobytes(), f"{what}: {key} {ra[key]!r} vs {rb[key]!r}"
    for key in ("grad_x", "grad_beta"):
        assert ra[key].dtype == rb[key].dtype and torch.equal(ra[key].view(torch.int32), rb[key].view(torch.int32)), f"{what}: {key}"


def _both_losses(device, ev, spatial, what):
    out = {}
    for mode in LOSSES:
        out[mode] = run(device, ev, mode, spatial)
        check(out[mode], reference(ev, mode), mode, f"{what} {mode} spatial={spatial}")
    return out


# ---------------------------------------------------------------------------------------------- cases
def case_width(device, dim, spatial):
    """A / B: 700 hits, K = 140 at one width on one path (DENSE_WIDTHS, SPATIAL_WIDTHS)"""
    _both_losses(device, make_event(700, 140, dim), spatial, f"width {dim}")


def case_width_fallback(device, dim):
    """B: above width 16 ``gnntrk_oc_spatial_workspace_bytes`` answers 0 and SPATIAL = "on" runs the dense kernels: the
    fp64 bars, and the SPATIAL = "off" run bit for bit"""
    ev = make_event(700, 140, dim)
    on, off = _both_losses(device, ev, "on", f"width {dim}"), _both_losses(device, ev, "off", f"width {dim}")
    for mode in LOSSES:
        _same_bits(on[mode], off[mode], f"width {dim} {mode}: spatial on (fall-back) vs off")


def case_width_refused(device, spatial, dim=33):
    """B: width 33 is refused with the library's error on both paths"""
    g = np.random.default_rng(33)
    ev = make_event(700, 140, 32)
    x = torch.from_numpy(g.standard_normal((ev.n, dim)).astype(np.float32)).to(device).requires_grad_(True)
    for mode in LOSSES:
        try:
            run(device, ev, mode, spatial, x=x)
        except ValueError as e:
            assert "oc_potential: bad sizes" in str(e), str(e)
        else:
            raise AssertionError(f"width {dim} {mode} spatial={spatial}: the call was not refused")


def case_k_edge(device, k, dim, spatial):
    """C: K at the tile edges (K_EDGES) at widths 3 and 8"""
    _both_losses(device, k_edge_event(k, dim), spatial, f"K {k} width {dim}")


def case_n_edge(device, n, spatial):
    """D: N at the tile edges (N_EDGES), width 3, K = 20"""
    _both_losses(device, n_edge_event(n), spatial, f"N {n}")


def case_second_cp_batch(device, mode):
    """E (device only): K = 16 520 > kOcCpBatch = 16 384 on the dense path - the ``kb > 0`` launches of
    ``gnntrk_oc_backward``; the oracle walks 2.9e8 pairs on the host in blocks of 256 hits"""
    ev = batch2_event()
    check(run(device, ev, mode, "off"), reference(ev, mode, chunk=256), mode, f"K {ev.k} {mode}")


def case_term_gradient(device, shape, spatial, mode, term):
    """F: ``loss_dct[term].backward()`` on a fresh forward - the other three upstream gradients are None - against the
    oracle with the one-hot weights; the coward and the noise term have no gradient w.r.t. x: exact zeros"""
    n, dim, k = shape
    ev = make_event(n, k, dim)
    res = run(device, ev, mode, spatial, term=term)
    od = reference(ev, mode, _one_hot(term))
    what = f"{n} hits width {dim} {mode} spatial={spatial} d {term}"
    _check_term(res[term], od[term], what)
    if term in ("coward", "noise"):
        assert float(od["grad_x"].abs().max()) == 0
    _check_grad(res["grad_x"], od["grad_x"], what + " grad_x")
    _check_grad(res["grad_beta"], od["grad_beta"], what + " grad_beta")


def case_odd_event(device, name, spatial):
    """G: the odd events (``odd_event``)"""
    ev = odd_event(name)
    modes = ("tiger",) if name == "negative_ids" else tuple(LOSSES)
    for mode in modes:
        what = f"{name} {mode} spatial={spatial}"
        if name == "no_noise":
            # both sides: mean of nothing.  The total (NaN * 0 on both sides) is not compared; its gradient is.
            w = dict(WEIGHTS, lw_noise=0.0)
            res, od = run(device, ev, mode, spatial, weights=w), reference(ev, mode, (1.0, 2.0, 0.25, 0.0))
            assert np.isnan(res["noise"]) and np.isnan(od["noise"]), f"{what}: noise term {res['noise']!r}, oracle {od['noise']!r}"
            check(res, od, mode, what, terms=("attractive", "repulsive", "coward"), total=False)
            want = od["attractive"] + 2.0 * od["repulsive"] + 0.25 * od["coward"]
            got = np.float32(res["attractive"]) + np.float32(2.0) * np.float32(res["repulsive"]) + np.float32(0.25) * np.float32(res["coward"])
            _check_term(float(got), want, what + " total without the noise term")
            continue
        res, od = run(device, ev, mode, spatial), reference(ev, mode)
        check(res, od, mode, what)
        if name in ("singletons",):
            assert od["attractive"] == 0 and res["attractive"] == 0
        if name == "one_particle":
            assert od["K"] == 1 and od["n_rep"] > 0   # (noise hits inside the radius are repelled: norm_rep is the bare 1e-9)
        if name == "far_outlier":
            far = ev.x[:, 0] > 5e3
            assert int(far.sum()) == 20 and bool((od["grad_x"][far] == 0).all())
            assert bool((res["grad_x"][far] == 0).all()), f"{what}: the outlier cluster has a gradient w.r.t. x"
        if name == "unmasked_particles":
            interest = torch.isin(ev.pid, torch.unique(ev.pid[ev.mask]))
            assert int(((ev.pid > 0) & ~interest).sum()) >= 4, "no hit of a particle without a passing hit"


def case_fp64_inputs(device, spatial):
    """H: fp64 ``beta`` and ``x`` (fp32 values): the gradients come back as fp64 and meet the bars"""
    ev = make_event(300, 60, 3)
    for mode in LOSSES:
        res = run(device, ev, mode, spatial, dtype=torch.float64)
        assert res["grad_x"].dtype == torch.float64 and res["grad_beta"].dtype == torch.float64
        check(res, reference(ev, mode), mode, f"fp64 inputs {mode} spatial={spatial}")


def case_transposed_x(device, spatial):
    """H: ``x`` as the transpose of a [width, hits] buffer gives the losses and gradients of its contiguous clone, bit
    for bit (and the fp64 bars)"""
    ev = make_event(300, 60, 3)
    for mode in LOSSES:
        buf = ev.x.t().contiguous().to(device, copy=True)
        xt = buf.t().detach().requires_grad_(True)
        assert not xt.is_contiguous() and xt.stride() == (1, ev.n)
        strided = run(device, ev, mode, spatial, x=xt)
        plain = run(device, ev, mode, spatial, x=xt.detach().clone().contiguous().requires_grad_(True))
        check(strided, reference(ev, mode), mode, f"transposed x {mode} spatial={spatial}")
        _same_bits(strided, plain, f"transposed x {mode} spatial={spatial}")
