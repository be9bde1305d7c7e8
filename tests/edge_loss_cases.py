"""Edge-loss and hinge-loss cases shared by the emulator tests (tests/test_edge_loss_emul.py) and the GPU tests
(tests/test_edge_loss_gpu.py): the loss kernels of csrc/segment.hip (two-pass BCE, ``bce_csr``, focal,
``edge_targets_csr``) and of csrc/hinge.hip where a wrong kernel passed the suite before - scores at the ends of
their range (the clamps of BCE, the unclamped focal loss), labels and pt values on the edges of ``bce_target``,
grids at their caps, the register widths, list lengths and strides of the hinge backward.

The reference is always the operation restated in torch float64 on the CPU, on the very fp32 values handed to the
kernel, with autograd for the gradients.  Losses are compared at the project's scalar bars (1e-6 for BCE, TOL_OUT
for focal and hinge).  Gradients are compared ELEMENT BY ELEMENT (``assert_grad_elementwise``): one saturated edge
has a gradient of 1e12 / n, and a bar scaled by the largest element of the tensor (``assert_close``) would accept
anything for all the others.  Every case asserts that its data is in the regime it claims to test."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from gnn_tracking_amd import _capi, ops, ops_ml
from layout_cases import Carved, _bits, _bce_csr_raw
from parity_cases import TOL_GRAD, TOL_OUT, assert_close, tt

F = torch.nn.functional
UP = 1.5   # the upstream value of every backward

_F32 = np.float32
_ULP_BELOW_ONE = float(np.nextafter(_F32(1), _F32(0)))   # 1 - 2^-24

#: the ends of the score range: what a sigmoid head in fp32 returns for logits beyond about -87 / +17, and the
#: neighbours of every clamp (log(w) < -100 only as log(0) = -inf; (1 - w) w < 1e-12 at 2^-60 and below)
VALUES = (0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -60, 1e-12, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -12, _ULP_BELOW_ONE, 1.0)
#: the list for the focal loss against fp64: without the exact 0 and 1 (their reference is not finite; case_focal_exact
#: takes them) and without 2^-149: at label 1 its reference gradient is alpha pw 2^149 / n - finite in fp64, above the
#: largest fp32 value, so no fp32 result can meet it and the reference, stored as the kernel stores it, is not finite
VALUES_FOCAL = VALUES[2:-1]

GAMMAS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
ALPHAS = (0.0, 0.3, 1.0)
POS_WEIGHTS = (1.0, 2.5)
THLD = 0.9


def assert_grad_elementwise(got, ref, n_selected, what, *, upstream=UP, tol=TOL_GRAD, where=None):
    """``|got_i - ref_i| <= tol * max(|ref_i|, floor)`` for every element, ``floor = |upstream| / n_selected``: the size
    of the gradient of one edge whose term has a derivative of one (derived, not measured).  ``where``: the elements
    compared (the caller says why the others are not)."""
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if where is not None:
        got, ref = got[where], ref[where]
    assert bool(torch.isfinite(ref).all()), f"{what}: the reference is not finite"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite gradient"
    bar = tol * torch.clamp(ref.abs(), min=abs(upstream) / max(int(n_selected), 1))
    bad = (got - ref).abs() > bar
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        g, r = got.reshape(-1)[i].item(), ref.reshape(-1)[i].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off, first at {i}: {g!r} vs {r!r} "
                             f"(|diff| {abs(g - r):.3e} > {bar.reshape(-1)[i].item():.3e})")


def _lib():
    return _capi.load()


def cu_count():
    return int(_lib().gnntrk_device_cu_count())


# ------------------------------------------------------------------------------------------ inputs
def saturated_scores(n, values, seed, head=None):
    """``(w, y)`` fp32 on the CPU: ``values`` crossed with both labels, tiled over the first ``head`` and the last
    ``2 * len(values) + 3`` entries (the tail of a length that is no multiple of four is saturated as well), seeded
    uniform values in (0.001, 0.999) and labels in between."""
    g = np.random.default_rng(seed)
    w = g.uniform(0.001, 0.999, size=n).astype(_F32)
    y = (g.random(n) < 0.4).astype(_F32)
    k = len(values)
    head = min(n, 10 * k if head is None else head)
    tail = min(n - head, 2 * k + 3)
    for lo, cnt in ((0, head), (n - tail, tail)):
        i = np.arange(cnt)
        w[lo:lo + cnt] = np.asarray(values, dtype=np.float64).astype(_F32)[i % k]
        y[lo:lo + cnt] = ((i // k) % 2).astype(_F32)
    return torch.from_numpy(w), torch.from_numpy(y)


def pt_inputs(n, n_nodes, seed):
    """source node per edge (int64) and a pt per node on both sides of ``THLD``"""
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.integers(0, n_nodes, size=n)), torch.from_numpy(g.lognormal(size=n_nodes).astype(_F32))


def falsified(y, src, pt, thld):
    """``bce_target``: the label as given without a threshold, else ``y != 0 && pt[src] > thld`` with the threshold
    as the fp32 value the kernel receives (NaN > thld is false)"""
    if not thld > 0:
        return y.double()
    return ((y != 0) & (pt[src] > float(_F32(thld)))).double()


def _assert_clamps_reached(w, t, what):
    """for each label at least one element takes each clamp of BCE"""
    w32 = w.numpy()
    prod = (_F32(1) - w32) * w32
    for lab in (0.0, 1.0):
        m = (t == lab).numpy()
        assert (m & (w32 == 0)).any(), f"{what}: no w = 0 (log(w) = -inf, clamped to -100) with label {lab}"
        assert (m & (w32 == 1)).any(), f"{what}: no w = 1 (log1p(-w) = -inf, clamped to -100) with label {lab}"
        assert (m & (prod < _F32(1e-12)) & (w32 > 0) & (w32 < 1)).any(), f"{what}: no 0 < (1 - w) w < 1e-12 with label {lab}"


# ------------------------------------------------------------------------------------------ references
def ref_bce(w, t):
    """torch's BCE in fp64 (the same -100 and 1e-12 clamps) -> (loss, gradient for the upstream value UP)"""
    wr = w.double().requires_grad_(True)
    loss = F.binary_cross_entropy(wr, t.to(wr.dtype))
    (loss * UP).backward()
    return loss.detach(), wr.grad


def focal_formula(w, target, pos_weight, alpha, gamma):
    """the reference's binary focal loss (metrics/losses/ec.py), written out: no clamp"""
    probs_pos, probs_neg = w, 1 - w
    pos_term = -alpha * pos_weight * probs_neg.pow(gamma) * target * probs_pos.log()
    neg_term = -(1.0 - alpha) * probs_pos.pow(gamma) * (1.0 - target) * probs_neg.log()
    return torch.mean(pos_term + neg_term)


def ref_focal(w, y, yf, alpha, gamma, pos_weight, haughty, dtype=torch.float64):
    """EdgeWeightFocalLoss (target = falsified label, scalar pos_weight) or HaughtyFocalLoss (target = the label as
    given, pos_weight = the falsified label) in ``dtype`` -> (loss, gradient for UP)"""
    wr = w.detach().clone().to(dtype).requires_grad_(True)
    target, pw = (y.to(dtype), yf.to(dtype)) if haughty else (yf.to(dtype), torch.tensor([pos_weight], dtype=dtype))
    loss = focal_formula(wr, target, pw, alpha, gamma)
    (loss * UP).backward()
    return loss.detach(), wr.grad


# ------------------------------------------------------------------------------------------ runners
def run_bce(device, w, y, src, pt, thld):
    wd = w.detach().clone().to(device).requires_grad_(True)
    on = thld > 0
    loss = ops._BCE.apply(wd, y.to(device), src.to(device) if on else None, pt.to(device) if on else None, float(thld))
    (loss * UP).backward()
    return loss.detach(), wd.grad


def run_bce_csr(device, w, lab8, src, pt, thld, need_grad=True):
    wd = w.detach().clone().to(device).requires_grad_(need_grad)
    on = thld > 0
    loss = ops._BCECsr.apply(wd, lab8.to(device), src.to(device).to(torch.int32) if on else None,
                             pt.to(device) if on else None, float(thld))
    if need_grad:
        (loss * UP).backward()
    return loss.detach(), wd.grad


def run_focal(device, w, y, src, pt, thld, alpha, gamma, pos_weight, haughty):
    wd = w.detach().clone().to(device).requires_grad_(True)
    on = thld > 0
    loss = ops._Focal.apply(wd, y.to(device), src.to(device) if on else None, pt.to(device) if on else None, float(thld),
                            float(alpha), float(gamma), float(pos_weight), bool(haughty))
    (loss * UP).backward()
    return loss.detach(), wd.grad


def _check_bce(device, w, y, src, pt, thld, tag, csr_without_grad=True):
    """two-pass BCE and bce_csr (uint8 labels) on the same values, each against fp64 only (the two promise no common
    bits: bce_csr sums four consecutive edges per thread, the two-pass kernel one)"""
    n = w.numel()
    t = falsified(y, src, pt, thld)
    lr, gr = ref_bce(w, t)
    assert bool(torch.isfinite(lr)) and bool(torch.isfinite(gr).all()), f"{tag}: the clamps make the reference finite"
    l, g = run_bce(device, w, y, src, pt, thld)
    assert bool(torch.isfinite(l)) and bool(torch.isfinite(g).all()), f"{tag}: two-pass BCE is not finite"
    assert_close(l, lr, 1e-6, f"{tag} two-pass loss")
    assert_grad_elementwise(g, gr, n, f"{tag} two-pass gradient")
    lab8 = (y != 0).to(torch.uint8) * 255   # (any non-zero byte is "true")
    for need_grad in ((False, True) if csr_without_grad else (True,)):
        l, g = run_bce_csr(device, w, lab8, src, pt, thld, need_grad)
        assert bool(torch.isfinite(l)), f"{tag}: bce_csr loss is not finite"
        assert_close(l, lr, 1e-6, f"{tag} bce_csr loss (gradient {need_grad})")
        if need_grad:
            assert bool(torch.isfinite(g).all()), f"{tag}: bce_csr gradient is not finite"
            assert_grad_elementwise(g, gr, n, f"{tag} bce_csr gradient")


def _check_focal(device, w, y, src, pt, thld, alpha, gamma, pos_weight, haughty, tag):
    n = w.numel()
    yf = falsified(y, src, pt, thld)
    lr, gr = ref_focal(w, y, yf, alpha, gamma, pos_weight, haughty)
    assert bool(torch.isfinite(lr)) and bool(torch.isfinite(gr.float()).all()), f"{tag}: the fp64 reference is not finite in fp32"
    l, g = run_focal(device, w, y, src, pt, thld, alpha, gamma, pos_weight, haughty)
    assert_close(l, lr, TOL_OUT, f"{tag} loss")
    assert_grad_elementwise(g, gr, n, f"{tag} gradient")


# ------------------------------------------------------------------------------------------ A. saturated scores
N_SAT = 4099   # the float4 body, the item tail (4099 = 4 * 1024 + 3) and 17 workgroups


def case_bce_saturated(device, thld):
    """``ops._BCE`` and ``ops._BCECsr`` (gradient requested and not) on scores at the ends of their range, both labels:
    the clamps ``fmaxf(logf(w), -100)``, ``fmaxf(log1pf(-w), -100)`` and ``fmaxf((1 - w) w, 1e-12)`` of
    bce_partial_kernel / bce_bwd_kernel / bce_csr_one.  Loss at 1e-6, gradient element-wise, everything finite."""
    w, y = saturated_scores(N_SAT, VALUES, seed=11)
    src, pt = pt_inputs(N_SAT, 41, seed=12)
    _assert_clamps_reached(w, falsified(y, src, pt, thld), f"saturated BCE thld={thld}")
    _check_bce(device, w, y, src, pt, thld, f"saturated BCE thld={thld}")


def case_focal_saturated(device, gamma):
    """``ops._Focal`` on VALUES_FOCAL crossed with both labels, for every alpha, pos_weight, ``haughty`` setting and
    the pt threshold off and on: loss at TOL_OUT, gradient element-wise against fp64.  ``gamma`` 1 is the branch of
    focal_pow / focal_dpow no other test runs; ``gamma`` 0.5 and 1.5 take ``powf(x, gamma - 1)`` at both ends."""
    w, y = saturated_scores(N_SAT, VALUES_FOCAL, seed=13)
    src, pt = pt_inputs(N_SAT, 41, seed=14)
    w32 = w.numpy()
    assert w32.min() == _F32(2.0 ** -126) and w32.max() == _F32(_ULP_BELOW_ONE)
    for thld in (0.0, THLD):
        yf = falsified(y, src, pt, thld)
        for v in VALUES_FOCAL:   # every value under both (falsified) labels, and under both raw labels
            for lab in (0.0, 1.0):
                assert bool(((w == float(_F32(v))) & (yf == lab)).any()) and bool(((w == float(_F32(v))) & (y == lab)).any()), (v, lab, thld)
        for alpha in ALPHAS:
            for haughty in (False, True):
                for pw in (POS_WEIGHTS if not haughty else POS_WEIGHTS[:1]):   # (haughty: the kernel ignores pos_weight)
                    _check_focal(device, w, y, src, pt, thld, alpha, gamma, pw, haughty,
                                 f"saturated focal gamma={gamma} alpha={alpha} pw={pw} haughty={haughty} thld={thld}")


def case_focal_exact(device, gamma):
    """The focal kernels at exact 0 and 1 (all of VALUES, n = 64): no clamp, "as the reference" - so against the
    reference formula in torch fp32 on the CPU, the reference's own arithmetic.  The loss is non-finite in both or in
    neither; the isfinite masks of the gradients are equal element by element; where both are finite the
    element-wise bar holds.

    The case found one disagreement, since fixed in focal_bwd_kernel: at ``w = 2^-149`` with a zero coefficient of the
    positive term (label 0, or alpha 0) the kernel formed ``(1 - w)^gamma / w`` first - ``1 / w`` overflows fp32 - and
    returned ``0 * inf = NaN``, where autograd divides the zero gradient by ``w`` and returns the finite derivative."""
    n = 64
    w, y = saturated_scores(n, VALUES, seed=15, head=n)
    # (seven nodes against the period of ten of the values: every value meets a pt on either side of the threshold)
    src, pt = torch.arange(n) % 7, torch.tensor([0.1, 5.0, 0.2, 5.0, 0.3, 5.0, 0.4])
    assert bool((w == 0).any()) and bool((w == 1).any())
    for thld in (0.0, THLD):
        yf = falsified(y, src, pt, thld)
        for lab in (0.0, 1.0):
            assert bool(((w == 0) & (yf == lab)).any()) and bool(((w == 1) & (yf == lab)).any()), (lab, thld)
        for alpha in ALPHAS:
            for haughty in (False, True):
                tag = f"focal at 0 and 1: gamma={gamma} alpha={alpha} haughty={haughty} thld={thld}"
                lr, gr = ref_focal(w, y, yf, alpha, gamma, 2.5, haughty, dtype=torch.float32)
                l, g = run_focal(device, w, y, src, pt, thld, alpha, gamma, 2.5, haughty)
                l, g = l.cpu(), g.cpu()
                assert bool(torch.isfinite(l)) == bool(torch.isfinite(lr)), f"{tag}: loss {l.item()!r}, torch fp32 {lr.item()!r}"
                fin, fin_r = torch.isfinite(g), torch.isfinite(gr)
                if not torch.equal(fin, fin_r):
                    i = int(torch.nonzero(fin != fin_r)[0])
                    raise AssertionError(f"{tag}: gradient at w={w[i].item()!r} y={y[i].item()} yf={yf[i].item()}: "
                                         f"{g[i].item()!r}, torch fp32 {gr[i].item()!r}")
                if bool(torch.isfinite(lr)):
                    assert_close(l, lr, TOL_OUT, tag + " loss")
                assert_grad_elementwise(g, gr, n, tag + " gradient", where=fin)


# ------------------------------------------------------------------------------------------ B. labels and pt
N_LAB = 257
_NON_BINARY = (0.0, 1.0, 0.25, 2.0, -1.0)


def _pt_edges(n, seed):
    """pt per node: exactly the threshold (false: strict ``>``), one ulp above (true), NaN (false), below, above, inf;
    every pt class meets a non-zero and a zero label"""
    thr = _F32(THLD)
    pt = np.array([thr, np.nextafter(thr, _F32(2)), np.nan, np.nextafter(thr, _F32(0)), 5.0, np.inf, 0.0], dtype=_F32)
    g = np.random.default_rng(seed)
    src = np.arange(n) % len(pt)
    w = g.uniform(0.02, 0.98, size=n).astype(_F32)
    return torch.from_numpy(w), torch.from_numpy(src), torch.from_numpy(pt)


def case_pt_threshold_edges(device):
    """``bce_target``: ``pt[src]`` exactly at the threshold and NaN count as false, one ulp above as true - in the
    two-pass BCE, bce_csr and both focal classes."""
    n = N_LAB
    w, src, pt = _pt_edges(n, seed=21)
    y = torch.from_numpy((np.arange(n) // len(pt) % 2).astype(_F32))
    t = falsified(y, src, pt, THLD)
    thr = _F32(THLD)
    for node, want in ((0, 0.0), (1, 1.0), (2, 0.0), (3, 0.0), (4, 1.0), (5, 1.0), (6, 0.0)):
        m = (src == node) & (y != 0)
        assert bool(m.any()) and bool((t[m] == want).all()) and bool(((src == node) & (y == 0)).any()), node
    assert pt[0].item() == float(thr) and pt[1].item() > float(thr) and pt[1].item() - float(thr) < 1e-7 and bool(torch.isnan(pt[2]))
    _check_bce(device, w, y, src, pt, THLD, "pt at the threshold, BCE")
    for haughty in (False, True):
        _check_focal(device, w, y, src, pt, THLD, 0.3, 1.5, 2.5, haughty, f"pt at the threshold, focal haughty={haughty}")


def case_non_binary_labels(device):
    """``pt_thld > 0`` binarises labels from {0, 1, 0.25, 2, -1} by ``!= 0`` (two-pass BCE, focal; haughty focal takes
    the raw label as target and the binarised one as weight); bce_csr takes any non-zero byte as true."""
    n = N_LAB
    g = np.random.default_rng(22)
    w = torch.from_numpy(g.uniform(0.02, 0.98, size=n).astype(_F32))
    src, pt = pt_inputs(n, 19, seed=23)
    y = torch.tensor(_NON_BINARY, dtype=torch.float32)[torch.arange(n) % len(_NON_BINARY)]
    t = falsified(y, src, pt, THLD)
    for v in _NON_BINARY[1:]:
        assert bool(((y == v) & (t == 1)).any()) and bool(((y == v) & (t == 0)).any()), v
    assert bool((t[y == 0] == 0).all())
    lr, gr = ref_bce(w, t)
    l, gw = run_bce(device, w, y, src, pt, THLD)
    assert_close(l, lr, 1e-6, "non-binary labels, two-pass BCE loss")
    assert_grad_elementwise(gw, gr, n, "non-binary labels, two-pass BCE gradient")
    lab8 = torch.tensor((0, 1, 2, 255, 128), dtype=torch.uint8)[torch.arange(n) % 5]
    for thld in (0.0, THLD):
        t8 = falsified(lab8, src, pt, thld) if thld > 0 else (lab8 != 0).double()
        lr, gr = ref_bce(w, t8)
        l, gw = run_bce_csr(device, w, lab8, src, pt, thld)
        assert_close(l, lr, 1e-6, f"non-binary bytes, bce_csr loss thld={thld}")
        assert_grad_elementwise(gw, gr, n, f"non-binary bytes, bce_csr gradient thld={thld}")
    for haughty in (False, True):
        _check_focal(device, w, y, src, pt, THLD, 0.3, 1.5, 2.5, haughty, f"non-binary labels, focal haughty={haughty}")


def case_soft_labels(device):
    """``pt_thld == 0`` with soft labels in (0, 1): BCE takes ``y`` as given (torch's BCE with the soft target), focal
    takes it as target, haughty focal as target and as weight."""
    n = N_LAB
    g = np.random.default_rng(24)
    w = torch.from_numpy(g.uniform(0.02, 0.98, size=n).astype(_F32))
    y = torch.from_numpy(g.uniform(0.05, 0.95, size=n).astype(_F32))
    src, pt = pt_inputs(n, 19, seed=25)
    assert bool(((y > 0) & (y < 1)).all())
    lr, gr = ref_bce(w, y.double())
    l, gw = run_bce(device, w, y, src, pt, 0.0)
    assert_close(l, lr, 1e-6, "soft labels, two-pass BCE loss")
    assert_grad_elementwise(gw, gr, n, "soft labels, two-pass BCE gradient")
    for haughty in (False, True):
        for gamma in (1.0, 1.5):
            _check_focal(device, w, y, src, pt, 0.0, 0.3, gamma, 2.5, haughty, f"soft labels, focal gamma={gamma} haughty={haughty}")


def case_edge_targets_csr(device, n_nodes=37):
    """``ops.edge_targets_csr``: float labels from {0, 1, 0.25, 2, -1} and uint8 labels holding other bytes than 0
    and 1, gathered through the graph index's permutation - exactly ``y[perm]`` without the threshold, the falsified
    0 / 1 with it (pt at the threshold, one ulp above, NaN)."""
    n = N_LAB
    g = np.random.default_rng(26)
    ei = tt(g.integers(0, n_nodes, size=(2, n)), device).long()
    pt = torch.from_numpy(g.lognormal(size=n_nodes).astype(_F32))
    thr = _F32(THLD)
    pt[:3] = torch.tensor([thr, np.nextafter(thr, _F32(2)), np.nan], dtype=torch.float32)
    gi = ops.graph_index(ei, n_nodes, cache=False)
    perm = gi.perm.cpu().long()
    assert not torch.equal(perm, torch.arange(n)), "the permutation is the identity"
    src = ei[0].cpu()[perm]
    assert torch.equal(gi.src.cpu().long(), src)
    assert all(bool((src == k).any()) for k in range(3))
    labels = (("float", torch.tensor(_NON_BINARY, dtype=torch.float32)[torch.arange(n) % 5]),
              ("uint8", torch.tensor((0, 1, 2, 255, 128), dtype=torch.uint8)[torch.arange(n) % 5]))
    for kind, y in labels:
        yd = y.to(device)
        got = ops.edge_targets_csr(yd, gi, None, 0.0).cpu()
        assert got.dtype == torch.float32 and torch.equal(got, y.float()[perm]), f"edge_targets_csr {kind}: not y[perm]"
        got = ops.edge_targets_csr(yd, gi, pt.to(device), THLD).cpu()
        want = ((y[perm] != 0) & (pt[src] > float(thr))).float()
        assert 0 < int(want.sum()) < int((y != 0).sum())
        assert torch.equal(got, want), f"edge_targets_csr {kind}: falsified labels differ"


# ------------------------------------------------------------------------------------------ C. grids at their caps
def grid_sizes():
    """``{name: n}`` from the launchers' formulas and the device's CU count: ``bce_grid(n) = min(ceil(n / 256), 8 CUs,
    1024)`` for the partial kernels and bce_csr (four edges per thread), ``blocks_for(n, 8) = min(ceil(n / 256), 8 CUs)``
    for the two backward kernels."""
    cap = min(8 * cu_count(), 1024)
    return {"final-257-partials": 65_537, "partial-second-trip": 256 * cap + 1, "csr-second-trip": 4 * (256 * cap + 1) + 3,
            "backward-second-trip": 256 * 8 * cu_count() + 1}


def _trips(n, per_thread, grid):
    return -(-n // (256 * per_thread * grid))


def case_grid_caps(device, which):
    """The two-pass BCE, bce_csr and one focal setting (gamma 1.5, threshold on), forward and backward, at a size
    where a grid is at its cap and the grid-stride loop takes a second trip - or, at 65 537 edges, where
    bce_final_kernel adds more than 256 partials.  VALUES / VALUES_FOCAL lie in the last 64 positions, the ones the
    extra trip reads.  Loss at 1e-6 / TOL_OUT, gradient element-wise."""
    n = grid_sizes()[which]
    cus = cu_count()
    cap = min(8 * cus, 1024)
    g_part = min(-(-n // 256), cap)          # bce_grid
    g_bwd = min(-(-n // 256), 8 * cus)       # blocks_for(n, 8)
    if which == "final-257-partials":
        assert g_part == 257, f"{g_part} partials: the device has too few CUs for a final reduction over more than 256"
    elif which == "partial-second-trip":
        assert g_part == cap and _trips(n, 1, g_part) == 2 and _trips(n - 1, 1, g_part) == 1
    elif which == "csr-second-trip":
        assert g_part == cap and _trips(n, 4, g_part) == 2 and 0 < n - 4 * 256 * g_part <= 64   # (the second trip reads planted values only)
    else:
        assert g_bwd == 8 * cus and _trips(n, 1, g_bwd) == 2 and _trips(n - 1, 1, g_bwd) == 1
    src, pt = pt_inputs(n, 1009, seed=32)
    src[n - 64:], pt[0] = 0, 5.0   # (the planted labels pass the threshold as they are)
    for values, seed in ((VALUES, 31), (VALUES_FOCAL, 33)):
        w, y = saturated_scores(n, values, seed=seed, head=0)
        w[n - 64:], y[n - 64:] = saturated_scores(64, values, seed=seed, head=64)
        assert set(w[n - 64:].tolist()) == {float(_F32(v)) for v in values}
        assert 0.001 <= float(w[:n - 64].min()) and float(w[:n - 64].max()) <= 0.999
        tag = f"{which} n={n} CUs={cus}"
        if values is VALUES:
            _assert_clamps_reached(w[n - 64:], falsified(y, src, pt, THLD)[n - 64:], tag)
            _check_bce(device, w, y, src, pt, THLD, tag + " BCE", csr_without_grad=False)
        else:
            _check_focal(device, w, y, src, pt, THLD, 0.3, 1.5, 2.5, False, tag + " focal")


# ------------------------------------------------------------------------------------------ D. hinge
HINGE_DIMS = (1, 3, 4, 5, 8, 9, 16, 17, 31, 32)
HINGE_POWERS = (1.0, 2.0, 0.5, 3.0)
R_EMB = 0.9


def ref_hinge(x, edges, mask, pid, r_emb, p, rep):
    """the expressions of parity_cases.case_hinge_terms in fp64 -> (loss, selected count, gradient for UP)"""
    xr = x.double().requires_grad_(True)
    keep = torch.ones(edges.shape[1], dtype=torch.bool)
    if mask is not None:
        keep &= mask[edges[0]]
    if pid is not None:
        keep &= pid[edges[0]] != pid[edges[1]]
    e = edges[:, keep]
    d = torch.linalg.norm(xr[e[0]] - xr[e[1]], dim=-1)
    terms = torch.relu(float(_F32(r_emb)) - torch.pow(d, p)) if rep else torch.pow(d, p)
    loss = terms.sum() / (e.shape[1] + 1e-9)
    (loss * UP).backward()
    return loss.detach(), int(e.shape[1]), xr.grad


def run_hinge(device, x, edges, mask, pid, r_emb, p, rep):
    xd = x.detach().clone().to(device).requires_grad_(True)
    l, cnt, _ = ops_ml.hinge_terms(xd, edges.to(device), node_mask=None if mask is None else mask.to(device),
                                   particle_id=None if pid is None else pid.to(device), r_emb=r_emb, p=p, repulsive=rep)
    (l * UP).backward()
    return l.detach(), int(cnt), xd.grad


#: An edge whose d^p is within this distance of r_emb may lie on the other side of the hinge in fp32 (d is a sum of
#: up to 32 squares and a root: some 2e-6 relative at the most) - its whole gradient would differ, by rounding and
#: not by an error.  The inputs keep clear of it (asserted); case_hinge_on_the_hinge takes the hinge itself.
HINGE_MARGIN = 1e-5


def _near_the_hinge(x, edges, r_emb, p):
    d = torch.linalg.norm(x.double()[edges[0]] - x.double()[edges[1]], dim=-1)
    return (float(_F32(r_emb)) - torch.pow(d, p)).abs() < HINGE_MARGIN


def off_the_hinge(x, edges, r_emb, powers):
    """``edges`` with every edge near the hinge for one of ``powers`` turned into a self edge of its source"""
    near = torch.zeros(edges.shape[1], dtype=torch.bool)
    for p in powers:
        near |= _near_the_hinge(x, edges, r_emb, p)
    edges = edges.clone()
    edges[1, near] = edges[0, near]
    return edges


def _check_hinge(device, x, edges, mask, pid, r_emb, p, rep, tag):
    assert not rep or not bool(_near_the_hinge(x, edges, r_emb, p).any()), f"{tag}: an edge within {HINGE_MARGIN} of the hinge"
    lr, cr, gr = ref_hinge(x, edges, mask, pid, r_emb, p, rep)
    l, cnt, gx = run_hinge(device, x, edges, mask, pid, r_emb, p, rep)
    assert cnt == cr, f"{tag}: {cnt} edges selected, the reference selects {cr}"
    assert_close(l, lr, TOL_OUT, tag + " loss")
    # (p < 1: d^(p - 1) is unbounded at d = 0 - compared where the reference itself is finite, as case_hinge_terms)
    where = torch.isfinite(gr) if p < 1.0 else None
    assert where is None or bool(where.any())
    assert_grad_elementwise(gx, gr, cr, tag + " gradient", where=where)
    return cr


def case_hinge_widths(device, dim, n=120, n_edges=700):
    """``hinge_bwd_kernel<DP>`` at every register width and its edges (``dim`` 4 | 5, 8 | 9, 16 | 17, 1 and 32): all
    powers, attractive and repulsive, node-mask and particle-id selection on, duplicates and self edges."""
    gen = torch.Generator().manual_seed(40 + dim)
    x = torch.randn(n, dim, generator=gen) * (0.5 / dim ** 0.5)   # (distances around 0.7: both sides of r_emb)
    pid = torch.randint(0, 20, (n,), generator=gen)
    mask = torch.rand(n, generator=gen) > 0.3
    edges = torch.randint(0, n, (2, n_edges), generator=gen)
    edges[:, :5] = edges[:, 5:10]
    edges[1, 10:14] = edges[0, 10:14]
    edges = off_the_hinge(x, edges, R_EMB, HINGE_POWERS)
    for rep in (False, True):
        for p in HINGE_POWERS:
            for use_pid in ((True, False) if p == 1.0 else (True,)):   # (without the particle ids the self edges are selected)
                sel = _check_hinge(device, x, edges, mask, pid if use_pid else None, R_EMB, p, rep,
                                   f"hinge dim={dim} rep={rep} p={p} pid={use_pid}")
                assert sel > n_edges // 2


def case_hinge_dim_refused(device):
    """``dim = 33``, one past the widest kernel, is refused with GNNTRK_EINVAL (a ValueError) by both entries."""
    x = torch.zeros(10, 33).to(device).requires_grad_(True)
    edges = torch.zeros(2, 4, dtype=torch.long).to(device)
    try:
        ops_ml.hinge_terms(x, edges, r_emb=R_EMB)
    except ValueError as e:
        assert "dim" in str(e)
    else:
        raise AssertionError("hinge: dim = 33 was accepted")
    lib = _lib()
    a = _hinge_raw_args(x.detach(), None, None, R_EMB, 1.0, False)
    gi = ops.graph_index(edges, 10, cache=False)
    d = _capi.GraphIndex(gi.n_nodes, gi.n_edges, ops._p(gi.perm), ops._p(gi.tgt), ops._p(gi.src), ops._p(gi.rowptr_t),
                         ops._p(gi.rowptr_s), ops._p(gi.spos), ops._p(gi.spos_inv))
    one = torch.ones(1, device=x.device)
    gx = torch.zeros(10, 33, device=x.device)
    rc = lib.gnntrk_hinge_backward(C.byref(a), C.byref(d), ops._p(one), ops._p(one), ops._p(gx), 33, 0, ops._stream(gx))
    assert rc == 1, f"hinge_backward with dim = 33 returned {rc}, not GNNTRK_EINVAL"


DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 300)


def degree_graph(n_nodes=345):
    """An edge list in which node k has in-degree AND out-degree ``DEGREES[k]``: its partners are the nodes from
    ``len(DEGREES)`` on, so no chosen node gains an edge from another one; the hub of 300 is source and target."""
    first, fill = len(DEGREES), n_nodes - len(DEGREES)
    assert fill >= max(DEGREES)
    rows = []
    for k, deg in enumerate(DEGREES):
        for j in range(deg):
            rows.append((first + (17 * k + j) % fill, k))         # into k
            rows.append((k, first + (29 * k + 5 + j) % fill))     # out of k
    e = torch.tensor(rows, dtype=torch.long).t().contiguous()
    return e[:, torch.randperm(e.shape[1], generator=torch.Generator().manual_seed(50))].contiguous()


def case_hinge_degrees(device):
    """The eight-lanes-per-node backward on lists of 0, 1, 7, 8, 9, 15, 16, 17 and 300 edges (in and out), with idle
    lanes in the last workgroup, and on a single node."""
    n = 345
    assert n * 8 % 256 != 0
    edges = degree_graph(n)
    gi = ops.graph_index(edges.to(device), n, cache=False)
    deg_in = (gi.rowptr_t[1:] - gi.rowptr_t[:-1]).cpu().tolist()
    deg_out = (gi.rowptr_s[1:] - gi.rowptr_s[:-1]).cpu().tolist()
    assert tuple(deg_in[:len(DEGREES)]) == DEGREES and tuple(deg_out[:len(DEGREES)]) == DEGREES
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(n, 6, generator=gen) * 0.25
    pid = torch.randint(0, 50, (n,), generator=gen)
    mask = torch.rand(n, generator=gen) > 0.1
    mask[:len(DEGREES)] = True
    for rep, p in ((False, 1.0), (False, 2.0), (True, 1.0), (True, 3.0)):
        _check_hinge(device, x, edges, mask, pid, R_EMB, p, rep, f"hinge degrees rep={rep} p={p}")
        _check_hinge(device, x, edges, None, None, R_EMB, p, rep, f"hinge degrees, no selection, rep={rep} p={p}")
    # one node: self edges only (d = 0: no gradient), seven of the eight lanes of the only workgroup idle
    one = torch.zeros(2, 5, dtype=torch.long)
    x1 = torch.tensor([[0.3, -0.2, 0.1]])
    for rep in (False, True):
        l, cnt, gx = run_hinge(device, x1, one, None, None, R_EMB, 1.0, rep)
        assert cnt == 5 and bool((gx == 0).all()) and tuple(gx.shape) == (1, 3)
        assert_close(l, torch.tensor(float(_F32(R_EMB)) if rep else 0.0, dtype=torch.float64), TOL_OUT, f"hinge one node rep={rep}")


def case_hinge_on_the_hinge(device, dim=3):
    """Repulsive edges, ``p = 1``, whose distance equals ``r_emb`` exactly in fp32 (on an axis: one non-zero difference,
    sqrt(d * d) = d): term 0 and gradient 0; the neighbours one ulp inside contribute 2^-24 each and a gradient of
    one edge; one ulp outside nothing.  ``r_emb = 0.75`` is an fp32 value, so the kernel and the reference hold the
    same radius.  The loss is a sum of exact fp32 terms in fp64, rounded to fp32 and divided in fp32: two roundings,
    3 * 2^-24 relative at the most - the bar is 1e-6 of the reference, not TOL_OUT (which is above the loss itself)."""
    r = _F32(0.75)
    d_of = {"on": r, "inside": np.nextafter(r, _F32(0)), "outside": np.nextafter(r, _F32(2))}
    kinds = ("on", "inside", "outside")
    n_pairs = 30
    x = torch.zeros(2 * n_pairs, dim)
    rows = []
    for i in range(n_pairs):
        x[2 * i + 1, i % dim] = float(d_of[kinds[i % 3]]) * (1 if i % 2 else -1)
        rows += [(2 * i, 2 * i + 1), (2 * i + 1, 2 * i)]   # (both directions: the walk by target and the one by source)
    edges = torch.tensor(rows, dtype=torch.long).t().contiguous()
    d32 = torch.linalg.norm(x[edges[0]] - x[edges[1]], dim=-1)
    for j, k in enumerate(kinds):
        assert bool((d32[j * 2::6] == float(d_of[k])).all())
    lr, cr, gr = ref_hinge(x, edges, None, None, float(r), 1.0, True)
    l, cnt, gx = run_hinge(device, x, edges, None, None, float(r), 1.0, True)
    gx = gx.cpu()
    assert cnt == cr == 2 * n_pairs
    assert abs(lr.item() - 20 * 2.0 ** -24 / 60) < 1e-15   # (ten pairs inside, two edges each, 2^-24 per edge)
    assert abs(l.item() - lr.item()) <= 1e-6 * lr.item(), f"hinge on the hinge: loss {l.item()!r} vs {lr.item()!r}"
    node_kind = [kinds[(v // 2) % 3] for v in range(2 * n_pairs)]
    for k in kinds:
        rows_k = torch.tensor([v for v in range(2 * n_pairs) if node_kind[v] == k])
        if k == "inside":
            assert bool((gr[rows_k].abs().sum(dim=1) > 0).all()) and bool((gx[rows_k].abs().sum(dim=1) > 0).all())
        else:
            assert bool((gr[rows_k] == 0).all()), k
            assert bool((gx[rows_k] == 0).all()), f"hinge on the hinge: a gradient for edges {k} the radius"
    assert_grad_elementwise(gx, gr, cr, "hinge on the hinge: gradient")


def _hinge_raw_args(x_view, mask8, pid, r_emb, p, rep):
    a = _capi.HingeArgs()
    a.x, a.dim, a.x_stride, a.n_nodes = ops._p(x_view), int(x_view.shape[1]), int(x_view.stride(0)), int(x_view.shape[0])
    a.node_mask, a.particle_id = ops._p(mask8), ops._p(pid)
    a.r_emb, a.p, a.repulsive = float(r_emb), float(p), int(rep)
    return a


def case_hinge_c_entry(device, dim, n=120, n_edges=700):
    """``gnntrk_hinge_forward`` / ``gnntrk_hinge_backward`` called as a C caller would: ``x`` a view with ``x_stride =
    dim + 3`` at +4 bytes inside a NaN buffer, ``gx`` a view with ``gx_stride = dim + 1``.  ``accumulate = 1`` onto a
    seeded base gives ``base + gradient`` (one fp32 addition: the bits of ``base + wrapper's gradient``) and leaves the
    bytes around the view alone; ``accumulate = 0`` onto NaN gives the wrapper's gradient bit for bit."""
    lib = _lib()
    gen = torch.Generator().manual_seed(60 + dim)
    xv = (torch.randn(n, dim, generator=gen) * (0.5 / dim ** 0.5)).to(device)
    pid = torch.randint(0, 20, (n,), generator=gen).to(device)
    mask = (torch.rand(n, generator=gen) > 0.3).to(device)
    edges = torch.randint(0, n, (2, n_edges), generator=gen)
    edges[1, 10:14] = edges[0, 10:14]
    edges = off_the_hinge(xv.cpu(), edges, R_EMB, (1.0, 3.0))
    base = torch.randn(n, dim, generator=gen).to(device)
    ed = edges.to(device)
    for rep, p in ((False, 2.0), (True, 1.0), (True, 3.0)):
        tag = f"hinge C entry dim={dim} rep={rep} p={p}"
        lr, cr, gr = ref_hinge(xv.cpu(), edges, mask.cpu(), pid.cpu(), R_EMB, p, rep)
        lw, cw, gw = run_hinge(device, xv, edges, mask, pid, R_EMB, p, rep)
        xc = Carved(xv, stride=dim + 3, off=1)
        assert xc.view.stride(0) == dim + 3 and xc.view.data_ptr() % 16 == 4
        m8 = mask.view(torch.uint8).contiguous()
        a = _hinge_raw_args(xc.view, m8, pid, R_EMB, p, rep)
        out = torch.empty(3, dtype=torch.float32, device=device)
        ws = ops._ws(lib.gnntrk_hinge_workspace_bytes(n_edges), xv)
        _capi.check(lib.gnntrk_hinge_forward(C.byref(a), ops._p(ed), n_edges, int(ed.stride(0)), None, ops._p(out), ops._p(ws),
                                             ws.numel(), ops._stream(xv)), lib)
        assert int(out[1]) == cr and torch.equal(_bits(out[0]), _bits(lw)), f"{tag}: the forward on the strided x differs"
        gi = ops.graph_index(ed, n, cache=False)
        d = _capi.GraphIndex(gi.n_nodes, gi.n_edges, ops._p(gi.perm), ops._p(gi.tgt), ops._p(gi.src), ops._p(gi.rowptr_t),
                             ops._p(gi.rowptr_s), ops._p(gi.spos), ops._p(gi.spos_inv))
        up = torch.tensor([UP], dtype=torch.float32, device=device)
        for accumulate, fill in ((1, base), (0, torch.full_like(base, float("nan")))):
            gc = Carved(fill, stride=dim + 1, off=3, poison=7.0)
            assert gc.view.stride(0) == dim + 1
            _capi.check(lib.gnntrk_hinge_backward(C.byref(a), C.byref(d), ops._p(up), ops._p(out[2:]), ops._p(gc.view), dim + 1,
                                                  accumulate, ops._stream(xv)), lib)
            gc.assert_surroundings_unchanged(f"{tag} accumulate={accumulate}")
            xc.assert_surroundings_unchanged(tag)
            got = gc.view
            assert bool(torch.isfinite(got).all()), f"{tag} accumulate={accumulate}: not finite"
            if accumulate:
                assert torch.equal(_bits(got), _bits(base + gw)), f"{tag}: accumulate = 1 is not base + gradient"
                # and against fp64: the sum is rounded once more, half an ulp of the sum
                diff = got.cpu().double() - base.cpu().double()
                slack = 2.0 ** -24 * got.cpu().double().abs()
                bar = TOL_GRAD * torch.clamp(gr.abs(), min=UP / cr) + slack
                assert bool(((diff - gr).abs() <= bar).all()), f"{tag}: accumulate = 1 against fp64"
            else:
                assert torch.equal(_bits(got), _bits(gw)), f"{tag}: accumulate = 0 differs from the wrapper's gradient"
                assert_grad_elementwise(got, gr, cr, f"{tag} accumulate=0 gradient")


def case_hinge_forward_cap(device, n_nodes=5000, dim=8):
    """The forward at its cap of 2048 workgroups: 2048 * 1024 + 1029 edges, so a block's contiguous share is 1025
    edges and a thread takes a fifth one; repulsive with both selections.  The count is exact, the loss at TOL_OUT,
    the gradient element-wise - over lists of about 800 edges per node (two walks of about 420)."""
    n_edges = 2048 * 1024 + 1029
    assert -(-n_edges // (4 * 256)) > 2048 and -(-n_edges // 2048) > 1024
    gen = torch.Generator().manual_seed(70)
    x = torch.randn(n_nodes, dim, generator=gen) * 0.25
    pid = torch.randint(0, 40, (n_nodes,), generator=gen)
    mask = torch.rand(n_nodes, generator=gen) > 0.3
    edges = off_the_hinge(x, torch.randint(0, n_nodes, (2, n_edges), generator=gen), R_EMB, (1.0,))
    sel = _check_hinge(device, x, edges, mask, pid, R_EMB, 1.0, True, f"hinge forward cap E={n_edges}")
    assert sel > n_edges // 2


# ------------------------------------------------------------------------------------------ bce_csr at the C entry
def case_bce_csr_unit_gradient_saturated(device):
    """``gnntrk_bce_csr`` on a C caller's gradient buffer: the unit gradient (upstream 1) at the saturated scores,
    element-wise."""
    w, y = saturated_scores(N_SAT, VALUES, seed=11)
    lab8 = (y != 0).to(torch.uint8).to(device)
    lr, gr = ref_bce(w, y.double())
    gwb = torch.full((N_SAT,), float("nan"), device=device)
    loss = _bce_csr_raw(w.to(device), lab8, None, None, 0.0, gwb)
    assert_close(loss, lr, 1e-6, "bce_csr raw loss")
    assert_grad_elementwise(gwb * UP, gr, N_SAT, "bce_csr raw unit gradient")
