"""Layout cases shared by the emulator tests (tests/test_layout_emul.py) and the GPU tests
(tests/test_layout_gpu.py): the kernel variants that a launcher selects by the low bits of a pointer, by a row
stride or by a length that is no multiple of the vector width ("Dispatch sites").  Fresh torch
allocations are aligned and contiguous, so the models only ever reach the fast variant; a sliced batch, a column
view, an odd edge count or a caller on the C ABI reaches the other one.

Every case follows one recipe:
  1. the input is carved out of a larger buffer and the case ASSERTS the alignment / stride class it is in;
  2. the rest of that buffer is poison - NaN for floating types, an id the operation would report for integers -
     results must be finite, and where the operation writes into a caller's view the bytes around the view must
     be bit-unchanged;
  3. the result is compared with a plain high-precision reference at the bars the suite already uses
     (parity_cases.TOL_OUT / TOL_GRAD / TOL16, 1e-6 for the fused BCE, equality for integers and conversions);
  4. and with the same operation on ``view.clone()`` (fresh, aligned, contiguous): bit for bit wherever the
     variants differ in access width only."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import gnn_tracking_amd as G
from gnn_tracking_amd import _capi, ops
from gnn_tracking_amd import ops_bf16 as B
import ref_cpu as O
from parity_cases import TOL16, TOL_GRAD, TOL_OUT, _check_graph_index, assert_close, load, load_params, tt

#: element counts around the vector widths (4, 8) and one block (256 threads, 1024 items of four)
COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4099)

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_POISON_ID = 1 << 40   # an id far outside every node range: counted as out of range, clamped, visibly mis-sorted


class Carved:
    """A ``[rows, cols]`` view (row stride ``stride`` elements, first element ``off`` elements into the buffer) of a
    flat buffer filled with ``poison``; ``tail`` poisoned elements lie behind the last row."""

    def __init__(self, values: torch.Tensor, stride: int | None = None, off: int = 0, poison=float("nan"),
                 device=None, tail: int = 16):
        values = values if values.dim() == 2 else values.reshape(-1, 1)
        rows, cols = values.shape
        stride = cols if stride is None else stride
        assert stride >= cols
        self.geom = ((rows, cols), (stride, 1), off)
        self.buf = torch.full((off + rows * stride + tail,), poison, dtype=values.dtype, device=device or values.device)
        assert self.buf.data_ptr() % 16 == 0, "a fresh allocation is expected to be 16-byte aligned"
        self.view = self.buf.as_strided(*self.geom)
        self.view.copy_(values)
        self.before = self.buf.clone()

    def flat(self):
        """the view as ``[rows]`` (one column)"""
        assert self.geom[0][1] == 1
        return self.view[:, 0]

    def assert_surroundings_unchanged(self, what, width=None):
        """every byte of the buffer outside the view (outside the first ``width`` columns of its rows) is as it was"""
        (rows, cols), strides, off = self.geom
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        inside.as_strided((rows, cols if width is None else width), strides, off).fill_(True)
        bits = _BITS[self.buf.element_size()]
        assert torch.equal(self.buf.view(bits)[~inside], self.before.view(bits)[~inside]), f"{what}: bytes around the view were overwritten"


def _mod16(t):
    return t.data_ptr() % 16


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.element_size()]).cpu()


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: differs from the aligned, contiguous launch"


def _finite(t, what):
    assert bool(torch.isfinite(t.detach().float()).all()), f"{what}: poison reached the result"


def _graph(g, N, E, device):
    ei = tt(g.integers(0, N, size=(2, E)), device).long()
    return ops.graph_index(ei, N, cache=False)


# ------------------------------------------------------------------------------------------ segment_sum (fp32)
#: (N, E, D, row stride, element offset of rows, the class the launcher must choose)
SEGMENT_SUM_F32 = (
    (300, 4000, 4, 4, 0, "sum4"), (300, 4000, 4, 4, 1, "scalar"), (300, 4000, 4, 4, 2, "scalar"), (300, 4000, 4, 4, 3, "scalar"),
    (300, 4000, 4, 8, 0, "v4"), (300, 4000, 4, 8, 1, "scalar"), (300, 4000, 4, 5, 0, "scalar"),
    (300, 4000, 8, 8, 0, "v4"), (300, 4000, 8, 12, 0, "v4"), (300, 4000, 8, 12, 1, "scalar"), (300, 4000, 8, 9, 0, "scalar"),
    (300, 100, 12, 12, 0, "v4"), (300, 100, 12, 12, 3, "scalar"), (64, 1500, 40, 40, 0, "v4"), (64, 1500, 40, 40, 2, "scalar"),
    (7, 20, 5, 5, 1, "scalar"), (5, 1, 3, 4, 1, "scalar"), (9, 2, 1, 1, 1, "scalar"), (1, 0, 4, 4, 1, "scalar"),
)


def _segment_sum_f32_class(rows, out):
    """the launcher's rule (gnntrk_segment_sum), restated on the tensors the wrapper hands over"""
    dim, rs, os_ = rows.shape[1], ops._row_stride(rows), ops._row_stride(out)
    if dim == 4 and rs == 4 and _mod16(rows) == 0:
        return "sum4"
    if dim % 4 == 0 and rs % 4 == 0 and os_ % 4 == 0 and _mod16(rows) == 0 and _mod16(out) == 0:
        return "v4"
    return "scalar"


def case_segment_sum_f32(device, spec):
    """``gnntrk_segment_sum``: the three kernels reached by POINTER as well as by stride - a column window at +4
    bytes (D = 4 in a stride of 8, D = 8 in a stride of 12), contiguous rows at +4 / +8 / +12 bytes, and aligned rows
    with a misaligned ``out`` in accumulate mode; both orders (``tgt``; ``src`` through ``pos``), empty segments.
    All three kernels add a segment's rows in CSR order (segment.hip), so the classes agree bit for bit."""
    N, E, D, stride, off, cls = spec
    g = np.random.default_rng(100 + 7 * D + off)
    gi = _graph(g, N, E, device)
    vals = tt(g.normal(size=(E, D)).astype(np.float32), device)
    c = Carved(vals, stride, off)
    rows = c.view
    assert (E == 0 or _mod16(rows) == 4 * off) and (E < 2 or rows.stride(0) == stride) and rows.stride(1) == 1
    fresh = rows.clone()
    assert (E == 0 or _mod16(fresh) == 0) and fresh.is_contiguous()
    tag = f"segment_sum {cls} N={N} E={E} D={D} stride={stride} +{4 * off}B"
    for by in ("tgt", "src"):
        rowptr, pos = (gi.rowptr_t, None) if by == "tgt" else (gi.rowptr_s, gi.spos)
        node = (gi.tgt if by == "tgt" else gi.src).cpu().long()
        ref = torch.zeros(N, D, dtype=torch.float64)
        if E:
            ref.index_add_(0, node, vals.cpu().double())
        out = ops._segment_sum_raw(rows, rowptr, pos, N)
        if E:
            assert _segment_sum_f32_class(ops._as_rows(rows), out) == cls, f"{tag}: the view is not in its class"
        _finite(out, tag)
        assert_close(out, ref.float(), TOL_OUT, f"{tag} {by}")
        _same_bits(out, ops._segment_sum_raw(fresh, rowptr, pos, N), f"{tag} {by}")
        # accumulate into a caller's view of a padded, poisoned buffer: aligned, and at +4 / +8 bytes
        base = tt(g.normal(size=(N, D)).astype(np.float32), device)
        want = None
        for ostride, ooff in ((D, 0), (D + 4 - D % 4, 0), (D + 4 - D % 4, 1), (D, 2), (D + 1, 0)):
            oc = Carved(base, ostride, ooff)
            assert _mod16(oc.view) == 4 * ooff
            ops._segment_sum_raw(rows, rowptr, pos, N, out=oc.view, accumulate=True)
            oc.assert_surroundings_unchanged(f"{tag} {by} accumulate out stride={ostride} +{4 * ooff}B")
            assert_close(oc.view, (base.cpu().double() + ref).float(), TOL_OUT, f"{tag} {by} accumulate")
            want = oc.view.clone() if want is None else want
            _same_bits(oc.view, want, f"{tag} {by} accumulate out stride={ostride} +{4 * ooff}B")


# ------------------------------------------------------------------------------------------ bce_csr, _BCE, _Focal
def _bce_csr_raw(w, label, src, pt, thld, gw):
    """``gnntrk_bce_csr`` on the caller's own buffers (the autograd wrapper allocates ``gw`` itself)"""
    lib = _capi.load()
    n = w.numel()
    loss = torch.empty(1, dtype=torch.float32, device=w.device)
    ws = ops._ws(lib.gnntrk_bce_workspace_bytes(n), w)
    _capi.check(lib.gnntrk_bce_csr(ops._p(w), ops._p(label), ops._p(src), ops._p(pt), thld, n, ops._p(loss), ops._p(gw),
                                   ops._p(ws), ws.numel(), ops._stream(w)), lib)
    return loss.view(())


def case_bce_csr(device, n):
    """``gnntrk_bce_csr``: ``float4`` + one label word per four edges, or item by item - chosen by the alignment of
    ``w`` (16), ``label_csr`` (4) and the gradient buffer (16; NULL counts as aligned), and per group of four by
    ``e0 + 4 <= n``.  Each of the three in and out of its class, pt threshold off and on, against torch's BCE in fp64
    (1e-6, as case_graph_index_carry) and against the aligned call bit for bit (bce_csr_kernel: "both forms give the
    same bits")."""
    g = np.random.default_rng(200 + n)
    N = 37
    wv = tt(g.uniform(0.001, 0.999, size=n).astype(np.float32), device)
    lv = tt((g.random(n) < 0.4).astype(np.uint8) * g.integers(1, 256, size=n).astype(np.uint8), device)   # (any non-zero byte is "true")
    src = tt(g.integers(0, N, size=n).astype(np.int32), device)
    pt = tt(g.lognormal(size=N).astype(np.float32), device)
    for thld in (0.0, 0.9):
        t = (lv != 0).double().cpu()
        if thld > 0:
            t = t * (pt[src.long()] > thld).double().cpu()
        wr = wv.cpu().double().requires_grad_(True)
        ref = torch.nn.functional.binary_cross_entropy(wr, t)
        (ref * 1.5).backward()
        args = (src if thld > 0 else None, pt if thld > 0 else None, thld)
        base = {}
        for w_off, l_off in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3)):
            wc, lc = Carved(wv, off=w_off), Carved(lv, off=l_off, poison=255)
            w, lab = wc.flat(), lc.flat()
            assert _mod16(w) == 4 * w_off and lab.data_ptr() % 4 == l_off and w.is_contiguous() and lab.is_contiguous()
            tag = f"bce_csr n={n} thld={thld} w+{4 * w_off}B label+{l_off}B"
            for need_grad in (False, True):   # (without a gradient buffer the launcher sees NULL: aligned)
                wl = w.detach().requires_grad_(need_grad)
                loss = ops._BCECsr.apply(wl, lab, *args)
                _finite(loss, tag)
                assert_close(loss, ref.detach(), 1e-6, tag)
                _same_bits(loss, base.setdefault("loss", loss.detach().clone()), tag)
                if need_grad:
                    (loss * 1.5).backward()
                    _finite(wl.grad, tag + " gradient")
                    assert_close(wl.grad, wr.grad, 1e-6, tag + " gradient")
                    _same_bits(wl.grad, base.setdefault("grad", wl.grad.clone()), tag + " gradient")
            wc.assert_surroundings_unchanged(tag), lc.assert_surroundings_unchanged(tag)
        # the gradient buffer of a C caller at +0 / +4 / +8 / +12 bytes, w and the labels aligned
        unit = None
        for g_off in (0, 1, 2, 3):
            gc = Carved(torch.zeros(n, dtype=torch.float32, device=device), off=g_off)
            gw = gc.flat()
            assert _mod16(gw) == 4 * g_off and _mod16(wv) == 0 and lv.data_ptr() % 4 == 0
            tag = f"bce_csr n={n} thld={thld} gw_unit+{4 * g_off}B"
            loss = _bce_csr_raw(wv, lv, args[0], args[1], thld, gw)
            gc.assert_surroundings_unchanged(tag)
            _same_bits(loss, base["loss"], tag)
            assert_close(gw * 1.5, wr.grad, 1e-6, tag)
            unit = gw.clone() if unit is None else unit
            _same_bits(gw, unit, tag)


def case_bce_focal_strided(device, n):
    """The two-pass losses (``ops._BCE``, ``ops._Focal``) on a ``w`` that is one column of an ``[E, 2]`` tensor and a
    ``y`` read through a stride: the wrappers' ``.contiguous()`` path.  Against fp64 (TOL_OUT for the loss, TOL_GRAD
    for the gradient) and against the call on the clones bit for bit."""
    g = np.random.default_rng(300 + n)
    N = 23
    wv = tt(g.uniform(0.02, 0.98, size=n).astype(np.float32), device)
    yv = tt((g.random(n) < 0.4).astype(np.float32), device)
    wc, yc = Carved(wv, stride=2, off=1), Carved(yv, stride=3, off=0)
    src = tt(g.integers(0, N, size=n), device).long()
    pt = tt(g.lognormal(size=N).astype(np.float32), device)
    assert n < 2 or (wc.flat().stride(0) == 2 and yc.flat().stride(0) == 3)
    assert _mod16(wc.flat()) == 4
    for thld in (0.0, 0.9):
        t = yv.cpu().double()
        if thld > 0:
            t = t * (pt[src] > thld).double().cpu()
        extra = (src if thld > 0 else None, pt if thld > 0 else None, thld)
        wr = wv.cpu().double().requires_grad_(True)
        alpha, gamma, pw = 0.3, 2.0, 1.5
        refs = {"bce": torch.nn.functional.binary_cross_entropy(wr, t),
                "focal": (-alpha * pw * (1 - wr) ** gamma * t * wr.log() - (1 - alpha) * wr ** gamma * (1 - t) * (1 - wr).log()).mean()}
        for name, fn in (("bce", lambda w, y: ops._BCE.apply(w, y, *extra)),
                         ("focal", lambda w, y: ops._Focal.apply(w, y, *extra, alpha, gamma, pw, False))):
            wr.grad = None
            (refs[name] * 1.5).backward()
            got = []
            for w, y in ((wc.flat(), yc.flat()), (wv.clone(), yv.clone())):
                wl = w.detach().requires_grad_(True)
                loss = fn(wl, y)
                (loss * 1.5).backward()
                got.append((loss.detach(), wl.grad))
            tag = f"{name} n={n} thld={thld} strided w / y"
            _finite(got[0][0], tag), _finite(got[0][1], tag)
            assert_close(got[0][0], refs[name].detach(), TOL_OUT, tag)
            assert_close(got[0][1], wr.grad, TOL_GRAD, tag + " gradient")
            _same_bits(got[0][0], got[1][0], tag), _same_bits(got[0][1], got[1][1], tag + " gradient")
    wc.assert_surroundings_unchanged("strided w"), yc.assert_surroundings_unchanged("strided y")


# ------------------------------------------------------------------------------------------ rows_to_bf16
def case_rows_to_bf16(device, n):
    """``gnntrk_rows_to_bf16``: ``rows4_to_bf16_kernel`` (dim 4, stride % 4 == 0, 16-byte aligned base: one 16-byte
    load per row) or the generic kernel - dim-4 rows at +4 / +8 / +12 bytes and at a stride of 5, against the aligned
    stride-4 and stride-8 forms, with and without the gather; other widths through a column window.  The result is
    the RNE conversion, exactly, and its padding columns are zero."""
    g = np.random.default_rng(400 + n)
    idx = tt(g.integers(0, n, size=n + 3).astype(np.int32), device)
    for D, stride, off, rows4 in ((4, 4, 0, True), (4, 8, 0, True), (4, 4, 1, False), (4, 4, 2, False), (4, 4, 3, False),
                                  (4, 5, 0, False), (4, 8, 1, False), (3, 4, 0, False), (5, 8, 1, False), (8, 12, 1, False)):
        vals = tt((g.normal(size=(n, D)) * 3).astype(np.float32), device)
        c = Carved(vals, stride, off)
        x = c.view
        assert _mod16(x) == 4 * off and (n < 2 or x.stride(0) == stride)
        if n > 1:
            assert (D == 4 and x.stride(0) % 4 == 0 and _mod16(x) == 0) == rows4, "the view is not in its class"
        tag = f"rows_to_bf16 n={n} D={D} stride={stride} +{4 * off}B"
        want = vals.cpu().to(torch.bfloat16)
        for ix in (None, idx):
            got = B.to_rows16(x, ix)
            assert got.stride(0) == B.pad4(D) and got.data_ptr() % 8 == 0
            _finite(got, tag)
            w = want if ix is None else want[ix.cpu().long()]
            assert torch.equal(_bits(got), _bits(w)), f"{tag}: not the RNE conversion" + (" of the gathered rows" if ix is not None else "")
            _same_bits(got, B.to_rows16(x.clone(), ix), tag)
            if B.pad4(D) > D:   # (the padding columns of the caller-visible buffer)
                full = got.as_strided((got.shape[0], B.pad4(D)), (B.pad4(D), 1), got.storage_offset())
                assert bool((full[:, D:].view(torch.int16) == 0).all()), f"{tag}: padding columns are not zero"


# ------------------------------------------------------------------------------------------ bf16 segment sums, permutations
#: (N, E): several blocks of segments, a ragged last wave, segments without rows, one segment holding everything
SEGSUM16_GRAPHS = ((300, 4000), (17, 301), (1, 37), (5, 1), (70, 33))


def _segsum16_class(rows, pos, addend):
    """the launcher's rule (segment_sum_bf16_launch), restated"""
    nch, rs = (rows.shape[1] + 3) // 4, rows.stride(0)
    if nch == 1 and rs == 4 and pos is None and addend is None and _mod16(rows) == 0:
        return "pair8"
    wide = nch % 2 == 0 and rs % 8 == 0 and _mod16(rows) == 0
    if nch == 2 and wide and rs == 8 and pos is None:
        return "stream16"
    return f"walk<{nch},{'true' if wide else 'false'}>"


def case_segment_sum_bf16(device, D):
    """``gnntrk_segment_sum_bf16[_add]``: ``pair8`` (contiguous 8-byte rows, 16-byte aligned, no ``pos`` / addend),
    ``stream16`` (contiguous aligned 16-byte rows, no ``pos``), the four-lane walk with 16-byte loads (``<N,true>``)
    or 8-byte loads (``<N,false>``).  ``[E, D <= 4]`` rows that start on an odd row are 8 mod 16 and leave ``pair8``;
    ``[E, D <= 8]`` rows inside a 12-wide buffer, or 8 mod 16, leave ``stream16`` and ``<2,true>``.  With and
    without ``pos`` and the addend.  Against index_add in fp64 at TOL16 (one rounding of an fp32 sum).

    Bit for bit against the launch on the clone wherever the kernels add in the same order: ``stream16``,
    ``<2,true>`` and ``<2,false>`` give lane j the rows k0 + j, k0 + j + 4, ... and add them in that order.
    ``pair8`` does NOT: its lane j takes the aligned row PAIRS p0 + j, p0 + j + 4, ... (rows 2p, 2p + 1), another
    assignment of rows to lanes than the walk's, so for D <= 4 without ``pos`` and addend only the fp64 bar holds
    between the aligned and the misaligned launch.  Byte offsets 2, 4 and 6 are no row tensors of the kernels:
    ``rows16`` copies them, same bits as the clone."""
    g = np.random.default_rng(500 + D)
    P = B.pad4(D)
    for N, E in SEGSUM16_GRAPHS:
        gi = _graph(g, N, E, device)
        vals = tt(g.normal(size=(E, D)).astype(np.float32), device).to(torch.bfloat16)
        addv = tt(g.normal(size=(N, D)).astype(np.float32), device).to(torch.bfloat16)
        layouts = [(P, 0), (P, 4), (P + 4, 0), (P + 4, 4), (2 * P, 0)]   # (row stride, element offset): +8 bytes = 4 elements
        copies = [(P, 1), (P, 2), (P, 3), (P + 1, 0)]                    # rows16 copies: +2 / +4 / +6 bytes, a stride that is no multiple of 4
        for by in ("tgt", "src"):
            rowptr, pos = (gi.rowptr_t, None) if by == "tgt" else (gi.rowptr_s, gi.spos)
            node = (gi.tgt if by == "tgt" else gi.src).cpu().long()
            ref = torch.zeros(N, D, dtype=torch.float64)
            ref.index_add_(0, node, vals.cpu().double())
            for with_add in (False, True):
                want = (ref + addv.cpu().double()) if with_add else ref
                want16 = want.float().to(torch.bfloat16).float()
                fresh_rows, fresh_add = B.rows16(vals.clone()), (B.rows16(addv.clone()) if with_add else None)
                aligned = B.segment_sum_raw(fresh_rows, rowptr, pos, N, addend=fresh_add)
                cls0 = _segsum16_class(fresh_rows, pos, fresh_add)
                seen = {cls0}
                for stride, off in layouts + copies:
                    rc = Carved(vals, stride, off)
                    ac = Carved(addv, stride, off) if with_add else None
                    rows = rc.view
                    assert rows.data_ptr() % 16 == (2 * off) % 16 and (E < 2 or rows.stride(0) == stride)
                    direct = B.rows16(rows) is rows
                    assert direct == ((stride, off) in layouts), "rows16: copy or no copy"
                    cls = _segsum16_class(B.rows16(rows), pos, ac)
                    seen.add(cls)
                    tag = f"segment_sum_bf16 {cls} {by} N={N} E={E} D={D} stride={stride} +{2 * off}B addend={with_add}"
                    out = B.segment_sum_raw(rows, rowptr, pos, N, addend=None if ac is None else ac.view)
                    _finite(out, tag)
                    assert_close(out.float(), want16, TOL16, tag)
                    if "pair8" not in (cls, cls0) or cls == cls0:
                        _same_bits(out, aligned, tag)
                    rc.assert_surroundings_unchanged(tag)
                if E > 1 and by == "tgt" and not with_add:
                    assert seen >= ({"pair8", "walk<1,false>"} if P == 4 else {"stream16", "walk<2,true>", "walk<2,false>"}), seen
        # the caller's padded output rows (C ABI): 8 mod 16, a stride beyond the padded width; whole 8-byte chunks
        # are written (padding columns: zero), nothing else
        oc = Carved(torch.zeros(N, P, dtype=torch.bfloat16, device=device), P + 4, 4, poison=float("nan"))
        rc = Carved(vals, P, 4)
        lib = _capi.load()
        _capi.check(lib.gnntrk_segment_sum_bf16(rc.view.data_ptr(), D, P, ops._p(gi.rowptr_t), None, N, oc.view.data_ptr(),
                                                P + 4, ops._stream(vals)), lib)
        oc.assert_surroundings_unchanged(f"segment_sum_bf16 out N={N} E={E} D={D}")
        ref = torch.zeros(N, D, dtype=torch.float64).index_add_(0, gi.tgt.cpu().long(), vals.cpu().double())
        assert_close(oc.view[:, :D].float(), ref.float().to(torch.bfloat16).float(), TOL16, f"segment_sum_bf16 out N={N} D={D}")
        assert bool((oc.view[:, D:].view(torch.int16) == 0).all())
        # permutations: whole 8-byte chunks are copied - the rows of the result are the rows of the source, exactly
        if E:
            perm = gi.perm
            for stride, off in layouts + copies:
                rows = Carved(vals, stride, off).view
                tag = f"permute_rows_bf16 N={N} E={E} D={D} stride={stride} +{2 * off}B"
                got = B.permute_raw(rows, perm, scatter=False)
                assert torch.equal(_bits(got), _bits(vals[perm.long()])), tag + " gather"
                back = B.permute_raw(got, perm, scatter=True)
                assert torch.equal(_bits(back), _bits(vals)), tag + " scatter"


# ------------------------------------------------------------------------------------------ graph_index build / carry / remap
#: (class, E, element offset of the flat [2 * E] id buffer): the vector key reads need edge_index AND edge_index + E
#: 16-byte aligned - an odd E breaks the second row, an 8-byte offset the first (with an odd E: the first only)
GRAPH_INDEX_LISTS = (("oddE", 301, 0), ("8mod16", 300, 1), ("oddE-8mod16", 3999, 1), ("oddE-tiny", 3, 0), ("one", 1, 1))


def case_graph_index(device, spec, N=57):
    """``gnntrk_graph_index_build_carry``, all three ``flags``: ``KeysCoo`` / ``gi_remap_count_kernel`` read four ids as
    two 16-byte loads only if both id rows are 16-byte aligned, the labels as one word only if they are 4-byte
    aligned (``KeysCoo`` / ``KeysCoo32``); otherwise item by item.  Odd ``E`` and an 8-mod-16 contiguous edge list,
    each with labels at byte offsets 0 .. 3, with carried rows, and with ``order_by`` (the renumbered build).  The
    buffers around the ids hold an id out of range: the build would count it (``validate=True`` raises) and sort
    it visibly wrong.  Against torch's stable sorts (``_check_graph_index``) and the gathers through ``perm``;
    against the build of the clones, every array bit for bit."""
    cls, E, off = spec
    g = np.random.default_rng(600 + E + off)
    ids = tt(g.integers(0, N, size=(2 * E,)), device).long()
    ids[::3] = 5   # (a hub: long runs of one key)
    ec = Carved(ids, off=off, poison=_POISON_ID)
    ei = ec.flat().view(2, E)
    assert ei.is_contiguous() and _mod16(ei) == 8 * off
    assert (_mod16(ei[0]) == 0 and _mod16(ei[1]) == 0) is False or E == 0, "both id rows aligned: the vector class"
    eic = ids.view(2, E).cpu()
    rows_v = tt((g.normal(size=(E, 4)) * 3).astype(np.float32), device)
    x = tt(g.normal(size=(N, 3)).astype(np.float32), device)
    x[::5, 1] = 0.25
    fresh = ei.clone()
    assert _mod16(fresh) == 0
    names = ("perm", "tgt", "src", "rowptr_t", "rowptr_s", "spos", "spos_inv")
    refs = {}
    for l_off in (0, 1, 2, 3):
        lc = Carved(tt((g.random(E) < 0.4), device).view(torch.uint8) * 255, off=l_off, poison=255)
        y = lc.flat()
        assert y.data_ptr() % 4 == l_off and y.is_contiguous()
        # the carried rows keep their contract (16-byte aligned, stride % 4 == 0): inside a wider, poisoned buffer
        rc = Carved(rows_v, stride=8, off=4)
        rows = rc.view
        assert ops._carry_rows_ok(rows, E, rows.device) and (E < 2 or rows.stride(0) == 8)
        for order in (False, True) if l_off in (0, 3) else (False,):
            order_by = (x, 1, None) if order else None
            for flags in (0, 1, 2):
                tag = f"graph_index {cls} E={E} label+{l_off}B order_by={order} flags={flags}"
                gi = ops.graph_index(ei, N, cache=False, flags=flags, validate=True, carry_label=y, carry_rows=rows, order_by=order_by)
                _check_graph_index(gi, gi.node_rank.cpu().long()[eic] if order else eic, N, tag)
                perm = gi.perm.long()
                lab, rcsr = ops.carried_label(gi, y), ops.carried_rows(gi, rows)
                assert lab is not None and rcsr is not None, tag
                assert torch.equal(lab.cpu(), (y[perm] != 0).to(torch.uint8).cpu()), tag + ": carried labels"
                assert torch.equal(_bits(rcsr), _bits(rows_v[perm].to(torch.bfloat16))), tag + ": carried rows"
                if (order, flags) not in refs:
                    refs[order, flags] = ops.graph_index(fresh, N, cache=False, flags=flags, order_by=order_by)
                ref = refs[order, flags]
                for k in names + (("node_perm", "node_rank") if order else ()):
                    assert torch.equal(getattr(gi, k), getattr(ref, k)), f"{tag}: {k} differs from the build of the aligned list"
        lc.assert_surroundings_unchanged("labels"), rc.assert_surroundings_unchanged("carried rows")
    ec.assert_surroundings_unchanged("edge list")


def case_carry_rows_fallback(device, name="skip1_L3_h40"):
    """``ops._carry_rows_ok``: an ``edge_attr`` view the build cannot carry (+4 bytes; a row stride of 5) is not
    carried - ``carried_rows`` returns None - and ``ECForGraphTCN`` takes the gather through ``perm``: the same ``W``
    and edge embedding bit for bit as on the contiguous clone (which IS carried).  As case_ec_carry_equals_gather."""
    z = load("g2_ec_variants.npz")
    x, ei, y = tt(z["x"], device), tt(z["edge_index"], device), tt(z["y"], device).bool()
    eav = tt(z["edge_attr"], device)
    E = eav.shape[0]
    out = {}
    for cls, stride, off in (("aligned", 4, 0), ("+4B", 4, 1), ("stride5", 5, 0), ("+8B-stride8", 8, 2)):
        c = Carved(eav, stride, off)
        ea = c.view
        assert _mod16(ea) == 4 * off and ea.stride(0) == stride
        ok = ops._carry_rows_ok(ea, E, ea.device)
        assert ok == (cls == "aligned"), f"edge_attr {cls}: not in its class"
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **_ec_variant(name))
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        ops.clear_graph_index_cache()
        with G.bf16_storage(), torch.no_grad():
            res = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y))
        gi = res["W"].graph_index
        assert (ops.carried_rows(gi, ea) is not None) == ok, f"edge_attr {cls}: carried_rows"
        out[cls] = (torch.as_tensor(res["W"]).detach().float().cpu(), torch.as_tensor(res["edge_embedding"]).detach().float().cpu())
        _finite(out[cls][0], f"W, edge_attr {cls}")
        c.assert_surroundings_unchanged(f"edge_attr {cls}")
    for cls in out:
        assert torch.equal(out[cls][0], out["aligned"][0]) and torch.equal(out[cls][1], out["aligned"][1]), \
            f"edge_attr {cls}: W / edge embedding differ from the carried build"


def _ec_variant(name):
    from parity_cases import EC_VARIANTS
    return EC_VARIANTS[name]


# ------------------------------------------------------------------------------------------ compaction (graph cut)
def _compact_ws(lib, n, like):
    return ops._ws(lib.gnntrk_compact_workspace_bytes(max(int(n), 1)), like)


def case_connected_nodes(device, n_nodes):
    """``gnntrk_connected_nodes``: ``FlagByte`` reads eight flags as one 8-byte word if ``hit`` is 8-byte aligned,
    else byte by byte - a caller's ``hit`` buffer at +1 .. +7 bytes (the Python wrapper allocates an aligned one),
    an ``edge_index`` that is an 8-mod-16 view.  Against the oracle, exactly; sentinels around every output."""
    lib = _capi.load()
    g = np.random.default_rng(700 + n_nodes)
    E = max(1, n_nodes // 2)
    ids = tt(g.integers(0, max(1, n_nodes - n_nodes // 3), size=(2 * E,)), device).long()
    ec = Carved(ids, off=1, poison=_POISON_ID)
    ei = ec.flat().view(2, E)
    assert _mod16(ei) == 8
    oh, oc, oe = O.connected_nodes(ids.view(2, E).cpu(), n_nodes)
    for h_off in range(8):
        hc = Carved(torch.zeros(n_nodes, dtype=torch.uint8, device=device), off=h_off, poison=0x5a)
        ic = Carved(torch.zeros(n_nodes, dtype=torch.int32, device=device), off=1, poison=-7)
        nc = Carved(torch.zeros(n_nodes, dtype=torch.int32, device=device), off=3, poison=-7)
        oec = Carved(torch.zeros(2 * E, dtype=torch.int64, device=device), off=1, poison=_POISON_ID)
        hit = hc.flat()
        assert hit.data_ptr() % 8 == h_off
        n_out = torch.empty(2, dtype=torch.int64, device=device)
        ws = _compact_ws(lib, n_nodes, hit)
        _capi.check(lib.gnntrk_connected_nodes(ops._p(ei), E, n_nodes, ops._p(hit), ops._p(ic.flat()), ops._p(nc.flat()),
                                               ops._p(n_out), ops._p(oec.flat()), ops._p(ws), ws.numel(), ops._stream(ei)), lib)
        n_conn, bad = (int(v) for v in n_out.tolist())
        tag = f"connected_nodes N={n_nodes} hit+{h_off}B"
        assert bad == 0 and n_conn == oc.numel(), tag
        assert torch.equal(hit.cpu().bool(), oh), tag + ": hit mask"
        assert torch.equal(ic.flat()[:n_conn].cpu().long(), oc), tag + ": connected nodes"
        assert torch.equal(oec.flat().view(2, E).cpu(), oe), tag + ": relabelled edge_index"
        newid = torch.full((n_nodes,), -1, dtype=torch.long)
        newid[oc] = torch.arange(oc.numel())
        assert torch.equal(nc.flat().cpu().long(), newid), tag + ": new ids"
        hc.assert_surroundings_unchanged(tag), nc.assert_surroundings_unchanged(tag), oec.assert_surroundings_unchanged(tag)
        ic.assert_surroundings_unchanged(tag, width=None)
    ec.assert_surroundings_unchanged("edge_index")


def case_threshold_compact(device, n):
    """``gnntrk_threshold_compact`` at the C ABI: ``w`` in and out of its 16-byte class, the caller's ``mask`` in and
    out of its 8-byte class (compact_write_kernel: ``mask_vec``) - one at a time and both.  Against the oracle,
    exactly; NaN around ``w`` (NaN > thr is false, but a NaN read as a kept entry would shift every index)."""
    lib = _capi.load()
    g = np.random.default_rng(800 + n)
    wv = tt(g.random(n).astype(np.float32), device)
    if n > 10:
        wv[3] = float("nan")
        wv[n - 1] = 0.5
    om, oi = O.threshold_compact(wv.cpu(), 0.5)
    for w_off, m_off in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 4), (0, 7), (1, 3)):
        wc = Carved(wv, off=w_off, poison=2.0)   # (a poison that WOULD be kept)
        mc = Carved(torch.zeros(n, dtype=torch.uint8, device=device), off=m_off, poison=0x5a)
        ic = Carved(torch.zeros(n, dtype=torch.int32, device=device), off=1, poison=-7)
        w, mask = wc.flat(), mc.flat()
        assert _mod16(w) == 4 * w_off and mask.data_ptr() % 8 == m_off
        n_out = torch.empty(1, dtype=torch.int64, device=device)
        ws = _compact_ws(lib, n, w)
        _capi.check(lib.gnntrk_threshold_compact(ops._p(w), n, 0.5, ops._p(mask), ops._p(ic.flat()), ops._p(n_out), ops._p(ws),
                                                 ws.numel(), ops._stream(w)), lib)
        tag = f"threshold_compact n={n} w+{4 * w_off}B mask+{m_off}B"
        k = int(n_out.item())
        assert k == oi.numel(), tag
        assert torch.equal(mask.cpu().bool(), om), tag + ": mask"
        assert torch.equal(ic.flat()[:k].cpu().long(), oi), tag + ": kept positions"
        mc.assert_surroundings_unchanged(tag), ic.assert_surroundings_unchanged(tag)


# ------------------------------------------------------------------------------------------ kNN emit (count scan)
def case_knn_emit(device, n, d=3, k=7, r=0.45):
    """``gnntrk_knn_emit`` / ``gnntrk_knn_emit_prefix``: ``scan_counts_kernel<true>`` loads four counts as one 16-byte
    word if ``cnt`` is 16-byte aligned, ``<false>`` one by one - a caller's ``cnt`` at +4 / +8 / +12 bytes (the Python
    wrapper allocates an aligned one).  The counts around it are huge: read into the scan they would move every
    offset.  Against the C oracle's edge list, exactly, for the full list and a prefix."""
    lib = _capi.load()
    g = np.random.default_rng(900 + n)
    x = tt(g.random((n, d)).astype(np.float32), device)
    kk = min(k, n - 1)
    st = ops._stream(x)
    nbr = torch.empty(n * kk, dtype=torch.int32, device=device)
    cnt0 = torch.empty(n, dtype=torch.int32, device=device)
    ops._knn_search(lib, x, kk, r, None, nbr, cnt0, st)
    for c_off in (0, 1, 2, 3):
        cc = Carved(cnt0, off=c_off, poison=1 << 20)
        cnt = cc.flat()
        assert _mod16(cnt) == 4 * c_off
        for k_take in (kk, max(1, kk // 2)):
            oc = Carved(torch.zeros(n + 1, dtype=torch.int64, device=device), off=1, poison=-7)
            off = oc.flat()
            _capi.check(lib.gnntrk_knn_emit_prefix(ops._p(nbr), ops._p(cnt), n, kk, k_take, ops._p(off), None, 0, st), lib)
            m = int(off[n].item())
            want = O.knn_graph_c(x.cpu(), k_take, r)
            tag = f"knn_emit n={n} cnt+{4 * c_off}B k_take={k_take}"
            assert m == want.shape[1], f"{tag}: {m} edges, the oracle has {want.shape[1]}"
            ei = torch.empty(2, m, dtype=torch.int64, device=device)
            if k_take == kk:
                _capi.check(lib.gnntrk_knn_emit(ops._p(nbr), ops._p(cnt), n, kk, ops._p(off), ops._p(ei), m, st), lib)
            else:
                _capi.check(lib.gnntrk_knn_emit_prefix(ops._p(nbr), ops._p(cnt), n, kk, k_take, ops._p(off), ops._p(ei), m, st), lib)
            assert torch.equal(ei.cpu(), want), tag
            oc.assert_surroundings_unchanged(tag)


# ------------------------------------------------------------------------------------------ strided point / node rows
def _x_views(vals):
    """``vals`` [n, d] as (class, view, carved buffer): a column window of a wider tensor at +4 bytes (row stride
    d + 3 > d), and a transposed view (column stride != 1: the wrappers copy)"""
    n, d = vals.shape
    w = Carved(vals, stride=d + 3, off=1)
    assert _mod16(w.view) == 4 and (n < 2 or w.view.stride(0) == d + 3) and w.view.stride(1) == 1
    t = Carved(vals.t().contiguous(), stride=n + 1, off=1)
    tv = t.view.t()
    assert tuple(tv.shape) == (n, d) and (d < 2 or tv.stride(1) == n + 1) and not (n > 1 and d > 1 and tv.is_contiguous())
    return (("window+4B", w.view, w), ("transposed", tv, t))


def case_knn_strided_x(device, n, d):
    """``ops.knn_graph`` / ``knn_scan`` / ``losses_ml.radius_graph`` (batched) / ``DBSCANFastRescan`` on point rows
    read through a row stride (a column window at +4 bytes) and on a transposed view: the C oracle's edge list and
    the oracle's DBSCAN labels, exactly, and the results on the clone bit for bit (integer outputs; fp64
    distances)."""
    from gnn_tracking_amd.losses_ml import radius_graph
    from gnn_tracking_amd.postprocessing import DBSCANFastRescan
    g = np.random.default_rng(1000 + 10 * n + d)
    vals = tt(g.random((n, d)).astype(np.float32), device)
    sizes = [n // 3, n - n // 3]
    batch = torch.cat([torch.full((s,), i, dtype=torch.long) for i, s in enumerate(sizes)]).to(device)
    k, r = 6, 0.5 if d <= 3 else 0.9
    want = O.knn_graph_c(vals.cpu(), k, r) if n > 1 else torch.empty(2, 0, dtype=torch.int64)
    fresh = vals.clone()
    rb0, db0 = radius_graph(fresh, r, batch, 8), DBSCANFastRescan(fresh, max_eps=r)
    for cls, x, c in _x_views(vals):
        tag = f"n={n} d={d} x {cls}"
        assert torch.equal(ops.knn_graph(x, k, r).cpu(), want), "knn_graph " + tag
        scan = ops.knn_scan(x, (1, k), r)
        assert torch.equal(scan[k].cpu(), want) and torch.equal(scan[1].cpu(), O.knn_graph_c(vals.cpu(), 1, r) if n > 1 else want), "knn_scan " + tag
        assert torch.equal(radius_graph(x, r, batch, 8), rb0), "radius_graph (batched) " + tag
        db = DBSCANFastRescan(x, max_eps=r)
        assert torch.equal(db._off, db0._off) and torch.equal(db._nbr, db0._nbr) and torch.equal(db._dist, db0._dist), "radius neighbours " + tag
        for eps, mp in ((r, 1), (0.6 * r, 3)):
            lab = db.cluster(eps, mp)
            assert np.array_equal(lab, db0.cluster(eps, mp)), "DBSCAN " + tag
            assert np.array_equal(lab, O.dbscan_labels(vals.cpu().numpy(), r, eps, mp)), "DBSCAN against the oracle " + tag
        c.assert_surroundings_unchanged(tag)


def case_edge_features_strided_x(device, n=41, d=5, n_edges=300):
    """``ops.edge_features`` (forward and the gradient w.r.t. ``x``) on a column window at +4 bytes and on a
    transposed ``x``, with an edge list that is an 8-mod-16 view: ``cat[x_i - x_j, x_i + x_j]`` in torch, exactly
    (one fp32 operation per element), its fp64 gradient at TOL_GRAD, and the clone's results bit for bit."""
    g = np.random.default_rng(1100)
    vals = tt(g.normal(size=(n, d)).astype(np.float32), device)
    ids = tt(g.integers(0, n, size=(2 * n_edges,)), device).long()
    ec = Carved(ids, off=1, poison=n - 1)   # (the kernel does not check ids: a poison inside the range, wrong if read)
    ei = ec.flat().view(2, n_edges)
    assert _mod16(ei) == 8 and ei.is_contiguous()
    r = tt(g.normal(size=(n_edges, 2 * d)).astype(np.float32), device)
    eic = ids.view(2, n_edges).cpu()
    xo = vals.cpu().double().requires_grad_(True)
    (torch.cat([xo[eic[0]] - xo[eic[1]], xo[eic[0]] + xo[eic[1]]], dim=1) * r.cpu().double()).sum().backward()
    want = torch.cat([vals[ei[0]] - vals[ei[1]], vals[ei[0]] + vals[ei[1]]], dim=1)
    xf = vals.clone().requires_grad_(True)
    (ops.edge_features(xf, ei.clone()) * r).sum().backward()
    for cls, x, c in _x_views(vals):
        xd = x.detach().requires_grad_(True)
        f = ops.edge_features(xd, ei)
        _finite(f, "edge_features " + cls)
        assert torch.equal(f.detach().cpu(), want.cpu()), f"edge_features, x {cls}"
        (f * r).sum().backward()
        assert_close(xd.grad, xo.grad, TOL_GRAD, f"edge_features grad x, x {cls}")
        _same_bits(xd.grad, xf.grad, f"edge_features grad x, x {cls}")
        c.assert_surroundings_unchanged("edge_features x " + cls)
    ec.assert_surroundings_unchanged("edge_features edge_index")


def case_hinge_strided(device, n=120, dim=8, n_edges=700):
    """``ops_ml.hinge_terms`` with the two rows of the edge list ``stride(0) > n_edges`` apart (the kernel takes the
    row distance; ops_ml._HingeTerm), with a column-strided edge list (copied), and with ``x`` as a column window /
    transposed.  The fp64 expressions of case_hinge_terms at TOL_OUT / TOL_GRAD; the clone's results bit for bit."""
    from gnn_tracking_amd import ops_ml
    g = np.random.default_rng(1200)
    vals = tt((g.normal(size=(n, dim)) * 0.4).astype(np.float32), device)
    pid = tt(g.integers(0, 20, size=n), device).long()
    mask = tt(g.random(n) > 0.3, device)
    ids = tt(g.integers(0, n, size=(2, n_edges)), device).long()
    # (the kernels do not check ids: the poison is an id inside the range, which changes the loss if it is read)
    far = Carved(ids, stride=n_edges + 3, off=1, poison=n - 1)        # rows n_edges + 3 apart, 8 mod 16
    cols = Carved(ids.t().contiguous(), stride=3, off=0, poison=n - 1)   # [E, 2] in a stride of 3, read as its transpose
    lists = (("rows far apart", far.view), ("column stride 3", cols.view.t()))
    assert far.view.stride(0) == n_edges + 3 and far.view.stride(1) == 1 and _mod16(far.view) == 8
    assert lists[1][1].stride(1) == 3 and tuple(lists[1][1].shape) == (2, n_edges)
    idc = ids.cpu()
    for rep, p in ((False, 1.0), (False, 2.0), (True, 1.0), (True, 3.0)):
        xr = vals.cpu().double().requires_grad_(True)
        keep = mask.cpu()[idc[0]] & (pid.cpu()[idc[0]] != pid.cpu()[idc[1]])
        e = idc[:, keep]
        dist = torch.linalg.norm(xr[e[0]] - xr[e[1]], dim=-1)
        terms = torch.relu(0.9 - torch.pow(dist, p)) if rep else torch.pow(dist, p)
        lr = terms.sum() / (e.shape[1] + 1e-9)
        (lr * 1.5).backward()

        def run(x, edges):
            xd = x.detach().requires_grad_(True)
            l, cnt, _ = ops_ml.hinge_terms(xd, edges, node_mask=mask, particle_id=pid, r_emb=0.9, p=p, repulsive=rep)
            (l * 1.5).backward()
            return l.detach(), int(cnt), xd.grad

        l0, c0, g0 = run(vals.clone(), ids.clone())
        for xcls, x, xc in (("contiguous", vals, None),) + _x_views(vals):
            for ecls, edges in lists:
                tag = f"hinge rep {rep} p {p}: x {xcls}, edges {ecls}"
                l, cnt, gx = run(x, edges)
                assert cnt == e.shape[1] == c0, tag
                _finite(l, tag), _finite(gx, tag)
                assert_close(l, lr.detach(), TOL_OUT, tag + " loss")
                assert_close(gx, xr.grad, TOL_GRAD, tag + " grad")
                _same_bits(l, l0, tag + " loss"), _same_bits(gx, g0, tag + " grad")
    far.assert_surroundings_unchanged("hinge edges"), cols.assert_surroundings_unchanged("hinge edges")


def case_condensation_strided_x(device, cases=("td1", "td3")):
    """``CondensationLossRG`` / ``CondensationLossTiger`` on cluster coordinates that are a column window at +4 bytes
    and a transposed view, dense and spatial passes: the golden values and gradients at the bars of
    case_condensation_losses (TOL_OUT; 2e-4 for the gradients), and the clone's results bit for bit."""
    from gnn_tracking_amd import losses_oc
    z = load("g5_oc.npz")
    old = losses_oc.SPATIAL
    try:
        for cn in cases:
            t = {k: tt(z[f"{cn}/{k}"]) for k in ("beta", "x", "particle_id", "pt", "eta", "reconstructable")}
            vals = t["x"].float().to(device)
            for mode in ("off", "on"):
                losses_oc.SPATIAL = mode
                for strat, cls in (("tiger", losses_oc.CondensationLossTiger), ("rg", losses_oc.CondensationLossRG)):
                    got = {}
                    for xcls, xv, c in (("clone", vals.clone(), None),) + _x_views(vals):
                        b = t["beta"].float().to(device).requires_grad_(True)
                        x = xv.detach().requires_grad_(True)
                        ret = cls(lw_repulsive=2.0, lw_noise=0.5, lw_coward=0.25)(
                            beta=b, x=x, particle_id=t["particle_id"].to(device), reconstructable=t["reconstructable"].float().to(device),
                            pt=t["pt"].float().to(device), eta=t["eta"].float().to(device))
                        ret.loss.backward()
                        tag = f"{cn} {strat} spatial {mode} x {xcls}"
                        for k in ("attractive", "repulsive", "coward", "noise"):
                            assert_close(ret.loss_dct[k], z[f"{cn}/f32/{strat}/{k}"], TOL_OUT, f"{tag} {k}")
                        assert_close(ret.loss, z[f"{cn}/f32/{strat}/total"], TOL_OUT, tag + " total")
                        assert_close(x.grad, z[f"{cn}/f32/{strat}/grad_x"], 2e-4, tag + " grad x")
                        assert_close(b.grad, z[f"{cn}/f32/{strat}/grad_beta"], 2e-4, tag + " grad beta")
                        got[xcls] = (ret.loss.detach(), x.grad, b.grad)
                        if c is not None:
                            c.assert_surroundings_unchanged(tag)
                    for xcls, v in got.items():
                        for a, b_, nm in zip(v, got["clone"], ("loss", "grad x", "grad beta")):
                            _same_bits(a, b_, f"{cn} {strat} spatial {mode} x {xcls} {nm}")
    finally:
        losses_oc.SPATIAL = old


def _assert_valid_order(perm, rank, batch, what):
    n = perm.numel()
    p, r = perm.cpu().long(), rank.cpu().long()
    assert torch.equal(torch.sort(p).values, torch.arange(n)), what + ": perm is no permutation"
    assert torch.equal(r[p], torch.arange(n)), what + ": rank does not invert perm"
    if batch is not None:
        assert torch.equal(batch.cpu()[p], batch.cpu()), what + ": an event left its id range"


def _node_order_inputs(device, sizes):
    g = np.random.default_rng(1300)
    batch = torch.cat([torch.full((s,), i, dtype=torch.long) for i, s in enumerate(sizes)]).to(device)
    vals = tt(g.standard_normal((int(batch.numel()), 3)).astype(np.float32), device)
    vals[::7, 1] = 0.25
    return g, batch, vals


def case_node_order_layout(device):
    """``ops.node_order``: the key column read through the row stride of a column window at +4 bytes (the kernels take
    the stride), and of a transposed ``x`` (copied by the wrapper) - ``perm`` / ``rank`` as on the clone, exactly, for
    the radix forms and the counting-sort form; the full-key radix form also against the keys themselves."""
    sizes = (130, 1, 257)
    g, batch, vals = _node_order_inputs(device, sizes)
    N = int(batch.numel())
    forms = ((batch, 1, 0), (batch, 2, 200), (None, 2, 0), (batch, 1, len(sizes)))
    views = _x_views(vals)
    for b, col, n_ev in forms:
        p0, r0 = ops.node_order(vals.clone(), col, b, n_ev)
        _assert_valid_order(p0, r0, b, "node_order")
        for cls, x, c in views:
            if cls == "transposed" and n_ev == len(sizes):
                continue   # (the copy made by the wrapper is the clone's layout: one counting-sort launch is enough)
            tag = f"node_order x {cls} col {col} n_events {n_ev}"
            perm, rank = ops.node_order(x, col, b, n_ev)
            assert torch.equal(perm, p0) and torch.equal(rank, r0), tag + ": differs from the order of the clone"
        if b is not None and n_ev == 0:   # (the full-key radix form sorts by the exact key; the others by a quantised one)
            key, ev = vals[:, col].cpu()[p0.cpu().long()], b.cpu()
            assert bool(((key[1:] >= key[:-1]) | (ev[1:] != ev[:-1])).all()), "node_order: keys not ascending inside an event"
    for cls, x, c in views:
        c.assert_surroundings_unchanged("node_order x " + cls)


def case_graph_index_order_by_layout(device):
    """``ops.graph_index(order_by=(x, col, None))`` with ``x`` a column window at +4 bytes, the three builds: every
    array of the index, the node order included, as with the contiguous ``x``."""
    g, batch, vals = _node_order_inputs(device, (130, 1, 257))
    N = int(batch.numel())
    ei = tt(g.integers(0, N, size=(2, 901)), device).long()
    cls, x, c = _x_views(vals)[0]
    for flags in (0, 1, 2):
        gi = ops.graph_index(ei, N, cache=False, flags=flags, order_by=(x, 1, None))
        ref = ops.graph_index(ei, N, cache=False, flags=flags, order_by=(vals, 1, None))
        _check_graph_index(gi, gi.node_rank.cpu().long()[ei.cpu()], N, f"graph_index(order_by) x {cls} flags={flags}")
        for k in ("perm", "tgt", "src", "rowptr_t", "rowptr_s", "spos", "spos_inv", "node_perm", "node_rank"):
            assert torch.equal(getattr(gi, k), getattr(ref, k)), f"graph_index(order_by) x {cls} flags={flags}: {k}"


def case_node_order_extreme_keys(device):
    """Keys the plain node-order cases leave out, as VALIDITY checks only - ``perm`` is a permutation,
    ``rank`` inverts it, events keep their id ranges; the order inside such an event is not pinned (the quantised
    key is known to lose locality there): +-inf keys, and key ranges whose ``hi - lo`` overflows fp32 (the scale of
    the quantised key becomes 0 or NaN).  Every form of the sort; contiguous ``x`` and a column window."""
    sizes = (130, 257)
    g, batch, vals = _node_order_inputs(device, sizes)
    big = float(np.finfo(np.float32).max)
    for name, edits in (("+-inf keys", ((slice(3, None, 11), float("inf")), (slice(5, None, 13), float("-inf")))),
                        ("hi - lo overflows", ((slice(2, None, 9), big), (slice(4, None, 9), -big), (slice(1, None, 17), float("inf"))))):
        xs = vals.clone()
        for where, v in edits:
            xs[where, 1] = v
        for cls, x in (("contiguous", xs), ("window+4B", _x_views(xs)[0][1])):
            forms = ((batch, 1, 0), (batch, 1, 200), (None, 1, 1)) + (((batch, 1, len(sizes)), (None, 1, 0)) if cls == "contiguous" else ())
            for b, col, n_ev in forms:
                perm, rank = ops.node_order(x, col, b, n_ev)
                _assert_valid_order(perm, rank, b, f"node_order {name}, x {cls}, n_events {n_ev}")


# ------------------------------------------------------------------------------------------ bf16 MLP forward / backward
MLP_ROWS = (1, 2, 3, 31, 32, 33, 75)
_T, _F = True, False
#: the three launch shapes of the edge classifier, as case_mlp_bf16_forward / _backward build them:
#: (segment dims, gathered?, relu?, hidden, out, L, bias, epilogue, upstream terms)
MLP16_SHAPES = {
    "relational": ((5, 5, 4), (_T, _T, _F), (_T, _T, _T), 40, 4, 3, True, "none", 2),
    "object": ((5, 4), (_F, _F), (_F, _F), 40, 5, 3, True, "residual", 1),
    "head": ((5, 5, 4, 4, 4, 4), (_T, _T, _F, _F, _F, _F), (_F,) * 6, 40, 1, 3, True, "sigmoid", 1),
}


class _KernelNames:
    """records what ``gnntrk_mlp_forward_bf16_kernel_name`` / ``..._backward_bf16_kernel_name`` answer for the very
    argument structs the wrappers launch with"""

    def __init__(self):
        self.fwd, self.bwd = [], []

    def __enter__(self):
        lib = self.lib = _capi.load()
        self.orig = (lib.gnntrk_mlp_forward_bf16, lib.gnntrk_mlp_backward_bf16)

        def name(probe, args):
            buf = C.create_string_buffer(200)
            _capi.check(probe(args, buf, len(buf)), lib)
            return buf.value.decode()

        def fwd(args, stream):
            self.fwd.append(name(lib.gnntrk_mlp_forward_bf16_kernel_name, args))
            return self.orig[0](args, stream)

        def bwd(args, ws, nbytes, stream):
            self.bwd.append(name(lib.gnntrk_mlp_backward_bf16_kernel_name, args))
            return self.orig[1](args, ws, nbytes, stream)

        lib.gnntrk_mlp_forward_bf16, lib.gnntrk_mlp_backward_bf16 = fwd, bwd
        return self

    def __exit__(self, *exc):
        self.lib.gnntrk_mlp_forward_bf16, self.lib.gnntrk_mlp_backward_bf16 = self.orig


def _carved_rows16(vals, off, stride=None):
    """bf16 ``[n, d]`` kernel rows (zero padding columns, as every producer of the library writes them) at ``off``
    elements into a NaN buffer; the last row is the last row of the buffer's payload, poison right behind it"""
    n, d = vals.shape
    padded = torch.zeros(n, B.pad4(d), dtype=torch.bfloat16, device=vals.device)
    padded[:, :d] = vals
    c = Carved(padded, stride, off)
    v = c.view[:, :d]
    assert B.rows16(v) is v, "not a kernel-ready row tensor"
    return v, c


def case_mlp_bf16_layout(device, shape, rows):
    """``gnntrk_mlp_forward_bf16`` / ``gnntrk_mlp_backward_bf16``, relational-, object- and head-shaped launches built
    as the instantiation table of parity_cases builds them (one node tensor gathered twice, tensors of the tile's
    rows, the source-side slice leaving through a row permutation).  The forward's wide loads (one 16-byte ``row16``
    / ``pair8`` load per lane and k-step, ``wide_ok``) need every segment pointer 16-byte aligned and, for ``pair8``,
    ``n_rows >= 2``; the backward's buffer-addressed classes need the 16-byte rows 16-byte aligned (``make_buf_plan``:
    ``row16``), else the launch takes the generic I/O.  One tensor at a time starts on an odd row of a stride-4
    buffer / at +8 bytes (8 mod 16): the node tensor, each tile tensor, the residual rows, each upstream term; then
    all of them; then the 16-byte rows alone, aligned, inside a 12-wide buffer (``stride % 8 != 0``: no ``row16``).  Odd row counts end with the last row of their buffer, NaN behind it (``pair_cap`` clamps the last
    pair of an odd-length ``pair8`` tensor; a lane that over-read it would mask the surplus half, so the poison
    shows a misplaced half, not the over-read itself); the gathered node tensor has an odd number of rows and its
    last row is used.

    Forward outputs and the per-row gradient slices equal those of the aligned launch bit for bit (a row's result
    does not depend on the width of its loads), and the oracle at TOL16 (TOL16_SIG for the head).  The weight and
    bias gradients equal the aligned launch's bit for bit (the rule of case_bf16_reproducible) where the backward
    kernel is the same; where the launch falls from a buffer-addressed class to the generic I/O it is another
    instantiation with its own grid, the per-wave partial sums are taken over other tiles, and only the oracle's bar
    holds (as bf16_instantiation_answers states it for the two I/O forms).

    Probes.  Forward: ``..., true>`` (wide) for the aligned relational and object launches of two or more rows,
    ``..., false>`` once a segment is 8 mod 16 or its 16-byte rows lie at a stride of 12; one row and the head (its chunk pairs join two segments) answer
    ``false`` either way.  Backward: the shape's buffer-addressed class while its 16-byte rows are aligned, ``IoNone``
    once they are not (or their stride is no power of two); 8-byte rows, the residual rows and the upstream terms at 8 mod 16 do not change it."""
    from parity_cases import TOL16_SIG, assert_rows_close
    dims, gath, relu, hid, out, L, bias, epi, n_gout = MLP16_SHAPES[shape]
    gen = torch.Generator().manual_seed(1400 + rows)
    torch.manual_seed(1400 + rows)
    n_src = 31
    epi_code = {"none": _capi.EPI_NONE, "residual": _capi.EPI_RESIDUAL, "sigmoid": _capi.EPI_SIGMOID}[epi]
    rnd16 = lambda n, d: torch.randn(n, d, generator=gen).to(torch.bfloat16).to(device)   # noqa: E731
    ids = lambda: torch.randint(0, n_src, (rows,), generator=gen)                          # noqa: E731
    # the tensors of the launch by name, and which of them each segment / term reads
    vals, seg_of, idxs, gidx = {}, [], [], [None] * len(dims)
    if shape == "object":
        for j, d in enumerate(dims):
            vals[f"tile{j}"] = rnd16(rows, d)
            seg_of.append(f"tile{j}")
            idxs.append(None)
        wide16 = ("tile0",)
    else:
        vals["x"] = rnd16(n_src, dims[0])
        tgt, src = torch.sort(ids()).values, ids()
        src[rows // 2] = n_src - 1   # (the odd last row of the node tensor is used)
        tgt[-1] = n_src - 1
        first, second = (tgt, src) if shape == "relational" else (src, tgt)
        seg_of, idxs = ["x", "x"], [first.int().to(device), second.int().to(device)]
        for j, d in enumerate(dims[2:]):
            vals[f"tile{j}"] = rnd16(rows, d)
            seg_of.append(f"tile{j}")
            idxs.append(None)
        gidx[1 if shape == "relational" else 0] = torch.randperm(rows, generator=gen).int().to(device)
        wide16 = ("x",)
    m = G.MLP(sum(dims), out, hid, L=L, bias=bias)
    weights = [l.weight.detach() for l in m.linears()]
    biases = [l.bias.detach() if bias else None for l in m.linears()]
    wd = [w.to(device).contiguous() for w in weights]
    bd = [None if b is None else b.to(device).contiguous() for b in biases]
    ca, cb = (0.6, 0.8) if epi == "residual" else ((0.001, 0.998) if epi == "sigmoid" else (0.0, 1.0))
    if epi == "residual":
        vals["res"] = rnd16(rows, out)
    out_idx = torch.randperm(rows, generator=gen).int().to(device) if epi == "sigmoid" else None
    if epi == "sigmoid":
        g32 = torch.randn(rows, out, generator=gen).to(device)
        g_sum, terms = g32.cpu(), []
    else:
        vals["gout0"] = rnd16(rows, out)
        terms, g_sum = [("gout0", None)], vals["gout0"].float().cpu()
        if n_gout == 2:   # the aggregation's share, gathered through the target ids
            vals["gout1"] = rnd16(n_src, out)
            terms.append(("gout1", idxs[0]))
            g_sum = g_sum + vals["gout1"].float().cpu()[idxs[0].cpu().long()]
    # oracle
    raw = [vals[nm].float().cpu() if ix is None else vals[nm].float().cpu()[ix.cpu().long()] for nm, ix in zip(seg_of, idxs)]
    xin = torch.cat([torch.relu(v) if r else v for v, r in zip(raw, relu)], 1)
    z, _ = O.mlp_bf16_forward(xin, weights, biases)
    yo = O.mlp_bf16_epilogue(z, epi, ca, cb, vals["res"].float().cpu() if epi == "residual" else None)
    if out_idx is not None:
        tmp = torch.empty_like(yo)
        tmp[out_idx.cpu().long()] = yo
        yo = tmp
    gin, dW, db = O.mlp_bf16_backward(xin, weights, biases, g_sum, epi, ca, cb)
    io_class = {"relational": "IoRelational<2, false> >", "object": "IoObject>", "head": "IoHeadT<false> >"}[shape]

    base = None
    variants = [("aligned", (), 0)] + [(t + "+8B", (t,), 0) for t in vals] + [("all+8B", tuple(vals), 0)]
    variants.append((wide16[0] + " stride 12", (wide16[0],), 12))   # 16-byte rows, aligned, at a stride % 8 != 0
    for vname, moved, stride in variants:
        tag = f"bf16 MLP {shape} rows={rows} {vname}"
        placed, carved = {}, []
        for nm, v in vals.items():
            off = 4 if nm in moved and not stride else 0
            placed[nm], c = _carved_rows16(v, off, stride if nm in moved and stride else None)
            assert placed[nm].data_ptr() % 16 == 2 * off and c.geom[1][0] == (stride if nm in moved and stride else B.pad4(v.shape[1])), tag
            carved.append(c)
        segs = [placed[nm] for nm in seg_of]
        gout = [(placed[nm], ix) for nm, ix in terms] if terms else [(g32, None)]
        mlp = ops._fill_mlp(wd, bd)
        with _KernelNames() as names:
            y = B.mlp_forward_raw(segs, idxs, relu, wd, bd, n_rows=rows, epilogue=epi_code, ca=ca, cb=cb, res=placed.get("res"),
                                  out_idx=out_idx, out_rows=rows, mlp=mlp)
            slices, gW, gb = B.mlp_backward_raw(segs, idxs, relu, wd, bd, n_rows=rows, epilogue=epi_code, ca=ca, cb=cb,
                                                gout=gout, need_seg=[True] * len(dims), want_dw=True, mlp=mlp, gidx=gidx)
        for c in carved:
            c.assert_surroundings_unchanged(tag)
        _finite(y, tag)
        assert_close(y.float(), yo, TOL16_SIG if epi == "sigmoid" else TOL16, tag)
        col = 0
        for j, d in enumerate(dims):
            want = gin[:, col:col + d] * ((raw[j] > 0) if relu[j] else 1.0)
            got_j = slices[j] if gidx[j] is None else slices[j][gidx[j].long()]
            assert_rows_close(got_j.float(), want, TOL16, f"{tag} gseg{j}")
            col += d
        for i in range(L):
            assert_close(gW[i], dW[i], TOL16, f"{tag} gW{i}")
            assert_close(gb[i], db[i], TOL16, f"{tag} gb{i}")
        rowwise = dict(y=y, **{f"gseg{j}": sl for j, sl in enumerate(slices)})
        params = dict(**{f"gW{i}": w for i, w in enumerate(gW)}, **{f"gb{i}": b_ for i, b_ in enumerate(gb)})
        fwd_name, bwd_name = names.fwd[0], names.bwd[0]
        if base is None:
            base = (rowwise, params, fwd_name, bwd_name)
            assert fwd_name.endswith("true>") == (shape != "head" and rows >= 2), f"{tag}: forward kernel {fwd_name}"
            assert bwd_name.endswith(io_class), f"{tag}: backward kernel {bwd_name}"
            continue
        for k, v in rowwise.items():
            _same_bits(v, base[0][k], f"{tag} {k}")
        seg_moved = any(t == "x" or t.startswith("tile") for t in moved)
        want_fwd = base[2][:-len("true>")] + "false>" if base[2].endswith("true>") and seg_moved else base[2]
        assert fwd_name == want_fwd, f"{tag}: forward kernel {fwd_name}, aligned {base[2]}"
        want_bwd = base[3][:-len(io_class)] + "IoNone>" if any(t in wide16 for t in moved) else base[3]
        assert bwd_name == want_bwd, f"{tag}: backward kernel {bwd_name}, aligned {base[3]}"
        if bwd_name == base[3]:
            for k, v in params.items():
                _same_bits(v, base[1][k], f"{tag} {k}")


# ------------------------------------------------------------------------------------------ wide fp32 MLP
#: tensors of a wide launch that can each leave the 16-byte / stride % 4 class on their own
MLP_WIDE_DIMS, MLP_WIDE_HIDDEN, MLP_WIDE_OUT = (8, 4, 4), 40, 8


def case_mlp_wide_layout(device, rows, epi_name):
    """``gnntrk_mlp_forward_wide`` / ``_backward_wide``: ``vec4`` (float4 input loads and gradient-slice stores: every
    segment and gradient slice 16-byte aligned, widths and strides multiples of 4) and ``vec4o`` (float4 output side:
    ``out``, ``res``, the upstream terms, the forward's output read by the RELU backward).  All widths are multiples
    of 4, so only a pointer or a stride decides: one launch per tensor with that tensor alone at +4 bytes, and one
    with it alone at a stride that is no multiple of 4 - segments, ``out``, ``res``, the upstream term, each gradient
    slice.  The caller's ``out`` and gradient slices lie in poisoned buffers: the bytes around them stay.

    Against the fp64 MLP of case_mlp_wide (TOL_OUT; TOL_GRAD for every gradient), and against the aligned launch bit
    for bit: the two forms differ in access width only, the launch grid does not depend on them."""
    lib = _capi.load()
    dims, hid, dout, L = MLP_WIDE_DIMS, MLP_WIDE_HIDDEN, MLP_WIDE_OUT, 3
    epi = {"relu": _capi.EPI_RELU, "residual": _capi.EPI_RESIDUAL}[epi_name]
    gen = torch.Generator().manual_seed(1500 + rows)
    n_src = 9
    idx0 = torch.randint(0, n_src, (rows,), generator=gen).int()
    idx0[rows // 2] = n_src - 1
    vals = {"seg0": torch.randn(n_src, dims[0], generator=gen), "seg1": torch.randn(rows, dims[1], generator=gen),
            "seg2": torch.randn(rows, dims[2], generator=gen), "gout": torch.randn(rows, dout, generator=gen)}
    if epi == _capi.EPI_RESIDUAL:
        vals["res"] = torch.randn(rows, dout, generator=gen)
    relu = (True, False, True)
    sizes = [sum(dims), hid, hid, dout]
    Ws = [torch.randn(sizes[i + 1], sizes[i], generator=gen) / sizes[i] ** 0.5 for i in range(L)]
    bs = [torch.randn(sizes[i + 1], generator=gen) * 0.3 for i in range(L)]
    ca, cb = 0.6, 0.8
    # fp64 reference: per-row gradients of the (gathered) segment rows
    T = [(vals["seg0"][idx0.long()], vals["seg1"], vals["seg2"])[j].double().clone().requires_grad_(True) for j in range(3)]
    Wr = [w.double().clone().requires_grad_(True) for w in Ws]
    br = [b.double().clone().requires_grad_(True) for b in bs]
    h = torch.cat([torch.relu(t) if r else t for t, r in zip(T, relu)], dim=1)
    for i in range(L):
        h = h @ Wr[i].t() + br[i]
        if i < L - 1:
            h = torch.relu(h)
    yr = torch.relu(h) if epi == _capi.EPI_RELU else ca * vals["res"].double() + cb * h
    (yr * vals["gout"].double()).sum().backward()
    W = [w.to(device).contiguous() for w in Ws]
    b = [v.to(device).contiguous() for v in bs]
    idx_d = idx0.to(device)
    outs = {"out": dout, "gseg0": dims[0], "gseg1": dims[1], "gseg2": dims[2]}   # caller-owned outputs: name -> width
    names = list(vals) + list(outs)
    variants = [("aligned", None, 0, 0)] + [(f"{nm}+4B", nm, 1, 0) for nm in names] + [(f"{nm} stride+1", nm, 0, 1) for nm in names]
    base = None
    for vname, moved, off, extra in variants:
        tag = f"mlp_wide rows={rows} {epi_name} {vname}"
        c = {}
        for nm, v in vals.items():
            c[nm] = Carved(v.to(device), v.shape[1] + (extra if nm == moved else 0), off if nm == moved else 0)
        for nm, wdt in outs.items():
            c[nm] = Carved(torch.zeros(rows, wdt, device=device), wdt + (extra if nm == moved else 0), off if nm == moved else 0)
        for nm in names:
            mis = nm == moved
            assert _mod16(c[nm].view) == (4 * off if mis else 0) and c[nm].geom[1][0] % 4 == (extra if mis else 0), tag
        st = lambda nm: c[nm].geom[1][0]   # noqa: E731
        a = _capi.MlpFwdArgs()
        a.mlp = ops._fill_mlp(W, b)
        a.n_seg, a.epilogue, a.n_rows, a.ca, a.cb = 3, epi, rows, ca, cb
        segs = [_capi.Seg(c[f"seg{j}"].view.data_ptr(), idx_d.data_ptr() if j == 0 else None, dims[j], st(f"seg{j}"), int(relu[j]), 0)
                for j in range(3)]
        for j in range(3):
            a.seg[j] = segs[j]
        if epi == _capi.EPI_RESIDUAL:
            a.res, a.res_stride = c["res"].view.data_ptr(), st("res")
        a.out, a.out_stride = c["out"].view.data_ptr(), st("out")
        hp = int(lib.gnntrk_mlp_wide_hidden_pad(hid))
        acts = torch.empty(L - 1, rows, hp, dtype=torch.float32, device=device)
        ws = ops._ws(lib.gnntrk_mlp_wide_forward_workspace_bytes(C.byref(a.mlp)), acts)
        stream = ops._stream(acts)
        _capi.check(lib.gnntrk_mlp_forward_wide(C.byref(a), ops._p(acts), ops._p(ws), ws.numel(), stream), lib)
        g = _capi.MlpBwdArgs()
        g.mlp = a.mlp
        g.n_seg, g.epilogue, g.n_rows, g.ca, g.cb, g.n_gout = 3, epi, rows, ca, cb, 1
        for j in range(3):
            g.seg[j] = segs[j]
            g.gseg[j] = _capi.GSeg(c[f"gseg{j}"].view.data_ptr(), None, st(f"gseg{j}"), 0)
        g.gout[0] = _capi.GTerm(c["gout"].view.data_ptr(), None, st("gout"), 0)
        gW, gb = [torch.empty_like(w) for w in W], [torch.empty_like(v) for v in b]
        for i in range(L):
            g.gW[i], g.gb[i] = gW[i].data_ptr(), gb[i].data_ptr()
        ws2 = ops._ws(lib.gnntrk_mlp_wide_backward_workspace_bytes(C.byref(g.mlp), rows), acts)
        fwd_out = c["out"].view if epi == _capi.EPI_RELU else None
        _capi.check(lib.gnntrk_mlp_backward_wide(C.byref(g), ops._p(acts), ops._p(fwd_out), st("out") if fwd_out is not None else 0,
                                                 ops._p(ws2), ws2.numel(), stream), lib)
        for nm in names:
            c[nm].assert_surroundings_unchanged(f"{tag}: {nm}")
        got = {"out": c["out"].view, **{f"gseg{j}": c[f"gseg{j}"].view for j in range(3)},
               **{f"gW{i}": gW[i] for i in range(L)}, **{f"gb{i}": gb[i] for i in range(L)}}
        for k, v in got.items():
            _finite(v, f"{tag} {k}")
        assert_close(got["out"], yr, TOL_OUT, tag + " y")
        for j in range(3):
            assert_close(got[f"gseg{j}"], T[j].grad, TOL_GRAD, f"{tag} grad seg {j}")
        for i in range(L):
            assert_close(gW[i], Wr[i].grad, TOL_GRAD, f"{tag} grad W{i}")
            assert_close(gb[i], br[i].grad, TOL_GRAD, f"{tag} grad b{i}")
        if base is None:
            base = {k: v.clone() for k, v in got.items()}
        for k, v in got.items():
            _same_bits(v, base[k], f"{tag} {k}")
