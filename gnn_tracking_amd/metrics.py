"""Figures of merit of edge classification, computed on the device
(``metrics/binary_classification.py`` and the validation step of ``training/ec.py:55-87``).

The reference evaluates ``BinaryClassificationStats`` at 200 thresholds per pt cut (about ten passes
over the masked edges and four to six host syncs each) and sorts the scores three times per cut for
torchmetrics' ``BinaryAUROC``.  Here the whole threshold scan is one histogram pass
(``gnntrk_bcs_counts``) and every AUC one radix sort plus integer scans (``gnntrk_roc_auc``); the host
reads a few KB once and finishes with the reference's own formulas:

* counts give TP / TN / FP / FN as exact integers; the rates, F1 and MCC are evaluated with the
  reference's expressions in float64 and collected in the dtype ``torch.asarray`` gives the reference's
  list of results - float64 as soon as one MCC denominator is non-zero (``np.sqrt`` makes it a numpy
  float64), float32 otherwise - before the first-occurrence ``argmax`` / ``argmin``;
* AUC = U2 / (2 P N) from an exact integer numerator; partial AUCs interpolate the crossing tie group
  linearly and standardise (McClish) in float64 as ``sklearn.metrics.roc_auc_score`` does.  A pt cut
  with one class only, or with a NaN score, gives NaN (the reference's wrapper turns the exception of
  the AUC into NaN).

When ``W`` is a model output still held in CSR order (``edge_order.EdgeOrdered``) for the graph of
``edge_index``, the metrics run on the CSR values, with the labels gathered through the graph index's
permutation: ``W`` is never scattered back into ``edge_index`` order.
"""

from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional

import numpy as np
import torch
from torch import Tensor

from . import _capi, ops
from .edge_order import as_tensor

__all__ = ["BinaryClassificationStats", "bcs_from_counts", "zero_divide", "get_maximized_bcs", "roc_auc_score",
           "get_roc_auc_scores", "ec_validation_metrics", "denote_pt"]


def zero_divide(a: float, b: float) -> float:
    """Normal division a/b but return 0 for x/0 (binary_classification.py:135-139)"""
    if b == 0:
        return 0
    return a / b


def denote_pt(inpt, pt_min=0.0):
    """``utils/nomenclature.py:denote_pt``: suffix ``_pt{pt_min:.1f}`` unless ``pt_min`` is 0."""
    suffix = "" if np.isclose(pt_min, 0.0) else f"_pt{pt_min:.1f}"
    if isinstance(inpt, str):
        return f"{inpt}{suffix}"
    if isinstance(inpt, dict):
        return {denote_pt(k, pt_min=pt_min): v for k, v in inpt.items()}
    raise ValueError(f"Cannot denote_pt for type {type(inpt)}.")


# ------------------------------------------------------------------ device inputs
class _Edges:
    """Pointers of one edge set for the metrics entries: scores, labels (through ``perm``), the two
    node ids of each edge and per-node pt - in CSR order when ``w`` is an EdgeOrdered output of the
    graph of ``edge_index`` (no scatter of ``w``), else in the caller's order."""

    def __init__(self, w, y: Tensor, pt: Optional[Tensor], edge_index: Optional[Tensor]):
        fast = ops._csr_fast_path(w, edge_index)
        self.perm = None
        if fast is not None:
            w_csr, gi = fast
            self.w = w_csr.detach()
            self.perm = gi.perm
            self.src, self.tgt, self.ids_i64 = gi.src, gi.tgt, 0
            if pt is not None:
                pt = gi.node_values(pt.detach().to(torch.float32)).contiguous()
        else:
            self.w = as_tensor(w).detach()
            self.src = self.tgt = None
            self.ids_i64 = 1
            if pt is not None:
                if edge_index is None:
                    raise ValueError("pt cuts need edge_index")
                ei = edge_index.detach().to(torch.int64)
                self.src, self.tgt = ei[0].contiguous(), ei[1].contiguous()
                pt = pt.detach().to(torch.float32).contiguous()
        self.w = self.w.reshape(-1)
        if self.w.dtype != torch.float32:
            self.w = self.w.to(torch.float32)
        self.w = self.w.contiguous()
        self.pt = pt
        y = y.detach().reshape(-1)
        _capi.require_device(self.w, y, self.pt, self.src, self.tgt)
        if y.dtype in (torch.bool, torch.uint8):
            self.y, self.y_kind = y.contiguous().view(torch.uint8), 0
        elif y.dtype == torch.float32:
            self.y, self.y_kind = y.contiguous(), 1
        else:   # (y.int() == 1 of any other dtype, as one byte)
            self.y, self.y_kind = (y.int() == 1).view(torch.uint8), 0
        self.n = self.w.numel()
        if self.y.numel() != self.n:
            raise ValueError(f"labels have {self.y.numel()} entries, the scores {self.n}")

    def args(self):
        p = ops._p
        return (p(self.w), p(self.y), self.y_kind, p(self.perm), p(self.src), p(self.tgt), self.ids_i64, p(self.pt))


def _cut_array(cuts):
    return (C.c_float * len(cuts))(*[float(c) for c in cuts])


def _launch_counts(e: _Edges, cuts, thr: Tensor, out: Tensor) -> None:
    lib = _capi.load()
    _capi.check(lib.gnntrk_bcs_counts(*e.args(), _cut_array(cuts), len(cuts), ops._p(thr), thr.numel(), e.n,
                                      ops._p(out), ops._stream(e.w)), lib)


def _launch_auc(e: _Edges, cuts, fprs, out: Tensor) -> None:
    lib = _capi.load()
    ws = ops._ws(lib.gnntrk_roc_auc_workspace_bytes(e.n), e.w)
    fa = (C.c_double * max(1, len(fprs)))(*[float(f) for f in fprs])
    _capi.check(lib.gnntrk_roc_auc(*e.args(), _cut_array(cuts), len(cuts), fa, len(fprs), e.n, ops._p(out),
                                   ops._p(ws), ws.numel(), ops._stream(e.w)), lib)


def _threshold_table(thlds: Tensor, device) -> Tensor:
    t = thlds.detach().reshape(-1).to(torch.float32)
    if t.numel() > _capi.METRICS_MAX_THR:
        raise ValueError(f"at most {_capi.METRICS_MAX_THR} thresholds, got {t.numel()}")
    if t.numel() > 1 and not bool((t[1:] >= t[:-1]).all()):
        raise ValueError("the thresholds must ascend")
    return t.to(device)


# --------------------------------------------------------------- host finishing
def _rates(tp: np.ndarray, fp: np.ndarray, P: int, N: int):
    """``BinaryClassificationStats`` of every threshold from exact integer counts: ba, F1, TPR, TNR, MCC
    (float64 arrays, the reference's expressions and zero_divide) and whether any MCC is a numpy
    float64 (non-zero denominator)."""
    tp = tp.astype(np.int64)
    fp = fp.astype(np.int64)
    fn, tn = P - tp, N - fp

    def zdiv(a, b):
        b = np.asarray(b, dtype=np.float64)
        return np.where(b == 0, 0.0, np.asarray(a, dtype=np.float64) / np.where(b == 0, 1.0, b))

    tpr, tnr = zdiv(tp, tp + fn), zdiv(tn, tn + fp)
    ba = (tpr + tnr) / 2
    f1 = zdiv(2 * tp, 2 * tp + fp + fn)
    # (TP + FP)(TP + FN)(TN + FP)(TN + FN) exceeds int64: exact in Python integers, rounded once by float()
    den = np.sqrt(np.array([float(a * b * c * d) for a, b, c, d in
                            zip((tp + fp).tolist(), (tp + fn).tolist(), (tn + fp).tolist(), (tn + fn).tolist())],
                           dtype=np.float64))
    mcc = zdiv(tp * tn - fp * fn, den)
    return np.stack([ba, f1, tpr, tnr, mcc]), bool((den != 0).any())


def _maximized(tp: np.ndarray, fp: np.ndarray, P: int, N: int, thlds: Tensor) -> dict[str, float]:
    """The tail of ``get_maximized_bcs`` (binary_classification.py:167-195) on the rates of every threshold."""
    rows, any_np64 = _rates(tp, fp, P, N)
    # torch.asarray of the reference's list: float64 if one MCC came out of np.sqrt, else the default dtype
    results = torch.from_numpy(rows).to(torch.float64 if any_np64 else torch.get_default_dtype())
    bas, f1s, tprs, tnrs, mccs = results
    r_diff = torch.abs(tprs - tnrs)
    min_diff_idx = torch.argmin(r_diff)
    tpr_eq_tnr = (tprs[min_diff_idx] + tnrs[min_diff_idx]) / 2
    dct = {}
    for key, vals in (("max_ba", bas), ("max_f1", f1s), ("max_mcc", mccs)):
        max_idx = torch.argmax(vals)
        dct[key] = vals[max_idx].item()
        dct[f"{key}_loc"] = thlds[max_idx].item()
    dct["tpr_eq_tnr"] = tpr_eq_tnr.item()
    dct["tpr_eq_tnr_loc"] = thlds[min_diff_idx].item()
    return dct


def _thresholds_from_counts(counts: np.ndarray):
    """counts [2, n_thr + 1] -> (TP, FP) per threshold j = edges with bin > j; P, N."""
    pos_gt = np.cumsum(counts[1, ::-1])[::-1]   # pos_gt[k] = sum over bins >= k
    neg_gt = np.cumsum(counts[0, ::-1])[::-1]
    return pos_gt[1:], neg_gt[1:], int(pos_gt[0]), int(neg_gt[0])


def _auc_from_row(row: np.ndarray, fprs) -> list[float]:
    """AUC and partial AUCs of one cut from the integers of gnntrk_roc_auc (sklearn's _binary_roc_auc_score)."""
    P, N, U2, n_nan = (int(v) for v in row[:4])
    if n_nan or P == 0 or N == 0:
        return [float("nan")] * (1 + len(fprs))
    full = U2 / (2 * P * N)
    res = [full]
    for m, f in enumerate(fprs):
        if f == 1:
            res.append(full)
            continue
        fp_lim, u2p, tpb, fpb, tpg, fpg = (int(v) for v in row[4 + 6 * m: 10 + 6 * m])
        x0, x1 = fpb / N, (fpb + fpg) / N
        y0, y1 = tpb / P, (tpb + tpg) / P
        y_interp = float(np.interp(f, [x0, x1], [y0, y1]))
        pauc = u2p / (2 * P * N) + (f - x0) * (y0 + y_interp) / 2
        min_area = 0.5 * f ** 2
        res.append(0.5 * (1 + (pauc - min_area) / (f - min_area)))
    return res


def bcs_from_counts(TP: int, FP: int, P: int, N: int) -> dict[str, float]:
    """``BinaryClassificationStats.get_all()`` (binary_classification.py:14-132) from the exact counts of one
    threshold: true and false positives, positives ``P`` and negatives ``N``, as Python ints.  The reference's
    expressions with ``zero_divide``; the class and the EC threshold scan (``graph_analysis.ec_threshold_scan``) share
    them."""
    FN, TN = P - TP, N - FP
    TPR, TNR = zero_divide(TP, TP + FN), zero_divide(TN, TN + FP)
    return {"acc": zero_divide(TP + TN, TP + TN + FP + FN), "TPR": TPR, "TNR": TNR, "FPR": zero_divide(FP, FP + TN),
            "FNR": zero_divide(FN, FN + TP), "balanced_acc": (TPR + TNR) / 2, "F1": zero_divide(2 * TP, 2 * TP + FP + FN),
            "MCC": zero_divide(TP * TN - FP * FN, np.sqrt(float((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN)))),
            "n_true": P, "n_false": N, "n_predicted_true": TP + FP, "n_predicted_false": TN + FN}


# ---------------------------------------------------------------------- public API
class BinaryClassificationStats:
    def __init__(self, output: Tensor, y: Tensor, thld: Tensor | float):
        """Calculator for binary classification metrics (binary_classification.py:14-132): one counts
        launch at the single threshold and one host copy, on first use of any property.

        Args:
            output: Output weights
            y: True labels
            thld: Threshold to consider something true
        """
        self._output, self._y, self._thld = output, y, thld
        self._c = None

    def _counts(self):
        if self._c is None:
            e = _Edges(self._output, self._y, None, None)
            thr = _threshold_table(torch.as_tensor(self._thld, dtype=torch.float32), e.w.device)
            out = torch.empty(2 * (thr.numel() + 1), dtype=torch.int64, device=e.w.device)
            _launch_counts(e, (0.0,), thr, out)
            tp, fp, P, N = _thresholds_from_counts(out.cpu().numpy().reshape(2, -1))
            self._c = (int(tp[0]), int(fp[0]), P, N)
        return self._c

    @property
    def n_true(self) -> int:
        return self._counts()[2]

    @property
    def n_false(self) -> int:
        return self._counts()[3]

    @property
    def TP(self) -> int:
        return self._counts()[0]

    @property
    def FP(self) -> int:
        return self._counts()[1]

    @property
    def FN(self) -> int:
        return self.n_true - self.TP

    @property
    def TN(self) -> int:
        return self.n_false - self.FP

    def get_all(self) -> dict[str, float]:
        return bcs_from_counts(*self._counts())


def _bcs_property(key):
    return property(lambda self: self.get_all()[key])


for _key in ("n_predicted_true", "n_predicted_false", "acc", "TPR", "TNR", "FPR", "FNR", "balanced_acc", "F1", "MCC"):
    setattr(BinaryClassificationStats, _key, _bcs_property(_key))


def get_maximized_bcs(*, output: Tensor, y: Tensor, n_samples=200) -> dict[str, float]:
    """The best binary classification stats over ``torch.linspace(0.0, 1.0, n_samples)``
    (binary_classification.py:147-195): one counts launch, one host copy."""
    thlds = torch.linspace(0.0, 1.0, n_samples)
    e = _Edges(output, y, None, None)
    out = torch.empty(2 * (n_samples + 1), dtype=torch.int64, device=e.w.device)
    _launch_counts(e, (0.0,), _threshold_table(thlds, e.w.device), out)
    tp, fp, P, N = _thresholds_from_counts(out.cpu().numpy().reshape(2, -1))
    return _maximized(tp, fp, P, N, thlds)


def roc_auc_score(*, y_true: Tensor, y_score: Tensor, max_fpr: float | None = None, device=None) -> float:
    """ROC AUC (``max_fpr``: McClish-standardised partial AUC) of the scores; NaN where the reference's
    wrapper returns NaN (one class only, NaN scores).  ``device`` is accepted for the reference's
    signature; the computation runs where the scores are."""
    fprs = () if max_fpr is None else (float(max_fpr),)
    e = _Edges(y_score, y_true, None, None)
    out = torch.empty(_capi.AUC_STRIDE, dtype=torch.int64, device=e.w.device)
    _launch_auc(e, (0.0,), fprs, out)
    return _auc_from_row(out.cpu().numpy(), fprs)[-1 if fprs else 0]


def get_roc_auc_scores(true, predicted, max_fprs: Iterable[float | None]):
    """Calculate ROC AUC scores for a given set of maximum FPRs (one sort for all of them)."""
    max_fprs = list(max_fprs)
    fprs = [float(f) for f in max_fprs if f is not None]
    e = _Edges(predicted, true, None, None)
    out = torch.empty(_capi.AUC_STRIDE, dtype=torch.int64, device=e.w.device)
    _launch_auc(e, (0.0,), fprs, out)
    vals = _auc_from_row(out.cpu().numpy(), fprs)
    metrics = {}
    if None in max_fprs:
        metrics["roc_auc"] = vals[0]
    for f, v in zip([f for f in max_fprs if f is not None], vals[1:]):
        metrics[f"roc_auc_{f}FPR"] = v
    return metrics


def ec_validation_metrics(w, y: Tensor, pt: Tensor, edge_index: Tensor, *, pt_thlds=(0.0, 0.5, 0.9, 1.5),
                          max_fprs=(None, 0.01, 0.001), n_samples=200,
                          total: Optional[Tensor] = None) -> dict[str, float]:
    """The metric dict of the edge classifier's validation step (training/ec.py:66-80): per pt cut,
    ``get_roc_auc_scores(max_fprs) | get_maximized_bcs`` of the edges with ``pt[src] > cut or
    pt[tgt] > cut`` (every edge for cut 0), keys suffixed by ``denote_pt``.  One counts launch and one
    AUC launch for all cuts, one host copy.  ``total``: a device scalar (the loss) read in the same copy
    and returned first, as ``float(total)``."""
    pt_thlds = [float(c) for c in pt_thlds]
    max_fprs = list(max_fprs)
    fprs = [float(f) for f in max_fprs if f is not None]
    if len(pt_thlds) > _capi.METRICS_MAX_CUTS:
        raise ValueError(f"at most {_capi.METRICS_MAX_CUTS} pt cuts")
    if len(fprs) > _capi.AUC_MAX_FPR:
        raise ValueError(f"at most {_capi.AUC_MAX_FPR} max_fpr values")
    order = sorted(range(len(pt_thlds)), key=lambda i: pt_thlds[i])   # (the kernels take ascending cuts)
    cuts = [pt_thlds[i] for i in order]
    thlds = torch.linspace(0.0, 1.0, n_samples)
    e = _Edges(w, y, pt, edge_index)
    dev = e.w.device
    nc, nb = len(cuts), n_samples + 1
    n_auc = nc * 2 * nb + nc * _capi.AUC_STRIDE
    buf = torch.empty(n_auc + 1, dtype=torch.int64, device=dev)
    _launch_counts(e, cuts, _threshold_table(thlds, dev), buf[: nc * 2 * nb])
    _launch_auc(e, cuts, fprs, buf[nc * 2 * nb: n_auc])
    metrics = {}
    if total is not None:   # (its float64 bits ride along in the last slot)
        buf[n_auc:] = total.detach().to(device=dev, dtype=torch.float64).reshape(1).view(torch.int64)
    host = buf.cpu().numpy()
    if total is not None:
        metrics["total"] = float(host[n_auc:].view(np.float64)[0])
    counts = host[: nc * 2 * nb].reshape(nc, 2, nb)
    auc = host[nc * 2 * nb: n_auc].reshape(nc, _capi.AUC_STRIDE)
    for i, cut in enumerate(pt_thlds):
        j = order.index(i)
        vals = _auc_from_row(auc[j], fprs)
        m = {}
        if None in max_fprs:
            m["roc_auc"] = vals[0]
        for f, v in zip([f for f in max_fprs if f is not None], vals[1:]):
            m[f"roc_auc_{f}FPR"] = v
        tp, fp, P, N = _thresholds_from_counts(counts[j])
        m |= _maximized(tp, fp, P, N, thlds)
        metrics |= denote_pt(m, cut)
    return metrics
