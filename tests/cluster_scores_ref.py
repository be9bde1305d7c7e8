"""numpy restatement of the clustering scores of ``common_metrics`` (metrics/cluster_metrics.py:427-456:
sklearn's v_measure / homogeneity / completeness / adjusted_rand / fowlkes_mallows scores) and of
``count_hits_per_cluster`` (:400-404).  TEST INFRASTRUCTURE ONLY.

It does NOT go through size spectra: labels are densified with ``np.unique``, the contingency counts are built
from the dense pairs, the entropies and the mutual information are formed from probabilities the way sklearn
forms them (per class ``p (ln count - ln n)``; per cell ``p (ln n_ij - ln n) + p (-ln(a_i b_j) + 2 ln n)`` with
terms below machine epsilon dropped and the sum clipped at 0), and the pair counts of the adjusted Rand index are
Python ints.  ``spectra`` gives what the device counts, from ``np.unique(..., return_counts=True)`` applied
twice."""

from __future__ import annotations

import math

import numpy as np

SCORE_KEYS = ("v_measure", "homogeneity", "completeness", "adjusted_rand", "fowlkes_mallows")


def contingency(truth, predicted):
    """Class sizes a [C], cluster sizes b [K] and the non-zero cells (class index, cluster index, count)."""
    truth, predicted = np.asarray(truth, dtype=np.int64), np.asarray(predicted, dtype=np.int64)
    _, ci, a = np.unique(truth, return_inverse=True, return_counts=True)
    _, ki, b = np.unique(predicted, return_inverse=True, return_counts=True)
    cell, nij = np.unique(ci.astype(np.int64) * len(b) + ki, return_counts=True)
    return a.astype(np.int64), b.astype(np.int64), cell // len(b), cell % len(b), nij.astype(np.int64)


def entropy(counts: np.ndarray) -> float:
    if len(counts) == 1:
        return 0.0
    pi = counts.astype(np.float64)
    s = pi.sum()
    return float(-np.sum((pi / s) * (np.log(pi) - math.log(s))))


def mutual_info(a, b, ci, ki, nij) -> float:
    if len(a) == 1 or len(b) == 1:
        return 0.0
    n = int(nij.sum())
    p = nij / n
    log_outer = -np.log(a[ci] * b[ki]) + math.log(int(a.sum())) + math.log(int(b.sum()))
    mi = p * (np.log(nij) - math.log(n)) + p * log_outer
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def entropies(truth, predicted) -> tuple[float, float]:
    """(H(C), H(K)) in nats."""
    a, b, *_ = contingency(truth, predicted)
    return entropy(a), entropy(b)


def scores(truth, predicted) -> dict[str, float]:
    a, b, ci, ki, nij = contingency(truth, predicted)
    n = int(a.sum())
    if n == 0:
        return dict(zip(SCORE_KEYS, (1.0, 1.0, 1.0, 1.0, 0.0)))
    h_c, h_k, mi = entropy(a), entropy(b), mutual_info(a, b, ci, ki, nij)
    hom = mi / h_c if h_c else 1.0
    com = mi / h_k if h_k else 1.0
    v = 0.0 if hom + com == 0.0 else 2 * hom * com / (hom + com)
    ss = sum(int(x) ** 2 for x in nij)
    sa, sb = sum(int(x) ** 2 for x in a), sum(int(x) ** 2 for x in b)
    tp, fp, fn = ss - n, sb - ss, sa - ss
    tn = n * n - fp - fn - ss
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    tk, pk, qk = ss - n, sb - n, sa - n
    fmi = math.sqrt(tk / pk) * math.sqrt(tk / qk) if tk != 0 else 0.0
    return dict(zip(SCORE_KEYS, (v, hom, com, ari, fmi)))


def count_hits_per_cluster(predicted) -> np.ndarray:
    _, counts = np.unique(np.asarray(predicted), return_counts=True)
    return np.bincount(counts)[1:].astype(np.int64)


def _spectrum(sizes: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    v, m = np.unique(sizes, return_counts=True)
    return v.astype(np.int64), m.astype(np.int64)


def spectra(labels, truth=None) -> dict[str, tuple[np.ndarray, np.ndarray]]:
    """``classes``, ``clusters``, ``cells`` of one labelling [n] as ascending (sizes, multiplicities)."""
    labels = np.asarray(labels, dtype=np.int64)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    clusters = _spectrum(np.unique(labels, return_counts=True)[1])
    if truth is None:
        return {"classes": empty, "clusters": clusters, "cells": empty}
    truth = np.asarray(truth, dtype=np.int64)
    classes = _spectrum(np.unique(truth, return_counts=True)[1])
    cells = _spectrum(np.unique(np.stack([labels, truth]), axis=1, return_counts=True)[1])
    return {"classes": classes, "clusters": clusters, "cells": cells}
