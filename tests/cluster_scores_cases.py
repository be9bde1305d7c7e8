"""What the CPU and GPU tests of the clustering scores share: the golden cases (G21, from the reference's
own ``common_metrics`` and ``count_hits_per_cluster``), random events, and the comparison rules.  TEST
INFRASTRUCTURE ONLY."""

from __future__ import annotations

import math
import pathlib

import numpy as np

import cluster_scores_ref as R

G21 = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "g21_cluster_scores.npz")
NAMES = tuple(str(k) for k in G21["names"])
SCORE_KEYS = tuple(str(k) for k in G21["score_keys"])
ENTROPY_SCORES = ("v_measure", "homogeneity", "completeness")
EXACT_SCORES = ("adjusted_rand", "fowlkes_mallows")


def case(name: str) -> tuple[np.ndarray, np.ndarray]:
    """(truth, predicted) of a golden case."""
    return G21[f"{name}/truth"], G21[f"{name}/predicted"]


def golden_scores(name: str) -> dict[str, float]:
    return dict(zip(SCORE_KEYS, (float(v) for v in G21[f"{name}/scores"])))


def golden_flat(name: str) -> dict[str, float]:
    return dict(zip((str(k) for k in G21[f"{name}/flat_keys"]), (float(v) for v in G21[f"{name}/flat_values"])))


def random_case(g: np.random.Generator, n: int, n_trials: int) -> tuple[np.ndarray, np.ndarray]:
    """Truth ids that are multiples of 2^40 minus 2^41 (negative, zero and beyond int32) of about 12 hits each
    and ``n_trials`` labellings drawn from [-3, n / 8): (truth [n], labels [n_trials, n])."""
    truth = g.integers(0, max(2, n // 12), size=n).astype(np.int64) * 2 ** 40 - 2 ** 41
    labels = g.integers(-3, max(2, n // 8), size=(n_trials, n)).astype(np.int64)
    return truth, labels


# ------------------------------------------------------------------ comparison rules
def entropy_tolerance(n: int, longest_spectrum: int, h: float) -> float:
    """Absolute tolerance of homogeneity, completeness and v-measure against sklearn:
    8 (D + 2) 2^-53 ln(n) / min(1, H), with D the longest spectrum of the case and H the entropy in the
    score's denominator (for v-measure, which has both, the smaller one).  It is the rounding of three fp64
    sums of D terms of magnitude up to n ln n, differenced, divided by n and then by H, doubled for sklearn's
    own sum.  Not for H == 0: those cases are exact (``assert_scores``)."""
    assert h > 0.0
    return 8 * (longest_spectrum + 2) * 2.0 ** -53 * math.log(n) / min(1.0, h)


def assert_scores(got: dict[str, float], want: dict[str, float], truth, predicted, what: str) -> None:
    """``got`` against sklearn's ``want``: the key order; adjusted_rand and fowlkes_mallows with ``==`` (one
    fp64 expression of the same integers); the three entropy scores within ``entropy_tolerance``, and with
    ``==`` where the entropy in the denominator is 0, which the rules map to exactly 1.0 or 0.0."""
    assert list(got) == list(SCORE_KEYS), what
    for k in EXACT_SCORES:
        assert got[k] == want[k], f"{what}: {k} {got[k]!r} != {want[k]!r}"
    n = len(truth)
    if n == 0:
        assert all(got[k] == want[k] for k in ENTROPY_SCORES), what
        return
    sp = R.spectra(predicted, truth)
    longest = max(len(s[0]) for s in sp.values())
    h_c, h_k = R.entropies(truth, predicted)
    for k, h in (("homogeneity", h_c), ("completeness", h_k), ("v_measure", min(h_c, h_k))):
        diff = abs(got[k] - want[k])
        if h == 0.0:
            assert got[k] == want[k] and got[k] in (0.0, 1.0), f"{what}: {k} {got[k]!r} != {want[k]!r} at zero entropy"
        else:
            tol = entropy_tolerance(n, longest, h)
            assert diff <= tol, f"{what}: {k} {got[k]!r} vs {want[k]!r}: differs by {diff:.3e} > {tol:.3e} (H = {h:.3e})"


def assert_spectra(got: dict, want: dict, n: int, what: str) -> None:
    """Spectra are integers: ``==`` on sizes and multiplicities, int64, ascending; the sizes sum to n."""
    assert list(got) == ["classes", "clusters", "cells"], what
    for k in got:
        (gv, gm), (wv, wm) = got[k], want[k]
        assert gv.dtype == np.int64 and gm.dtype == np.int64, f"{what}: {k}"
        assert np.array_equal(gv, wv) and np.array_equal(gm, wm), f"{what}: {k} differs"
        assert np.all(np.diff(gv) > 0), f"{what}: {k} is not ascending"
        assert int((gv * gm).sum()) == (n if len(gv) else 0), f"{what}: the sizes of {k} do not sum to n"


def assert_hist(got: np.ndarray, want: np.ndarray, what: str) -> None:
    assert got.dtype.kind == "i" and np.array_equal(got, want), f"{what}: histogram differs"
