"""Cases and comparisons shared by the CPU and GPU tests of the binned tracking metrics: the golden
values of the reference (G20) with their inputs (G17), and random events with random windows.

TEST INFRASTRUCTURE ONLY."""

from __future__ import annotations

import pathlib

import numpy as np
import pytest

HERE = pathlib.Path(__file__).resolve().parent
G17 = np.load(HERE / "golden" / "g17_tracking_metrics.npz")
G20 = np.load(HERE / "golden" / "g20_tracking_binned.npz")
BINNED = ("td3_0", "td3_1", "blobs", "ptedge", "naneta", "recomix", "recobool")
MULTI = tuple(str(n) for n in G20["multi/names"])
TABLES = ("td3_0", "blobs", "ptedge", "naneta", "recomix", "recobool")
TABLE_COLUMNS = tuple(str(k) for k in G20["table_columns"])
TABLE_DTYPES = {"maj_pid": np.int64, "maj_hits": np.int64, "cluster_size": np.int64, "valid_cluster": np.bool_,
                "maj_reconstructable": np.float32, "maj_eta": np.float32, "maj_pt": np.float32,
                "maj_pid_hits": np.int64, "maj_frac": np.float64, "maj_pid_frac": np.float64,
                "perfect_match": np.bool_, "double_majority": np.bool_, "lhc_match": np.bool_}
COUNT_KEYS = ("n_particles", "n_cleaned_clusters", "perfect", "double_majority", "lhc", "fake_perfect",
              "fake_double_majority", "fake_lhc")


def batch(name: str) -> dict:
    """The hits of a G17 case: labels, pid, pt, eta, reco."""
    return {k: G17[f"{name}/{k}"] for k in ("labels", "pid", "pt", "eta", "reco")}


def scan_batch(i: int) -> dict:
    """Scan batch i of G17 with the labels the reference's DBSCAN gave it (G20)."""
    b = {k: G17[f"scan/b{i}/{k}"] for k in ("H", "pid", "pt", "eta", "reco")}
    b["labels"] = G20[f"scan/b{i}/labels"].astype(np.int64)
    return b


def hit_record(b: dict, to=lambda a: a) -> dict:
    """The hit record of tracking_metrics_vs_pt / _vs_eta (``to``: e.g. a copy to the device)."""
    return {"c": to(b["labels"]), "id": to(b["pid"]), "reconstructable": to(b["reco"]), "pt": to(b["pt"]),
            "eta": to(b["eta"])}


def golden_rows(prefix: str, which: str) -> list[dict]:
    keys = [str(k) for k in G20[f"{which}_keys"]]
    return [dict(zip(keys, row.tolist())) for row in G20[f"{prefix}{which}"]]


def golden_table(prefix: str) -> dict:
    return {k: G20[f"{prefix}{k}"] for k in ("c",) + TABLE_COLUMNS}


def assert_rows(got: list[dict], want: list[dict], what: str):
    """Keys in order; the bin edges and, for ONE batch, every value ``==`` (NaN equals NaN): they are
    integers and ratios of integers.  Over several batches the means and ``_err`` at rel 1e-12."""
    assert len(got) == len(want), f"{what}: {len(got)} rows, want {len(want)}"
    for j, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), f"{what}: row {j} keys {list(g)} vs {list(w)}"
        one_batch = all(w[k + "_err"] != w[k + "_err"] for k in COUNT_KEYS)
        for k, v in w.items():
            x = float(g[k])
            if one_batch or not k.startswith(COUNT_KEYS):
                assert x == v or (x != x and v != v), f"{what}: row {j} {k} = {g[k]!r}, want {v!r}"
            else:
                assert x == pytest.approx(v, rel=1e-12, abs=1e-15, nan_ok=True), f"{what}: row {j} {k}"


def assert_table(got: dict, want: dict, what: str, dtypes: bool = False, exact_means: bool = False):
    """Columns in order and every value ``==`` (NaN equals NaN), except the three fp32 means against the
    GOLDEN: pandas' groupby().mean() of a float32 column is a Kahan sum in fp32 divided in fp32, the
    table's is the fp64 sum rounded once.  With u = 2^-24 and values of one sign within a particle (all
    golden cases: pt > 0, reconstructable >= 0, eta constant per particle) the compensated sum is within
    2u of the exact one, its division and the single rounding add u each: |got - want| <= 4u |want| =
    2^-22 |want|.  ``exact_means``: ``==`` for them too (against the restatement, which rounds once).
    The golden's maj_reconstructable is fp64 where reconstructable was bool: rounded to fp32 first."""
    assert list(got) == ["c", *TABLE_COLUMNS], f"{what}: columns {list(got)}"
    for k in got:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if dtypes and k != "c":
            assert g.dtype == TABLE_DTYPES[k], f"{what}: {k} is {g.dtype}"
        if k == "maj_reconstructable":
            w = w.astype(np.float32)
        assert g.shape == w.shape, f"{what}: {k} has {g.shape} rows, want {w.shape}"
        assert g.dtype.kind == w.dtype.kind, f"{what}: {k} is {g.dtype}, want {w.dtype}"
        ok = (g == w) | ((g != g) & (w != w))
        if k in ("maj_reconstructable", "maj_eta", "maj_pt") and not exact_means:
            with np.errstate(invalid="ignore"):
                ok |= np.abs(g.astype(np.float64) - w.astype(np.float64)) <= 2.0 ** -22 * np.abs(w.astype(np.float64))
        assert ok.all(), f"{what}: {k} differs in rows {np.flatnonzero(~ok)[:8]}"


def random_event(g, n, n_part, big_ids):
    """An event of NaN-laden value sets (as the tracking-metrics tests draw them)."""
    pid = g.integers(0, n_part, n).astype(np.int64)
    if big_ids:
        pid = pid * (2 ** 40) - 2 ** 41
    pt = g.choice(np.array([0.3, 0.5, 0.9, 0.95, 1.5, 2.0, np.nan], np.float32), n)
    eta = g.choice(np.array([0.1, -3.9, 4.0, -4.0, 2.5, np.nan], np.float32), n)
    reco = g.choice(np.array([0, 1, np.nan], np.float32), n, p=[0.2, 0.75, 0.05])
    return pid, pt, eta, reco


def random_windows(g) -> np.ndarray:
    """32 windows (pt_lo, pt_hi, eta_lo, eta_hi): disjoint pt and eta slices, overlapping ones, a NaN
    bound on each side, an empty and an all-open window, in random order."""
    nan, inf = np.nan, np.inf
    w = [(0.0, 0.5, nan, 4.0), (0.5, 0.9, nan, 4.0), (0.9, 1.5, nan, 4.0), (1.5, inf, nan, 4.0),    # vs_pt
         (0.9, nan, -4.0, -2.0), (0.9, nan, -2.0, 0.0), (0.9, nan, 0.0, 2.0), (0.9, nan, 2.0, 4.0),  # vs_eta
         (nan, nan, nan, nan), (nan, 0.9, nan, nan), (0.9, nan, nan, nan), (nan, nan, nan, 0.0),
         (nan, nan, 0.0, nan), (2.0, 0.3, nan, nan), (0.3, 2.0, -4.0, 4.0), (0.3, 2.0001, -4.0, 4.0001),
         (0.5, 0.5, nan, nan), (0.95, 0.950001, 0.1, 2.5), (-inf, inf, -inf, inf), (inf, nan, nan, nan)]
    while len(w) < 32:   # overlapping random boxes, a bound left open now and then
        lo, hi = np.sort(g.choice([0.0, 0.3, 0.5, 0.9, 0.95, 1.5, 2.0, 3.0], 2, replace=False))
        elo, ehi = np.sort(g.choice([-5.0, -4.0, -3.9, 0.1, 2.5, 4.0, 5.0], 2, replace=False))
        box = [lo, hi, elo, ehi]
        if g.random() < 0.4:
            box[int(g.integers(4))] = nan
        w.append(tuple(box))
    return np.array(w, dtype=np.float32)[g.permutation(32)]
