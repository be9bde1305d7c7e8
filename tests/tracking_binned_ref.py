"""numpy-only restatement of the reference's cluster table and binned tracking metrics
(metrics/cluster_metrics.py:76-149, 292-384 with pandas 2 / numpy 2 semantics), in fp64 where the
reference is.

TEST INFRASTRUCTURE ONLY.  As ``tracking_metrics_ref``: the majority particle of a cluster is the
smallest particle id among those with the most hits in it; the table has rows for labels >= 0 only.
"""

from __future__ import annotations

import itertools
import math

import numpy as np

from tracking_metrics_ref import KEYS, _mean32, metrics_from_counts

TABLE_COLUMNS = ("maj_pid", "maj_hits", "cluster_size", "valid_cluster", "maj_reconstructable", "maj_eta", "maj_pt",
                 "maj_pid_hits", "maj_frac", "maj_pid_frac", "perfect_match", "double_majority", "lhc_match")


def cluster_table(labels, pid, pt, eta, reco, predicted_count_thld=3) -> dict:
    """tracking_metric_df's rows with c >= 0: ``c`` and the 13 columns."""
    labels = np.asarray(labels, dtype=np.int64)
    pid = np.asarray(pid, dtype=np.int64)
    pt, eta, reco = (np.asarray(a, dtype=np.float32) for a in (pt, eta, reco))
    upid, pinv = np.unique(pid, return_inverse=True)
    P = max(len(upid), 1)
    p_hits = np.bincount(pinv, minlength=P)
    m_pt, m_eta, m_reco = (_mean32(pinv, v, P) for v in (pt, eta, reco))
    keep = labels >= 0
    ulab, linv = np.unique(labels[keep], return_inverse=True)
    pp = pinv[keep]
    uk, kc = np.unique(linv * P + pp, return_counts=True)
    k_lab, k_p = uk // P, uk % P
    # majority pair per cluster: most hits, then the smallest particle id (k_p ascends with the id)
    order = np.lexsort((k_p, -kc, k_lab))
    first = np.ones(len(order), dtype=bool)
    first[1:] = k_lab[order][1:] != k_lab[order][:-1]
    best = order[first]
    size = np.bincount(linv, minlength=len(ulab)).astype(np.int64)
    maj, mp = kc[best].astype(np.int64), k_p[best]
    valid = size >= predicted_count_thld
    pid_hits = p_hits[mp].astype(np.int64)
    frac, pid_frac = maj / size, maj / pid_hits
    return {"c": ulab, "maj_pid": upid[mp] if len(mp) else np.zeros(0, np.int64), "maj_hits": maj,
            "cluster_size": size, "valid_cluster": valid, "maj_reconstructable": m_reco[mp], "maj_eta": m_eta[mp],
            "maj_pt": m_pt[mp], "maj_pid_hits": pid_hits, "maj_frac": frac, "maj_pid_frac": pid_frac,
            "perfect_match": (pid_hits == maj) & (frac > 0.99) & valid,
            "double_majority": (pid_frac > 0.5) & (frac > 0.5) & valid, "lhc_match": (frac > 0.75) & valid}


def _in_windows(pt: np.ndarray, eta: np.ndarray, windows: np.ndarray) -> np.ndarray:
    """[n, n_win]: lo <= value < hi for pt and signed eta; a NaN bound is not tested, a NaN value fails
    every test that is."""
    w = np.asarray(windows, dtype=np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return ((np.isnan(w[:, 0]) | (pt[:, None] >= w[:, 0])) & (np.isnan(w[:, 1]) | (pt[:, None] < w[:, 1]))
                & (np.isnan(w[:, 2]) | (eta[:, None] >= w[:, 2])) & (np.isnan(w[:, 3]) | (eta[:, None] < w[:, 3])))


def window_counts(labels, pid, pt, eta, reco, windows, predicted_count_thld=3):
    """-> (n_particles [n_win], counts [n_win, 4] = clusters, perfect, double majority, lhc)."""
    pid = np.asarray(pid, dtype=np.int64)
    pt, eta, reco = (np.asarray(a, dtype=np.float32) for a in (pt, eta, reco))
    nw = len(np.asarray(windows).reshape(-1, 4))
    n_part = np.zeros(nw, dtype=np.int64)
    counts = np.zeros((nw, 4), dtype=np.int64)
    if pid.size == 0:
        return n_part, counts
    h = _in_windows(pt, eta, windows) & (reco != 0)[:, None]
    t = cluster_table(labels, pid, pt, eta, reco, predicted_count_thld)
    mr = t["maj_reconstructable"]
    c = _in_windows(t["maj_pt"], t["maj_eta"], windows) & ((mr != 0) & ~np.isnan(mr) & t["valid_cluster"])[:, None]
    for j in range(nw):
        n_part[j] = len(np.unique(pid[h[:, j]]))
        m = c[:, j]
        counts[j] = (m.sum(), (t["perfect_match"] & m).sum(), (t["double_majority"] & m).sum(),
                     (t["lhc_match"] & m).sum())
    return n_part, counts


def pt_windows(edges, max_eta=4.0) -> np.ndarray:
    return np.array([(lo, hi, np.nan, max_eta) for lo, hi in itertools.pairwise(edges)], dtype=np.float32)


def eta_windows(edges, pt_thld=0.9) -> np.ndarray:
    return np.array([(pt_thld, np.nan, lo, hi) for lo, hi in itertools.pairwise(edges)], dtype=np.float32)


def binned_rows(batches, edges, windows, names) -> list[dict]:
    """tracking_metrics_vs_pt / _vs_eta: per bin the NaN-skipping mean over the batches, then the
    ddof = 1 std / sqrt(number of batches) as ``_err``, then the bin's edges.  ``batches``: dicts with
    labels, pid, pt, eta, reco."""
    per = [window_counts(b["labels"], b["pid"], b["pt"], b["eta"], b["reco"], windows) for b in batches]
    rows = []
    for j, (lo, hi) in enumerate(itertools.pairwise(edges)):
        ms = [metrics_from_counts(n_part[j], counts[j]) for n_part, counts in per]
        row, err = {}, {}
        for k in KEYS:
            v = np.array([float(m[k]) for m in ms], dtype=np.float64)
            v = v[~np.isnan(v)]
            row[k] = float(v.mean()) if v.size else float("nan")
            err[k + "_err"] = (float(v.std(ddof=1)) if v.size > 1 else float("nan")) / math.sqrt(len(ms))
        rows.append({**row, **err, names[0]: lo, names[1]: hi})
    return rows


def vs_pt(batches, edges, max_eta=4.0):
    return binned_rows(batches, edges, pt_windows(edges, max_eta), ("pt_min", "pt_max"))


def vs_eta(batches, edges, pt_thld=0.9):
    return binned_rows(batches, edges, eta_windows(edges, pt_thld), ("eta_min", "eta_max"))
