"""numpy-only restatement of the reference's tracking metrics (metrics/cluster_metrics.py:76-257 with
pandas 2 / numpy 2 semantics) and of ``OCScanResults`` aggregation, in fp64 where the reference is.

TEST INFRASTRUCTURE ONLY.  One deliberate choice where the reference has none: the majority particle
of a cluster is the smallest particle id among those with the most hits in it (pandas' value_counts
orders ties by an unstable sort).
"""

from __future__ import annotations

import math

import numpy as np

KEYS = ("n_particles", "n_cleaned_clusters", "perfect", "double_majority", "lhc", "fake_perfect",
        "fake_double_majority", "fake_lhc")


def _mean32(inv: np.ndarray, v: np.ndarray, n_groups: int) -> np.ndarray:
    """groupby().mean() of a float32 column: NaN skipped, fp64 sum, float32 result."""
    ok = ~np.isnan(v)
    s = np.bincount(inv[ok], weights=v[ok].astype(np.float64), minlength=n_groups)
    c = np.bincount(inv[ok], minlength=n_groups)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(c > 0, s / np.maximum(c, 1), np.nan)
    return m.astype(np.float32)


def tracking_counts(labels, pid, pt, eta, reco, cuts, *, predicted_count_thld=3, max_eta=4.0):
    """-> (n_particles [n_cuts], counts [n_cuts, 4] = clusters, perfect, double majority, lhc)."""
    labels = np.asarray(labels, dtype=np.int64)
    pid = np.asarray(pid, dtype=np.int64)
    pt, eta, reco = (np.asarray(a, dtype=np.float32) for a in (pt, eta, reco))
    c32 = np.asarray(cuts, dtype=np.float32)
    me = np.float32(max_eta)
    nc = len(c32)
    n_part = np.zeros(nc, dtype=np.int64)
    counts = np.zeros((nc, 4), dtype=np.int64)
    if labels.size == 0:
        return n_part, counts
    upid, pinv = np.unique(pid, return_inverse=True)
    P = len(upid)
    p_hits = np.bincount(pinv, minlength=P)
    m_pt, m_eta, m_reco = (_mean32(pinv, v, P) for v in (pt, eta, reco))
    p_ok = (m_reco != 0) & ~np.isnan(m_reco) & (np.abs(m_eta) < me)
    p_cls = np.where(p_ok, (m_pt[:, None] >= c32[None, :]).sum(1), 0)
    h_mask = (pt[:, None] >= c32[None, :]) & (reco != 0)[:, None] & (np.abs(eta) < me)[:, None]
    for c in range(nc):
        n_part[c] = len(np.unique(pid[h_mask[:, c]]))
    keep = labels >= 0
    if not keep.any():
        return n_part, counts
    lab, pp = labels[keep], pinv[keep]
    key = lab * P + pp
    uk, kc = np.unique(key, return_counts=True)
    k_lab, k_p = uk // P, uk % P
    # majority pair per cluster: most hits, then the smallest particle id (k_p ascends with the id)
    order = np.lexsort((k_p, -kc, k_lab))
    first = np.ones(len(order), dtype=bool)
    first[1:] = k_lab[order][1:] != k_lab[order][:-1]
    best = order[first]
    c_lab = k_lab[best]
    c_size = np.bincount(np.searchsorted(c_lab, lab), minlength=len(c_lab))
    maj, mp = kc[best], k_p[best]
    valid = c_size >= predicted_count_thld
    frac = maj / c_size
    pid_frac = maj / p_hits[mp]
    perfect = (p_hits[mp] == maj) & (frac > 0.99) & valid
    dm = (pid_frac > 0.5) & (frac > 0.5) & valid
    lhc = (frac > 0.75) & valid
    for c in range(nc):
        m = valid & (p_cls[mp] > c)
        counts[c] = (m.sum(), (perfect & m).sum(), (dm & m).sum(), (lhc & m).sum())
    return n_part, counts


def _zdiv(a, b):
    return float("nan") if b == 0 else a / b


def metrics_from_counts(n_particles: int, c) -> dict:
    nc, pm, dm, lhc = (int(v) for v in c)
    n = int(n_particles)
    return {"n_particles": n, "n_cleaned_clusters": nc, "perfect": _zdiv(pm, n), "double_majority": _zdiv(dm, n),
            "lhc": _zdiv(lhc, nc), "fake_perfect": _zdiv(nc - pm, nc), "fake_double_majority": _zdiv(nc - dm, nc),
            "fake_lhc": _zdiv(nc - lhc, nc)}


def denote_pt(k: str, pt: float) -> str:
    return k if np.isclose(pt, 0.0) else f"{k}_pt{pt:.1f}"


def tracking_metrics_flat(labels, pid, pt, eta, reco, pt_thlds=(0.0, 0.5, 0.9, 1.5), **kw) -> dict:
    """flatten_track_metrics(tracking_metrics(...)) (cuts given ascending)."""
    n_part, counts = tracking_counts(labels, pid, pt, eta, reco, pt_thlds, **kw)
    out = {}
    for j, p in enumerate(pt_thlds):
        out.update({denote_pt(k, p): v for k, v in metrics_from_counts(n_part[j], counts[j]).items()})
    return out


def get_foms(records: list[dict], guide="double_majority_pt0.9") -> dict:
    """OCScanResults(records).get_foms(guide) of the reference, restated."""
    params = ("eps", "min_samples")
    cols = []
    for r in records:
        cols += [k for k in r if k not in params and k not in cols]
    groups: dict = {}
    for r in records:
        groups.setdefault((r["eps"], r["min_samples"]), []).append(r)
    rows = []
    for key in sorted(groups):
        v = {c: np.array([float(r[c]) for r in groups[key]]) for c in cols}
        row = {"eps": key[0], "min_samples": key[1]}
        for c in cols:
            x = v[c][~np.isnan(v[c])]
            row[c] = float(x.mean()) if x.size else float("nan")
        for c in cols:
            x = v[c][~np.isnan(v[c])]
            row[c + "_std"] = (float(x.std(ddof=1)) if x.size > 1 else float("nan")) / math.sqrt(len(groups))
        rows.append(row)
    g = np.array([r[guide] for r in rows])
    best = rows[int(np.nanargmax(g))]
    foms = {f"trk.{c}": float(best[c]) for c in best if c not in params}
    foms["best_dbscan_eps"] = float(best["eps"])
    foms["best_dbscan_min_samples"] = float(best["min_samples"])
    return foms
