"""numpy-only restatement of the k-scan of the metric-learning validation (graph_construction/k_scanner.py:
31-285, analysis/graphs.py:281-343, metrics/graph_construction.py:8-31): union-find in Python, integer
counts, float32 quotients for efficiency / purity, pandas' skip-NaN Kahan means and an own not-a-knot
spline.  TEST INFRASTRUCTURE ONLY; the large-input oracle of the GPU tests.

Labels follow the product's rule: a component is labelled by its smallest node index.
"""

from __future__ import annotations

import math

import numpy as np

import tracking_metrics_ref as TR

COLUMNS = ("n_edges", "n_masked", "n_true_masked", "n_true_edges_masked", "n_pids", "n50", "n75", "n100", "n_bad")
EXTRA = ("k", "frac75", "frac100", "efficiency", "purity")


def good_node_mask(pid, pt, eta, reco, pt_thld=0.9, max_eta=4.0):
    """utils/graph_masks.py:19-28 on float32 columns (numpy 2: the Python scalar is cast to float32)."""
    pt, eta, reco = (np.asarray(a, dtype=np.float32) for a in (pt, eta, reco))
    return (pt > np.float32(pt_thld)) & (np.asarray(pid) > 0) & (reco > 0) & (np.abs(eta) < np.float32(max_eta))


def neighbour_table(x, kmax, max_radius):
    """Brute force in float64: per query the kmax nearest other points (ties -> lower index) with
    distance < max_radius; -> (nbr [n, kmax] int32, cnt [n] int32).  Small inputs only."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    kmax = min(kmax, n - 1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :kmax]
    dist = np.take_along_axis(d, idx, axis=1)
    ok = np.isfinite(dist) if max_radius is None else dist < max_radius
    assert (np.diff(ok.astype(np.int8), axis=1) <= 0).all()
    return idx.astype(np.int32), ok.sum(1).astype(np.int32)


def table_edges(nbr, cnt, k):
    """Edge list [2, M] of the k-graph: (neighbour, query), grouped by query."""
    nbr = np.asarray(nbr).reshape(len(cnt), -1)
    take = np.arange(nbr.shape[1])[None, :] < np.minimum(cnt, k)[:, None]
    q = np.broadcast_to(np.arange(len(cnt))[:, None], nbr.shape)
    return np.stack([nbr[take].astype(np.int64), q[take].astype(np.int64)])


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, a):
        p = self.parent
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        return a

    def union_edges(self, e0, e1):
        p, find = self.parent, self.find
        for a, b in zip(e0.tolist(), e1.tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                if ra < rb:
                    p[rb] = ra
                else:
                    p[ra] = rb

    def labels(self):
        return np.array([self.find(i) for i in range(len(self.parent))], dtype=np.int64)


def cc_labels(edge_index, n, same_pid=None, node_mask=None):
    """Smallest node index of every node's component; optional filters as gnntrk_cc_labels."""
    e = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    keep = np.ones(e.shape[1], dtype=bool)
    if same_pid is not None:
        keep &= np.asarray(same_pid)[e[0]] == np.asarray(same_pid)[e[1]]
    if node_mask is not None:
        keep &= np.asarray(node_mask, dtype=bool)[e[0]] & np.asarray(node_mask, dtype=bool)[e[1]]
    uf = UnionFind(n)
    uf.union_edges(e[0][keep], e[1][keep])
    return uf.labels()


def segment_counts(labels, pid, mask):
    """(n_pids, n50, n75, n100) of one labelling restricted to the mask, in integers."""
    mask = np.asarray(mask, dtype=bool)
    if not mask.any():
        return 0, 0, 0, 0
    upid, pinv, c = np.unique(np.asarray(pid)[mask], return_inverse=True, return_counts=True)
    _, linv, lc = np.unique(np.asarray(labels)[mask], return_inverse=True, return_counts=True)
    s = np.zeros(len(upid), dtype=np.int64)
    np.maximum.at(s, pinv, lc[linv])
    return len(upid), int((2 * s > c).sum()), int((4 * s > 3 * c).sum()), int((s == c).sum())


def largest_segment_fracs(edge_index, pid, mask):
    """Sorted fractions of analysis/graphs.py:281-328 for y = same-id edges."""
    mask = np.asarray(mask, dtype=bool)
    labels = cc_labels(edge_index, len(pid), same_pid=pid, node_mask=mask)
    if not mask.any():
        return np.array([])
    upid, pinv, c = np.unique(np.asarray(pid)[mask], return_inverse=True, return_counts=True)
    _, linv, lc = np.unique(labels[mask], return_inverse=True, return_counts=True)
    s = np.zeros(len(upid), dtype=np.int64)
    np.maximum.at(s, pinv, lc[linv])
    return np.sort(s / c)


def scan_table(nbr, cnt, ks, pid, mask, true_edge_index):
    """What gnntrk_kscan_counts returns: (int64 [n_ks, 9] counts, int64 [n_ks, n] labels)."""
    pid = np.asarray(pid, dtype=np.int64)
    mask = np.asarray(mask, dtype=bool)
    n = len(pid)
    nbr = np.asarray(nbr).reshape(n, -1)
    te = np.zeros((2, 0), np.int64) if true_edge_index is None else np.asarray(true_edge_index).reshape(2, -1)
    n_te = int((mask[te[0]] & mask[te[1]]).sum())
    out = np.zeros((len(ks), len(COLUMNS)), dtype=np.int64)
    labels = np.zeros((len(ks), n), dtype=np.int64)
    ufa, ufb, lo = UnionFind(n), UnionFind(n), 0
    for r in np.argsort(np.asarray(ks), kind="stable"):
        k = int(ks[r])
        if k > lo:   # the edges of rank [lo, k)
            ranks = np.arange(lo, k)
            take = ranks[None, :] < cnt[:, None]
            j = nbr[:, lo:k][take].astype(np.int64)
            q = np.broadcast_to(np.arange(n)[:, None], take.shape)[take]
            y = pid[j] == pid[q]
            ufa.union_edges(j[y], q[y])
            both = y & mask[j] & mask[q]
            ufb.union_edges(j[both], q[both])
            lo = k
        e = table_edges(nbr, cnt, k)
        y = pid[e[0]] == pid[e[1]]
        m = mask[e[0]] | mask[e[1]]
        labels[r] = ufa.labels()
        out[r, :4] = e.shape[1], m.sum(), (y & m).sum(), n_te
        out[r, 4:8] = segment_counts(ufb.labels(), pid, mask)
    return out, labels


def f32_ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float32(a) / np.float32(b))


def records(counts, labels, ks, pid, pt, eta, reco, max_edges=5_000_000):
    """The scanner's records of one batch (k_scanner.py:248-285) from the integer table."""
    out = []
    for row, lab, k in zip(counts, labels, ks):
        c = dict(zip(COLUMNS, (int(v) for v in row)))
        if c["n_edges"] > max_edges:
            break
        z = lambda a, b: float("nan") if b == 0 else a / b   # noqa: E731
        ub = TR.tracking_metrics_flat(lab, pid, pt, eta, reco, (0.9,))
        out.append({"k": int(k), "frac50": z(c["n50"], c["n_pids"]), "frac75": z(c["n75"], c["n_pids"]),
                    "frac100": z(c["n100"], c["n_pids"]), "n_edges": c["n_edges"],
                    "efficiency": f32_ratio(c["n_true_masked"], 2 * c["n_true_edges_masked"]),
                    "purity": f32_ratio(c["n_true_masked"], c["n_masked"]),
                    **{"max_" + key: v for key, v in ub.items()}})
    return out


def batch_records(x, pid, pt, eta, reco, true_edge_index, ks, *, max_radius=1.0, pt_thld=0.9, max_eta=4.0,
                  max_edges=5_000_000):
    nbr, cnt = neighbour_table(x, max(ks), max_radius)
    mask = good_node_mask(pid, pt, eta, reco, pt_thld, max_eta)
    kk = [min(int(k), nbr.shape[1]) for k in ks]
    counts, labels = scan_table(nbr, cnt, kk, pid, mask, true_edge_index)
    return records(counts, labels, ks, pid, pt, eta, reco, max_edges)


def mean_skipna(values):
    """pandas' groupby().mean(): NaN skipped, Kahan summation."""
    total, comp, n = 0.0, 0.0, 0
    for v in values:
        if v != v:
            continue
        n += 1
        y = v - comp
        t = total + y
        comp = t - total - y
        total = t
    return total / n if n else float("nan")


def mean_rows(recs):
    by_k = {}
    for r in recs:
        by_k.setdefault(r["k"], []).append(r)
    return [{"k": k, **{c: mean_skipna([float(r[c]) for r in by_k[k]]) for c in by_k[k][0] if c != "k"}}
            for k in sorted(by_k)]


def spline_coeffs(x, y):
    """Not-a-knot cubic spline (scipy CubicSpline's default): piecewise coefficients [4, n-1, cols]."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64).reshape(len(x), -1)
    n, dx = len(x), np.diff(x)
    sl = np.diff(y, axis=0) / dx[:, None]
    if n == 2:
        s = np.vstack([sl[0], sl[0]])
    else:
        a, b = np.zeros((n, n)), np.zeros_like(y)
        for i in range(1, n - 1):
            a[i, i - 1:i + 2] = dx[i], 2 * (dx[i - 1] + dx[i]), dx[i - 1]
            b[i] = 3 * (dx[i] * sl[i - 1] + dx[i - 1] * sl[i])
        if n == 3:
            a[0, :2], a[2, 1:] = (1, 1), (1, 1)
            b[0], b[2] = 2 * sl[0], 2 * sl[1]
        else:
            d = x[2] - x[0]
            a[0, :2] = dx[1], d
            b[0] = ((dx[0] + 2 * d) * dx[1] * sl[0] + dx[0] ** 2 * sl[1]) / d
            d = x[-1] - x[-3]
            a[-1, -2:] = d, dx[-2]
            b[-1] = (dx[-1] ** 2 * sl[-2] + (2 * d + dx[-1]) * dx[-2] * sl[-1]) / d
        s = np.linalg.solve(a, b)
    t = (s[:-1] + s[1:] - 2 * sl) / dx[:, None]
    return np.stack([t / dx[:, None], (sl - s[:-1]) / dx[:, None] - t, s[:-1], y[:-1]])


def spline_eval(x, c, k):
    k = np.asarray(k, np.float64)
    i = np.clip(np.searchsorted(x, k, side="right") - 1, 0, len(x) - 2)
    h = (k - x[i])[..., None]
    return ((c[0][i] * h + c[1][i]) * h + c[2][i]) * h + c[3][i]


def foms(rows, targets):
    """KScanResults.get_foms (k_scanner.py:50-65) on the per-k mean rows; the k of a target by bracketing
    the crossing nearest the mid-point on a 2 001-point grid and bisecting (end point without crossing)."""
    rows = sorted(rows, key=lambda r: r["k"])
    cols = [c for c in rows[0] if c != "k"] + ["k"]
    tab = {c: np.array([float(r[c]) for r in rows]) for c in cols}
    good = [c for c in cols if not np.isnan(tab[c]).any()]
    nan_row = {c: float("nan") for c in cols}
    x = tab["k"]
    coeffs = spline_coeffs(x, np.stack([tab[c] for c in good], 1)) if len(rows) >= 2 else None

    def at(k):
        r = dict(nan_row)
        r.update(zip(good, spline_eval(x, coeffs, float(k)).tolist()))
        return r

    def f50(k):
        return spline_eval(x, coeffs, k)[..., good.index("frac50")]

    def target_k(t):
        if "frac50" not in good or t > tab["frac50"].max():
            return float("nan")
        grid = np.linspace(x.min(), x.max(), 2001)
        g = f50(grid) - t
        mid = (x.min() + x.max()) / 2
        zero = [(abs(grid[i] - mid), i, 0) for i in np.flatnonzero(g == 0)]
        cross = [(abs((grid[i] + grid[i + 1]) / 2 - mid), i, 1) for i in np.flatnonzero(g[:-1] * g[1:] < 0)]
        if not zero + cross:
            i = int(np.argmin(np.abs(g)))
            assert i in (0, len(grid) - 1), "restatement: interior minimum without a crossing is not covered"
            return float(grid[i])
        _, i, kind = min(zero + cross)
        if kind == 0:
            return float(grid[i])
        a, b = float(grid[i]), float(grid[i + 1])
        for _ in range(200):
            m = (a + b) / 2
            if m in (a, b):
                break
            if (float(f50(m)) - t < 0) == (g[i] < 0):
                a = m
            else:
                b = m
        return (a + b) / 2

    out = {}
    for t in targets:
        k = target_k(t) if len(rows) >= 2 else float("nan")
        fat = nan_row if math.isnan(k) else at(k)
        out[f"n_edges_frac_segment50_{t * 100:.0f}"] = fat["n_edges"]
        for v in EXTRA:
            out[f"{v}_at_segment50_{t * 100:.0f}"] = fat[v]
    f = tab["frac50"]
    idx = len(f) - 1 if np.isnan(f).all() else int(np.nanargmax(f))
    out["max_frac_segment50"] = float(f[idx])
    out["n_edges_max_frac_segment50"] = float(tab["n_edges"][idx])
    for v in EXTRA:
        out[f"{v}_at_max_frac_segment50"] = float(tab[v][idx])
    return out
