"""numpy restatement of the geometric graph builder (``gnn_tracking_amd.graph_builder``), independent of the product:
the cuts of ``graph_construction/graph_builder.py:162-227`` evaluated in FLOAT64 from the float32 point-cloud columns
(the reference evaluates them in float32), the truth relabelling of ``correct_truth_labels`` (229-306), the undirected
doubling of ``to_pyg_data`` (431-438), ``get_n_truth_edges`` (457-469) and the measurement record of ``process``
(531-549).  tools/make_golden_graph_builder.py pins it to the reference's own output, tests/graph_builder_cases.py
holds the device against it.  TEST INFRASTRUCTURE ONLY.

Order of the edges: layer pairs in the order of the list, inside a pair hit 1 ascending in hit index, then hit 2
ascending in hit index (pandas' cross join of two groups that keep the frame's order).  Events of a collated batch
(``sizes``): pairs are formed inside an event only, the edges are event-major, node ids global.
"""

from __future__ import annotations

import numpy as np

PAIRS = ((7, 8), (8, 9), (9, 10), (7, 6), (8, 6), (9, 6), (10, 6), (7, 11), (8, 11), (9, 11), (10, 11), (0, 1), (1, 2),
         (2, 3), (3, 4), (4, 5), (5, 6), (11, 12), (12, 13), (13, 14), (14, 15), (15, 16), (16, 17))
RADIUS = {7: 71.56298065185547, 8: 115.37811279296875}     # layer 1 of a pair whose layer 2 is 6 or 11
Z_EDGE = 490.975
PT_THLDS = (0, 0.1, 0.5, 0.9, 1.0)
DEFAULTS = dict(phi_slope_max=0.005, z0_max=200, dR_max=1.7)
FEATURE_SCALE = np.array([1000.0, np.pi, 1000.0, 1, 1 / 1000.0, 1 / 1000.0] + [1.0] * 8)


def two_hop(pairs):
    """the pairs ``get_two_hop_tuples`` adds, ascending, without those the list already holds twice over"""
    return sorted({(a, d) for a, b in pairs for c, d in pairs if b == c})


def pairs_of(pixel_only=True, edge_augmentation=None):
    pairs = list(PAIRS) if pixel_only else []
    if edge_augmentation == "add_two_hop":
        pairs = pairs + two_hop(pairs)
    elif edge_augmentation is not None:
        raise ValueError(f"Invalid augmentation mode: {edge_augmentation}")
    return pairs


def eta64(r, z):
    with np.errstate(all="ignore"):
        return -np.log(np.tan(np.arctan2(np.asarray(r, np.float64), np.asarray(z, np.float64)) / 2.0))


def pair_quantities(r1, phi1, z1, eta1, r2, phi2, z2, eta2, l1, l2):
    """float64 columns of the cross join of two groups, hit 1 major: dr, dphi, dz, dR, phi_slope, z0, z_coord (nan
    where the pair has no intersect cut)"""
    n1, n2 = len(r1), len(r2)
    rep = lambda a: np.repeat(np.asarray(a, np.float64), n2)      # noqa: E731
    til = lambda a: np.tile(np.asarray(a, np.float64), n1)        # noqa: E731
    with np.errstate(all="ignore"):
        dphi = til(phi2) - rep(phi1)
        dphi[dphi > np.pi] -= 2 * np.pi
        dphi[dphi < -np.pi] += 2 * np.pi
        dz, dr = til(z2) - rep(z1), til(r2) - rep(r1)
        deta = til(eta2) - rep(eta1)
        dR = np.sqrt(deta ** 2 + dphi ** 2)
        phi_slope = dphi / dr
        z0 = rep(z1) - rep(r1) * dz / dr
        if l1 in RADIUS and l2 in (6, 11):
            z_coord = RADIUS[l1] * dz / dr + z0
        else:
            z_coord = np.full(n1 * n2, np.nan)
    return dr, dphi, dz, dR, phi_slope, z0, z_coord


def select(q, phi_slope_max, z0_max, dR_max, remove_intersecting):
    dr, dphi, dz, dR, phi_slope, z0, z_coord = q
    with np.errstate(all="ignore"):
        good = (np.abs(phi_slope) < phi_slope_max) & (np.abs(z0) < z0_max) & (dR < dR_max)
        if remove_intersecting:
            good &= ~((z_coord > -Z_EDGE) & (z_coord < Z_EDGE))
    return good


def margins(q, phi_slope_max, z0_max, dR_max, remove_intersecting):
    """per candidate pair the smallest relative distance of a cut quantity to its cut (inf for nan / inf quantities)"""
    dr, dphi, dz, dR, phi_slope, z0, z_coord = q
    with np.errstate(all="ignore"):
        m = [np.abs(np.abs(phi_slope) / phi_slope_max - 1), np.abs(np.abs(z0) / z0_max - 1), np.abs(dR / dR_max - 1)]
        if remove_intersecting:
            m.append(np.abs(np.abs(z_coord) / Z_EDGE - 1))
        m = np.stack(m)
    m[~np.isfinite(m)] = np.inf
    return m.min(0)


def starts(sizes, n):
    sizes = [n] if sizes is None else list(sizes)
    assert sum(sizes) == n
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def build_edges(x, layer, pid, pt, *, pairs=None, phi_slope_max=0.005, z0_max=200, dR_max=1.7, remove_intersecting=True,
                sizes=None, want_margins=False):
    """dict: edge_index int64 [2, E], attr64 float64 [4, E], edge_attr float32 [4, E], y float32 [E] (relabelled when
    ``remove_intersecting``), y_naive, edge_pt float32 [E], n_corrected [events], edge_ptr [events + 1], n_candidates,
    margins (``want_margins``)"""
    x = np.asarray(x)
    layer, pid, pt = np.asarray(layer, np.int64), np.asarray(pid, np.int64), np.asarray(pt, np.float32)
    n = len(layer)
    pairs = list(PAIRS) if pairs is None else list(pairs)
    r, phi, z = (x[:, i] if n else np.zeros(0, np.float32) for i in range(3))
    eta = eta64(r, z)
    s = starts(sizes, n)
    cols, marg, n_cand, edge_ptr = [], [], 0, [0]
    for e in range(len(s) - 1):
        idx = np.arange(s[e], s[e + 1])
        for l1, l2 in pairs:
            h1, h2 = idx[layer[idx] == l1], idx[layer[idx] == l2]
            if not len(h1) or not len(h2):
                continue
            q = pair_quantities(r[h1], phi[h1], z[h1], eta[h1], r[h2], phi[h2], z[h2], eta[h2], l1, l2)
            good = select(q, phi_slope_max, z0_max, dR_max, remove_intersecting)
            n_cand += len(good)
            if want_margins:
                marg.append(margins(q, phi_slope_max, z0_max, dR_max, remove_intersecting))
            i1, i2 = np.repeat(h1, len(h2))[good], np.tile(h2, len(h1))[good]
            cols.append(np.stack([i1.astype(np.float64), i2.astype(np.float64), q[0][good] / 1000.0, q[1][good] / np.pi,
                                  q[2][good] / 1000.0, q[3][good]]))
        edge_ptr.append(sum(c.shape[1] for c in cols))
    cat = np.concatenate(cols, axis=1) if cols else np.zeros((6, 0))
    ei = cat[:2].astype(np.int64)
    y = ((pid[ei[0]] == pid[ei[1]]) & (pid[ei[0]] > 0)).astype(np.float32)
    out = dict(edge_index=ei, attr64=cat[2:], edge_attr=cat[2:].astype(np.float32), y_naive=y.copy(),
               edge_pt=pt[ei[0]], edge_ptr=np.array(edge_ptr, np.int64), n_candidates=n_cand)
    n_corr = np.zeros(len(s) - 1, np.int64)
    if remove_intersecting:
        y, n_corr = correct_truth_labels(layer, pid, ei, y, out["edge_ptr"])
    out.update(y=y, n_corrected=n_corr)
    if want_margins:
        out["margins"] = np.concatenate(marg) if marg else np.zeros(0)
    return out


def correct_truth_labels(layer, pid, ei, y, edge_ptr):
    """per (event, particle): with more than one barrel-to-endcap layer pair among its true edges, those of a
    precedence (barrel layer - 7) below the particle's largest become false"""
    y = y.copy()
    n_corr = np.zeros(len(edge_ptr) - 1, np.int64)
    l1, l2 = layer[ei[0]], layer[ei[1]]
    trans = (y == 1) & (l1 >= 7) & (l1 <= 10) & ((l2 == 6) | (l2 == 11))
    for e in range(len(edge_ptr) - 1):
        sel = np.zeros(len(y), bool)
        sel[edge_ptr[e]:edge_ptr[e + 1]] = True
        sel &= trans
        p1 = pid[ei[0]]
        for p in np.unique(p1[sel]):
            mine = sel & (p1 == p)
            kinds = set(zip(l1[mine].tolist(), l2[mine].tolist()))
            if len(kinds) > 1:
                top = max(a for a, _ in kinds)
                relabel = mine & (l1 < top)
                y[relabel] = 0
                n_corr[e] += int(relabel.sum())
    return y, n_corr


def n_truth_edges(layer, pid, pt, sizes=None):
    """per event ``{thld: n}``: per particle with id > 0 the products of its hit counts on consecutive occupied
    layers, counted where the pt of its first hit is > thld (compared in float32, as numpy compares a float32 scalar
    with a Python float)"""
    layer, pid, pt = np.asarray(layer, np.int64), np.asarray(pid, np.int64), np.asarray(pt, np.float32)
    s = starts(sizes, len(layer))
    out = []
    for e in range(len(s) - 1):
        d = dict.fromkeys(PT_THLDS, 0)
        lo, hi = s[e], s[e + 1]
        for p in np.unique(pid[lo:hi]):
            if p <= 0:
                continue
            hits = lo + np.flatnonzero(pid[lo:hi] == p)
            _, counts = np.unique(layer[hits], return_counts=True)
            n_segs = int(sum(int(a) * int(b) for a, b in zip(counts[1:], counts[:-1])))
            for t in d:
                if pt[hits[0]] > np.float32(t):
                    d[t] += n_segs
        out.append(d)
    return out


def measurement(y, edge_pt, n_truth):
    """the record of ``process`` for one event; a zero denominator gives numpy's inf / nan"""
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        n_true = y.sum()
        rec = {"n_edges": len(y), "n_true_edges": n_true, "n_false_edges": len(y) - n_true,
               **{f"n_truth_edge_{t}": n for t, n in n_truth.items()},
               "edge_purity": np.float64(n_true) / np.float64(len(y))}
        for t, den in n_truth.items():
            rec[f"edge_efficiency_{t}"] = np.float64(y[edge_pt > np.float32(t)].sum()) / np.float64(den)
    return rec


def get_measurements(records):
    """``GraphBuilder.get_measurements``: mean and std (ddof = 1) of every key"""
    out = {}
    with np.errstate(all="ignore"):
        for k in records[0]:
            v = np.array([float(r[k]) for r in records], np.float64)
            out[k] = v.mean()
            out[k + "_err"] = v.std(ddof=1) if len(v) > 1 else np.float64("nan")
    return out


def double(b):
    """the undirected doubling of ``to_pyg_data``, per event: [row|col ; col|row], three attributes negated, y twice"""
    ei, ea, y, ptr = b["edge_index"], b["edge_attr"], b["y"], b["edge_ptr"]
    neg = np.array([[-1], [-1], [-1], [1]], np.float32)
    eis, eas, ys = [], [], []
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        eis += [ei[:, lo:hi], ei[::-1, lo:hi]]
        eas += [ea[:, lo:hi], neg * ea[:, lo:hi]]
        ys += [y[lo:hi], y[lo:hi]]
    return np.concatenate(eis, axis=1), np.concatenate(eas, axis=1), np.concatenate(ys)
