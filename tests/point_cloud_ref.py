"""TEST INFRASTRUCTURE ONLY: a float64 numpy restatement of the point cloud builder (preprocessing/
point_cloud_builder.py, exatrkx_cell_features.py of the reference), written from its semantics: joins by key, the
selection and order of the hits, the feature columns, the truth columns, the sector wedges, the measurement records,
``stats`` and the truth edges.  tools/make_golden_point_cloud.py proves it against the reference on every
configuration of the golden file; the emulator and GPU tests then use it as the expected value of synthetic tables.

Everything is evaluated in float64 and rounded once to float32, as the product does.  The reference differs in places
by a float64 rounding (pandas' compensated group sums, BLAS in the rotation), which the one-ulp float32 rule absorbs.
"""

from __future__ import annotations

import numpy as np

DEFAULT_FEATURES = ("r", "phi", "z", "eta_rz", "u", "v", "charge_frac", "leta", "lphi", "lx", "ly", "lz", "geta", "gphi")
VOLUMES = (7, 8, 9, 12, 13, 14, 16, 17, 18)
PIXEL_LAYERS = sorted([(8, 2), (8, 4), (8, 6), (8, 8)] + [(7, l) for l in range(2, 16, 2)] + [(9, l) for l in range(2, 16, 2)])
CLOUD_KEYS = ("x", "edge_index", "layer", "particle_id", "pt", "reconstructable", "sector", "eta", "n_hits", "n_layers_hit")
DETECTOR_KEYS = ("volume_id", "layer_id", "module_id", "rot_xu", "rot_xv", "rot_xw", "rot_yu", "rot_yv", "rot_yw", "rot_zu",
                 "rot_zv", "rot_zw", "module_t", "pitch_u", "pitch_v")


def calc_eta(r, z):
    with np.errstate(all="ignore"):
        return -np.log(np.tan(np.arctan2(r, z) / 2.0))


def _angles(x, y, z):
    with np.errstate(all="ignore"):
        r3 = np.sqrt(x * x + y * y + z * z)
        return -np.log(np.tan(0.5 * np.arccos(z / r3))), np.arctan2(y, x)


def _lookup(keys, table_keys):
    """row of table_keys that holds each key, -1 where none; table_keys without duplicates"""
    order = np.argsort(table_keys, kind="stable")
    sk = table_keys[order]
    at = np.searchsorted(sk, keys)
    at = np.minimum(at, max(len(sk) - 1, 0))
    found = (sk[at] == keys) if len(sk) else np.zeros(len(keys), bool)
    return np.where(found, order[at] if len(sk) else 0, -1)


def truth_edge_index(pid):
    """[2, E]: the pairs i < j with the same non-zero id, lexicographic"""
    pid = np.asarray(pid, np.int64)
    out = []
    order = np.argsort(pid, kind="stable")
    sp = pid[order]
    starts = np.flatnonzero(np.r_[True, sp[1:] != sp[:-1]]) if len(sp) else np.zeros(0, np.int64)
    for a, b in zip(starts, np.r_[starts[1:], len(sp)]):
        if sp[a] == 0 or b - a < 2:
            continue
        idx = order[a:b]
        i, j = np.triu_indices(b - a, 1)
        out.append(np.stack([idx[i], idx[j]]))
    if not out:
        return np.zeros((2, 0), np.int64)
    e = np.concatenate(out, axis=1)
    return e[:, np.lexsort((e[1], e[0]))].astype(np.int64)


def build(tables, detector, *, n_sectors, pixel_only=True, sector_di=1e-4, sector_ds=1.1, measurement_mode=False, thld=0.5,
          remove_noise=False, feature_names=DEFAULT_FEATURES, feature_scale=None, add_true_edges=False):
    """(clouds: list of dicts of numpy arrays, records: list of dicts, stats: dict, margins: dict).  ``detector``: the
    columns of the detector table.  Raises ValueError where the product does."""
    hits, cells, parts, truth = ({k: np.asarray(v) for k, v in tables[t].items()} for t in ("hits", "cells", "particles", "truth"))
    scale = np.ones(len(feature_names)) if feature_scale is None else np.asarray(feature_scale, np.float64)
    hid = hits["hit_id"].astype(np.int64)
    if len(np.unique(hid)) != len(hid):
        raise ValueError("duplicate hit_ids")
    vol, lid, mod = (hits[k].astype(np.int64) for k in ("volume_id", "layer_id", "module_id"))
    pairs = PIXEL_LAYERS if pixel_only else sorted(set(zip(vol.tolist(), lid.tolist())))
    number = {p: i for i, p in enumerate(pairs)}
    layer = np.array([number.get(p, -1) for p in zip(vol.tolist(), lid.tolist())], np.int64)
    # cells of every hit on a layer, in cell order
    chit = _lookup(cells["hit_id"].astype(np.int64), hid)
    ok = chit >= 0
    n_cells = np.bincount(chit[ok], minlength=len(hid))
    if (n_cells[layer >= 0] == 0).any():
        raise ValueError("hits on a layer without cells")
    csum = np.bincount(chit[ok], weights=cells["value"].astype(np.float64)[ok], minlength=len(hid))
    ext = []
    for ch in ("ch0", "ch1"):
        c = cells[ch].astype(np.int64)[ok]
        lo, hi = np.full(len(hid), np.iinfo(np.int64).max), np.full(len(hid), np.iinfo(np.int64).min)
        np.minimum.at(lo, chit[ok], c)
        np.maximum.at(hi, chit[ok], c)
        ext.append(np.where(n_cells > 0, hi - lo + 1, 0))
    # truth and particles
    trow = _lookup(hid, truth["hit_id"].astype(np.int64))
    pid = np.where(trow >= 0, truth["particle_id"].astype(np.int64)[np.maximum(trow, 0)], 0)
    prow = _lookup(pid, parts["particle_id"].astype(np.int64))
    keep = (layer >= 0) & (trow >= 0) & np.where(pid == 0, not remove_noise, prow >= 0)
    k = np.flatnonzero(keep)
    x, y, z = (hits[c].astype(np.float64)[k] for c in "xyz")
    vol, lid, mod, layer, pid, prow = vol[k], lid[k], mod[k], layer[k], pid[k], prow[k]
    # the module of every kept hit
    dv, dl, dm = (np.asarray(detector[c]).astype(np.int64) for c in ("volume_id", "layer_id", "module_id"))
    span = int(max(dv.max(initial=0), dl.max(initial=0), dm.max(initial=0), vol.max(initial=0), lid.max(initial=0),
                   mod.max(initial=0))) + 1
    drow = _lookup((vol * span + lid) * span + mod, (dv * span + dl) * span + dm)
    if (drow < 0).any():
        raise ValueError("kept hits on a module that the detector table lacks")
    det = {c: np.asarray(detector[c]).astype(np.float64)[drow] for c in DETECTOR_KEYS[3:]}
    f = {"x": x, "y": y, "z": z}
    with np.errstate(all="ignore"):
        f["r"] = np.sqrt(x * x + y * y)
        f["phi"] = np.arctan2(y, x)
        f["eta_rz"] = calc_eta(f["r"], z)
        f["u"], f["v"] = x / (x * x + y * y), y / (x * x + y * y)
        cnt = n_cells[k].astype(np.float64)
        f["charge_frac"], f["cell_count"] = csum[k] / cnt, cnt
        f["cell_val"] = csum[k].astype(np.float32).astype(np.float64)
        lu, lv, lw = ext[0][k] * det["pitch_u"], ext[1][k] * det["pitch_v"], 2.0 * det["module_t"]
        g = [det[f"rot_{a}u"] * lu + det[f"rot_{a}v"] * lv + det[f"rot_{a}w"] * lw for a in "xyz"]
        f["lx"], f["ly"], f["lz"] = lu, lv, lw
        f["leta"], f["lphi"] = _angles(lu, lv, lw)
        f["geta"], f["gphi"] = _angles(*g)
        for v in VOLUMES:
            f[f"V{v}"] = (vol == v).astype(np.float64)
        X = np.stack([f[n] / s for n, s in zip(feature_names, scale)], axis=1).astype(np.float32) if len(k) else \
            np.zeros((0, len(feature_names)), np.float32)
        px, py, pz = (parts[c].astype(np.float64) for c in ("px", "py", "pz"))
        ppt = np.sqrt(px * px + py * py)
        peta = calc_eta(ppt, pz)
    noise = pid == 0
    pt = np.where(noise, 0.0, ppt[np.maximum(prow, 0)] if len(ppt) else 0.0)
    eta = np.where(noise, np.nan, peta[np.maximum(prow, 0)] if len(ppt) else np.nan)
    ids, inv, n_per = np.unique(pid, return_inverse=True, return_counts=True)
    n_layers = np.array([len(np.unique(lid[pid == i])) for i in ids], np.int64)
    n_hits, n_layers_hit = n_per[inv].astype(np.int64), n_layers[inv] if len(ids) else np.zeros(0, np.int64)
    cols = dict(layer=layer, particle_id=pid, pt=pt.astype(np.float32), eta=eta.astype(np.float32), n_hits=n_hits,
                n_layers_hit=n_layers_hit, reconstructable=((n_layers_hit >= 3) & (pid > 0)).astype(np.int64))
    stats = dict(n_hits=len(k), n_particles=len(ids), n_noise=int(noise.sum()), n_sector_hits=0, n_sector_particles=0)
    margins = dict(pt=np.abs(ppt[np.unique(prow[prow >= 0])] / thld - 1.0) if thld else np.zeros(0), wedge=[])
    margins["pt"] = margins["pt"][margins["pt"] != 0.0]          # (pt exactly equal to thld: placed on purpose)

    def cloud(sel, sector):
        c = {"x": X[sel], **{n: v[sel] for n, v in cols.items()}, "sector": sector.astype(np.int64)}
        c["edge_index"] = truth_edge_index(c["particle_id"]) if add_true_edges else np.zeros((2, 0), np.int64)
        return c

    clouds, records = [], []
    if n_sectors == 1:
        clouds.append(cloud(np.arange(len(k)), np.zeros(len(k))))
        stats["n_sector_hits"], stats["n_sector_particles"] = len(k), len(ids)
        margins["wedge"] = np.zeros(0)
        return clouds, records, stats, margins
    theta = np.pi / n_sectors
    slope = np.arctan(theta)
    u, v = f["u"], f["v"]
    for s in range(n_sectors):
        c_, s_ = np.cos(2 * s * theta), np.sin(2 * s * theta)
        ur = u * c_ - v * s_
        vr = u * s_ + v * c_
        inner = (vr > -slope * ur) & (vr < slope * ur)
        lower, upper = -sector_ds * slope * ur - sector_di, sector_ds * slope * ur + sector_di
        outer = (vr > lower) & (vr < upper)
        wedge, ext_w = inner & (ur > 0), outer & (ur > 0)
        with np.errstate(all="ignore"):
            for bound in (slope * ur, -slope * ur, lower, upper):
                margins["wedge"].append(np.abs(vr - bound) / np.maximum(np.abs(vr), np.abs(bound)))
        in_wedge = np.bincount(inv[wedge], minlength=len(ids))
        # the reference divides by the length of the particle's row of its per-particle table, which is 1
        assigned = (in_wedge / 1 >= 0.5) & (ids != 0)
        sel = np.flatnonzero(ext_w)
        clouds.append(cloud(sel, np.where(assigned[inv[sel]], s, -1)))
        there = np.unique(pid[sel])
        stats["n_sector_hits"] += len(sel)
        stats["n_sector_particles"] += len(there)
        if measurement_mode:
            num = den = 0
            for i in there:
                if i == 0:
                    continue
                g_ = pid == i
                n_total = 1          # (as above)
                if int((inner & g_ & (pt >= thld)).sum()) / n_total < 0.5:
                    continue
                den += 1
                num += int((outer & g_ & (pt > thld)).sum()) == n_total
            nw, ne = int(wedge.sum()), len(sel)
            records.append({"n_hits": nw, "n_hits_ext": ne, "n_hits_ratio": ne / nw if nw > 0 else 0,
                            "n_unique_pids": len(there), "majority_contained": num / den if den != 0 else 0})
    margins["wedge"] = np.concatenate(margins["wedge"]) if margins["wedge"] else np.zeros(0)
    return clouds, records, stats, margins


def get_measurements(records):
    out = {}
    if not records:
        return out
    with np.errstate(all="ignore"):
        for var in records[0]:
            v = np.array([float(r[var]) for r in records], np.float64)
            out[var] = v.mean()
            out[var + "_err"] = v.std(ddof=1) if len(v) > 1 else np.float64("nan")
    return out


def float_ok(got, want):
    """the float rule: every float32 value within one float32 ulp of the expected one or within 2^-40 absolute; NaN
    and infinities must coincide"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        near = (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.maximum(
            np.spacing(np.abs(want)).astype(np.float64), 2.0 ** -40)) & np.isfinite(got) & np.isfinite(want)
    return bool((same | near).all())
