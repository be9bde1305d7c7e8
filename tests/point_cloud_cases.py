"""TEST INFRASTRUCTURE ONLY: the cases of the point cloud builder, shared by the emulator and GPU runners
(test_point_cloud_emul.py, test_point_cloud_gpu.py); a case takes the device.

Expected values: the reference's own output for its bundled event (tests/golden/g24_point_cloud.npz, and the sector
clouds and graphs of g23_graph_builder.npz for the end-to-end case), and for synthetic tables the float64 restatement
tests/point_cloud_ref.py, which tools/make_golden_point_cloud.py proves against the reference.

Acceptance: the hit selection and order, layer, particle_id, reconstructable, sector, n_hits, n_layers_hit, edge_index
and every integer of the records and of stats are exact; x, pt and eta lie within one float32 ulp of the expected value
or within 2^-40 (both sides evaluate in float64 and round once: library functions that differ by a few float64 ulps
move the rounded value by at most one float32 step); record and summary floats within 1e-12 relative.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
import graph_builder_cases as GB
import point_cloud_ref as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "g24_point_cloud.npz"
TABLES = {"hits": ("hit_id", "x", "y", "z", "volume_id", "layer_id", "module_id"), "cells": ("hit_id", "ch0", "ch1", "value"),
          "particles": ("particle_id", "px", "py", "pz", "q", "vx", "vy"), "truth": ("hit_id", "particle_id")}
EXACT = ("layer", "particle_id", "reconstructable", "sector", "n_hits", "n_layers_hit", "edge_index")
FLOATS = ("x", "pt", "eta")
CONFIGS = {
    "g23": dict(n_sectors=2, pixel_only=True, measurement_mode=True, thld=0.9, add_true_edges=True),
    "one": dict(n_sectors=1),
    "eight_no_noise": dict(n_sectors=8, remove_noise=True, measurement_mode=True),
    "strips": dict(n_sectors=2, pixel_only=False, measurement_mode=True),
    "features": dict(n_sectors=2, feature_names=("x", "cell_count", "V8", "cell_val", "y", "geta", "V13", "eta_rz"),
                     feature_scale=(1000.0, 2.0, 1.0, 0.5, 100.0, 3.0, 1.0, 4.0)),
}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def golden_tables():
    g = golden()
    return {t: {c: g[f"{t}_{c}"] for c in cols} for t, cols in TABLES.items()}


def golden_detector():
    g = golden()
    return {c: g[f"detector_{c}"] for c in R.DETECTOR_KEYS}


def golden_clouds(name):
    g = golden()
    out = []
    for s in range(CONFIGS[name]["n_sectors"]):
        c = {k: g[f"{name}_s{s}_{k}"] for k in (*FLOATS, *EXACT[:-1])}
        e = g.get(f"{name}_s{s}_edge_index")
        c["edge_index"] = np.zeros((2, 0), np.int64) if e is None else e.astype(np.int64)
        out.append(c)
    return out


def on(tables, device):
    return {t: {c: torch.from_numpy(np.ascontiguousarray(v)).to(device) for c, v in cols.items()} for t, cols in tables.items()}


def assert_cloud(got, want, what):
    assert got.y.shape == (0,) and got.y.dtype == torch.float32, what
    for k in EXACT:
        a = getattr(got, k)
        assert a.dtype == torch.int64 and str(a.device).startswith(str(got.x.device).split(":")[0]), f"{what}: {k}"
        assert np.array_equal(a.cpu().numpy(), want[k]), f"{what}: {k} differs"
    for k in FLOATS:
        a = getattr(got, k)
        assert a.dtype == torch.float32 and R.float_ok(a.cpu().numpy(), want[k]), f"{what}: {k} outside the float rule"


def assert_records(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert list(a) == list(b), what
        for k in ("n_hits", "n_hits_ext", "n_unique_pids"):
            assert int(a[k]) == int(b[k]), f"{what}: {k} {a[k]} against {b[k]}"
        for k in ("n_hits_ratio", "majority_contained"):
            assert abs(float(a[k]) - float(b[k])) <= 1e-12 * abs(float(b[k])), f"{what}: {k} {a[k]} against {b[k]}"


def assert_same_data(a, b, what):
    assert sorted(a.keys()) == sorted(b.keys()), what
    for k in a.keys():
        u, v = getattr(a, k), getattr(b, k)
        assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u.cpu().view(torch.uint8), v.cpu().view(torch.uint8)), \
            f"{what}: {k}"


def check(device, tables, detector, what="", **kw):
    """the builder against the restatement: clouds, records, stats, and the collated batch against collate(list)"""
    want_clouds, want_records, want_stats, _ = R.build(tables, detector, **kw)
    b = G.PointCloudBuilder(detector=G.load_detector(detector), **kw)
    got = b.build(on(tables, device), evtid=7)
    assert isinstance(got, list) and len(got) == kw["n_sectors"], what
    for s, (c, w) in enumerate(zip(got, want_clouds)):
        assert_cloud(c, w, f"{what} sector {s}")
    assert b.stats == {7: want_stats}, f"{what}: stats {b.stats} against {want_stats}"
    assert_records(b.measurements, want_records, what)
    batch = b.build(on(tables, device), evtid=7, collated=True)
    assert_same_data(batch, G.collate(got), f"{what}: collated")
    return got, b


# ----------------------------------------------------------------------------------------- the reference's event
def golden_case(name):
    def case(device):
        g, kw = golden(), CONFIGS[name]
        b = G.PointCloudBuilder(detector=G.load_detector(golden_detector()), **kw)
        clouds = b.build(on(golden_tables(), device), evtid=1)
        for s, (c, w) in enumerate(zip(clouds, golden_clouds(name))):
            assert_cloud(c, w, f"{name} sector {s}")
        assert list(b.stats[1]) == [str(k) for k in g["stats_keys"]]
        assert list(b.stats[1].values()) == g[f"{name}_stats"].tolist()
        keys = [str(k) for k in g["record_keys"]]
        assert_records(b.measurements, [dict(zip(keys, row)) for row in g[f"{name}_records"]], name)
        total = b.get_measurements()
        assert len(total) == len(g[f"{name}_measurements"])
        if total:
            assert list(total) == [str(k) for k in g["measurements_keys"]]
            for k, w in zip(total, g[f"{name}_measurements"]):
                assert abs(float(total[k]) - w) <= 1e-12 * abs(w), k

    case.__name__ = f"case_golden_{name}"
    return case


def case_end_to_end(device):
    """event tables -> PointCloudBuilder -> GraphBuilder -> the reference's graphs of g23_graph_builder.npz"""
    g23 = GB.golden()
    b = G.PointCloudBuilder(detector=G.load_detector(golden_detector()), **CONFIGS["g23"])
    batch = b.build(on(golden_tables(), device), collated=True)
    ptr = batch.ptr.cpu().tolist()
    assert ptr == [0, 843, 843 + 750]
    for s in (0, 1):
        a, z = ptr[s], ptr[s + 1]
        for k in ("layer", "particle_id", "reconstructable", "sector"):
            assert np.array_equal(getattr(batch, k)[a:z].cpu().numpy(), g23[f"sector{s}_{k}"]), (s, k)
        for k in FLOATS:
            assert R.float_ok(getattr(batch, k)[a:z].cpu().numpy(), g23[f"sector{s}_{k}"]), (s, k)
    gb = G.GraphBuilder(measurement_mode=True)
    graph = gb.build(batch)
    edges = graph.edge_index.cpu().numpy()
    keys = [str(k) for k in g23["measurement_keys"]]
    at = 0
    for s in (0, 1):
        want = g23[f"sector{s}_edge_index"]
        m = want.shape[1]
        assert np.array_equal(edges[:, at:at + m] - ptr[s], want), f"sector {s}: the graph's edges"
        assert np.array_equal(graph.y[at:at + m].cpu().numpy(), g23[f"sector{s}_y"])
        GB.assert_attr(graph.edge_attr[at:at + m].cpu().numpy().T, g23[f"sector{s}_edge_attr"].T, f"sector {s}",
                       extra=g23[f"sector{s}_attr_bound"])
        GB.assert_record(gb.measurements[s], dict(zip(keys, g23[f"sector{s}_measurement"])), f"sector {s}")
        at += m
    assert at == edges.shape[1]


# ------------------------------------------------------------------------------------------------ synthetic tables
def detector_table(seed=0):
    g = np.random.default_rng(seed)
    rows = [(v, l, m) for v in (7, 8, 9, 12, 13) for l in range(2, 16, 2) for m in range(3)]
    d = {k: np.array([r[i] for r in rows], np.int64) for i, k in enumerate(("volume_id", "layer_id", "module_id"))}
    for k in R.DETECTOR_KEYS[3:12]:
        d[k] = g.uniform(-1, 1, len(rows))
    d["module_t"], d["pitch_u"] = g.choice([0.15, 0.25], len(rows)), np.full(len(rows), 0.05)
    d["pitch_v"] = g.choice([0.05625, 1.2], len(rows))
    return d


def event(rows, particles, seed=0, cells_per_hit=None, shuffle=True):
    """tables from hit rows (phi in degrees, r, z, volume_id, layer_id, particle id or None: no truth row) and particles
    {id: (px, py, pz)}; hit ids are neither dense nor sorted, the other tables are shuffled"""
    g = np.random.default_rng(seed)
    n = len(rows)
    hid = (g.permutation(n) * 3 + 11).astype(np.int64)
    phi = np.deg2rad(np.array([r[0] for r in rows], np.float64))
    rr = np.array([r[1] for r in rows], np.float64)
    hits = dict(hit_id=hid, x=rr * np.cos(phi), y=rr * np.sin(phi), z=np.array([r[2] for r in rows], np.float64),
                volume_id=np.array([r[3] for r in rows], np.int64), layer_id=np.array([r[4] for r in rows], np.int64),
                module_id=g.integers(0, 3, n))
    per = np.asarray(g.integers(1, 9, n) if cells_per_hit is None else cells_per_hit, np.int64)
    chit = np.repeat(hid, per)
    cells = dict(hit_id=chit, ch0=g.integers(0, 400, len(chit)), ch1=g.integers(0, 1200, len(chit)),
                 value=g.uniform(0.01, 1.0, len(chit)))
    has = np.array([r[5] is not None for r in rows], bool)
    truth = dict(hit_id=hid[has], particle_id=np.array([r[5] for r in rows if r[5] is not None], np.int64))
    ids = list(particles)
    parts = dict(particle_id=np.array(ids, np.int64), **{k: np.array([particles[i][j] for i in ids], np.float64)
                                                          for j, k in enumerate(("px", "py", "pz"))})
    parts.update(q=np.ones(len(ids)), vx=np.zeros(len(ids)), vy=np.zeros(len(ids)))
    tables = dict(hits=hits, cells=cells, particles=parts, truth=truth)
    if shuffle:
        for t in ("cells", "particles", "truth"):
            o = g.permutation(len(next(iter(tables[t].values()))))
            tables[t] = {k: v[o] for k, v in tables[t].items()}
    return tables


PIXEL = [(8, l) for l in (2, 4, 6, 8)] + [(v, l) for v in (7, 9) for l in range(2, 16, 2)]


def random_event(seed, n, n_particles=None):
    g = np.random.default_rng(seed)
    n_particles = max(1, n // 6) if n_particles is None else n_particles
    ids = [int(i) for i in g.integers(1, 2 ** 60, n_particles)]
    particles = {i: tuple(g.normal(0, 0.6, 3)) for i in ids}
    rows = []
    for _ in range(n):
        v, l = PIXEL[g.integers(len(PIXEL))] if g.uniform() < 0.85 else (int(g.choice([12, 13])), int(g.choice([2, 4])))
        u = g.uniform()
        pid = 0 if u < 0.1 else (987654321 if u < 0.15 else (None if u < 0.18 else ids[g.integers(len(ids))]))
        rows.append((g.uniform(-180, 180), g.uniform(30, 170), g.uniform(-500, 500), v, l, pid))
    return event(rows, particles, seed)


def case_hit_counts(device):
    """0, 1, 63, 64, 65 and 257 hits (a wave, its edges, more than one block); 1, 2, 3 and 64 sectors"""
    det = detector_table()
    for n, sectors in ((0, 1), (0, 3), (1, 64), (63, 2), (64, 3), (65, 1), (257, 64), (257, 2)):
        check(device, random_event(n, n), det, f"{n} hits, {sectors} sectors", n_sectors=sectors, measurement_mode=True,
              add_true_edges=True, thld=0.4)
    check(device, random_event(5, 257), det, "257 hits with strips, no noise", n_sectors=3, pixel_only=False,
          remove_noise=True, measurement_mode=True)


def case_cells_per_hit(device):
    """hits with 1, 63, 64, 65 and 300 cells, cells of dropped hits and of hits that are not in the table"""
    det = detector_table()
    rows = [(10.0 * i, 50.0 + i, 5.0 * i, 8, 2, 5) for i in range(5)] + [(0.0, 60.0, 1.0, 12, 2, 5), (5.0, 61.0, 1.0, 8, 4, None)]
    t = event(rows, {5: (1.0, 0.5, 0.2)}, 3, cells_per_hit=[1, 63, 64, 65, 300, 7, 9])
    t["cells"] = {k: np.concatenate([v, np.array([999999, 5, 5, 0.5][i:i + 1], v.dtype)]) for i, (k, v) in enumerate(t["cells"].items())}
    got, _ = check(device, t, det, "cells per hit", n_sectors=1, feature_names=("cell_count", "cell_val", "charge_frac", "lx", "ly"))
    assert got[0].x[:, 0].cpu().tolist() == [1, 63, 64, 65, 300]
    t = event(rows, {5: (1.0, 0.5, 0.2)}, 3, cells_per_hit=[1, 2, 0, 4, 5, 6, 7])
    with pytest.raises(ValueError, match="without cells"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=1).build(on(t, device))
    with pytest.raises(ValueError, match="without cells"):
        R.build(t, det, n_sectors=1)


def case_filtering_and_layers(device):
    """a truth id missing from particles, hits on non-pixel volumes, hits without a truth row; a particle on (7, 2),
    (8, 2), (9, 2) and twice on (7, 4) has two distinct layer_ids: not reconstructable"""
    det = detector_table()
    rows = [(0, 40, -600, 7, 2, 21), (1, 50, 0, 8, 2, 21), (2, 60, 600, 9, 2, 21), (3, 45, -700, 7, 4, 21), (4, 46, -700, 7, 4, 21),
            (5, 40, 0, 8, 2, 22), (6, 80, 0, 8, 4, 22), (7, 120, 0, 8, 6, 22),       # reconstructable
            (8, 40, 0, 8, 2, 99), (9, 40, 0, 12, 2, 22), (10, 40, 0, 8, 2, None), (11, 40, 0, 8, 8, 0)]
    t = event(rows, {21: (1, 0, 0), 22: (0, 2, 1), 23: (1, 1, 1)}, 4)
    got, b = check(device, t, det, "filtering", n_sectors=1)
    c = got[0]
    assert c.particle_id.cpu().tolist() == [21] * 5 + [22] * 3 + [0]
    assert c.layer.cpu().tolist() == [0, 7, 11, 1, 1, 7, 8, 9, 10]
    assert c.n_layers_hit.cpu().tolist() == [2] * 5 + [3] * 3 + [1] and c.n_hits.cpu().tolist() == [5] * 5 + [3] * 3 + [1]
    assert c.reconstructable.cpu().tolist() == [0] * 5 + [1] * 3 + [0]
    assert b.stats[7] == dict(n_hits=9, n_particles=3, n_noise=1, n_sector_hits=9, n_sector_particles=3)
    assert torch.isnan(c.eta[-1]) and c.pt[-1] == 0
    got, _ = check(device, t, det, "filtering, strips, no noise", n_sectors=1, pixel_only=False, remove_noise=True)
    assert got[0].layer.cpu().tolist() == [0, 2, 6, 1, 1, 2, 3, 4, 7]      # (12, 2) is the event's eighth pair
    assert got[0].n_hits.cpu().tolist() == [5] * 5 + [4] * 4


def case_sector_assignment(device):
    """three sectors, sector_ds = 3: the wedge's half angle is 38.9 degrees, the extended wedge's 67.6 degrees, sector 0
    around phi = 0, sector 1 around -120, sector 2 around +120 degrees.  The reference divides the hits in the wedge by
    the LENGTH OF THE PARTICLE'S ROW of its per-particle table (1), so one hit in the wedge assigns the particle."""
    det = detector_table()
    rows = ([(0, 50, 0, 8, 2, 1), (10, 90, 0, 8, 4, 1), (50, 120, 0, 8, 6, 1), (55, 170, 0, 8, 8, 1)]     # half in wedge 0
            + [(5, 50, 0, 8, 2, 2)] + [(45 + i, 60 + 9 * i, 0, 8, 4, 2) for i in range(3)]                   # a quarter
            + [(50, 50, 0, 8, 2, 3), (52, 90, 0, 8, 4, 3)]                                                    # none in a wedge
            + [(62, 50, 0, 8, 2, 4), (64, 90, 0, 8, 4, 4)]                                                    # in two extended wedges
            + [(0, 100, 0, 8, 2, 0)])
    t = event(rows, {i: (1.0, 0.0, 0.3 * i) for i in (1, 2, 3, 4)}, 5)
    got, b = check(device, t, det, "sector assignment", n_sectors=3, sector_ds=3.0, measurement_mode=True, add_true_edges=True)
    c0, c1, c2 = got
    assert c0.particle_id.cpu().tolist() == [1] * 4 + [2] * 4 + [3] * 2 + [4] * 2 + [0]
    assert c0.sector.cpu().tolist() == [0] * 8 + [-1] * 5          # 3 and 4 have no hit in the wedge; noise never
    # the extended wedge of sector 2 starts at 52.4 degrees: the last hit of 1 and both of 4
    assert c1.particle_id.numel() == 0 and c2.particle_id.cpu().tolist() == [1, 4, 4] and c2.sector.cpu().tolist() == [-1] * 3
    assert b.measurements[1]["n_hits_ratio"] == 0 and b.measurements[1]["n_hits"] == 0 and b.measurements[1]["n_unique_pids"] == 0
    assert b.measurements[0]["n_hits"] == 4 and b.measurements[0]["n_hits_ext"] == 13 and b.measurements[0]["n_unique_pids"] == 5


def case_threshold(device):
    """pt exactly equal to thld (0.5 = sqrt(0.5^2 + 0^2), exactly representable): the first wedge test takes it
    (>=), the extended one does not (>)"""
    det = detector_table()
    rows = [(1, 50, 0, 8, 2, 1), (2, 50, 0, 8, 2, 2), (3, 50, 0, 8, 2, 3), (4, 60, 0, 8, 4, 3), (5, 50, 0, 8, 2, 4)]
    t = event(rows, {1: (0.5, 0.0, 0.1), 2: (0.75, 0.0, 0.1), 3: (0.0, 0.75, 0.2), 4: (0.25, 0.0, 0.1)}, 6)
    _, b = check(device, t, det, "threshold", n_sectors=2, measurement_mode=True, thld=0.5)
    # 1: counted, not contained; 2: contained (one hit); 3: two hits, the reference wants exactly one; 4: below
    assert b.measurements[0]["majority_contained"] == 1 / 3 and b.measurements[1]["majority_contained"] == 0
    assert b.get_measurements()["majority_contained"] == 1 / 6


def case_truth_edges(device):
    """an all-noise event, a particle with one hit, one with 70 (rows longer than a wave), ids above 2^53 that differ
    in the lowest bit; get_truth_edge_index against the reference's own output for a toy input"""
    det = detector_table()
    g = golden()
    e = G.get_truth_edge_index(torch.from_numpy(g["toy_pid"]).to(device))
    assert e.dtype == torch.int64 and np.array_equal(e.cpu().numpy(), g["toy_edges"])
    for pid in (np.zeros(0, np.int64), np.zeros(9, np.int64), np.array([4]), np.array([0, 3, 3])):
        assert np.array_equal(G.get_truth_edge_index(torch.from_numpy(pid).to(device)).cpu().numpy(), R.truth_edge_index(pid))
    big = 2 ** 54
    rows = ([(i % 40 - 20, 40 + i, i, 8, 2 + 2 * (i % 4), big) for i in range(70)] + [(0, 50, 0, 8, 2, big + 1)] * 3
            + [(3, 50, 0, 8, 2, 17)] + [(2, 50, 0, 8, 2, 0)] * 4)
    rows = [rows[i] for i in np.random.default_rng(1).permutation(len(rows))]
    t = event(rows, {big: (1, 0, 0), big + 1: (0, 1, 0), 17: (1, 1, 0)}, 7)
    got, _ = check(device, t, det, "truth edges", n_sectors=2, add_true_edges=True)
    assert got[0].edge_index.shape == (2, 70 * 69 // 2 + 3)
    rows = [(i, 50, 0, 8, 2, 0) for i in range(-20, 20)]
    got, _ = check(device, event(rows, {}, 8), det, "all noise", n_sectors=2, add_true_edges=True, measurement_mode=True)
    assert got[0].edge_index.shape == (2, 0) and got[0].sector.cpu().tolist() == [-1] * 40


def case_errors(device):
    det = detector_table()
    t = random_event(9, 40)
    t["hits"]["hit_id"][5] = t["hits"]["hit_id"][30]
    with pytest.raises(ValueError, match="duplicate hit_ids"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=2).build(on(t, device))
    t = random_event(9, 40)
    t["hits"]["module_id"][:] = 5
    with pytest.raises(ValueError, match="module"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=2).build(on(t, device))
    t = random_event(9, 40)
    t["hits"]["volume_id"][3] = 64
    with pytest.raises(ValueError, match=r"outside \[0, 64\)"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=2).build(on(t, device))
    with pytest.raises(ValueError, match="unknown"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=2, feature_names=("r", "nope"), feature_scale=(1, 1))
    with pytest.raises(ValueError, match="lacks the columns"):
        G.PointCloudBuilder(detector=G.load_detector(det), n_sectors=2).build(dict(random_event(9, 4), truth={}))


def case_determinism(device):
    det = detector_table()
    t = on(random_event(11, 257), device)
    kw = dict(detector=G.load_detector(det), n_sectors=5, add_true_edges=True, measurement_mode=True)
    a, b = G.PointCloudBuilder(**kw), G.PointCloudBuilder(**kw)
    for u, v in zip(a.build(t), b.build(t)):
        assert_same_data(u, v, "two runs")
    assert a.measurements == b.measurements and a.stats == b.stats
    assert dict(a.hparams)["n_sectors"] == 5 and "detector" not in a.hparams


CASES = (*(golden_case(n) for n in CONFIGS), case_end_to_end, case_hit_counts, case_cells_per_hit, case_filtering_and_layers,
         case_sector_assignment, case_threshold, case_truth_edges, case_errors, case_determinism)
