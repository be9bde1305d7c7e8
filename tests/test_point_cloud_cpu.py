"""The float64 restatement of the point cloud builder (tests/point_cloud_ref.py) against the reference's own output
(tests/golden/g24_point_cloud.npz, tools/make_golden_point_cloud.py) and against the sector clouds of
g23_graph_builder.npz: the oracle of the emulator and GPU tests is pinned here, without the device.  Also the host-only
parts of the product: load_detector, read_event, get_measurements."""

import gzip

import numpy as np
import pytest

import gnn_tracking_amd as G
import graph_builder_cases as GB
import point_cloud_cases as C
import point_cloud_ref as R


def test_golden_holds_every_configuration():
    g = C.golden()
    assert tuple(str(c) for c in g["configs"]) == tuple(C.CONFIGS)
    assert C.GOLDEN.stat().st_size < 1 << 20
    assert len(g["hits_hit_id"]) == 5527 and len(g["cells_hit_id"]) == 18564 and len(g["particles_particle_id"]) == 548


@pytest.mark.parametrize("name", C.CONFIGS)
def test_restatement_reproduces_the_reference(name):
    g = C.golden()
    clouds, records, stats, margins = R.build(C.golden_tables(), C.golden_detector(), **C.CONFIGS[name])
    want = C.golden_clouds(name)
    assert len(clouds) == len(want)
    for s, (a, b) in enumerate(zip(clouds, want)):
        for k in C.EXACT:
            assert a[k].dtype == np.int64 and np.array_equal(a[k], b[k]), (s, k)
        for k in C.FLOATS:
            assert a[k].dtype == np.float32 and R.float_ok(a[k], b[k]), (s, k)
    assert list(stats.values()) == g[f"{name}_stats"].tolist() and list(stats) == [str(k) for k in g["stats_keys"]]
    keys = [str(k) for k in g["record_keys"]]
    C.assert_records(records, [dict(zip(keys, row)) for row in g[f"{name}_records"]], name)
    total = R.get_measurements(records)
    assert len(total) == len(g[f"{name}_measurements"])
    for k, w in zip(total, g[f"{name}_measurements"]):
        assert abs(float(total[k]) - w) <= 1e-12 * abs(w), k
    # the conditions on the inputs
    assert not (margins["pt"] < 1e-9).any() and not (margins["wedge"] < 1e-12).any()


def test_restatement_reproduces_the_clouds_of_the_graph_builder_golden():
    g23 = GB.golden()
    clouds = R.build(C.golden_tables(), C.golden_detector(), **C.CONFIGS["g23"])[0]
    for s, c in enumerate(clouds):
        for k in ("layer", "particle_id", "reconstructable", "sector"):
            assert np.array_equal(c[k], g23[f"sector{s}_{k}"]), (s, k)
        for k in C.FLOATS:
            assert R.float_ok(c[k], g23[f"sector{s}_{k}"]), (s, k)


def test_pinned_reference_behaviour():
    """noise has pt 0 and eta NaN; n_layers_hit counts layer_id values; a particle is assigned to every sector whose
    wedge holds one of its hits"""
    g = C.golden()
    c = C.golden_clouds("g23")
    noise = c[0]["particle_id"] == 0
    assert noise.any() and np.isnan(c[0]["eta"][noise]).all() and not np.isnan(c[0]["eta"][~noise]).any()
    assert (c[0]["pt"][noise] == 0).all() and (c[0]["sector"][noise] == -1).all()
    both = np.intersect1d(c[0]["particle_id"][c[0]["sector"] == 0], c[1]["particle_id"][c[1]["sector"] == 1])
    assert len(both) > 0, "no particle of the bundled event is assigned to both sectors"
    assert g["g23_stats"].tolist() == [2783, 419, 152, 1593, 253]
    assert np.array_equal(R.truth_edge_index(g["toy_pid"]), g["toy_edges"])
    assert len(np.unique(g["toy_pid"].astype(np.float64))) < len(np.unique(g["toy_pid"]))


def test_float_rule():
    one = np.float32(1.0)
    assert R.float_ok([np.nextafter(one, np.float32(2))], [one]) and not R.float_ok([one + 3 * np.spacing(one)], [one])
    assert R.float_ok([np.float32(2.0 ** -41)], [np.float32(0)]) and not R.float_ok([np.float32(2.0 ** -39)], [np.float32(0)])
    assert R.float_ok([np.nan], [np.nan]) and not R.float_ok([np.nan], [one]) and not R.float_ok([np.inf], [one])


def test_load_detector():
    d = C.golden_detector()
    det = G.load_detector(d)
    assert det["rows"].shape == (len(d["volume_id"]), 12) and det["rows"].dtype == np.float64
    assert det["index"].dtype == np.int32 and det["index"].nbytes == 4 * int(np.prod(det["dims"]))   # (the reference: 72 bytes each)
    assert tuple(det["dims"]) == tuple(int(d[k].max()) + 1 for k in ("volume_id", "layer_id", "module_id"))
    for j in (0, 17, len(d["volume_id"]) - 1):
        row = det["index"][d["volume_id"][j], d["layer_id"][j], d["module_id"][j]]
        assert row == j
        assert det["rows"][row].tolist() == [float(d[k][j]) for k in R.DETECTOR_KEYS[3:]]
    assert (det["index"] >= 0).sum() == len(d["volume_id"])
    with pytest.raises(ValueError):
        G.load_detector(dict(d, module_id=-d["module_id"] - 1))
    with pytest.raises(KeyError):
        G.load_detector({k: v for k, v in d.items() if k != "pitch_u"})


def test_read_event_round_trip(tmp_path):
    t = C.golden_tables()
    for name, cols in C.TABLES.items():
        with gzip.open(tmp_path / f"event000000009-{name}.csv.gz", "wt") as f:
            f.write(",".join(cols) + "\n")
            for j in range(4):
                f.write(",".join(repr(t[name][c][j].item()) for c in cols) + "\n")
    got = G.read_event(tmp_path / "event000000009")
    for name, cols in C.TABLES.items():
        for c in cols:
            assert got[name][c].dtype == t[name][c].dtype and np.array_equal(got[name][c], t[name][c][:4]), (name, c)


def test_get_measurements():
    b = G.PointCloudBuilder(detector=G.load_detector(C.golden_detector()), n_sectors=2, measurement_mode=True)
    assert b.get_measurements() == {} and b.hparams.n_sectors == 2 and b.hparams.thld == 0.5
    g = C.golden()
    keys = [str(k) for k in g["record_keys"]]
    b.measurements.extend(dict(zip(keys, row)) for row in g["g23_records"])
    total = b.get_measurements()
    assert list(total) == [str(k) for k in g["measurements_keys"]]
    for k, w in zip(total, g["g23_measurements"]):
        assert abs(float(total[k]) - w) <= 1e-12 * abs(w), k
    b.measurements[:] = b.measurements[:1]
    assert np.isnan(b.get_measurements()["n_hits_err"])
