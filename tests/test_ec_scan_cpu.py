"""The restatement of the EC threshold scan (oracle (b) of tests/ec_scan_cases.py: ``track_graph_ref`` on
``edge_index[:, w > t]`` and ``ec_metrics_ref.bcs_at``) against the reference's own ``get_all_ec_stats`` records
(``tests/golden/g22_ec_scan.npz``, tools/make_golden_ec_scan.py), and the host-only parts of the scan.  No GPU, no
emulator."""

import numpy as np
import pytest

import ec_scan_cases as C
import ec_scan_golden as GOLD
import gnn_tracking_amd as G


def test_fixture_shape():
    z = GOLD.golden()
    assert GOLD.GOLDEN.stat().st_size < 64 * 1024
    assert z["thresholds"].tolist() == [0.1, 0.3, 0.5, 0.7, 0.9] and min(z["thresholds"]) > 0
    assert tuple(z["keys"].tolist()) == C.KEYS and len(C.KEYS) == 1 + 12 + 12 + 3 + 9
    for name in GOLD.GRAPHS:
        ei, pid, good, w, y = GOLD.inputs(name)
        assert pid.shape == (600,) and ei.shape == (2, len(w)) and y.shape == w.shape and w.dtype == np.float32
        assert z[f"{name}_records"].shape == (5, len(C.KEYS))
        assert np.array_equal(y, C.labels_of(ei, pid)) and 0.5 < good.mean() < 0.9
        for t in (0.3, 0.7):     # weights equal to a threshold, of both labels
            at = w == np.float32(t)
            assert (at & y).sum() == 3 and (at & ~y).sum() == 3


@pytest.mark.parametrize("name", GOLD.GRAPHS)
def test_restatement_equals_the_reference(name):
    ei, pid, good, w, y = GOLD.inputs(name)
    want, tables = C.restated(ei, pid, good, w, y, GOLD.thresholds())
    GOLD.assert_against_reference(want, name, "the restatement on")
    for t in tables:   # at every threshold a particle is split and a particle is whole
        assert (t["n_segments"] == 1).any() and (t["n_segments"] > 1).any() and len(t["pid"]) > 40
    ref = GOLD.reference_records(name)
    assert all(r[k] == 0 for r in ref for k in C.ORPHAN_KEYS), "the reference counts orphans now"
    assert all(r["n_orphan_total"] > 0 for r in want), "the restated orphan counts have nothing to show"
    assert ref[1]["TPR"] != ref[1]["TPR_thld"] and ref[0]["n_segments"] < ref[4]["n_segments"]


def test_bcs_from_counts_is_the_restatement():
    """the expressions that the class and the scan share, on counts with every zero denominator"""
    import ec_metrics_ref as E

    for tp, fp, p, n in ((3, 2, 5, 7), (0, 0, 0, 0), (0, 0, 4, 0), (0, 3, 0, 3), (4, 0, 4, 6), (5, 7, 5, 7)):
        got = G.metrics.bcs_from_counts(tp, fp, p, n)
        assert tuple(got) == C.BCS_KEYS
        w = np.r_[np.ones(tp), np.zeros(p - tp), np.ones(fp), np.zeros(n - fp)].astype(np.float32)
        y = np.r_[np.ones(p, dtype=bool), np.zeros(n, dtype=bool)]
        assert got == E.bcs_at(w, y, 0.5), (tp, fp, p, n)
    big = G.metrics.bcs_from_counts(2 ** 31, 5, 2 ** 32, 2 ** 33)    # (the MCC's product exceeds int64)
    assert 0 < big["MCC"] < 1 and big["n_predicted_true"] == 2 ** 31 + 5 and big["TPR"] == 0.5


def test_host_side_refusals_need_no_device():
    with pytest.raises(ValueError, match="NaN"):
        G.ec_threshold_scan(None, None, [0.5, float("nan")])
    with pytest.raises(ValueError, match="257"):
        G.ec_threshold_scan(None, None, np.linspace(0, 1, 257).tolist())
