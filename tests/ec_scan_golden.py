"""The reference's own ``get_all_ec_stats`` records (``tests/golden/g22_ec_scan.npz``, written by
tools/make_golden_ec_scan.py) for the tests of the EC threshold scan: the restatement of ``ec_scan_cases`` is held
against them on the CPU (tests/test_ec_scan_cpu.py), the device on the emulator and on the GPU.  All keys are compared
except the three orphan counts, which the reference returns as zeros (the defect ``get_orphan_counts`` documents).
Integer-derived keys are compared exactly, the three means of the summary at 1e-12 (relative): a float64 mean of 49
values in [0, 50] carries at most n * eps of rounding, whatever the order of the additions."""

from __future__ import annotations

import functools
import pathlib

import numpy as np

import ec_scan_cases as C
import track_graph_cases as TC

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "g22_ec_scan.npz"
GRAPHS = ("g0", "g1", "g2")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def inputs(name):
    z = golden()
    return z[f"{name}_edge_index"], z[f"{name}_pid"], z[f"{name}_pt"] > 0.9, z[f"{name}_w"], z[f"{name}_y"]


def thresholds():
    return golden()["thresholds"].tolist()


def reference_records(name):
    z = golden()
    keys = tuple(z["keys"].tolist())
    assert keys == C.KEYS, keys
    return [dict(zip(keys, row)) for row in z[f"{name}_records"].tolist()]


def assert_against_reference(got, name, what):
    """every key but the orphan counts"""
    want = reference_records(name)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g) == C.KEYS
        for k in C.KEYS:
            if k in C.ORPHAN_KEYS:
                continue
            if k in TC.MEANS:
                assert abs(g[k] - w[k]) <= 1e-12 * abs(w[k]), f"{what} {name}: {k} = {g[k]!r}, the reference {w[k]!r}"
            else:
                assert g[k] == w[k], f"{what} {name}: {k} = {g[k]!r}, the reference {w[k]!r}"


def check_device(name, device):
    """the scan on the golden inputs against the reference's records and, exactly, against the restatement's orphans"""
    import gnn_tracking_amd as G

    ei, pid, good, w, y = inputs(name)
    data = TC.data_of(ei, pid, good, device)
    assert np.array_equal(data.y.cpu().numpy(), y)
    got = G.ec_threshold_scan(data, C.tensor(w, device), thresholds())
    assert_against_reference(got, name, "the device on")
    want, _ = C.restated(ei, pid, good, w, y, thresholds())
    assert [{k: r[k] for k in C.ORPHAN_KEYS} for r in got] == [{k: r[k] for k in C.ORPHAN_KEYS} for r in want]
