"""The float64 restatement of the geometric graph builder (tests/graph_builder_ref.py) against the reference's own
output (tests/golden/g23_graph_builder.npz, tools/make_golden_graph_builder.py): the oracle of the emulator and GPU
tests is pinned here, without the product.  The edge list AND its order, ``y`` and ``edge_pt`` are exact; ``edge_attr``
lies within the per-column bound the tool measured for the case (the reference evaluates in float32); the quotients of
a measurement record within 1e-12 relative."""

import numpy as np
import pytest

import graph_builder_cases as C
import graph_builder_ref as R


def restated(name):
    pc, kw = C.golden_cloud(name), C.golden_kw(name)
    return pc, kw, R.build_edges(pc["x"], pc["layer"], pc["particle_id"], pc["pt"], **C.ref_kw(kw))


def test_golden_holds_every_case():
    g = C.golden()
    assert tuple(str(c) for c in g["cases"]) == C.GOLDEN_CASES
    assert C.GOLDEN.stat().st_size < 1 << 20
    assert all(len(g[f"{n}_layer"]) <= 900 for n in C.GOLDEN_CASES)


@pytest.mark.parametrize("name", C.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    g = C.golden()
    pc, kw, want = restated(name)
    ei, ea, y, pt = (g[f"{name}_be_{k}"] for k in ("edge_index", "edge_attr", "y", "edge_pt"))
    assert ei.shape == want["edge_index"].shape
    if kw["edge_augmentation"] is None:
        o = p = slice(None)
    else:
        o, p = np.lexsort((ei[1], ei[0])), np.lexsort((want["edge_index"][1], want["edge_index"][0]))
    assert np.array_equal(ei[:, o], want["edge_index"][:, p])
    assert np.array_equal(y[o], want["y"][p]) and np.array_equal(pt[o], want["edge_pt"][p])
    err = np.abs(ea.astype(np.float64)[:, o] - want["attr64"][:, p]).max(axis=1)
    assert (err <= g[f"{name}_attr_bound"]).all(), err
    assert (g[f"{name}_attr_bound"] < 1e-5).all()
    # the doubling of to_pyg_data
    rei, rea, ry = g[f"{name}_edge_index"], g[f"{name}_edge_attr"], g[f"{name}_y"]
    if kw["directed"]:
        assert np.array_equal(rei, ei) and np.array_equal(ry, y)
    elif kw["edge_augmentation"] is None:
        dei, dea, dy = R.double(want)
        assert np.array_equal(rei, dei) and np.array_equal(ry, dy)
        assert np.abs(rea.T.astype(np.float64) - dea).max() <= g[f"{name}_attr_bound"].max() + 1e-7
    nt = R.n_truth_edges(pc["layer"], pc["particle_id"], pc["pt"])[0]
    assert [nt[t] for t in R.PT_THLDS] == g[f"{name}_n_truth"].tolist()


def test_relabelling_cases_relabel():
    for name, expect in (("syn_relabel", True), ("syn_relabel_directed", True), ("syn_relabel_off", False),
                         ("sector0", False), ("sector1", False)):
        pc, _, want = restated(name)
        assert (want["n_corrected"].sum() > 0) == expect, name
        assert int((want["y"] != want["y_naive"]).sum()) == int(want["n_corrected"].sum())
    pc, _, want = restated("syn_relabel")
    big = pc["particle_id"][pc["particle_id"] > 2 ** 53]
    assert len(np.unique(big)) == 2 and len(np.unique(big.astype(np.float64))) == 1, "ids that float64 tells apart"
    l1, l2 = pc["layer"][want["edge_index"][0]], pc["layer"][want["edge_index"][1]]
    gone = want["y"] != want["y_naive"]
    assert set(zip(l1[gone].tolist(), l2[gone].tolist())) >= {(9, 6), (7, 6)}
    kept = (want["y"] == 1) & np.isin(l1, (7, 8, 9, 10)) & np.isin(l2, (6, 11))
    assert {(8, 6), (8, 11), (10, 6), (10, 11)} <= set(zip(l1[kept].tolist(), l2[kept].tolist()))


def test_pinned_reference_numbers():
    g = C.golden()
    for name, (n, e, t, xs) in C.PINS.items():
        assert len(g[f"{name}_layer"]) == n and g[f"{name}_edge_index"].shape == (2, e)
        assert int(g[f"{name}_y"].sum()) == t and int(g[f"{name}_x_sum"][0]) == xs
        _, _, want = restated(name)
        assert 2 * want["edge_index"].shape[1] == e and 2 * int(want["y"].sum()) == t


def test_measurements():
    g = C.golden()
    keys = [str(k) for k in g["measurement_keys"]]
    records = []
    for name in ("sector0", "sector1"):
        pc, _, want = restated(name)
        rec = R.measurement(want["y"], want["edge_pt"], R.n_truth_edges(pc["layer"], pc["particle_id"], pc["pt"])[0])
        C.assert_record(rec, dict(zip(keys, g[f"{name}_measurement"])), name)
        records.append(rec)
    total = R.get_measurements(records)
    assert list(total) == [str(k) for k in g["measurements_keys"]]
    for k, w in zip(total, g["measurements"]):
        assert abs(float(total[k]) - w) <= 1e-12 * abs(w), k
    with np.errstate(all="ignore"):
        empty = R.measurement(np.zeros(0, np.float32), np.zeros(0, np.float32), dict.fromkeys(R.PT_THLDS, 0))
    assert np.isnan(empty["edge_purity"]) and np.isnan(empty["edge_efficiency_0.5"])
