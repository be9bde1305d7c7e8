"""The edge filters on the device: the cases of tests/edge_filter_cases.py
against the float64 restatement."""

import pytest

import edge_filter_cases as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("n_edges", F.EDGE_COUNTS)
def test_efmlp_against_the_restatement(shape, n_edges):
    with F.kernel_path():
        F.case_shape("cuda", shape, n_edges)


def test_efmlp_switched_off_is_the_composed_path():
    with F.kernel_path(False):
        F.case_shape("cuda", F.SHAPES[0], 130)


def test_efmlp_noncontiguous_edge_index():
    with F.kernel_path():
        F.case_noncontiguous_edge_index("cuda")


def test_efmlp_backward_in_three_chunks_is_deterministic():
    with F.kernel_path():
        F.case_backward_chunking("cuda")


def test_efmlp_gradients_accumulate_as_autograd_does():
    with F.kernel_path():
        F.case_grad_accumulation("cuda")


def test_efmlp_derived_edge_features_same_bits():
    with F.kernel_path():
        F.case_derived_features("cuda")


def test_efmlp_composed_path_when_inputs_need_a_gradient():
    with F.kernel_path():
        F.case_composed_when_inputs_need_grad("cuda")


def test_graph_construction_fused_cut_same_data():
    with F.kernel_path():
        F.case_fused_cut("cuda")


@pytest.mark.parametrize("case", ("efmlp_a", "efmlp_b", "efmlp_c"))
def test_golden_efmlp(case):
    with F.kernel_path():
        F.case_golden_efmlp("cuda", case)


def test_golden_deepset_and_geometric():
    with F.kernel_path():
        F.case_golden_deepset("cuda")
        F.case_golden_geometric("cuda")


def test_pair_invariants_backward():
    with F.kernel_path():
        F.case_pair_invariants("cuda")


def test_ec_module_trains_and_validates_an_efmlp():
    with F.kernel_path():
        F.case_ec_module("cuda")
