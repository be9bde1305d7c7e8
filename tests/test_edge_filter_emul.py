"""The edge filters on the CPU wave64 emulator (the real kernel sources): the cases of tests/edge_filter_cases.py
against the float64 restatement."""

import pytest

import edge_filter_cases as F
from emul_util import emulated

pytestmark = pytest.mark.emul


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("n_edges", F.EDGE_COUNTS)
def test_efmlp_against_the_restatement(shape, n_edges):
    with emulated(), F.kernel_path():
        F.case_shape("cpu", shape, n_edges)


def test_efmlp_switched_off_is_the_composed_path():
    with emulated(), F.kernel_path(False):
        F.case_shape("cpu", F.SHAPES[0], 130)


def test_efmlp_noncontiguous_edge_index():
    with emulated(), F.kernel_path():
        F.case_noncontiguous_edge_index("cpu")


def test_efmlp_backward_in_three_chunks_is_deterministic():
    with emulated(), F.kernel_path():
        F.case_backward_chunking("cpu")


def test_efmlp_gradients_accumulate_as_autograd_does():
    with emulated(), F.kernel_path():
        F.case_grad_accumulation("cpu")


def test_efmlp_derived_edge_features_same_bits():
    with emulated(), F.kernel_path():
        F.case_derived_features("cpu")


def test_efmlp_composed_path_when_inputs_need_a_gradient():
    with emulated(), F.kernel_path():
        F.case_composed_when_inputs_need_grad("cpu")


def test_graph_construction_fused_cut_same_data():
    with emulated(), F.kernel_path():
        F.case_fused_cut("cpu")


@pytest.mark.parametrize("case", ("efmlp_a", "efmlp_b", "efmlp_c"))
def test_golden_efmlp(case):
    with emulated(), F.kernel_path():
        F.case_golden_efmlp("cpu", case)


def test_golden_deepset_and_geometric():
    with emulated(), F.kernel_path():
        F.case_golden_deepset("cpu")
        F.case_golden_geometric("cpu")


def test_pair_invariants_backward():
    with emulated(), F.kernel_path():
        F.case_pair_invariants("cpu")


def test_ec_module_trains_and_validates_an_efmlp():
    with emulated(), F.kernel_path():
        F.case_ec_module("cpu")
