"""The dynamic edge convolution on the CPU wave64 emulator (the real kernel sources of csrc/edge_conv.hip): the cases
of tests/edge_conv_cases.py against the float64 restatement, with the kernel path forced, and the host-side argument
checks of the three C entries."""

import pytest

import edge_conv_cases as E
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul


@pytest.mark.parametrize("row", E.SWEEP, ids=E.sweep_id)
def test_operator_against_the_restatement(row):
    with emulated(), E.kernel_path():
        E.case_sweep("cpu", row)


def test_short_table_and_queries_without_a_slot():
    with emulated(), E.kernel_path():
        E.case_short_table("cpu")


def test_winning_slots_are_the_restatements():
    with emulated(), E.kernel_path():
        E.case_winning_slots("cpu")


def test_strided_rows_no_input_gradient_and_same_bits_twice():
    with emulated(), E.kernel_path():
        E.case_strided_and_no_input_grad("cpu")


def test_gradients_accumulate_as_autograd_does():
    with emulated(), E.kernel_path():
        E.case_grad_accumulation("cpu")


def test_ids_out_of_range_are_clamped():
    with emulated(), E.kernel_path():
        E.case_bad_table_is_clamped("cpu")


@pytest.mark.parametrize("shape", E.OVER_LIMIT, ids=lambda s: "-".join(map(str, s)))
def test_over_limit_shapes_take_the_composed_path(shape):
    with emulated(), E.kernel_path():
        E.case_over_limit("cpu", shape)


def test_bf16_rows_take_the_composed_path():
    with emulated(), E.kernel_path():
        E.case_bf16_input("cpu")


def test_switched_off_is_the_composed_path():
    with emulated(), E.kernel_path(False):
        E.case_switched_off("cpu")


@pytest.mark.parametrize("case", E.DEC_GOLDEN)
def test_golden_dynamic_edge_conv(case):
    with emulated(), E.kernel_path():
        E.case_golden_dec("cpu", case)


def test_golden_in_conv_block():
    with emulated(), E.kernel_path():
        E.case_golden_inconv("cpu")


def test_golden_point_cloud_tcn():
    with emulated(), E.kernel_path():
        E.case_golden_pctcn("cpu")


def test_edge_index_is_the_knn_graph_with_self_edges():
    with emulated(), E.kernel_path():
        E.case_edge_index_is_the_knn_graph("cpu")


def test_collated_batch_is_the_events_one_by_one():
    with emulated(), E.kernel_path():
        E.case_collated_batch("cpu")


def test_tc_module_trains_a_point_cloud_tcn():
    with emulated(), E.kernel_path():
        E.case_tc_module_trains("cpu")


def test_interaction_network_mean_still_raises():
    E.case_interaction_network_still_sum_only()


def test_entries_validate_on_the_host():
    E.check_entries_validate(emulator_lib())
