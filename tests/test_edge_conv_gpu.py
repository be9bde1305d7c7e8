"""The dynamic edge convolution on the device: the cases of tests/edge_conv_cases.py against the float64
restatement, with the kernel path forced."""

import pytest

import edge_conv_cases as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", E.SWEEP, ids=E.sweep_id)
def test_operator_against_the_restatement(row):
    with E.kernel_path():
        E.case_sweep("cuda", row)


def test_short_table_and_queries_without_a_slot():
    with E.kernel_path():
        E.case_short_table("cuda")


def test_winning_slots_are_the_restatements():
    with E.kernel_path():
        E.case_winning_slots("cuda")


def test_strided_rows_no_input_gradient_and_same_bits_twice():
    with E.kernel_path():
        E.case_strided_and_no_input_grad("cuda")


def test_gradients_accumulate_as_autograd_does():
    with E.kernel_path():
        E.case_grad_accumulation("cuda")


def test_ids_out_of_range_are_clamped():
    with E.kernel_path():
        E.case_bad_table_is_clamped("cuda")


@pytest.mark.parametrize("shape", E.OVER_LIMIT, ids=lambda s: "-".join(map(str, s)))
def test_over_limit_shapes_take_the_composed_path(shape):
    with E.kernel_path():
        E.case_over_limit("cuda", shape)


def test_bf16_rows_take_the_composed_path():
    with E.kernel_path():
        E.case_bf16_input("cuda")


def test_switched_off_is_the_composed_path():
    with E.kernel_path(False):
        E.case_switched_off("cuda")


@pytest.mark.parametrize("case", E.DEC_GOLDEN)
def test_golden_dynamic_edge_conv(case):
    with E.kernel_path():
        E.case_golden_dec("cuda", case)


def test_golden_in_conv_block():
    with E.kernel_path():
        E.case_golden_inconv("cuda")


def test_golden_point_cloud_tcn():
    with E.kernel_path():
        E.case_golden_pctcn("cuda")


def test_edge_index_is_the_knn_graph_with_self_edges():
    with E.kernel_path():
        E.case_edge_index_is_the_knn_graph("cuda")


def test_collated_batch_is_the_events_one_by_one():
    with E.kernel_path():
        E.case_collated_batch("cuda")


def test_tc_module_trains_a_point_cloud_tcn():
    with E.kernel_path():
        E.case_tc_module_trains("cuda")


def test_interaction_network_mean_still_raises():
    E.case_interaction_network_still_sum_only()
