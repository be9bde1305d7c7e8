"""The alignment- and stride-selected kernel variants on the CPU wave64 emulator (the real kernel sources): the
cases of tests/layout_cases.py against fp64 references and against the aligned, contiguous launch."""

import pytest

import layout_cases as L
from emul_util import emulated

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@pytest.mark.parametrize("spec", L.SEGMENT_SUM_F32, ids=lambda s: f"{s[5]}-D{s[2]}-stride{s[3]}-off{4 * s[4]}B-N{s[0]}")
def test_segment_sum_f32_by_pointer_and_stride(spec):
    with emulated():
        L.case_segment_sum_f32(DEVICE, spec)


@pytest.mark.parametrize("n", L.COUNTS)
def test_bce_csr_vector_and_item_loads(n):
    with emulated():
        L.case_bce_csr(DEVICE, n)


@pytest.mark.parametrize("n", (1, 5, 257, 4099))
def test_bce_focal_two_pass_strided_inputs(n):
    with emulated():
        L.case_bce_focal_strided(DEVICE, n)


@pytest.mark.parametrize("n", (1, 2, 3, 5, 257, 1025))
def test_rows_to_bf16_rows4_and_generic(n):
    with emulated():
        L.case_rows_to_bf16(DEVICE, n)


@pytest.mark.parametrize("D", (3, 4, 5, 7, 8))
def test_segment_sum_bf16_pair8_stream16_walk(D):
    with emulated():
        L.case_segment_sum_bf16(DEVICE, D)


@pytest.mark.parametrize("spec", L.GRAPH_INDEX_LISTS, ids=lambda s: f"{s[0]}-E{s[1]}")
def test_graph_index_scalar_key_and_label_reads(spec):
    with emulated():
        L.case_graph_index(DEVICE, spec)


def test_carry_rows_fallback_to_the_gather():
    with emulated():
        L.case_carry_rows_fallback(DEVICE)


@pytest.mark.parametrize("n_nodes", (1, 7, 8, 9, 300, 2049))
def test_connected_nodes_hit_buffer_off_the_8_byte_grid(n_nodes):
    with emulated():
        L.case_connected_nodes(DEVICE, n_nodes)


@pytest.mark.parametrize("n", L.COUNTS)
def test_threshold_compact_w_and_mask_off_their_grids(n):
    with emulated():
        L.case_threshold_compact(DEVICE, n)


@pytest.mark.parametrize("n", (2, 5, 255, 257, 300))
def test_knn_emit_count_scan_item_loads(n):
    with emulated():
        L.case_knn_emit(DEVICE, n)


@pytest.mark.parametrize("n,d", ((2, 3), (130, 3), (300, 8)))
def test_knn_radius_dbscan_strided_x(n, d):
    with emulated():
        L.case_knn_strided_x(DEVICE, n, d)


def test_edge_features_strided_x():
    with emulated():
        L.case_edge_features_strided_x(DEVICE)


def test_hinge_edge_rows_far_apart_and_strided_x():
    with emulated():
        L.case_hinge_strided(DEVICE)


def test_condensation_losses_strided_x():
    with emulated():
        L.case_condensation_strided_x(DEVICE)


def test_node_order_strided_x():
    with emulated():
        L.case_node_order_layout(DEVICE)


def test_graph_index_order_by_strided_x():
    with emulated():
        L.case_graph_index_order_by_layout(DEVICE)


def test_node_order_extreme_keys_stay_valid():
    with emulated():
        L.case_node_order_extreme_keys(DEVICE)


@pytest.mark.parametrize("rows", L.MLP_ROWS)
@pytest.mark.parametrize("shape", tuple(L.MLP16_SHAPES))
def test_mlp_bf16_segments_off_the_16_byte_grid(shape, rows):
    with emulated():
        L.case_mlp_bf16_layout(DEVICE, shape, rows)


@pytest.mark.parametrize("rows", L.MLP_ROWS)
@pytest.mark.parametrize("epilogue", ("relu", "residual"))
def test_mlp_wide_one_tensor_off_the_float4_grid(epilogue, rows):
    with emulated():
        L.case_mlp_wide_layout(DEVICE, rows, epilogue)
