"""The neighbour-search units on the device (csrc/knn.hip, csrc/dbscan.hip) against the C kNN oracle and the fp64
radius / DBSCAN oracles: every case of tests/neighbor_cases.py."""

import pytest

import neighbor_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


# ------------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("dim", C.KNN_WIDTHS)
def test_knn_brute_force_every_width(dim):
    C.case_knn_width(DEVICE, dim, C.BRUTE)


@pytest.mark.parametrize("dim", C.KNN_PRUNED_WIDTHS)
def test_knn_pruned_every_width(dim):
    C.case_knn_width(DEVICE, dim, C.PRUNED)


@pytest.mark.parametrize("dim", C.FALLBACK_WIDTHS)
def test_knn_pruned_falls_back_above_width_16(dim):
    C.case_knn_width_fallback(DEVICE, dim)


@pytest.mark.parametrize("flags", (0,) + C.FLAGS)
def test_knn_width_33_is_refused(flags):
    C.case_knn_width_refused(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("dim", C.K_CLASS_WIDTHS)
@pytest.mark.parametrize("k", C.K_CLASSES)
def test_knn_every_k_class(k, dim, flags):
    C.case_knn_k_class(DEVICE, k, dim, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_knn_k_449_is_refused(flags):
    C.case_knn_k_refused(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_knn_k_beyond_n_is_clipped(flags):
    C.case_knn_k_clipped(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("k,n", C.OVERFLOW_SHAPES)
def test_knn_buffers_overflow_and_are_cut(k, n, flags):
    C.case_knn_overflow(DEVICE, k, n, flags)


@pytest.mark.parametrize("dim", C.KNN_N_EDGE_WIDTHS)
@pytest.mark.parametrize("n", C.KNN_N_EDGES)
def test_knn_brute_force_tile_edges_in_n(n, dim):
    C.case_knn_n_edge(DEVICE, n, dim)


@pytest.mark.parametrize("n", tuple(C.KNN_PRUNED_N))
def test_knn_pruned_tile_and_batch_edges_in_n(n):
    C.case_knn_pruned_n_edge(DEVICE, n)


def test_knn_pruned_two_batches_without_radius():
    C.case_knn_pruned_no_radius(DEVICE)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("name", tuple(C.EVENTS))
def test_knn_collated_events(name, flags):
    C.case_knn_events(DEVICE, name, flags)


def test_knn_pruned_events_straddle_batches():
    C.case_knn_big_events(DEVICE)


def test_radius_graph_batch_vector():
    C.case_radius_graph_batch(DEVICE)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_knn_radius_is_strict(flags):
    C.case_knn_radius_exact(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_knn_radius_extremes(flags):
    C.case_knn_radius_extremes(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("r", C.NO_EDGE_RADII)
def test_knn_radius_that_admits_nothing(r, flags):
    C.case_knn_no_edge_radius(DEVICE, r, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_kth_neighbor(flags):
    C.case_kth_neighbor(DEVICE, flags)


def test_max_radius_count():
    C.case_max_radius_count(DEVICE)


@pytest.mark.parametrize("clip", (True, False), ids=("clipped", "unclipped"))
@pytest.mark.parametrize("n", C.SCAN_N)
def test_count_scan(n, clip):
    C.case_count_scan(DEVICE, n, clip)


def test_count_scan_beyond_int32():
    C.case_count_scan_beyond_int32(DEVICE)


# ------------------------------------------------------------------------------------- radius graph, DBSCAN
@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("dim", C.RADIUS_WIDTHS)
def test_radius_graph_every_width(dim, flags):
    C.case_radius_width(DEVICE, dim, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_radius_graph_width_33_is_refused(flags):
    C.case_radius_width_refused(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("dim", C.RADIUS_N_EDGE_WIDTHS)
@pytest.mark.parametrize("n", C.RADIUS_N_EDGES)
def test_radius_graph_tile_edges_in_n(n, dim, flags):
    C.case_radius_n_edge(DEVICE, n, dim, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("n", C.RADIUS_BOX_LOOP_N)
def test_radius_graph_second_turn_of_the_box_loop(n, flags):
    C.case_radius_box_loop(DEVICE, n, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("m", C.LIST_LENGTHS)
def test_radius_lists_at_the_ordering_capacity(m, flags):
    C.case_radius_list_length(DEVICE, m, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
def test_radius_exact_thresholds(flags):
    C.case_radius_exact(DEVICE, flags)


@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("name", C.DBSCAN_SHAPES)
def test_dbscan_component_shapes(name, flags):
    C.case_dbscan_shape(DEVICE, name, flags)
