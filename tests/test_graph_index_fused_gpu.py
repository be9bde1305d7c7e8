"""The graph-index build with the by-target count inside the remap pass, one zero fill and two scan launches per
sort, on the MI355X: the cases of tests/graph_index_cases.py (chunk geometry, renumbering, the slow paths with
carried rows, ids out of range, the table scan at its tile edges), bit for bit against torch's stable argsort."""

import pytest

import graph_index_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.GEOMETRY))
def test_chunk_geometry(name):
    C.case_geometry("cuda", name)


@pytest.mark.parametrize("name", list(C.RENUMBER))
def test_renumbered(name):
    C.case_renumber("cuda", name)


def test_window_slow_path_renumbered_with_rows():
    C.case_window_slow_path("cuda")


@pytest.mark.parametrize("name", list(C.HUBS))
def test_bucket_over_the_lds_capacity_with_rows(name):
    C.case_hub("cuda", name)


def test_ids_out_of_range_renumbered():
    C.case_out_of_range("cuda")


def test_row_stride_and_special_values():
    C.case_rows("cuda")


@pytest.mark.parametrize("name", list(C.SCAN))
def test_table_scan_at_its_tile_edges(name):
    C.case_scan("cuda", name)
