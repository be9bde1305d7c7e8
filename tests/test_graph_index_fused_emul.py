"""The graph-index build with the by-target count inside the remap pass, one zero fill and two scan launches per
sort, on the CPU wave64 emulator (the real kernel sources): chunk geometry, renumbering, the slow paths with carried
rows, ids out of range and the table scan at its tile edges, bit for bit against torch's stable argsort
(tests/graph_index_cases.py)."""

import pytest

import graph_index_cases as C
from emul_util import emulated

pytestmark = pytest.mark.emul


@pytest.mark.parametrize("name", list(C.GEOMETRY))
def test_chunk_geometry(name):
    with emulated():
        C.case_geometry("cpu", name)


@pytest.mark.parametrize("name", list(C.RENUMBER))
def test_renumbered(name):
    with emulated():
        C.case_renumber("cpu", name)


def test_window_slow_path_renumbered_with_rows():
    with emulated():
        C.case_window_slow_path("cpu")


@pytest.mark.parametrize("name", list(C.HUBS))
def test_bucket_over_the_lds_capacity_with_rows(name):
    with emulated():
        C.case_hub("cpu", name)


def test_ids_out_of_range_renumbered():
    with emulated():
        C.case_out_of_range("cpu")


def test_row_stride_and_special_values():
    with emulated():
        C.case_rows("cpu")


@pytest.mark.parametrize("name", list(C.SCAN))
def test_table_scan_at_its_tile_edges(name):
    with emulated():
        C.case_scan("cpu", name)
