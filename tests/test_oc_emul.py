"""The condensation losses on the CPU wave64 emulator (the real kernel sources) against the blocked fp64 oracle:
every case of tests/oc_cases.py except the second condensation-point batch (2.9e8 pairs: device only)."""

import pytest

import oc_cases as C
from emul_util import emulated

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@pytest.mark.parametrize("dim", C.DENSE_WIDTHS)
def test_dense_passes_every_width(dim):
    with emulated():
        C.case_width(DEVICE, dim, "off")


@pytest.mark.parametrize("dim", C.SPATIAL_WIDTHS)
def test_spatial_passes_every_width(dim):
    with emulated():
        C.case_width(DEVICE, dim, "on")


@pytest.mark.parametrize("dim", C.FALLBACK_WIDTHS)
def test_spatial_falls_back_to_dense_above_width_16(dim):
    with emulated():
        C.case_width_fallback(DEVICE, dim)


@pytest.mark.parametrize("spatial", C.PATHS)
def test_width_33_is_refused(spatial):
    with emulated():
        C.case_width_refused(DEVICE, spatial)


@pytest.mark.parametrize("spatial", C.PATHS)
@pytest.mark.parametrize("dim", C.K_EDGE_WIDTHS)
@pytest.mark.parametrize("k", C.K_EDGES)
def test_tile_edges_in_k(k, dim, spatial):
    with emulated():
        C.case_k_edge(DEVICE, k, dim, spatial)


@pytest.mark.parametrize("spatial", C.PATHS)
@pytest.mark.parametrize("n", C.N_EDGES)
def test_tile_edges_in_n(n, spatial):
    with emulated():
        C.case_n_edge(DEVICE, n, spatial)


@pytest.mark.parametrize("term", C.TERMS)
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
@pytest.mark.parametrize("spatial", C.PATHS)
@pytest.mark.parametrize("shape", C.TERM_SHAPES, ids=lambda s: f"N{s[0]}-D{s[1]}")
def test_each_term_differentiated_alone(shape, spatial, mode, term):
    with emulated():
        C.case_term_gradient(DEVICE, shape, spatial, mode, term)


@pytest.mark.parametrize("spatial", C.PATHS)
@pytest.mark.parametrize("name", C.ODD_EVENTS)
def test_odd_events(name, spatial):
    with emulated():
        C.case_odd_event(DEVICE, name, spatial)


@pytest.mark.parametrize("spatial", C.PATHS)
def test_fp64_inputs(spatial):
    with emulated():
        C.case_fp64_inputs(DEVICE, spatial)


@pytest.mark.parametrize("spatial", C.PATHS)
def test_transposed_x(spatial):
    with emulated():
        C.case_transposed_x(DEVICE, spatial)
