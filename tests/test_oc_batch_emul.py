"""The condensation losses on a collated batch of events on the CPU wave64 emulator (the real kernel sources): every
case of tests/oc_batch_cases.py."""

import pytest

import oc_batch_cases as B
import oc_cases as C
from emul_util import emulated as ctx

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@pytest.mark.parametrize("reverse", (False, True), ids=("forward", "reversed"))
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_events_that_align_with_no_tile(mode, reverse):
    with ctx():
        B.case_tile_edges(DEVICE, mode, reverse)


@pytest.mark.parametrize("dim", B.CHUNK_WIDTHS)
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_point_ranges_across_the_lds_chunk(mode, dim):
    with ctx():
        B.case_chunk_edges(DEVICE, mode, dim)


@pytest.mark.parametrize("kind", ("copies", "shared"))
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_colliding_particle_ids(mode, kind):
    with ctx():
        B.case_colliding_ids(DEVICE, mode, kind)


@pytest.mark.parametrize("dim", B.WIDTHS)
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_every_width_class(mode, dim):
    with ctx():
        B.case_width(DEVICE, mode, dim)


@pytest.mark.parametrize("term", C.TERMS)
@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_each_term_differentiated_alone(mode, term):
    with ctx():
        B.case_term_gradient(DEVICE, mode, term)


@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_ec_hit_mask(mode):
    with ctx():
        B.case_ec_hit_mask(DEVICE, mode)


def test_kth_neighbor_inside_the_event():
    with ctx():
        B.case_kth_neighbor(DEVICE)


def test_neighbor_cap_nearest():
    with ctx():
        B.case_neighbor_cap(DEVICE)


@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_no_behaviour_change_without_a_multi_event_batch(mode):
    with ctx():
        B.case_no_change(DEVICE, mode)


def test_refusals():
    with ctx():
        B.case_refusals(DEVICE)


@pytest.mark.parametrize("mode", tuple(C.LOSSES))
def test_odd_events_in_one_batch(mode):
    with ctx():
        B.case_odd_events(DEVICE, mode)
