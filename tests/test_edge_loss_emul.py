"""The edge losses and the hinge loss on the CPU wave64 emulator (the real kernel sources): the cases of
tests/edge_loss_cases.py against fp64 references, gradients element by element.

The emulated device has 2 CUs (tests/emul/shim/hip/hip_runtime.h), so its loss grids are capped at 16 workgroups:
the grid-stride second trips are reached at a few thousand edges, but ``bce_final_kernel`` never sees more than 16
partials - its trip beyond 256 partials runs on the device only (tests/test_edge_loss_gpu.py), as does the hinge
forward at its cap of 2048 workgroups."""

import pytest

import edge_loss_cases as E
from emul_util import emulated

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@pytest.mark.parametrize("thld", (0.0, E.THLD))
def test_bce_two_pass_and_csr_at_saturated_scores(thld):
    with emulated():
        E.case_bce_saturated(DEVICE, thld)


def test_bce_csr_unit_gradient_at_saturated_scores():
    with emulated():
        E.case_bce_csr_unit_gradient_saturated(DEVICE)


@pytest.mark.parametrize("gamma", E.GAMMAS)
def test_focal_at_saturated_scores(gamma):
    with emulated():
        E.case_focal_saturated(DEVICE, gamma)


@pytest.mark.parametrize("gamma", E.GAMMAS)
def test_focal_at_exact_zero_and_one_as_torch_fp32(gamma):
    with emulated():
        E.case_focal_exact(DEVICE, gamma)


def test_pt_at_the_threshold_one_ulp_above_and_nan():
    with emulated():
        E.case_pt_threshold_edges(DEVICE)


def test_non_binary_labels_binarise_with_the_threshold():
    with emulated():
        E.case_non_binary_labels(DEVICE)


def test_soft_labels_without_the_threshold():
    with emulated():
        E.case_soft_labels(DEVICE)


def test_edge_targets_csr_float_and_byte_labels():
    with emulated():
        E.case_edge_targets_csr(DEVICE)


@pytest.mark.parametrize("which", ("partial-second-trip", "csr-second-trip", "backward-second-trip"))
def test_loss_grids_at_their_caps(which):
    """The sizes the 2-CU device gives (4097, 16 391, 4097 edges); the 257-partial trip of ``bce_final_kernel``
    cannot occur here."""
    with emulated():
        E.case_grid_caps(DEVICE, which)


@pytest.mark.parametrize("dim", E.HINGE_DIMS)
def test_hinge_every_register_width(dim):
    with emulated():
        E.case_hinge_widths(DEVICE, dim)


def test_hinge_dim_33_is_refused():
    with emulated():
        E.case_hinge_dim_refused(DEVICE)


def test_hinge_degrees_around_the_lane_count():
    with emulated():
        E.case_hinge_degrees(DEVICE)


def test_hinge_distance_exactly_r_emb():
    with emulated():
        E.case_hinge_on_the_hinge(DEVICE)


@pytest.mark.parametrize("dim", (3, 8, 17))
def test_hinge_c_entry_strides_and_accumulate(dim):
    with emulated():
        E.case_hinge_c_entry(DEVICE, dim)
