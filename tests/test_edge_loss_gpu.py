"""The edge losses and the hinge loss on the device: the cases of tests/edge_loss_cases.py against fp64 references,
gradients element by element - and the sizes only the device reaches: a final reduction over 257 partials, the
grid-stride second trips at the device's CU count, the hinge forward at its cap of 2048 workgroups."""

import pytest

import edge_loss_cases as E

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("thld", (0.0, E.THLD))
def test_bce_two_pass_and_csr_at_saturated_scores(thld):
    E.case_bce_saturated(DEVICE, thld)


def test_bce_csr_unit_gradient_at_saturated_scores():
    E.case_bce_csr_unit_gradient_saturated(DEVICE)


@pytest.mark.parametrize("gamma", E.GAMMAS)
def test_focal_at_saturated_scores(gamma):
    E.case_focal_saturated(DEVICE, gamma)


@pytest.mark.parametrize("gamma", E.GAMMAS)
def test_focal_at_exact_zero_and_one_as_torch_fp32(gamma):
    E.case_focal_exact(DEVICE, gamma)


def test_pt_at_the_threshold_one_ulp_above_and_nan():
    E.case_pt_threshold_edges(DEVICE)


def test_non_binary_labels_binarise_with_the_threshold():
    E.case_non_binary_labels(DEVICE)


def test_soft_labels_without_the_threshold():
    E.case_soft_labels(DEVICE)


def test_edge_targets_csr_float_and_byte_labels():
    E.case_edge_targets_csr(DEVICE)


@pytest.mark.parametrize("which", ("final-257-partials", "partial-second-trip", "csr-second-trip", "backward-second-trip"))
def test_loss_grids_at_their_caps(which):
    E.case_grid_caps(DEVICE, which)


@pytest.mark.parametrize("dim", E.HINGE_DIMS)
def test_hinge_every_register_width(dim):
    E.case_hinge_widths(DEVICE, dim)


def test_hinge_dim_33_is_refused():
    E.case_hinge_dim_refused(DEVICE)


def test_hinge_degrees_around_the_lane_count():
    E.case_hinge_degrees(DEVICE)


def test_hinge_distance_exactly_r_emb():
    E.case_hinge_on_the_hinge(DEVICE)


@pytest.mark.parametrize("dim", (3, 8, 17))
def test_hinge_c_entry_strides_and_accumulate(dim):
    E.case_hinge_c_entry(DEVICE, dim)


def test_hinge_forward_at_its_block_cap():
    E.case_hinge_forward_cap(DEVICE)
