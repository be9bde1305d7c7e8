"""``MLGraphConstruction`` on a collated batch on the device: tests/mlgc_batch_cases.py."""

import contextlib

import pytest

import mlgc_batch_cases as M

pytestmark = pytest.mark.gpu
DEVICE = "cuda"
ctx = contextlib.nullcontext

@pytest.mark.parametrize("ratio_of_false", (None, 0.5))
@pytest.mark.parametrize("radius", M.RADII)
@pytest.mark.parametrize("k", M.KS)
def test_batch_equals_the_events_alone(k, radius, ratio_of_false):
    with ctx():
        M.case_batch_equals_events(DEVICE, k, radius, ratio_of_false)


def test_per_event_false_is_the_reference_mixing():
    with ctx():
        M.case_reference_mixing(DEVICE)
