"""``MLGraphConstruction`` on a collated batch on the CPU wave64 emulator: tests/mlgc_batch_cases.py."""

import pytest

import mlgc_batch_cases as M
from emul_util import emulated as ctx

pytestmark = pytest.mark.emul
DEVICE = "cpu"

@pytest.mark.parametrize("ratio_of_false", (None, 0.5))
@pytest.mark.parametrize("radius", M.RADII)
@pytest.mark.parametrize("k", M.KS)
def test_batch_equals_the_events_alone(k, radius, ratio_of_false):
    with ctx():
        M.case_batch_equals_events(DEVICE, k, radius, ratio_of_false)


def test_per_event_false_is_the_reference_mixing():
    with ctx():
        M.case_reference_mixing(DEVICE)
