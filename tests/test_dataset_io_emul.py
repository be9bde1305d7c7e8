"""The dataset writer on the CPU wave64 emulator (the real kernel source of csrc/pack.hip): every case of
tests/dataset_io_cases.py, and the host-side argument checks of gnntrk_pack_segments."""

import contextlib

import pytest
import torch

import dataset_io_cases as C
from emul_util import emulated, emulator_lib

pytestmark = pytest.mark.emul
DEVICE = "cpu"


@contextlib.contextmanager
def emulated_cpu():
    """the emulator takes host pointers: nothing may move its inputs to a GPU that happens to be there"""
    old = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with emulated():
            yield
    finally:
        torch.cuda.is_available = old


@pytest.mark.parametrize("case", C.PACK_CASES + C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    with emulated_cpu():
        case(DEVICE)


@pytest.mark.parametrize("case", C.DIR_CASES, ids=lambda c: c.__name__[5:])
def test_dir_case(case, tmp_path):
    with emulated_cpu():
        case(DEVICE, tmp_path)


def test_entry_validates_on_the_host():
    C.host_validation(emulator_lib())
