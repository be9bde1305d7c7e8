"""The host layer under the six fused-MLP autograd nodes on the CPU wave64 emulator (the real kernel sources):
the C entries each node calls, in order, and the errors of the host code (tests/mlp_nodes_cases.py)."""

import pytest

import mlp_nodes_cases as M
from emul_util import emulated

pytestmark = pytest.mark.emul


def test_launch_sequences_emulated():
    with emulated():
        M.case_launch_sequences("cpu")


def test_host_errors_emulated():
    with emulated():
        M.case_host_errors("cpu")
