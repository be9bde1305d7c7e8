"""The host layer under the six fused-MLP autograd nodes on the MI355X: the C entries each node calls, in order,
and the errors of the host code (tests/mlp_nodes_cases.py)."""

import pytest

import mlp_nodes_cases as M

pytestmark = pytest.mark.gpu


def test_launch_sequences():
    M.case_launch_sequences("cuda")


def test_host_errors():
    M.case_host_errors("cuda")
