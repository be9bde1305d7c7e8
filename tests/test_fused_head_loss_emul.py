"""The edge-weight head folded into its backward launch, on the CPU wave64 emulator (the real kernel sources):
bit for bit against the step with the deferral switched off.  The premise comes first - the fused launch's W is
the forward launch's W - because everything else follows from it (tests/fused_head_cases.py)."""

import pytest

import fused_head_cases as F
from emul_util import emulated

pytestmark = pytest.mark.emul


def test_fused_launch_writes_the_forward_launch_w():
    with emulated():
        F.case_fused_w_equals_forward_w("cpu", F.testgraph_data("cpu"))
        F.case_fused_w_equals_forward_w("cpu", F.random_data("cpu"))


def test_backward_step_on_off_testgraph():
    with emulated():
        F.case_on_off("cpu", [F.testgraph_data("cpu")], tag="test graph")


def test_backward_step_on_off_random_graph_tail_isolated_scaled():
    with emulated():
        d = F.random_data("cpu")
        F.case_on_off("cpu", [d], tag="random graph")
        F.case_on_off("cpu", [d], scale=0.5, tag="random graph, scale 0.5")
        F.case_on_off("cpu", [d, F.random_data("cpu", seed=9, n_hits=300, n_edges=2021, isolated=0)], scale=0.5,
                      tag="two micro-batches, scale 0.5")


def test_backward_step_on_off_saturated_logits():
    with emulated():
        F.case_on_off_saturated("cpu", F.random_data("cpu"))


def test_other_head_shapes_take_todays_launches_inside_the_backward():
    """A head that is not the buffer-addressed shape (no node embedding in its input) defers as well and runs the
    forward launch, the loss pass and the ordinary backward from the node's backward: same bits."""
    with emulated():
        F.case_on_off("cpu", [F.random_data("cpu", n_hits=200, n_edges=1003, isolated=3)], tag="no_node",
                      expect_fused=False, module_kw=dict(L_ec=2, hidden_dim=8, use_node_embedding=False))


def test_readers_of_w_other_losses_and_external_backward_fall_back():
    with emulated():
        F.case_fallbacks("cpu", F.random_data("cpu", n_hits=300, n_edges=2021, isolated=5))


def test_metadata_of_a_pending_w_launches_nothing():
    with emulated():
        F.case_metadata_does_not_resolve("cpu", F.random_data("cpu", n_hits=300, n_edges=2021, isolated=5))
