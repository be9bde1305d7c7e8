"""The edge-weight head folded into its backward launch on the MI355X: the step with the deferral on against the
step with it off, bit for bit, at the size the headline is measured at (one event of cfg3: seed 100, 150 000 hits,
2 000 000 edges, bf16 storage) and over two micro-batches with ``scale = 0.5`` (tests/fused_head_cases.py)."""

import pytest
import torch

import fused_head_cases as F

pytestmark = pytest.mark.gpu


def _event(seed, n_hits, n_edges):
    from gnn_tracking_amd import synthetic

    ev = synthetic.make_event(seed, n_hits, n_edges, "cpu").to("cuda")
    ev.y = ev.y.bool()
    return ev


def test_fused_launch_writes_the_forward_launch_w_small():
    F.case_fused_w_equals_forward_w("cuda", F.random_data("cuda"))


def test_backward_step_on_off_saturated_logits():
    F.case_on_off_saturated("cuda", F.random_data("cuda"))


def test_backward_step_on_off_cfg3_event():
    on = F.case_on_off("cuda", [_event(100, 150_000, 2_000_000)], tag="cfg3 event, seed 100")
    assert 0.0 < float(on["loss"][0]) < 10.0
    torch.cuda.synchronize()


def test_backward_step_on_off_two_micro_batches_scaled():
    F.case_on_off("cuda", [_event(101, 150_000, 2_000_000), _event(102, 60_000, 700_002)], scale=0.5,
                  tag="two micro-batches, scale 0.5")


def test_readers_of_w_other_losses_and_external_backward_fall_back():
    F.case_fallbacks("cuda", F.random_data("cuda", n_hits=3000, n_edges=40_003, isolated=11))
