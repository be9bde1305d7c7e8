"""The geometric graph builder on the device: every case of tests/graph_builder_cases.py (the restatement, the
reference's golden output, the edges of the traversal, batches, determinism, downstream use) and the refusal of host
tensors."""

import pytest
import torch

import gnn_tracking_amd as G
import graph_builder_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    case(DEVICE)


def test_host_tensors_are_refused():
    pc = C.to_data(C.golden_cloud("syn_directed"), "cpu")
    for call in (G.GraphBuilder().build_edges, G.GraphBuilder().build, G.GraphBuilder().get_n_truth_edges):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call(pc)


def test_one_host_read_per_build():
    """``build`` synchronises once (the edge count); the measurement record waits on the device until it is looked at"""
    b = G.GraphBuilder(measurement_mode=True)
    pc = C.to_data(C.golden_cloud("syn_default"), DEVICE)
    b.build(pc)
    torch.cuda.synchronize()
    reads = []
    real = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1]
    try:
        b.build(pc)
        assert len(reads) == 1, reads
        assert len(b.measurements) == 2 and len(reads) == 3     # (one copy per build that was waiting)
    finally:
        torch.Tensor.cpu = real
