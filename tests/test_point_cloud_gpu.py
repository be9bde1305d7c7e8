"""The point cloud builder on the device: every case of tests/point_cloud_cases.py (the reference's golden output for
its bundled event in five configurations, the end-to-end run into the graph builder, synthetic tables against the
restatement), the refusal of host tensors and the single host read of a build."""

import pytest
import torch

import gnn_tracking_amd as G
import point_cloud_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    case(DEVICE)


def test_host_tensors_are_refused():
    b = G.PointCloudBuilder(detector=G.load_detector(C.detector_table()), n_sectors=2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        b.build(C.on(C.random_event(1, 10), "cpu"))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.get_truth_edge_index(torch.zeros(4, dtype=torch.int64))


def test_one_host_read_per_build():
    """``build`` synchronises once per event: the sizes and every counter in one copy, truth edges included"""
    b = G.PointCloudBuilder(detector=G.load_detector(C.detector_table()), n_sectors=3, measurement_mode=True,
                            add_true_edges=True)
    tables = C.on(C.random_event(2, 257), DEVICE)
    b.build(tables)
    torch.cuda.synchronize()
    reads = []
    real = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1]
    try:
        b.build(tables)
        b.build(tables, collated=True)
    finally:
        torch.Tensor.cpu = real
    assert len(reads) == 2, reads
