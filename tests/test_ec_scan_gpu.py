"""The EC threshold scan on the GPU: every case of tests/ec_scan_cases.py against the composition of the single-threshold
functions (exact) and the networkx / numpy restatement, the reference's own records of tests/golden/g22_ec_scan.npz, and
the refusal of host tensors."""

import pytest
import torch

import ec_scan_cases as C
import ec_scan_golden as GOLD
import gnn_tracking_amd as G
import track_graph_cases as TC

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    case(DEVICE)


@pytest.mark.parametrize("name", GOLD.GRAPHS)
def test_reference_records(name):
    GOLD.check_device(name, DEVICE)


def test_host_tensors_are_refused():
    ei, pid = TC.chain_graph(4)
    data = TC.data_of(ei, pid, pid > 0, "cpu")
    w = torch.full((ei.shape[1],), 0.7)
    for call in (lambda: G.ec_threshold_scan(data, w, [0.5]), lambda: G.get_all_ec_stats(0.5, w, data),
                 lambda: G.collect_all_ec_stats(C.StoredW([w]), [data], [0.5])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.ec_threshold_scan(TC.data_of(ei, pid, pid > 0, DEVICE), w, [0.5])
