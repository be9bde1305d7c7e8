"""The track-graph statistics on the GPU: every case of tests/track_graph_cases.py against the networkx restatement
(exact, ``inf`` included), and the refusal of host tensors."""

import pytest
import torch

import gnn_tracking_amd as G
import track_graph_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    case(DEVICE)


def test_host_tensors_are_refused():
    ei, pid = C.chain_graph(4)
    data = C.data_of(ei, pid, pid > 0, "cpu")
    for fn in (G.get_track_graph_info_from_data, G.get_orphan_counts, G.get_basic_counts,
               G.get_all_graph_construction_stats):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            fn(data)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.get_track_graph_info_from_data(C.data_of(ei, pid, pid > 0, DEVICE), w=torch.ones(ei.shape[1]), threshold=0.5)
