"""The dataset writer on the device: every case of tests/dataset_io_cases.py (the packer against its numpy restatement,
the round trips through uncollate, the files and the stages), the refusal of host tensors, and the writer's side
stream with more batches than pinned buffers."""

import pytest
import torch

import gnn_tracking_amd as G
import dataset_io_cases as C

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.mark.parametrize("case", C.PACK_CASES + C.CASES, ids=lambda c: c.__name__[5:])
def test_case(case):
    case(DEVICE)


@pytest.mark.parametrize("case", C.DIR_CASES, ids=lambda c: c.__name__[5:])
def test_dir_case(case, tmp_path):
    case(DEVICE, tmp_path)


def test_host_tensors_are_refused():
    batch = G.collate(C.make_events("cpu"))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.pack_events(batch)


def test_writer_reuses_its_pinned_buffers(tmp_path):
    """six batches through two pinned buffers, each batch dropped by the caller as soon as it is queued"""
    gs = C.make_events(DEVICE)
    with G.GraphWriter(tmp_path, depth=2, pack=True) as w:
        for r in range(6):
            batch = G.collate(gs)
            w.write(batch, names=[f"r{r}_e{i}.pt" for i in range(len(gs))])
            del batch
    assert w._n_buffers <= 2 and len(w.written) == 6 * len(gs)
    want = [g.cpu() for g in gs]
    for r in range(6):
        C.assert_same_events([G.load_graph(tmp_path / f"r{r}_e{i}.pt") for i in range(len(gs))], want, f"round {r}")


def test_default_path_is_one_of_the_two(tmp_path):
    """pack=None follows io.PACK_BY_DEFAULT / GNNTRK_PACK_EVENTS: either way the files are the events"""
    gs = C.make_events(DEVICE)
    G.save_graphs(G.collate(gs), [tmp_path / f"e{i}.pt" for i in range(len(gs))])
    C.assert_same_events([G.load_graph(tmp_path / f"e{i}.pt") for i in range(len(gs))], [g.cpu() for g in gs], "default")
