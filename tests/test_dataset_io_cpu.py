"""Host-only logic of the dataset writer: the argument checks of gnntrk_pack_segments on the built library (no launch,
no GPU), ``uncollate`` and the composed writer on host tensors, and the directory logic of ``DataTransformer``."""

import ctypes
import random

import pytest
import torch

import gnn_tracking_amd as G
import dataset_io_cases as C


def test_pack_entry_validates_on_the_host():
    """every EINVAL of include/gnntrk.h, through _capi on the library built for gfx950, before any launch"""
    from gnn_tracking_amd import _build, _capi

    C.host_validation(_capi.bind(ctypes.CDLL(str(_build.build_lib()))))


def test_uncollate_and_composed_writer_on_the_host(tmp_path):
    """the path without the kernel needs no device: uncollate, save_graph(s), GraphWriter, GraphDataset"""
    C.case_uncollate_round_trip("cpu")
    gs = C.make_events("cpu")
    paths = [tmp_path / f"e{i}.pt" for i in range(len(gs))]
    G.save_graphs(G.collate(gs), paths)            # (host tensors never go through the packer)
    C.assert_same_events([G.load_graph(p) for p in paths], gs, "save_graphs on the host")
    alone = tmp_path / "alone.pt"
    G.save_graph(gs[4], alone)
    assert paths[0].stat().st_size < alone.stat().st_size
    assert isinstance(torch.load(paths[3], weights_only=True), dict)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.save_graphs(G.collate(gs), paths, pack=True)
    for what, batch in C.bad_batches("cpu"):
        with pytest.raises(ValueError, match=what):
            G.uncollate(batch)


def test_ec_score_is_edge_level():
    d = C.make_events("cpu")[2]
    d.ec_score = torch.rand(d.num_edges)
    assert d.is_edge_attr("ec_score") and not d.is_node_attr("ec_score")
    mask = torch.rand(d.num_edges) > 0.5
    assert torch.equal(d.edge_subgraph(mask).ec_score, d.ec_score[mask])


class Identity(torch.nn.Module, C.HyperparametersMixin):
    def __init__(self, scale: float = 2.0, label: str = "id"):
        super().__init__()
        self.save_hyperparameters()

    def forward(self, data):
        return data


def test_process_directories(tmp_path):
    gs = C.make_events("cpu")
    names = C.write_inputs(gs, tmp_path / "in")
    dt = G.DataTransformer(Identity(), device="cpu")
    with pytest.raises(ValueError, match="must have the same length"):
        dt.process_directories([tmp_path / "in"], [tmp_path / "a", tmp_path / "b"])
    assert not (tmp_path / "a").exists()

    # the hparams file: the transform's hyperparameters plus input_dir
    dt.process_directories([tmp_path / "in"], [tmp_path / "all"], max_processes=4, chunk_size=2)
    import yaml
    hp = yaml.safe_load((tmp_path / "all" / "hparams").read_text())
    assert hp == {"scale": 2.0, "label": "id", "input_dir": str(tmp_path / "in")}
    assert sorted(p.name for p in (tmp_path / "all").glob("*.pt")) == names
    C.assert_same_events([G.load_graph(tmp_path / "all" / n) for n in names], gs, "identity transform")

    # start and n_files over the sorted names
    dt.process_directories([tmp_path / "in"], [tmp_path / "part"], start=2, n_files=3)
    assert sorted(p.name for p in (tmp_path / "part").glob("*.pt")) == names[2:5]
    dt.process_directories([tmp_path / "in"], [tmp_path / "tail"], start=5)
    assert sorted(p.name for p in (tmp_path / "tail").glob("*.pt")) == names[5:]

    # seed=1 selects exactly the order of random.seed(1); random.shuffle(sorted(names))
    want = sorted(names)
    random.seed(1)
    random.shuffle(want)
    assert want != sorted(names)
    dt.process_directories([tmp_path / "in"], [tmp_path / "shuffled"], n_files=3, seed=1)
    assert sorted(p.name for p in (tmp_path / "shuffled").glob("*.pt")) == sorted(want[:3])
    dt.process_directories([tmp_path / "in"], [tmp_path / "shuffled2"], start=3, n_files=2, seed=1, batch_size=2)
    assert sorted(p.name for p in (tmp_path / "shuffled2").glob("*.pt")) == sorted(want[3:5])

    # redo=False: existing files are not rewritten, the others are; a stale extra output trips the subset assertion
    (tmp_path / "part" / names[3]).write_bytes(b"sentinel")
    dt.process_directories([tmp_path / "in"], [tmp_path / "part"], redo=False)
    assert (tmp_path / "part" / names[3]).read_bytes() == b"sentinel"
    assert sorted(p.name for p in (tmp_path / "part").glob("*.pt")) == names
    (tmp_path / "part" / "data99999_s0.pt").write_bytes(b"stale")
    with pytest.raises(AssertionError):
        dt.process_directories([tmp_path / "in"], [tmp_path / "part"], redo=False)

    # two pairs of directories
    dt.process_directories([tmp_path / "in", tmp_path / "all"], [tmp_path / "o1", tmp_path / "o2"], n_files=1)
    assert [p.name for p in (tmp_path / "o1").glob("*.pt")] == [p.name for p in (tmp_path / "o2").glob("*.pt")] == names[:1]
    assert yaml.safe_load((tmp_path / "o2" / "hparams").read_text())["input_dir"] == str(tmp_path / "all")


def test_file_names():
    from gnn_tracking_amd.data_transformer import get_event_id_sector_from_str
    from gnn_tracking_amd.io import graph_file_name

    assert get_event_id_sector_from_str("data21003_s17.pt") == (21003, 17)
    assert graph_file_name({"evtid": torch.tensor([21003]), "s": torch.tensor([17])}) == "data21003_s17.pt"
    assert graph_file_name({"evtid": 5, "s": 0}) == "data5_s0.pt"
    for bad in ("cloud7.pt", "data12.pt", "datax_s1.pt"):
        with pytest.raises(ValueError):
            get_event_id_sector_from_str(bad)
