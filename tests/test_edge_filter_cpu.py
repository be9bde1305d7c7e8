"""The edge filters without a device: the float64 restatement (tests/edge_filter_ref.py) against golden vectors of
the reference's own classes (tests/golden/g19_edge_filter.npz, tools/make_golden_edge_filter.py), and the public
surface: ``state_dict`` keys, ``hparams``, initialisation, ``MLGraphConstruction``'s argument check."""

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G

import edge_filter_ref as R
import parity_cases as P

Z = P.load("g19_edge_filter.npz")
EFMLP_CASES = ("efmlp_a", "efmlp_b", "efmlp_c")


def _hp(case):
    return dict(kv.split("=") for kv in Z[case + ".hp"])


def _efmlp(case):
    return G.EFMLP(**{k: (float(v) if k == "beta" else int(v)) for k, v in _hp(case).items()})


@pytest.mark.parametrize("case", EFMLP_CASES)
def test_restatement_agrees_with_the_reference_efmlp(case):
    # (state_dict order: encoder, decoder, layers; the restatement takes the weights in layer order)
    keys = sorted(Z[case + ".keys"], key=lambda k: (k.startswith("decoder"), not k.startswith("encoder"), k))
    assert keys[0] == "encoder.weight" and keys[-1] == "decoder.weight"
    ea = Z[case + ".edge_attr"] if case + ".edge_attr" in Z.files else None
    W, grads = R.ef_mlp_with_grads(Z[case + ".x"], P.tt(Z[case + ".edge_index"]), ea,
                                   [P.tt(Z[f"{case}.p.{k}"]) for k in keys], float(_hp(case)["beta"]), Z[case + ".r"])
    P.assert_close(W, Z[case + ".W"], P.TOL_OUT, case + " W")
    for k, g in zip(keys, grads):
        P.assert_close(g, Z[f"{case}.g.{k}"], P.TOL_GRAD, f"{case} grad {k}")


def test_restatement_agrees_with_the_reference_deepset():
    keys = list(Z["deepset.keys"])
    enc, agg = [k for k in keys if k.startswith("node_encoder.")], [k for k in keys if k.startswith("aggregator.")]
    assert enc + agg == keys
    W, ge, ga = R.ef_deepset_with_grads(Z["deepset.x"], P.tt(Z["deepset.edge_index"]), [P.tt(Z["deepset.p." + k]) for k in enc],
                                        [P.tt(Z["deepset.p." + k]) for k in agg], Z["deepset.r"])
    P.assert_close(W, Z["deepset.W"], P.TOL_OUT, "deepset W")
    for k, g in zip(enc + agg, ge + ga):
        P.assert_close(g, Z["deepset.g." + k], P.TOL_GRAD, "deepset grad " + k)


def test_restatement_agrees_with_the_reference_geometric():
    hp = {k: float(v) for k, v in _hp("geometric").items()}
    ei = P.tt(Z["geometric.edge_index"])
    mask = R.geometric_ef(Z["geometric.x"], ei, **hp)
    want = Z["geometric.mask"]
    assert np.array_equal(mask.numpy(), want)
    # the self-loops (dR = 0) and the edge with dr = 0 are cut: NaN and inf compare false
    assert (ei[0, 2] == ei[1, 2]) and (ei[0, 3] == ei[1, 3]) and not want[2] and not want[3]
    assert Z["geometric.x"][ei[0, 4], 0] == Z["geometric.x"][ei[1, 4], 0] and not want[4]
    assert 0 < want.sum() < want.size


@pytest.mark.parametrize("case", EFMLP_CASES)
def test_state_dict_keys_and_hparams_efmlp(case):
    model = _efmlp(case)
    assert list(model.state_dict()) == list(Z[case + ".keys"])
    model.load_state_dict({k: P.tt(Z[f"{case}.p.{k}"]) for k in Z[case + ".keys"]}, strict=True)
    hp = _hp(case)
    assert dict(model.hparams) == dict(node_indim=int(hp["node_indim"]), edge_indim=int(hp["edge_indim"]),
                                       hidden_dim=int(hp["hidden_dim"]), depth=int(hp["depth"]), beta=0.4)


def test_state_dict_keys_and_hparams_deepset_and_geometric():
    model = G.EFDeepSet(in_dim=14, hidden_dim=24, depth=3)
    assert list(model.state_dict()) == list(Z["deepset.keys"])
    model.load_state_dict({k: P.tt(Z["deepset.p." + k]) for k in Z["deepset.keys"]}, strict=True)
    assert dict(model.hparams) == dict(in_dim=14, hidden_dim=24, depth=3)
    assert dict(G.EFDeepSet().hparams) == dict(in_dim=14, hidden_dim=128, depth=3)
    geo = G.GeometricEF(0.8, 2.0, dR_max=1.7)
    assert dict(geo.hparams) == dict(phi_slope_max=0.8, z0_max=2.0, dR_max=1.7) and not list(geo.state_dict())


def test_efmlp_initialisation_variances():
    torch.manual_seed(0)
    model = G.EFMLP(node_indim=14, edge_indim=28, hidden_dim=128, depth=5)
    assert len(model.layers) == 4 and model.decoder.weight.shape == (1, 128) and model.encoder.weight.shape == (128, 56)
    assert all(p.dim() == 2 for p in model.parameters())   # no biases
    # sample variance of n normal draws: relative standard error sqrt(2 / n); five of them as the bound
    for w, var in ((model.encoder.weight, 1 / 56), *((l.weight, 2 / 128) for l in model.layers)):
        assert abs(float(w.detach().var()) / var - 1) < 5 * (2 / w.numel()) ** 0.5
        assert abs(float(w.detach().mean())) < 5 * (var / w.numel()) ** 0.5
    assert abs(float(model.decoder.weight.detach().var()) / (2 / 128) - 1) < 5 * (2 / 128) ** 0.5


def test_graph_construction_needs_a_threshold_and_records_the_filter():
    ef = G.EFMLP(node_indim=6, edge_indim=12, hidden_dim=16, depth=2)
    with pytest.raises(ValueError, match="ec_threshold"):
        G.MLGraphConstruction(ec=ef)
    gc = G.MLGraphConstruction(ec=ef, ec_threshold=0.3)
    assert gc.hparams.ec == {"class_path": "gnn_tracking_amd.edge_filter.EFMLP",
                             "init_args": dict(node_indim=6, edge_indim=12, hidden_dim=16, depth=2, beta=0.4)}
    again = G.MLGraphConstruction(ec=gc.hparams.ec, ec_threshold=0.3)
    assert isinstance(again._ef, G.EFMLP) and all(not p.requires_grad for p in again._ef.parameters())


def test_filters_refuse_cpu_tensors():
    data = G.Data(x=torch.zeros(3, 6), edge_index=torch.zeros(2, 4, dtype=torch.long), edge_attr=torch.zeros(4, 12))
    for model in (G.EFMLP(node_indim=6, edge_indim=12, hidden_dim=16, depth=2), G.EFDeepSet(in_dim=6, hidden_dim=8),
                  G.GeometricEF(1.0, 1.0, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            model(data)
