"""The float64 restatement of the dynamic edge convolution and of the point-cloud model (tests/edge_conv_ref.py)
reproduces what the reference itself computed (tests/golden/g25_edge_conv.npz, written by
tools/make_golden_edge_conv.py): outputs, edge lists and every gradient.  No GPU and no kernel: these tests pin the
reference the emulator and GPU tests compare with."""

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
from gnn_tracking_amd import ops

import edge_conv_cases as E
import edge_conv_ref as R
import parity_cases as P

TOL = 1e-5   # the golden file is float32 arithmetic of the reference, the restatement float64


def _state(z, c, shapes):
    keys, flat, sd, at = [str(k) for k in z[c + ".keys"]], z[c + ".p"], {}, 0
    for k in keys:
        n = int(np.prod(shapes[k]))
        sd[k] = P.tt(flat[at:at + n]).reshape(shapes[k]).double()
        at += n
    assert at == flat.shape[0]
    return sd


def _grads_by_key(sd, gkeys):
    """leaves for the ``named_parameters`` keys; the aliases of a shared tensor point at the same leaf"""
    leaves = {k: sd[k].clone().requires_grad_() for k in gkeys}
    full = dict(sd)
    for k in sd:
        if k in leaves:
            full[k] = leaves[k]
        elif ".edge_conv.nn." in k or k.startswith("edge_conv.nn."):
            full[k] = leaves[k.replace("edge_conv.nn.", "node_encoder.")]
    return leaves, full


def _compare_grads(leaves, gkeys, flat, tag, thin=False):
    at = 0
    for k in gkeys:
        g = leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])
        g = g.reshape(-1)
        if thin and g.numel() > 512:
            g = g[::8]
        P.assert_close(g, flat[at:at + g.numel()], P.TOL_GRAD, f"{tag} grad {k}")
        at += g.numel()
    assert at == flat.shape[0]


@pytest.mark.parametrize("c", E.DEC_GOLDEN)
def test_restatement_reproduces_dynamic_edge_conv(c):
    z = P.load(E.GOLD)
    aggr, tag = c.split("_")[1:]
    k = {"k4": 4, "k1": 1, "n3k5": 5}[tag]
    model = G.DynamicEdgeConv(G.MLP(12, 5, hidden_dim=16, L=2), k=k, aggr=aggr)
    sd = _state(z, c, {k_: tuple(v.shape) for k_, v in model.state_dict().items()})
    gkeys = [str(k_) for k_ in z[c + ".gkeys"]]
    leaves, full = _grads_by_key(sd, gkeys)
    x = P.tt(z[c + ".x"]).double().requires_grad_()
    h, ei, (kgap, tgap) = R.dynamic_edge_conv(full, "nn.", x, k, aggr)
    assert np.array_equal(ei.numpy(), z[c + ".edge_index"])
    scale = max(1.0, float(x.detach().abs().max()), float(h.detach().abs().max()))
    assert kgap > 1e-4 * scale and (aggr != "max" or tgap > 2 * P.TOL_OUT * scale)   # the tool's margins
    (h * P.tt(z[c + ".r.h"]).double()).sum().backward()
    P.assert_close(h, z[c + ".out.h"], TOL, c + " h")
    P.assert_close(x.grad, z[c + ".gx"], P.TOL_GRAD, c + " grad x")
    _compare_grads(leaves, gkeys, z[c + ".g"], c)


def test_restatement_reproduces_in_conv_block():
    z = P.load(E.GOLD)
    model = G.INConvBlock(6, 5, 4, L=2, k=3, hidden_dim=16)
    sd = _state(z, "inconv", {k: tuple(v.shape) for k, v in model.state_dict().items()})
    # the reference's state_dict holds the shared encoder under both names, with the same values
    for k in sd:
        if k.startswith("edge_conv.nn."):
            assert torch.equal(sd[k], sd[k.replace("edge_conv.nn.", "node_encoder.")])
    gkeys = [str(k) for k in z["inconv.gkeys"]]
    assert not any(k.startswith("edge_conv.nn.") for k in gkeys)
    leaves, full = _grads_by_key(sd, gkeys)
    x = P.tt(z["inconv.x"]).double().requires_grad_()
    h, (kgap, _t) = R.in_conv_block(full, "", x, 3, 2)
    assert kgap > 1e-4 * max(1.0, float(x.detach().abs().max()))
    (h * P.tt(z["inconv.r.h"]).double()).sum().backward()
    P.assert_close(h, z["inconv.out.h"], TOL, "inconv h")
    P.assert_close(x.grad, z["inconv.gx"], P.TOL_GRAD, "inconv grad x")
    _compare_grads(leaves, gkeys, z["inconv.g"], "inconv")


def test_restatement_reproduces_point_cloud_tcn():
    z = P.load(E.GOLD)
    torch.manual_seed(int(z["pctcn.pseed"]))
    model = G.PointCloudTCN(6, h_dim=5, e_dim=4, h_outdim=3, hidden_dim=16, N_blocks=2, L=2)
    own = model.state_dict()
    assert list(own) == [str(k) for k in z["pctcn.keys"]]
    assert [float(v.double().sum()) for v in own.values()] == [float(s) for s in z["pctcn.psum"]]
    # (the blocks are 100 wide whatever hidden_dim says; the heads take it)
    assert own["layers.0.node_encoder.layers.0.weight"].shape == (100, 12) and own["B.layers.0.weight"].shape == (16, 5)
    sd = {k: v.detach().double() for k, v in own.items()}
    gkeys = [str(k) for k in z["pctcn.gkeys"]]
    leaves, full = _grads_by_key(sd, gkeys)
    x = P.tt(z["pctcn.x"]).double().requires_grad_()
    out, kgap, scale = R.point_cloud_tcn(full, x, 2, 2)
    assert kgap > 1e-4 * scale
    sum((out[n] * P.tt(z[f"pctcn.r.{n}"]).double()).sum() for n in ("H", "B")).backward()
    for n in ("H", "B"):
        P.assert_close(out[n], z[f"pctcn.out.{n}"], TOL, "pctcn " + n)
    P.assert_close(x.grad, z["pctcn.gx"], P.TOL_GRAD, "pctcn grad x")
    _compare_grads(leaves, gkeys, z["pctcn.g"], "pctcn", thin=True)


def test_golden_file_is_small():
    assert (P.GOLD / E.GOLD).stat().st_size < 200 * 1024


@pytest.mark.parametrize("row", [r for r in E.SWEEP if r[7] == "max"], ids=E.sweep_id)
def test_max_rows_of_the_sweep_have_the_gap(row):
    """the seeds of the max rows: the restatement's top-two gap exceeds the kernels' tolerance, so a max and its
    gradient cannot go to another slot"""
    n, k, D, H, O, bias, relu, aggr, include_self, seed = row
    assert seed is not None
    ref = E.reference(E.problem(seed, n, k, D, H, O, bias, "cpu"), aggr, include_self, relu)
    assert E.gap_holds(ref)


def test_table_edges_is_the_restatements_edge_list():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 3, generator=g)
    nbr, cnt = E.knn_table(x, 4, k_stride=6)
    assert torch.equal(ops.table_edges(nbr, cnt, 4, True), R.knn_edges(x, 5))
    cnt[::4] = 1
    cnt[3] = 0
    ei = ops.table_edges(nbr, cnt, 4, False)
    ids, present = R.table_slots(nbr, cnt, 4, False)
    assert torch.equal(ei[0], ids[present]) and int(ei.shape[1]) == int(cnt.sum()) and 3 not in ei[1].tolist()
    assert ops.table_edges(nbr[:0], cnt[:0], 4, True).shape == (2, 0)


def test_exports_and_switch_default():
    for name in ("DynamicEdgeConv", "INConvBlock", "PointCloudTCN"):
        assert name in G.__all__ and hasattr(G, name)
    assert G.PointCloudTCN.per_event is True
    assert ops.edge_conv_supported(14, 100, 10, 4) and not ops.edge_conv_supported(33, 100, 10, 4)
    assert not ops.edge_conv_supported(14, 129, 10, 4) and not ops.edge_conv_supported(14, 100, 33, 4)
    assert not ops.edge_conv_supported(14, 100, 10, 65)
    with pytest.raises(NotImplementedError):
        G.DynamicEdgeConv(G.MLP(12, 5, 16, L=2), k=3, aggr="min")
    E.case_interaction_network_still_sum_only()
