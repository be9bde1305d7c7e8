#!/usr/bin/env python3
"""Golden vectors of the dynamic edge convolution and the point-cloud model, FROM THE REFERENCE ITSELF:
``tests/golden/g25_edge_conv.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``, default
``/root/reference``).  It installs the stand-ins of ``oracle/_ref_standins.py`` (unchanged) for the third-party
packages the reference imports, then replaces ``torch_geometric.nn.conv.MessagePassing`` - that third-party class
only - with a stand-in of its own that takes a pair ``x`` and aggregates with add, mean or max
(``scatter_reduce``, ``include_self=False``, a node without a message gives 0), and runs the reference's own
``DynamicEdgeConv`` (models/dynamic_edge_conv.py), ``INConvBlock`` and ``PointCloudTCN``
(models/track_condensation_networks.py): outputs and all parameter and input gradients.

Per case ``<c>``: ``<c>.x``, ``<c>.keys`` (the ``state_dict`` key list, in order), ``<c>.p`` (the parameters,
flattened and joined in that order), ``<c>.r.<name>`` (random weights of the outputs), ``<c>.out.<name>``,
``<c>.edge_index`` (``DynamicEdgeConv``), ``<c>.gkeys`` and ``<c>.g`` (the ``named_parameters`` keys and the gradients of
``sum_name (out * r).sum()``, flattened and joined in that order) and ``<c>.gx``.  ``pctcn`` has, instead of
its parameters, ``pctcn.pseed`` (``torch.manual_seed(pseed)`` before the constructor gives them) with ``pctcn.psum``
(their float64 sums, in key order), and of every gradient above 512 elements every 8th element: its blocks are 100
wide whatever ``hidden_dim`` says, and the file stays under 200 KB.

Cases: ``DynamicEdgeConv`` with add, mean and max on 50 hits (D 6, H 16, O 5) with k = 4 and k = 1, and on 3 hits
with k = 5; ``INConvBlock(6, 5, 4, L=2, k=3, hidden_dim=16)``; ``PointCloudTCN(6, h_dim=5, e_dim=4, h_outdim=3,
hidden_dim=16, N_blocks=2, L=2)``.

The seeds are searched until two margins of the float64 restatement (tests/edge_conv_ref.py) hold, so that an error
of TOL_OUT cannot change a neighbourhood or a maximum: in every block the gap between the last neighbour taken and
the first left out exceeds 1e-4 x scale (ten times TOL_OUT: an error of TOL_OUT in h moves a distance by at most
twice that), and for max the gap between the two largest messages exceeds 2 x TOL_OUT x scale.  The margins are
printed.

Usage:  python tools/make_golden_edge_conv.py [--ref PATH]
"""

from __future__ import annotations

import argparse
import os
import pathlib
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "g25_edge_conv.npz"
TOL_OUT = 1e-5
DEC_CASES = {"k4": (50, 4), "k1": (50, 1), "n3k5": (3, 5)}
D, H, O = 6, 16, 5


class MessagePassing(torch.nn.Module):
    """``torch_geometric.nn.conv.MessagePassing`` for ``flow="source_to_target"``: ``x`` a tensor or a pair
    ``(x_src, x_dst)``, ``x_j = x_src[edge_index[0]]``, ``x_i = x_dst[edge_index[1]]``, the messages aggregated onto
    ``edge_index[1]`` with add, mean or max; a node without a message gets 0."""

    def __init__(self, aggr="add", flow="source_to_target", **_kw):
        super().__init__()
        assert aggr in ("add", "mean", "max") and flow == "source_to_target"
        self.aggr = aggr

    def propagate(self, edge_index, size=None, **kwargs):
        x = kwargs["x"]
        x_src, x_dst = x if isinstance(x, tuple) else (x, x)
        rest = {k: v for k, v in kwargs.items() if k != "x"}
        msg = self.message(x_i=x_dst.index_select(0, edge_index[1]), x_j=x_src.index_select(0, edge_index[0]), **rest)
        out = torch.zeros(x_dst.shape[0], msg.shape[1], dtype=msg.dtype)
        idx = edge_index[1].view(-1, 1).expand_as(msg)
        if self.aggr == "add":
            out = out.scatter_add(0, idx, msg)
        else:
            out = out.scatter_reduce(0, idx, msg, "mean" if self.aggr == "mean" else "amax", include_self=False)
        return self.update(out)

    def update(self, aggr_out):
        return aggr_out


SUBSAMPLE_ABOVE, SUBSAMPLE_STRIDE = 512, 8


def thin(g):
    """a gradient as it is stored: whole up to SUBSAMPLE_ABOVE elements, every SUBSAMPLE_STRIDE-th element of the
    flattened tensor above (the 100 x 100 matrices of the model at its default width)"""
    g = np.asarray(g)
    return g if g.size <= SUBSAMPLE_ABOVE else g.reshape(-1)[::SUBSAMPLE_STRIDE].copy()


def record(out: dict, c: str, model, x, outputs: dict, seed: int, params_from_seed: bool = False):
    sd = model.state_dict()
    out[f"{c}.keys"] = np.array(list(sd))
    if params_from_seed:
        # the blocks of PointCloudTCN are 100 wide whatever its hidden_dim is (it does not hand the argument on:
        # models/track_condensation_networks.py:93-95): the parameters are those torch.manual_seed(seed) gives the
        # constructor, recorded as their float64 sums, and the large gradients are thinned
        out[f"{c}.pseed"] = np.array(seed)
        out[f"{c}.psum"] = np.array([float(v.detach().double().sum()) for v in sd.values()])
    else:
        out[f"{c}.p"] = np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])
    g = torch.Generator().manual_seed(seed)
    loss = 0.0
    for name, t in outputs.items():
        r = torch.randn(t.shape, generator=g)
        out[f"{c}.out.{name}"], out[f"{c}.r.{name}"] = t.detach().numpy(), r.numpy()
        loss = loss + (t * r).sum()
    model.zero_grad()
    loss.backward()
    grads = [p.grad.numpy().reshape(-1) for _k, p in model.named_parameters()]
    out[f"{c}.gkeys"] = np.array([k for k, _p in model.named_parameters()])
    out[f"{c}.g"] = np.concatenate([thin(g) if params_from_seed else g for g in grads])
    out[f"{c}.x"], out[f"{c}.gx"] = x.detach().numpy(), x.grad.numpy().copy()


def sd64(model):
    return {k: v.detach().double() for k, v in model.state_dict().items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", type=pathlib.Path, default=pathlib.Path("/root/reference"))
    args = ap.parse_args()
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(REPO / "tests"))
    sys.path.insert(0, str(args.ref / "src"))
    import _ref_standins

    _ref_standins.install()
    conv = types.ModuleType("torch_geometric.nn.conv")
    conv.MessagePassing = MessagePassing
    sys.modules["torch_geometric.nn.conv"] = conv
    import edge_conv_ref as R
    from gnn_tracking.models.dynamic_edge_conv import DynamicEdgeConv
    from gnn_tracking.models.mlp import MLP
    from gnn_tracking.models.track_condensation_networks import INConvBlock, PointCloudTCN

    Data = _ref_standins.Data
    out: dict = {}

    def scale_of(*ts):
        return max(1.0, *[float(t.detach().abs().max()) for t in ts])

    # ---- DynamicEdgeConv
    for aggr in ("add", "mean", "max"):
        for tag, (n, k) in DEC_CASES.items():
            c = f"dec_{aggr}_{tag}"
            for seed in range(2500, 2600):
                torch.manual_seed(seed)
                x = torch.randn(n, D, requires_grad=True)
                model = DynamicEdgeConv(MLP(2 * D, O, hidden_dim=H, L=1), k=k, aggr=aggr)
                h, ei = model(x)
                hr, eir, (kgap, tgap) = R.dynamic_edge_conv(sd64(model), "nn.", x.detach().double(), k, aggr)
                assert torch.equal(ei, eir), c
                assert float((h.detach().double() - hr).abs().max()) < 1e-5 * scale_of(hr), c
                s = scale_of(x, hr)
                if kgap > 1e-4 * s and (aggr != "max" or tgap > 2 * TOL_OUT * s):
                    break
            else:
                raise SystemExit(f"{c}: no seed with the margins")
            print(f"{c}: seed {seed}, knn gap {kgap:.3e}, top-two gap {tgap:.3e}, scale {s:.3g}, {ei.shape[1]} edges")
            assert model.get_edge_index() is ei
            record(out, c, model, x, {"h": h}, seed)
            out[f"{c}.edge_index"] = ei.numpy()

    # ---- INConvBlock
    for seed in range(2600, 2700):
        torch.manual_seed(seed)
        x = torch.randn(50, 6, requires_grad=True)
        model = INConvBlock(6, 5, 4, L=2, k=3, hidden_dim=16)
        h = model(x)
        hr, (kgap, _t) = R.in_conv_block(sd64(model), "", x.detach().double(), 3, 2)
        assert float((h.detach().double() - hr).abs().max()) < 1e-5 * scale_of(hr)
        if kgap > 1e-4 * scale_of(x):
            break
    else:
        raise SystemExit("inconv: no seed with the margin")
    print(f"inconv: seed {seed}, knn gap {kgap:.3e}")
    record(out, "inconv", model, x, {"h": h}, seed)

    # ---- PointCloudTCN
    for seed in range(2700, 2900):
        torch.manual_seed(seed)   # (the constructor first: the test draws the same parameters from the seed)
        model = PointCloudTCN(6, h_dim=5, e_dim=4, h_outdim=3, hidden_dim=16, N_blocks=2, L=2)
        x = torch.randn(50, 6, requires_grad=True)
        res = model(Data(x=x))
        assert res["W"] is None and res["P"] is None
        rr, kgap, s = R.point_cloud_tcn(sd64(model), x.detach().double(), 2, 2)
        for name in ("H", "B"):
            assert float((res[name].detach().double() - rr[name]).abs().max()) < 1e-5 * scale_of(rr[name]), name
        if kgap > 1e-4 * s:
            break
    else:
        raise SystemExit("pctcn: no seed with the margin")
    print(f"pctcn: seed {seed}, smallest knn gap over the blocks {kgap:.3e}, scale {s:.3g}")
    record(out, "pctcn", model, x, {"H": res["H"], "B": res["B"]}, seed, params_from_seed=True)

    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < 200 * 1024, size
    print(f"wrote {OUT} ({size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
