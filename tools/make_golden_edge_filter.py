#!/usr/bin/env python3
"""Golden vectors of the edge filters, FROM THE REFERENCE ITSELF: ``tests/golden/g19_edge_filter.npz``.

TEST INFRASTRUCTURE ONLY; runs on a CPU machine next to a checkout of the reference (``--ref``, default
``/root/reference``).  It installs the stand-ins of ``oracle/_ref_standins.py`` for the third-party packages the
reference imports and runs the reference's own ``EFMLP``, ``EFDeepSet`` and ``GeometricEF``
(models/edge_filter.py) on small random graphs: about 60 hits and 203 edges with duplicate edges, self-loops
and hits without an edge.

Per case ``<c>``: ``<c>.x``, ``<c>.edge_index``, ``<c>.edge_attr`` (where used), ``<c>.keys`` (the
``state_dict`` key list, in order), ``<c>.p.<key>`` (parameters), ``<c>.W`` (or the bool ``<c>.mask``),
``<c>.r`` (random [E]) and ``<c>.g.<key>`` (gradients of ``(W * r).sum()``), ``<c>.hp`` (constructor arguments,
as ``name=value`` strings).

Cases: EFMLP (node 14, edge 28, hidden 40, depth 3), (14, 0, 16, 1), (3, 4, 33, 2); EFDeepSet (in 14, hidden 24,
depth 3); GeometricEF with an edge whose dr is 0 and a self-loop (dR = 0).

Usage:  python tools/make_golden_edge_filter.py [--ref PATH]
"""

from __future__ import annotations

import argparse
import os
import pathlib
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "g19_edge_filter.npz"

N_HITS, N_EDGES = 60, 203
EFMLP_CASES = {
    "efmlp_a": dict(node_indim=14, edge_indim=28, hidden_dim=40, depth=3),
    "efmlp_b": dict(node_indim=14, edge_indim=0, hidden_dim=16, depth=1),
    "efmlp_c": dict(node_indim=3, edge_indim=4, hidden_dim=33, depth=2),
}


def graph(seed: int, node_dim: int, edge_dim: int):
    """Hits 0 .. 54 carry edges, 55 .. 59 none; edges 0 and 1 are equal, edges 2 and 3 self-loops."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_HITS, node_dim, generator=g)
    ei = torch.randint(0, N_HITS - 5, (2, N_EDGES), generator=g)
    ei[:, 1] = ei[:, 0]
    ei[1, 2] = ei[0, 2]
    ei[1, 3] = ei[0, 3]
    ea = torch.randn(N_EDGES, edge_dim, generator=g) if edge_dim else None
    r = torch.randn(N_EDGES, generator=g)
    return x, ei, ea, r


def record(out: dict, c: str, model, hp: dict, W, r):
    out[f"{c}.hp"] = np.array([f"{k}={v}" for k, v in hp.items()])
    sd = model.state_dict()
    out[f"{c}.keys"] = np.array(list(sd))
    for k, v in sd.items():
        out[f"{c}.p.{k}"] = v.detach().numpy()
    out[f"{c}.W"] = W.detach().numpy()
    out[f"{c}.r"] = r.numpy()
    (W * r).sum().backward()
    for k, p in model.named_parameters():
        out[f"{c}.g.{k}"] = p.grad.numpy()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", type=pathlib.Path, default=pathlib.Path("/root/reference"))
    args = ap.parse_args()
    sys.path.insert(0, str(REPO / "oracle"))
    sys.path.insert(0, str(args.ref / "src"))
    import _ref_standins

    _ref_standins.install()
    from gnn_tracking.models.edge_filter import EFMLP, EFDeepSet, GeometricEF

    Data = _ref_standins.Data
    out: dict = {}
    for n, (c, hp) in enumerate(EFMLP_CASES.items()):
        torch.manual_seed(190 + n)
        x, ei, ea, r = graph(290 + n, hp["node_indim"], hp["edge_indim"])
        model = EFMLP(**hp)
        W = model(Data(x=x, edge_index=ei, edge_attr=ea))["W"]
        out[f"{c}.x"], out[f"{c}.edge_index"] = x.numpy(), ei.numpy()
        if ea is not None:
            out[f"{c}.edge_attr"] = ea.numpy()
        record(out, c, model, dict(hp, beta=0.4), W, r)

    torch.manual_seed(195)
    hp = dict(in_dim=14, hidden_dim=24, depth=3)
    x, ei, _ea, r = graph(295, 14, 0)
    model = EFDeepSet(**hp)
    W = model(Data(x=x, edge_index=ei))["W"]
    out["deepset.x"], out["deepset.edge_index"] = x.numpy(), ei.numpy()
    record(out, "deepset", model, hp, W, r)

    # GeometricEF: (r, phi, z, eta) and two more columns; edge 4 joins two hits of equal r (dr = 0: z0 is inf
    # or NaN), edges 2 and 3 are self-loops (dR = 0: phi_slope is NaN); cuts near the medians
    x, ei, _ea, _r = graph(296, 6, 0)
    x[:, 0] = x[:, 0].abs() + 0.5
    x[int(ei[1, 4]), 0] = x[int(ei[0, 4]), 0]
    hp = dict(phi_slope_max=0.8, z0_max=2.0, dR_max=1.7)
    mask = GeometricEF(**hp)(Data(x=x, edge_index=ei))
    assert mask.dtype == torch.bool and not bool(mask[2]) and not bool(mask[3]) and not bool(mask[4])
    assert 0.1 < mask.float().mean() < 0.9, mask.float().mean()
    out["geometric.x"], out["geometric.edge_index"], out["geometric.mask"] = x.numpy(), ei.numpy(), mask.numpy()
    out["geometric.hp"] = np.array([f"{k}={v}" for k, v in hp.items()])

    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < 200 * 1024, size
    print(f"wrote {OUT} ({size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
