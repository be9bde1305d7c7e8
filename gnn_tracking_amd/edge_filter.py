"""Edge filters: decisions from the features of the edge under consideration alone, without message
passing (reference: models/edge_filter.py).  The second learned stage of the pipeline, between the
metric-learning embedding and the GraphTCN: ``MLGraphConstruction(ec=EFMLP(...), ec_threshold=...)``.

Constructors, ``hparams``, ``state_dict`` keys and outputs are the reference's, so its checkpoints load.

* ``EFMLP``: one launch for the whole residual MLP on gathered edge rows (``ops_ml.ef_mlp``:
  csrc/edge_filter.hip), a chunked backward that keeps no edge-sized activations.  Outside the kernel's
  limits, or when ``data.x`` / ``data.edge_attr`` need a gradient, the same operator composed from library
  ops.  ``GNNTRK_EFMLP=1`` selects the kernel path, ``0`` (the default until the kernel path is measured
  faster at event size) the composed path.
* ``EFDeepSet``: two ``MLP`` s (the package's fused or GEMM paths) around the pair-invariant kernel.
* ``GeometricEF``: geometric cuts, one elementwise expression over the edges (no kernel: DESIGN.md 4.15).
"""

from __future__ import annotations

import math
import os

import torch
from torch import Tensor, nn

from . import _capi, ops_ml
from .hparams import HyperparametersMixin, assert_feat_dim
from .mlp import MLP

_EFMLP_KERNEL = os.environ.get("GNNTRK_EFMLP", "0") != "0"


class EFDeepSet(nn.Module, HyperparametersMixin):
    def __init__(self, *, in_dim: int = 14, hidden_dim: int = 128, depth: int = 3):
        """EdgeFilter based on the deep sets architecture (models/edge_filter.py:22-65)."""
        super().__init__()
        self.save_hyperparameters()
        self.node_encoder = MLP(input_size=in_dim, output_size=hidden_dim, hidden_dim=hidden_dim, L=depth, bias=False,
                                include_last_activation=True)
        self.aggregator = MLP(input_size=2 * hidden_dim, output_size=1, L=depth, hidden_dim=2 * hidden_dim, bias=False)

    def forward(self, data) -> dict[str, Tensor]:
        _capi.require_device(data.x, data.edge_index)
        x = nn.functional.normalize(data.x.float(), p=2.0, dim=1, eps=1e-12)
        h = self.node_encoder(x).float()
        z = self.aggregator(ops_ml.pair_invariants(h, data.edge_index)).float()
        epsilon = 1e-8
        return {"W": epsilon + (1 - 2 * epsilon) * torch.sigmoid(z).squeeze(-1)}


class EFMLP(nn.Module, HyperparametersMixin):
    def __init__(self, *, node_indim: int, edge_indim: int = 0, hidden_dim: int, depth: int, beta: float = 0.4):
        """EdgeFilter based on an MLP architecture (models/edge_filter.py:68-141).

        Args:
            node_indim: dimension of the node features
            edge_indim: dimension of the edge features; 0: do not use edge features
            hidden_dim: dimension of the hidden layers
            depth: number of hidden layers
            beta: weight of a residual layer's update: ``sqrt(beta) layer(relu(x)) + sqrt(1 - beta) x``
        """
        super().__init__()
        self.save_hyperparameters()
        self.encoder = nn.Linear(node_indim * 2 + edge_indim, hidden_dim, bias=False)
        self.decoder = nn.Linear(hidden_dim, 1, bias=False)
        self.layers = nn.ModuleList([nn.Linear(hidden_dim, hidden_dim, bias=False) for _ in range(depth - 1)])
        self.reset_parameters()

    def reset_parameters(self):
        hp = self.hparams
        self._reset_layer_parameters(self.encoder, var=1 / (2 * hp.node_indim + hp.edge_indim))
        for layer in self.layers:
            self._reset_layer_parameters(layer, var=2 / hp.hidden_dim)
        self._reset_layer_parameters(self.decoder, var=2 / hp.hidden_dim)

    @staticmethod
    def _reset_layer_parameters(layer, var: float):
        layer.reset_parameters()
        for p in layer.parameters():
            nn.init.normal_(p.data, mean=0, std=math.sqrt(var))

    def weights(self) -> list[Tensor]:
        return [self.encoder.weight, *[layer.weight for layer in self.layers], self.decoder.weight]

    def kernel_supported(self) -> bool:
        """The shape is one ``gnntrk_efmlp_*`` holds and the kernel path is switched on."""
        hp = self.hparams
        return _EFMLP_KERNEL and ops_ml.ef_mlp_supported(hp.node_indim, hp.edge_indim, hp.hidden_dim, hp.depth)

    def score(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor | None, *, derived: bool = False,
              workspace_cap: int | None = None) -> Tensor:
        """``W`` [E].  ``derived``: ``edge_attr`` is None and stands for ``ops.edge_features(x, edge_index)``
        (kernel path only)."""
        hp = self.hparams
        _capi.require_device(x, edge_index)
        assert_feat_dim(x, hp.node_indim)
        if hp.edge_indim > 0 and not derived:
            assert_feat_dim(edge_attr, hp.edge_indim)
        ea = edge_attr if hp.edge_indim > 0 else None
        # (bf16 storage mode: the filter computes in fp32 on converted inputs, as ResFCNN.forward)
        x = x.float()
        ea = None if ea is None else ea.float()
        needs_input_grad = torch.is_grad_enabled() and (x.requires_grad or (ea is not None and ea.requires_grad))
        if self.kernel_supported() and not needs_input_grad:
            return ops_ml.ef_mlp(x, edge_index, ea, self.weights(), beta=hp.beta, derived=derived,
                                 workspace_cap=workspace_cap)
        if derived:
            raise RuntimeError("EFMLP.score(derived=True) needs the kernel path")
        i, j = edge_index[0], edge_index[1]
        features = [x.index_select(0, i), x.index_select(0, j)]
        if ea is not None:
            features.append(ea)
        h = self.encoder(torch.cat(features, dim=1))
        for layer in self.layers:
            h = math.sqrt(hp.beta) * layer(torch.relu(h)) + math.sqrt(1 - hp.beta) * h
        return 0.001 + 0.998 * torch.sigmoid(self.decoder(torch.relu(h))).squeeze(-1)

    def forward(self, data) -> dict[str, Tensor]:
        return {"W": self.score(data.x, data.edge_index, getattr(data, "edge_attr", None))}


class GeometricEF(nn.Module, HyperparametersMixin):
    def __init__(self, phi_slope_max, z0_max, dR_max):
        """Edge filter with geometric cuts only, no learning required (models/edge_filter.py:144-171):
        ``x[:, :4] = (r, phi, z, eta)``.  Division by zero (``dr = 0``, ``dR = 0``) gives inf or NaN, which
        compares false, as in the reference."""
        super().__init__()
        self.save_hyperparameters()

    def forward(self, data) -> Tensor:
        _capi.require_device(data.x, data.edge_index)
        hp = self.hparams
        xi = data.x.index_select(0, data.edge_index[0])[:, :4]
        xj = data.x.index_select(0, data.edge_index[1])[:, :4]
        d = xi - xj
        dr, dphi, dz, deta = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        dR = torch.sqrt(deta**2 + dphi**2)
        phi_slope = dphi / dR
        z0 = xi[:, 2] - xi[:, 0] * dz / dr
        return (phi_slope.abs() < hp.phi_slope_max) & (z0.abs() < hp.z0_max) & (dR.abs() < hp.dR_max)
