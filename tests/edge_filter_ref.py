"""float64 restatement of the three edge filters (``gnn_tracking_amd/edge_filter.py``), written from their
formulae.  TEST INFRASTRUCTURE ONLY: plain torch on the CPU, autograd for the gradients.

  EFMLP       v = [x_i, x_j, a_e];  h = W_enc v;  h <- sqrt(beta) W_l relu(h) + sqrt(1 - beta) h;
              W = 0.001 + 0.998 sigmoid(w_dec . relu(h))
  EFDeepSet   h = relu-terminated MLP(x / max(|x|, 1e-12));  u_e = [|h_i - h_j|, h_i + h_j];
              W = 1e-8 + (1 - 2e-8) sigmoid(MLP(u_e))
  GeometricEF (r, phi, z, eta) = x[:, :4];  dR = sqrt(deta^2 + dphi^2);
              |dphi / dR| < phi_slope_max  &  |z_i - r_i dz / dr| < z0_max  &  |dR| < dR_max
with i = edge_index[0], j = edge_index[1] and d. = ._i - ._j.
"""

import math

import torch


def _d(t):
    """float64 on the CPU; a float64 CPU tensor passes as it is (it may be a leaf of the caller's graph)."""
    if t is None or (torch.is_tensor(t) and t.dtype == torch.float64 and t.device.type == "cpu"):
        return t
    return torch.as_tensor(t).detach().cpu().double()


def edge_features(x, edge_index):
    """``ops.edge_features``: [x_i - x_j, x_i + x_j]."""
    x, i, j = _d(x), edge_index[0].cpu(), edge_index[1].cpu()
    return torch.cat((x[i] - x[j], x[i] + x[j]), dim=1)


def ef_mlp(x, edge_index, edge_attr, weights, beta):
    """``W`` [E] (float64, on the autograd graph of ``weights``, a list of float64 tensors)."""
    x, ea = _d(x), _d(edge_attr)
    i, j = edge_index[0].cpu(), edge_index[1].cpu()
    v = torch.cat([x[i], x[j]] + ([ea] if ea is not None and ea.shape[1] > 0 else []), dim=1)
    h = v @ weights[0].T
    for w in weights[1:-1]:
        h = math.sqrt(beta) * (torch.relu(h) @ w.T) + math.sqrt(1 - beta) * h
    return 0.001 + 0.998 * torch.sigmoid(torch.relu(h) @ weights[-1].T).reshape(-1)


def ef_mlp_with_grads(x, edge_index, edge_attr, weights, beta, r):
    """``(W, [d (W . r).sum() / d weight])``."""
    ws = [_d(w).requires_grad_() for w in weights]
    W = ef_mlp(x, edge_index, edge_attr, ws, beta)
    if W.numel() == 0:
        return W.detach(), [torch.zeros_like(w) for w in ws]
    grads = torch.autograd.grad((W * _d(r)).sum(), ws)
    return W.detach(), list(grads)


def _mlp(v, weights, last_relu):
    for n, w in enumerate(weights):
        if n > 0:
            v = torch.relu(v)
        v = v @ w.T
    return torch.relu(v) if last_relu else v


def pair_invariants(h, edge_index):
    i, j = edge_index[0].cpu(), edge_index[1].cpu()
    return torch.cat(((h[i] - h[j]).abs(), h[i] + h[j]), dim=1)


def ef_deepset(x, edge_index, enc_weights, agg_weights):
    x = _d(x)
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    u = pair_invariants(_mlp(x, enc_weights, True), edge_index)
    return 1e-8 + (1 - 2e-8) * torch.sigmoid(_mlp(u, agg_weights, False)).reshape(-1)


def ef_deepset_with_grads(x, edge_index, enc_weights, agg_weights, r):
    we, wa = [_d(w).requires_grad_() for w in enc_weights], [_d(w).requires_grad_() for w in agg_weights]
    W = ef_deepset(x, edge_index, we, wa)
    grads = torch.autograd.grad((W * _d(r)).sum(), we + wa)
    return W.detach(), list(grads[:len(we)]), list(grads[len(we):])


def geometric_ef(x, edge_index, phi_slope_max, z0_max, dR_max, dtype=torch.float32):
    """The bool mask, evaluated in ``dtype`` (the cuts compare rounded fp32 values: the mask is defined at the
    inputs' precision)."""
    x = torch.as_tensor(x).detach().cpu().to(dtype)
    i, j = edge_index[0].cpu(), edge_index[1].cpu()
    r, phi, z, eta = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    dz, dr, dphi, deta = z[i] - z[j], r[i] - r[j], phi[i] - phi[j], eta[i] - eta[j]
    dR = torch.sqrt(deta**2 + dphi**2)
    return ((dphi / dR).abs() < phi_slope_max) & ((z[i] - r[i] * dz / dr).abs() < z0_max) & (dR.abs() < dR_max)
