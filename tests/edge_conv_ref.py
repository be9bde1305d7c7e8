"""Float64 restatement of the dynamic edge convolution and of the point-cloud model built on it, written from their
semantics (reference: models/dynamic_edge_conv.py:14-64, models/track_condensation_networks.py:23-115,
models/interaction_network.py:54-103, models/mlp.py:18-62).  TEST INFRASTRUCTURE ONLY: plain torch on the CPU.

``edge_conv`` is the operator on a neighbour table with all gradients; it also returns the restatement's own margins:
the smallest gap between the two largest messages of a (node, feature) - what decides a max - and ``knn_gap`` the
smallest gap between the k-th and (k+1)-th neighbour distance - what decides a neighbourhood."""

from __future__ import annotations

import torch


def _f64(t):
    return None if t is None else t.detach().cpu().double()


def table_slots(nbr, cnt, k, include_self):
    """``(ids int64 [N, S], present bool [N, S])`` of a neighbour table (ids clamped as the kernels clamp them)"""
    n = int(cnt.shape[0])
    nbr, cnt = nbr.detach().cpu().long()[:, :k], cnt.detach().cpu().long().clamp(0, k)
    ids = nbr.clamp(0, max(n - 1, 0))
    present = torch.arange(k)[None, :] < cnt[:, None]
    if include_self:
        ids = torch.cat([torch.arange(n)[:, None], ids], dim=1)
        present = torch.cat([torch.ones(n, 1, dtype=torch.bool), present], dim=1)
    return ids, present


def edge_conv(x, nbr, cnt, k, weights, biases, *, aggr, include_self, relu=False):
    """``(h, top-two gap)`` in float64, differentiable with respect to float64 leaves passed in; the gap is the
    smallest difference between the largest and the second largest message over the (node, feature) pairs with two
    or more slots (``inf`` if there is none)."""
    n = int(x.shape[0])
    ids, present = table_slots(nbr, cnt, k, include_self)
    S = ids.shape[1]
    W1, W2 = weights
    b1, b2 = biases
    xi = x[:, None, :].expand(n, S, x.shape[1])
    xj = x[ids.reshape(-1)].reshape(n, S, -1) if n else xi
    hid = torch.cat([xi, xj - xi], dim=-1) @ W1.T
    hid = torch.relu(hid if b1 is None else hid + b1)
    msg = hid @ W2.T
    msg = msg if b2 is None else msg + b2          # [N, S, O]
    pm = present[:, :, None]
    count = present.sum(1)
    if aggr == "max":
        masked = msg.masked_fill(~pm, float("-inf"))
        h = masked.max(dim=1).values
        h = torch.where(count[:, None] > 0, h, torch.zeros_like(h))
    else:
        h = (msg * pm).sum(1)
        if aggr == "mean":
            h = h / count.clamp(min=1)[:, None]
    gap = float("inf")
    two = count >= 2
    if bool(two.any()):
        top = msg.detach().masked_fill(~pm, float("-inf"))[two].topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
    return (torch.relu(h) if relu else h), gap


def edge_conv_with_grads(x, nbr, cnt, k, weights, biases, r, *, aggr, include_self, relu=False):
    """``(h, [gx, gW1, gb1, gW2, gb2], gap)`` of ``(h * r).sum()``; absent biases give None"""
    leaves = [_f64(t) for t in (x, weights[0], biases[0], weights[1], biases[1])]
    for t in leaves:
        if t is not None:
            t.requires_grad_()
    xx, W1, b1, W2, b2 = leaves
    h, gap = edge_conv(xx, nbr, cnt, k, [W1, W2], [b1, b2], aggr=aggr, include_self=include_self, relu=relu)
    (h * _f64(r)).sum().backward()
    grads = [None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)) for t in leaves]
    return h.detach(), grads, gap


# ------------------------------------------------------------------------------------- neighbour search
def _distances(x, batch=None):
    d = torch.cdist(x.double(), x.double())
    if batch is not None:
        b = batch.detach().cpu().long()
        d = d.masked_fill(b[:, None] != b[None, :], float("inf"))
    return d


def knn_edges(x, k, batch=None):
    """``torch_cluster.knn(x, x, k).flip([0])``: int64 ``[2, M]``, row 0 the neighbour, row 1 the query, grouped by
    query, ascending distance with the query itself first (distance 0; ties: self, then the lower index)."""
    x = x.detach().cpu()
    n = int(x.shape[0])
    d = _distances(x, batch)
    d[torch.arange(n), torch.arange(n)] = -1.0
    dist, idx = torch.sort(d, dim=1, stable=True)
    kk = min(k, n)
    dist, idx = dist[:, :kk], idx[:, :kk]
    ok = torch.isfinite(dist)
    q = torch.arange(n)[:, None].expand_as(idx)
    return torch.stack([idx[ok], q[ok]])


def knn_gap(x, k, batch=None):
    """the smallest gap between the distance of the last neighbour taken (the query itself is the first of the ``k``)
    and the first one left out, over the queries that leave one out; ``inf`` if none does"""
    x = x.detach().cpu()
    n = int(x.shape[0])
    d = _distances(x, batch)
    d[torch.arange(n), torch.arange(n)] = -1.0
    dist = torch.sort(d, dim=1).values
    if k >= n or k < 1:
        return float("inf")
    g = dist[:, k] - dist[:, k - 1]
    g = g[torch.isfinite(dist[:, k])]
    return float(g.min()) if g.numel() else float("inf")


# ------------------------------------------------------------------------------------- modules
def mlp(sd, prefix, x, n_linear):
    """Linear -> ReLU -> ... -> Linear over the keys ``<prefix>layers.{0, 2, ..}``"""
    for i in range(n_linear):
        x = x @ sd[f"{prefix}layers.{2 * i}.weight"].T + sd[f"{prefix}layers.{2 * i}.bias"]
        if i < n_linear - 1:
            x = torch.relu(x)
    return x


def _aggregate(msg, tgt, n, aggr):
    out = torch.zeros(n, msg.shape[1], dtype=msg.dtype)
    idx = tgt[:, None].expand_as(msg)
    if aggr == "add":
        return out.scatter_add(0, idx, msg)
    return out.scatter_reduce(0, idx, msg, {"mean": "mean", "max": "amax"}[aggr], include_self=False)


def dynamic_edge_conv(sd, prefix, x, k, aggr, batch=None, n_linear=2):
    """``(h, edge_index, gaps)``; ``gaps = (knn gap, top-two message gap)``"""
    ei = knn_edges(x, k, batch)
    xi, xj = x[ei[1]], x[ei[0]]
    msg = mlp(sd, prefix, torch.cat([xi, xj - xi], dim=1), n_linear)
    h = _aggregate(msg, ei[1], int(x.shape[0]), aggr)
    top_gap = float("inf")
    if aggr == "max":
        n = int(x.shape[0])
        for i in range(n):
            m = msg.detach()[ei[1] == i]
            if m.shape[0] >= 2:
                t = m.topk(2, dim=0).values
                top_gap = min(top_gap, float((t[0] - t[1]).min()))
    return h, ei, (knn_gap(x, k, batch), top_gap)


def interaction_network(sd, prefix, x, ei, e):
    src, tgt = ei[0], ei[1]
    e_new = mlp(sd, prefix + "relational_model.", torch.cat([x[tgt], x[src], e], dim=1), 3)
    aggr = _aggregate(e_new, tgt, int(x.shape[0]), "add")
    return mlp(sd, prefix + "object_model.", torch.cat([x, aggr], dim=1), 3), e_new


def in_conv_block(sd, prefix, x, k, L, alpha=0.5, batch=None):
    """``(h, gaps of its neighbour search)``"""
    h, ei, gaps = dynamic_edge_conv(sd, prefix + "node_encoder.", x, k, "add", batch)
    h = torch.relu(h)
    e = torch.relu(mlp(sd, prefix + "edge_encoder.", torch.cat([h[ei[0]], h[ei[1]]], dim=1), 2))
    for l in range(L):
        dh, e = interaction_network(sd, f"{prefix}layers.{l}.", h, ei, e)
        h = alpha * h + (1 - alpha) * dh
    return h, gaps


def point_cloud_tcn(sd, x, N_blocks, L, batch=None):
    """``({"H", "B"}, smallest knn gap over the blocks, scale)``; the scale is the largest magnitude of a block's
    input, at least 1"""
    ks = [N_blocks] + [N_blocks - i for i in range(N_blocks)]
    h, gap, scale = x, float("inf"), 1.0
    for b, k in enumerate(ks):
        scale = max(scale, float(h.detach().abs().max())) if h.numel() else scale
        h, gaps = in_conv_block(sd, f"layers.{b}.", h, k, L, batch=batch)
        gap = min(gap, gaps[0])
    beta = torch.sigmoid(mlp(sd, "B.", h, 3)).squeeze() + 10e-12
    return {"H": mlp(sd, "X.", h, 3), "B": beta}, gap, scale
