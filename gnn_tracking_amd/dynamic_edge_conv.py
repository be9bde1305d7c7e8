"""``DynamicEdgeConv`` on the device (reference: models/dynamic_edge_conv.py:14-64): a k-nearest-neighbour graph
built from the features it convolves, and the edge convolution
``h_i = aggr_{j in kNN(i)} nn(cat[x_i, x_j - x_i])`` over it.

Same constructor keywords, ``state_dict`` keys (``nn.*``) and return value ``(h, edge_index)`` as the reference.
The search is the package's exact kNN with ``k - 1`` neighbours plus the query itself as slot 0 (in
``torch_cluster.knn(x, x, k)`` the query is its own nearest neighbour); the convolution is ``ops.edge_conv`` on
that table: one launch each way (csrc/edge_conv.hip) for a two-linear ``MLP`` in fp32 when the kernel path is
on, the composed path otherwise.
"""

from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor, nn

from . import _capi, events, ops
from .mlp import MLP


class DynamicEdgeConv(nn.Module):
    def __init__(self, nn: Callable, k: int, aggr: str = "max", num_workers: int = 1, **kwargs):
        """Args:
            nn: maps ``[x_i, x_j - x_i]`` (``[-1, 2 * in]``) to the messages (``[-1, out]``)
            k: number of nearest neighbours, the query itself included
            aggr: "add", "mean" or "max"
            num_workers: accepted for the reference's signature (the search runs on the device)
        """
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"DynamicEdgeConv: unsupported MessagePassing arguments {sorted(kwargs)}")
        if aggr not in ("add", "mean", "max"):
            raise NotImplementedError("DynamicEdgeConv: aggr must be 'add', 'mean' or 'max'")
        self.aggr = aggr
        self.flow = "source_to_target"
        self.nn = nn
        self.k = k
        self.num_workers = num_workers
        self.reset_parameters()
        self.edge_index = None

    def reset_parameters(self):
        self.nn.reset_parameters()

    def get_edge_index(self):
        return self.edge_index

    def neighbour_table(self, x: Tensor, seg_ptr: Tensor | None = None):
        """``(nbr int32 [N, max(k', 1)], cnt int32 [N], k')`` of the ``k' = min(k - 1, N - 1)`` nearest OTHER rows
        of every row (inside its own event with ``seg_ptr``), ascending distance."""
        lib = _capi.load()
        xs = ops._as_rows(x.detach().float())
        n = int(xs.shape[0])
        kk = max(0, min(int(self.k) - 1, n - 1))
        nbr = torch.zeros(n, max(kk, 1), dtype=torch.int32, device=x.device)
        cnt = torch.zeros(n, dtype=torch.int32, device=x.device)
        if kk > 0:
            sp = seg_ptr.to(device=x.device, dtype=torch.int64).contiguous() if seg_ptr is not None else None
            ops._knn_search(lib, xs, kk, -1.0, sp, nbr, cnt, ops._stream(xs))
        return nbr, cnt, kk

    def forward(self, x, batch=None, *, relu: bool = False):
        """``(h, edge_index)``: ``edge_index`` int64 ``[2, M]``, row 0 the neighbour, row 1 the query, grouped by
        query, the query itself first, then ascending distance (``torch_cluster.knn(x, x, k).flip([0])``).
        ``batch``: neighbours are searched inside the query's event.  ``relu``: ReLU on ``h`` (what
        ``INConvBlock`` applies at once), inside the kernel."""
        if isinstance(x, (tuple, list)):
            if len(x) != 2 or x[0] is not x[1]:
                raise NotImplementedError("DynamicEdgeConv: a pair (x_src, x_dst) of two different tensors (a bipartite "
                                          "graph) is not implemented; pass one tensor")
            x = x[0]
        if isinstance(batch, (tuple, list)):
            if len(batch) != 2 or batch[0] is not batch[1]:
                raise NotImplementedError("DynamicEdgeConv: a pair of two different batch vectors is not implemented")
            batch = batch[0]
        if x.dim() != 2:
            raise ValueError("Static graphs not supported in DynamicEdgeConv")
        _capi.require_device(x)
        seg_ptr = events.event_ptr(batch=batch, who="DynamicEdgeConv") if batch is not None else None
        nbr, cnt, kk = self.neighbour_table(x, seg_ptr)
        k_tab = max(kk, 1)
        self.edge_index = ops.table_edges(nbr, cnt, k_tab, True)
        two_linear = isinstance(self.nn, MLP) and self.nn.L == 2 and not self.nn._last_act
        if two_linear:
            lin = self.nn.linears()
            h = ops.edge_conv(x, nbr, cnt, [m.weight for m in lin], [m.bias for m in lin], aggr=self.aggr,
                              include_self=True, relu=relu, k=k_tab, edge_index=self.edge_index)
        else:
            h = ops.edge_conv_composed(x, nbr, cnt, k_tab, self.nn, aggr=self.aggr, include_self=True, relu=relu,
                                       edge_index=self.edge_index)
        return h, self.edge_index

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(nn={self.nn}, k={self.k})"
