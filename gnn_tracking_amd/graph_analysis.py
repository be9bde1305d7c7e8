"""Graph analysis of the metric-learning validation on the device (``analysis/graphs.py:281-343``,
``metrics/graph_construction.py:8-31``): connected-component labels, the largest-segment fraction of
every particle and the edge efficiency / purity of a built graph.

The reference copies the edges to the host, builds a networkx graph and walks its components in
Python.  Here the components are a lock-free union-find (``gnntrk_cc_labels``, ``csrc/kscan.hip``)
and everything else is an integer count (``gnntrk_kscan_counts`` for the k-scan,
``k_scanner.GraphConstructionKNNScanner``).  Differences that are not contract in the reference:

* ``get_cc_labels`` labels a component by its SMALLEST node index (networkx: by discovery order).  The
  partition is the same; the labels are unique and repeatable.
* ``get_largest_segment_fracs`` returns the fractions ordered by the particle's first masked hit (the
  reference: the insertion order of a Python dict filled while walking networkx's components, then a
  ``set`` difference).  Only the multiset of fractions is contract; every use in the reference is a
  mean of a comparison.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from . import _capi, ops
from .graph_masks import get_good_node_mask

__all__ = ["get_cc_labels", "get_largest_segment_fracs", "get_efficiency_purity_edges"]


def cc_labels(edge_index: Tensor, num_nodes: int, *, same_pid: Tensor | None = None,
              node_mask: Tensor | None = None, check: bool = True) -> Tensor:
    """Int64 labels ``[num_nodes]`` of the connected components of the undirected graph ``edge_index``
    (``[2, M]``): the smallest node index of every component.  ``same_pid`` (int64 ``[num_nodes]``): keep
    an edge only if its ends carry the same value; ``node_mask`` (bool ``[num_nodes]``): keep an edge only
    if both ends pass - both evaluated in the kernel.  ``check``: read the number of edges with an end
    outside ``[0, num_nodes)`` back (one host read) and raise if there are any."""
    _capi.require_device(edge_index)
    lib = _capi.load()
    n = int(num_nodes)
    ei = edge_index.detach().to(torch.int64).contiguous()
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError(f"cc_labels: edge_index must be [2, M], got {tuple(ei.shape)}")
    dev = ei.device
    pid = None if same_pid is None else same_pid.detach().to(device=dev, dtype=torch.int64).contiguous()
    mask = None if node_mask is None else node_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    for name, t in (("same_pid", pid), ("node_mask", mask)):
        if t is not None and (t.dim() != 1 or int(t.shape[0]) != n):
            raise ValueError(f"cc_labels: {name} has shape {tuple(t.shape)}, expected ({n},)")
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = ops._ws(lib.gnntrk_cc_labels_workspace_bytes(n), ei)
    p = ops._p
    _capi.check(lib.gnntrk_cc_labels(p(ei), int(ei.shape[1]), None, None, 0, 0, p(pid), p(mask), n, p(labels), p(bad),
                                     p(ws), ws.numel(), ops._stream(ei)), lib)
    if check and int(bad.item()):
        raise ValueError(f"cc_labels: {int(bad.item())} edges have an end outside [0, {n})")
    return labels


def get_cc_labels(edge_index: Tensor, num_nodes: int) -> Tensor:
    """``analysis/graphs.py:331-343``: labels for the connected components of a graph, on the device of
    ``edge_index``.  A component's label is its smallest node index (see the module docstring)."""
    return cc_labels(edge_index, num_nodes)


def _segment_counts(data, pt_thld: float, max_eta: float):
    """(mask, labels of the masked same-id components, particle ids) of ``data`` on the device."""
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    pid = data.particle_id.to(torch.int64)
    n = int(pid.shape[0])
    y = getattr(data, "y", None)
    ei = data.edge_index
    if y is not None:   # (the reference strips every edge that is not flagged true: edge_index[:, data.y])
        ei = ei[:, y.bool()]
    # every component has to be single-id (graphs.py:319 reads the id of one of its hits): as in the
    # k-scan, where y = pid[e0] == pid[e1], the id filter is applied in the kernel as well
    labels = cc_labels(ei, n, same_pid=pid, node_mask=mask)
    return mask, labels, pid


def get_largest_segment_fracs(data, *, pt_thld=0.9, n_particles_sampled=None, max_eta=4) -> np.ndarray:
    """``analysis/graphs.py:281-328``: for every particle with hits in the good-node mask, the fraction
    of its masked hits that lie in its largest segment (connected component of the ``data.y`` edges whose
    both ends are masked).  ``data.y`` must flag same-particle edges only, as the k-scan's does.  Returns
    a float64 numpy array; its ORDER is by the particle's first masked hit (the reference's order is an
    implementation detail of dict / set iteration).  ``n_particles_sampled`` draws that many particles at
    random, as the reference does, after the exact computation (it exists there to shorten a host loop)."""
    mask, labels, pid = _segment_counts(data, float(pt_thld), float(max_eta))
    if not bool(mask.any()):
        return np.array([], dtype=np.float64)
    pm, lm = pid[mask], labels[mask]
    upid, pinv, pcount = torch.unique(pm, return_inverse=True, return_counts=True)
    _, linv, lcount = torch.unique(lm, return_inverse=True, return_counts=True)
    largest = torch.zeros_like(pcount).scatter_reduce(0, pinv, lcount[linv], reduce="amax")
    first = torch.full_like(pcount, pm.numel()).scatter_reduce(
        0, pinv, torch.arange(pm.numel(), device=pm.device), reduce="amin")
    order = torch.argsort(first)
    fr = (largest.double() / pcount.double())[order].cpu().numpy()
    if n_particles_sampled is not None:
        fr = fr[torch.randperm(len(fr)).numpy()[:n_particles_sampled]]
    return fr


def efficiency_purity_from_counts(n_true_masked: int, n_true_edges_masked: int, n_masked: int) -> dict[str, float]:
    """The two divisions of ``metrics/graph_construction.py:23-24`` as torch evaluates them: both int64
    counts cast to float32, the quotient in float32 (0 / 0 = nan, x / 0 = inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        num = np.float32(n_true_masked)
        eff = num / np.float32(2 * int(n_true_edges_masked))
        pur = num / np.float32(n_masked)
    return {"efficiency": float(eff), "purity": float(pur)}


def get_efficiency_purity_edges(data, pt_thld: float = 0.9, max_eta: float = 4.0) -> dict[str, float]:
    """``metrics/graph_construction.py:8-31``: efficiency and purity of ``data.edge_index`` (labels
    ``data.y``) against ``data.true_edge_index``; only edges with at least one end in the good-node mask
    count.  Masked sums on the device, one host copy of three integers."""
    mask = get_good_node_mask(data, pt_thld=pt_thld, max_eta=max_eta)
    ei, te = data.edge_index, data.true_edge_index
    edge_mask = mask[ei[0]] | mask[ei[1]]
    counts = torch.stack([(data.y.bool() & edge_mask).sum(), (mask[te[0]] & mask[te[1]]).sum(), edge_mask.sum()])
    return efficiency_purity_from_counts(*(int(v) for v in counts.tolist()))
