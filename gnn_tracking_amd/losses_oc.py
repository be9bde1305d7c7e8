"""Object-condensation losses on fused HIP reductions.

Reference: metrics/losses/__init__.py:13-41 (``MultiLossFctReturn``) and
metrics/losses/oc.py:164-436 (``CondensationLossRG``, ``CondensationLossTiger``): same
constructor keywords, ``hparams`` and return type.  Neither the N x K matrices of the Tiger
variant nor the radius graph of the RG variant are materialised: both are sums over
(hit, condensation point) pairs evaluated by ``gnntrk_oc_forward/backward`` (csrc/oc.hip).  A collated ``batch`` of
several events is one launch sequence in which every event is its own problem (``_CondensationLoss.per_event``).

``sample_pids < 1`` and Tiger's ``max_n_rep > 0`` (random sub-sampling switches the reference
has for memory) are honoured for parity of the training dynamics; the random draws differ from
the reference's (as they do between its own CPU and GPU runs).
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Any

import torch
from torch import Tensor as T

from . import _capi, events, ops
from .graph_masks import get_good_node_mask_tensors
from .hparams import HyperparametersMixin


@dataclass(kw_only=True)
class MultiLossFctReturn:
    """Return type of loss functions with several terms (losses/__init__.py:13-35)."""

    #: individual loss terms
    loss_dct: dict[str, T]
    #: their weights
    weight_dct: dict[str, T] | dict[str, float]
    #: other things to log
    extra_metrics: dict[str, Any] = field(default_factory=dict)

    def __post_init__(self) -> None:
        assert self.loss_dct.keys() == self.weight_dct.keys()

    @property
    def loss(self) -> T:
        loss = sum(self.weighted_losses.values())
        assert isinstance(loss, torch.Tensor)
        return loss

    @property
    def weighted_losses(self) -> dict[str, T]:
        return {k: v * self.weight_dct[k] for k, v in self.loss_dct.items()}


class MultiLossFct(torch.nn.Module):
    """Base class of loss functions returning ``MultiLossFctReturn``."""

    def forward(self, *args: Any, **kwargs: Any) -> MultiLossFctReturn: ...


#: "auto": the spatial passes from SPATIAL_MIN_HITS hits on (below, sorting the hits costs more than
#: the dense N x K walk); "on" / "off": always / never (tests, measurements)
SPATIAL = os.environ.get("GNNTRK_OC_SPATIAL", "auto")
SPATIAL_MIN_HITS = 16384


def _use_spatial(n: int) -> bool:
    if SPATIAL not in ("auto", "on", "off"):
        raise ValueError(f"losses_oc.SPATIAL must be 'auto', 'on' or 'off', got {SPATIAL!r}")
    return SPATIAL == "on" or (SPATIAL == "auto" and n >= SPATIAL_MIN_HITS)


class _CondensationPotentials(torch.autograd.Function):
    """(attractive, repulsive, coward, noise) and their gradients w.r.t. (beta, x)."""

    @staticmethod
    def forward(ctx, beta, x, particle_id, mask, q_min: float, radius: float, eps_sqrt: float,
                mode: int, keep: float = 1.0, seed: int = 0, cap_nbr=None, stash=None, seg_ptr=None):
        """``stash`` (a dict): the condensation-point selection of a call is left in it / taken from
        it, so that a second pass over the same hits (``max_n_rep`` sub-sampling) does not select -
        sort and scan - again.

        ``seg_ptr`` (int64 ``[B + 1]``, B > 1): the hits are a collated batch of B events (sorted by event) and every
        event is its own problem (``gnntrk_oc_*_batched``); the four terms are the means over the events, ``n_rep`` the
        sum."""
        _capi.require_device(beta, x, particle_id, mask)
        lib = _capi.load()
        dev = x.device
        beta_c = beta.detach().to(torch.float32).contiguous()
        x_c = x.detach().to(torch.float32).contiguous()
        pid = particle_id.to(torch.int64).contiguous()
        mask8 = mask.to(torch.uint8).contiguous()
        n, dim = int(x_c.shape[0]), int(x_c.shape[1])
        st, p = ops._stream(x_c), ops._p
        b = int(seg_ptr.numel()) - 1 if seg_ptr is not None else 0
        if b and (keep < 1.0 or stash is not None):
            raise ValueError("the sub-sampling of repulsive pairs is per event: not supported in a batch")
        cp_ptr = None
        if stash is not None and "sel" in stash:
            alphas, gid, n_cp = stash["sel"]
        else:
            alphas = torch.empty(n, dtype=torch.int32, device=dev)
            gid = torch.empty(n, dtype=torch.int32, device=dev)
            n_cp = torch.zeros(1, dtype=torch.int32, device=dev)
            hits = (p(beta_c), p(pid), p(mask8), n, mode)
            if b:
                cp_ptr = torch.empty(b + 1, dtype=torch.int32, device=dev)
                ws = ops._ws(lib.gnntrk_oc_select_batched_workspace_bytes(n), x_c)
                _capi.check(lib.gnntrk_oc_select_cps_batched(*hits, p(seg_ptr), b, p(alphas), p(gid), p(cp_ptr), p(n_cp),
                                                             p(ws), ws.numel(), st), lib)
            else:
                ws = ops._ws(lib.gnntrk_oc_select_workspace_bytes(n), x_c)
                _capi.check(lib.gnntrk_oc_select_cps(*hits, p(alphas), p(gid), p(n_cp), p(ws), ws.numel(), st), lib)
            if stash is not None:
                stash["sel"] = (alphas, gid, n_cp)
        saved = (beta_c, x_c, pid, mask8, gid, alphas, n_cp)
        ctx.cfg = (q_min, radius, eps_sqrt, mode, beta.dtype, x.dtype, float(keep), int(seed))
        ctx.cap_nbr, ctx.batch, ctx.spatial = cap_nbr, None, None
        a = _oc_args(saved, ctx.cfg, cap_nbr)
        out = torch.empty((b, 9) if b else 9, dtype=torch.float32, device=dev)
        if b:
            ctx.batch = (seg_ptr, cp_ptr)
            ws2 = ops._ws(lib.gnntrk_oc_forward_batched_workspace_bytes(n, b), x_c)
            _capi.check(lib.gnntrk_oc_forward_batched(C.byref(a), p(seg_ptr), p(cp_ptr), b, p(out), p(ws2), ws2.numel(),
                                                      st), lib)
        elif _use_spatial(n) and (nb := int(lib.gnntrk_oc_spatial_workspace_bytes(n, dim))):
            # large events: the pair loops only visit (chunk of hits, condensation point) pairs within the
            # radius (csrc/oc.hip "spatial" passes; same pairs, same per-pair arithmetic); the buffer the
            # forward fills is what the backward reads
            ctx.spatial = ops._ws(nb, x_c)
            _capi.check(lib.gnntrk_oc_forward_spatial(C.byref(a), p(out), p(ctx.spatial), nb, st), lib)
        else:
            ws2 = ops._ws(lib.gnntrk_oc_forward_workspace_bytes(n), x_c)
            _capi.check(lib.gnntrk_oc_forward(C.byref(a), p(out), p(ws2), ws2.numel(), st), lib)
        ctx.save_for_backward(*saved, out)
        # a batch: the terms are the means over the events, n_rep the sum.  n_rep is a plain count: no gradient, no
        # hold on this node's saved tensors
        terms, n_rep = (out[:, :4].mean(0), out[:, 7].double().sum()) if b else (out, out[7].clone())
        ctx.mark_non_differentiable(n_rep)
        return terms[0], terms[1], terms[2], terms[3], n_rep

    @staticmethod
    def backward(ctx, g_att, g_rep, g_cow, g_noise, _g_nrep):
        lib = _capi.load()
        *saved, out = ctx.saved_tensors
        x_c = saved[1]
        bdt, xdt = ctx.cfg[4:6]
        n, dim = int(x_c.shape[0]), int(x_c.shape[1])
        g = torch.stack([t.to(torch.float32).reshape(()) if t is not None
                         else torch.zeros((), device=x_c.device)
                         for t in (g_att, g_rep, g_cow, g_noise)]).contiguous()
        a = _oc_args(saved, ctx.cfg, ctx.cap_nbr)
        gx = torch.empty_like(x_c)
        gbeta = torch.empty_like(saved[0])
        if ctx.batch is not None:
            seg_ptr, cp_ptr = ctx.batch
            b = int(seg_ptr.numel()) - 1
            g = (g / b).contiguous()   # the terms are means over the events
            ws = ops._ws(lib.gnntrk_oc_backward_batched_workspace_bytes(n, dim), x_c)
            _capi.check(lib.gnntrk_oc_backward_batched(C.byref(a), ops._p(seg_ptr), ops._p(cp_ptr), b, ops._p(g),
                                                       ops._p(out), ops._p(gx), ops._p(gbeta), ops._p(ws), ws.numel(),
                                                       ops._stream(x_c)), lib)
        elif ctx.spatial is not None:
            _capi.check(lib.gnntrk_oc_backward_spatial(C.byref(a), ops._p(g), ops._p(out), ops._p(gx), ops._p(gbeta),
                                                       n, ops._p(ctx.spatial), ctx.spatial.numel(),
                                                       ops._stream(x_c)), lib)
        else:
            ws = ops._ws(lib.gnntrk_oc_backward_workspace_bytes(n, dim), x_c)
            _capi.check(lib.gnntrk_oc_backward(C.byref(a), ops._p(g), ops._p(out), ops._p(gx),
                                               ops._p(gbeta), n, ops._p(ws), ws.numel(), ops._stream(x_c)), lib)
        return gbeta.to(bdt), gx.to(xdt), None, None, None, None, None, None, None, None, None, None, None


def _oc_args(saved, cfg, cap_nbr) -> "_capi.OcArgs":
    """the argument block of every ``gnntrk_oc_*`` forward and backward entry, from the tensors a node saves"""
    beta_c, x_c, pid, mask8, gid, alphas, n_cp = saved
    q_min, radius, eps_sqrt, mode, _bdt, _xdt, keep, seed = cfg
    n, dim = int(x_c.shape[0]), int(x_c.shape[1])
    return _capi.OcArgs(ops._p(x_c), ops._p(beta_c), ops._p(pid), ops._p(mask8), ops._p(gid), ops._p(alphas),
                        ops._p(n_cp), n, dim, dim, q_min, radius, eps_sqrt, mode, keep, 0, seed, ops._p(cap_nbr))


class _CondensationLoss(MultiLossFct, HyperparametersMixin):
    _mode = 0
    _eps_sqrt = 1e-9
    #: a ``batch`` of more than one event: every event is its own problem (condensation points per (event, particle
    #: id), attraction, repulsion and all norms inside the event) and each term is the mean over the events - the
    #: gradient of accumulating over single-event steps.  False: the reference's behaviour, which ignores ``batch``
    #: (particle ids repeat from event to event: hits of different events share a condensation point).  A class
    #: attribute so that YAML configurations stay those of the reference.
    per_event = True

    def _neighbor_cap(self, x, seg_ptr=None):   # (only the radius-graph variant has one)
        return None

    def _forward(self, *, beta: T, x: T, particle_id: T, reconstructable: T, pt: T,
                 ec_hit_mask: T | None, eta: T, mask_eta: bool, batch: T | None = None) -> MultiLossFctReturn:
        if batch is not None and not self.per_event:
            batch = None
        if batch is not None and batch.shape[0] != particle_id.shape[0]:
            raise ValueError(f"`batch` has {batch.shape[0]} entries for {particle_id.shape[0]} hits")
        if ec_hit_mask is not None and not getattr(ec_hit_mask, "_gnntrk_all_true", False):
            # model outputs already carry the post-EC node mask, data attributes do not
            particle_id = particle_id[ec_hit_mask]
            reconstructable = reconstructable[ec_hit_mask]
            pt = pt[ec_hit_mask]
            if mask_eta:
                eta = eta[ec_hit_mask]
            if batch is not None:
                batch = batch[ec_hit_mask]
        seg_ptr = events.event_ptr(batch=batch, who=None)   # (its order: in the read below)
        mask = get_good_node_mask_tensors(pt=pt, particle_id=particle_id,
                                          reconstructable=reconstructable, eta=eta,
                                          pt_thld=self.hparams.pt_thld,
                                          max_eta=self.hparams.max_eta)
        if self.hparams.sample_pids < 1:
            # oc.py:222-226 / :403-407: a random subset of the hits of interest (the reference does
            # it to save memory; kept for parity of the training dynamics)
            mask = mask & (torch.rand_like(beta, dtype=torch.float16) < self.hparams.sample_pids)
        # If there are no hits left after masking, then we get a NaN loss.
        max_n_rep = int(getattr(self.hparams, "max_n_rep", 0) or 0)
        if seg_ptr is None:
            assert bool(mask.any()), "No hits left after masking"
        else:
            if max_n_rep > 0:
                raise ValueError("CondensationLossTiger(max_n_rep > 0) samples the repulsive pairs per event: not "
                                 "supported with more than one event in `batch`")
            # per event, and whether `batch` is sorted, in the one host read the assertion costs
            seen = torch.cat((mask.new_zeros(1, dtype=torch.int64), torch.cumsum(mask, 0, dtype=torch.int64)))
            flags = torch.cat(((seen[seg_ptr[1:]] > seen[seg_ptr[:-1]]), events.unsorted(batch).reshape(1))).tolist()
            if flags[-1]:
                raise ValueError("condensation loss: `batch` must be sorted (PyG convention)")
            for e, left in enumerate(flags[:-1]):
                assert left, f"No hits left after masking (event {e})"
        args = (beta, x, particle_id, mask, float(self.hparams.q_min), 1.0, self._eps_sqrt, self._mode)
        cap = self._neighbor_cap(x, seg_ptr)
        stash = {} if max_n_rep > 0 else None
        att, rep, cow, noise, n_rep = _CondensationPotentials.apply(*args, 1.0, 0, cap, stash, seg_ptr)
        if max_n_rep > 0 and int(n_rep) > max_n_rep:
            # oc.py:322-328: keep repulsive pairs with probability max_n_rep / n_rep and scale the
            # normalisation accordingly.  The pairs are chosen by a hash of (seed, hit, condensation
            # point) inside the kernels (no N x K random matrix); the seed comes from torch's
            # generator, so runs are reproducible under torch.manual_seed.  n_rep is reported
            # before the sub-sampling, as the reference does.
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            att, rep, cow, noise, _ = _CondensationPotentials.apply(*args, max_n_rep / float(n_rep), seed, cap, stash)
        losses = {"attractive": att, "repulsive": rep, "coward": cow, "noise": noise}
        weights = {"attractive": 1.0, "repulsive": self.hparams.lw_repulsive,
                   "noise": self.hparams.lw_noise, "coward": self.hparams.lw_coward}
        extra = {"n_rep": n_rep} if self._mode == 1 else {}
        return MultiLossFctReturn(loss_dct=losses, weight_dct=weights, extra_metrics=extra)


class CondensationLossRG(_CondensationLoss):
    _mode = 0
    _eps_sqrt = 1e-9

    def __init__(self, *, lw_repulsive: float = 1.0, lw_noise: float = 0.0, lw_coward: float = 0.0,
                 q_min: float = 0.01, pt_thld: float = 0.9, max_eta: float = 4.0,
                 max_num_neighbors: int = 256, sample_pids: float = 1.0):
        """Condensation loss, radius-graph formulation (oc.py:164-248).

        Args:
            lw_repulsive: weight of the repulsive potential
            lw_noise: weight of the noise loss
            lw_coward: weight of the coward loss
            q_min: minimal charge (object condensation paper)
            pt_thld: pt threshold of the particles of interest
            max_eta: eta threshold of the particles of interest
            max_num_neighbors: neighbour cap of the reference's radius graph (oc.py:115-117).  Applied when
                it can bind (``neighbor_cap``, below): the fused kernel sums over ALL hits within the unit
                radius, which is the reference's result whenever no hit has more neighbours than the cap
            sample_pids: fraction of the hits of interest that take part (random, per call)
        """
        super().__init__()
        self.save_hyperparameters()

    _cap_notice_given = False
    #: "auto" (default): a count pass over the hits (``ops.max_radius_count``) decides - if no hit has more than
    #: ``max_num_neighbors`` other hits inside the unit radius the cap cannot bind and every hit inside the radius of
    #: a condensation point contributes (= the reference); if one has, the cap is applied nearest first (and a notice
    #: is logged once).  The count is a hits x hits pass (4.6 ms at 200 k hits - the fused loss itself only ever looks
    #: at (hit, condensation point) pairs, 0.6 ms), so it runs on the first call and then on every
    #: ``cap_check_every``-th one; calls in between reuse the last decision (an embedding space drifts over many
    #: steps; ``cap_check_every = 1`` decides on every call).  "nearest": always applied nearest first - a
    #: condensation point only repels a hit if it is among that hit's ``max_num_neighbors`` nearest hits (one extra
    #: kNN search per call; what the CPU oracle's radius graph does; torch_cluster itself keeps an
    #: implementation-defined subset: the first ones found, differently on CPU and GPU).  "off": never applied.
    #: Class attributes so that YAML configurations stay those of the reference.
    neighbor_cap = "auto"
    cap_check_every = 64

    def _neighbor_cap(self, x, seg_ptr=None):
        # a batch: the count below runs over the hits of all events together - an upper bound of every event's own
        # count - and the k-th neighbour is searched inside the hit's event
        mode = self.neighbor_cap
        if mode == "off":
            return None
        if mode not in ("auto", "nearest"):
            raise ValueError(f"CondensationLossRG.neighbor_cap must be 'auto', 'nearest' or 'off', got {mode!r}")
        k = int(self.hparams.max_num_neighbors)
        if mode == "auto":
            if x.shape[0] - 1 <= k:
                return None
            calls = self._cap_calls = getattr(self, "_cap_calls", -1) + 1
            known = getattr(self, "_cap_binds", None)
            if x.is_cuda and torch.cuda.is_current_stream_capturing():
                # the decision needs a device read: a captured step replays the one its eager warm-up made
                if known is None:
                    raise RuntimeError("CondensationLossRG(neighbor_cap='auto') inside a stream capture needs one eager "
                                       "call first (or neighbor_cap = 'off' / 'nearest')")
                binds = known
            elif known is None or calls % max(int(self.cap_check_every), 1) == 0:
                # (radius widened by 1e-6: the count's fp64 `d2 <= r^2` then covers the fp32 `dist < 1` of the graph)
                binds = self._cap_binds = bool(int(ops.max_radius_count(x, 1.0 + 1e-6)) > k)
            else:
                binds = known
            if not binds:
                return None
            if not CondensationLossRG._cap_notice_given:
                CondensationLossRG._cap_notice_given = True
                import logging
                logging.getLogger("gnn_tracking_amd").warning(
                    "CondensationLossRG: a hit has more than max_num_neighbors=%s hits inside the unit radius - the cap "
                    "is applied nearest first (torch_cluster.radius_graph keeps an implementation-defined subset there, "
                    "differently on CPU and GPU).", k)
        return ops.knn_kth_neighbor(x, k, 1.0, seg_ptr=seg_ptr)

    def forward(self, *, beta: T, x: T, particle_id: T, reconstructable: T, pt: T,
                ec_hit_mask: T | None = None, eta: T, batch: T | None = None, **kwargs) -> MultiLossFctReturn:
        # NB: like the reference (oc.py:207-213) eta is NOT sliced by ec_hit_mask here
        return self._forward(beta=beta, x=x, particle_id=particle_id,
                             reconstructable=reconstructable, pt=pt, ec_hit_mask=ec_hit_mask,
                             eta=eta, mask_eta=False, batch=batch)


class CondensationLossTiger(_CondensationLoss):
    _mode = 1
    _eps_sqrt = 0.0

    def __init__(self, *, lw_repulsive: float = 1.0, lw_noise: float = 0.0, lw_coward: float = 0.0,
                 q_min: float = 0.01, pt_thld: float = 0.9, max_eta: float = 4.0, max_n_rep: int = 0,
                 sample_pids: float = 1.0):
        """Condensation loss, dense formulation (oc.py:350-436) without the N x K matrices.

        Args: as ``CondensationLossRG``; ``max_n_rep``: if more repulsive pairs than this are
            inside the unit radius, a random subset of about that size is used (0: all).
        """
        super().__init__()
        self.save_hyperparameters()

    def forward(self, *, beta: T, x: T, particle_id: T, reconstructable: T, pt: T,
                ec_hit_mask: T | None = None, eta: T, batch: T | None = None, **kwargs) -> MultiLossFctReturn:
        return self._forward(beta=beta, x=x, particle_id=particle_id,
                             reconstructable=reconstructable, pt=pt, ec_hit_mask=ec_hit_mask,
                             eta=eta, mask_eta=True, batch=batch)
