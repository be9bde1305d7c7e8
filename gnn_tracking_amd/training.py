"""One optimisation step of the hot path without Lightning.

Reference: ``training/base.py:72-116`` (``TrackingModule``: ``data_preproc`` -> ``forward`` ->
``get_losses`` -> backward -> ``configure_optimizers``' Adam), ``training/ec.py:25-53``
(``ECModule``), ``training/tc.py:20-84`` (``TCModule``) and ``training/ml.py:25-78`` (``MLModule``).  The Lightning trainer around them
(logging, checkpointing, schedulers, OOM tolerance) is control plane and stays in the
reference; what is here is the arithmetic of one step, under the reference's method names, so
that bench.py, the parity tests and a user's own loop run the same code:

    step = TCModule(model=GraphTCN(...), loss_fct=CondensationLossRG(...),
                    preproc=MLGraphConstruction(...))
    loss = step.optimisation_step(batch)

Data parallelism: pass ``flat=dist.FlatParameters(model)``; gradients are then accumulated in
the flat bucket and all-reduced over RCCL before the optimizer step (dist.py).
"""

from __future__ import annotations

from typing import Any, Callable, Optional

import torch
from torch import Tensor, nn

from . import ops
from .precision import bf16_storage


class TrackingModule:
    """``training/base.py:72-116`` without the Lightning base class."""

    def __init__(self, model: nn.Module, *, optimizer: Callable[..., torch.optim.Optimizer] = torch.optim.Adam,
                 scheduler: Optional[Callable[..., Any]] = torch.optim.lr_scheduler.ConstantLR,
                 preproc: Optional[nn.Module] = None, flat=None, bf16: bool = False):
        """
        Args:
            model: the network (``forward(data) -> dict``)
            optimizer: called with the parameters, as Lightning calls ``OptimizerCallable``
                (default Adam, base.py:77); built on first use
            scheduler: called with the optimizer (default ``ConstantLR``, base.py:78 - note that
                its default factor 1/3 applies from construction on, i.e. the reference's first
                five epochs run at a third of the learning rate); ``None`` for none.  Stepping
                it (once per epoch in Lightning) is the caller's business: ``self.scheduler``
            preproc: optional module applied to every batch first (``MLGraphConstruction``)
            flat: ``dist.FlatParameters`` of ``model`` (+ ``preproc`` parameters if trained): one
                gradient bucket, all-reduced before the optimizer step
            bf16: run forward / backward in bf16 storage mode (Lightning ``precision="bf16-mixed"``)
        """
        self.model, self.preproc, self.flat, self.bf16 = model, preproc, flat, bool(bf16)
        self._optimizer_fn, self._optimizer = optimizer, None
        self._scheduler_fn, self.scheduler = scheduler, None

    # -- base.py:94-104
    def forward(self, data, _preprocessed: bool = False):
        if not _preprocessed:
            data = self.data_preproc(data)
        return self.model(data)

    __call__ = forward

    def data_preproc(self, data):
        if self.preproc is not None:
            return self.preproc(data)
        return data

    def parameters(self):
        seen = set()
        for m in (self.model, self.preproc):
            if m is None:
                continue
            for p in m.parameters():
                if p.requires_grad and id(p) not in seen:
                    seen.add(id(p))
                    yield p

    # -- base.py:106-112
    def configure_optimizers(self) -> torch.optim.Optimizer:
        if self._optimizer is None:
            params = [self.flat.flat_param] if self.flat is not None else list(self.parameters())
            self._optimizer = self._optimizer_fn(params)
            if self._scheduler_fn is not None:
                self.scheduler = self._scheduler_fn(self._optimizer)
        return self._optimizer

    def get_losses(self, out: dict[str, Any], data):
        raise NotImplementedError

    @staticmethod
    def _loss_metrics(losses) -> dict[str, float]:
        """The metric dict of a ``MultiLossFct`` result (the float conversions synchronise with the device)."""
        m = dict(losses.loss_dct)
        m.update({k + "_weighted": float(v) for k, v in losses.weighted_losses.items()})
        m.update({k: float(v) for k, v in losses.extra_metrics.items()})
        m["total"] = float(losses.loss)
        return m

    def _scanned_validation_step(self, data, scanner, scan, last_batch: bool) -> dict[str, float]:
        """The validation step of ``TCModule`` / ``MLModule``: the losses' metrics, ``scan(data, out)`` if there
        is a ``scanner`` and, on the last batch, its figures of merit."""
        with torch.no_grad(), bf16_storage(self.bf16):
            data = self.data_preproc(data)
            out = self(data, _preprocessed=True)
            _, metrics = self.get_losses(out, data, metrics=True)
            if scanner is not None:
                scan(data, out)
                if last_batch:
                    metrics |= scanner.get_foms()
        return metrics

    def _loss(self, data) -> Tensor:
        r = self.training_step(data, 0)
        return r[0] if isinstance(r, tuple) else r

    def zero_grad(self) -> None:
        if self.flat is not None:
            self.flat.zero_grad()
        else:
            self.configure_optimizers().zero_grad(set_to_none=False)

    def backward_step(self, data, *, scale: float = 1.0) -> Tensor:
        """forward + loss + backward of one (micro-)batch; gradients ACCUMULATE."""
        with bf16_storage(self.bf16):
            # forward, loss and backward in one call and nobody in between: the edge classifier's head and its BCE
            # loss may run inside the head's backward launch (ops.head_loss_deferral) - the loss VALUE then exists
            # after the backward, and `scale` travels to the launch as a host constant
            with ops.head_loss_deferral(scale, enabled=self._may_defer_head_loss()) as deferral:
                loss = self._loss(data)
            fused = deferral is not None and deferral.loss is not None
            if fused and deferral.loss is not loss:
                raise RuntimeError("backward_step: the deferred head loss was wrapped before the backward")
            # (a plain backward of this module's own loss: parameters re-homed by dist.FlatParameters may
            #  take their gradients in place from the backward launches, see ops.grad_sinks_armed)
            with ops.grad_sinks_armed():
                (loss if scale == 1.0 or fused else loss * scale).backward()
        return loss.detach()

    def _may_defer_head_loss(self) -> bool:
        """Nothing of this module looks at the loss value or at ``W`` between ``training_step`` and the backward."""
        return False

    def optimisation_step(self, data) -> Tensor:
        """What one ``Trainer`` iteration does to the parameters (automatic optimisation):
        zero the gradients, ``training_step``, backward, (all-reduce,) optimizer step."""
        opt = self.configure_optimizers()
        self.zero_grad()
        loss = self.backward_step(data)
        if self.flat is not None:
            self.flat.all_reduce_grads()
        opt.step()
        return loss


class ECModule(TrackingModule):
    """Edge-classifier training and validation (``training/ec.py:25-87``)."""

    def __init__(self, model: nn.Module, *, loss_fct: nn.Module, **kwargs):
        super().__init__(model, **kwargs)
        self.loss_fct = loss_fct

    def get_losses(self, out: dict[str, Any], data) -> Tensor:
        # (the reference passes ``data.y.float()``; this package's losses also take the dataset's
        # 1-byte bool labels as they are and skip the conversion pass)
        y = data.y if data.y.dtype in (torch.bool, torch.uint8) else data.y.float()
        return self.loss_fct(w=out["W"], y=y, pt=data.pt, edge_index=data.edge_index)

    def training_step(self, batch, batch_idx: int = 0) -> Tensor:
        batch = self.data_preproc(batch)
        out = self(batch, _preprocessed=True)
        return self.get_losses(out, batch)

    def _may_defer_head_loss(self) -> bool:
        from .losses_ec import EdgeWeightBCELoss

        # (this class's own training_step / get_losses hand the loss of exactly that loss class straight back)
        cls = type(self)
        return (cls.training_step is ECModule.training_step and cls.get_losses is ECModule.get_losses
                and cls.forward is TrackingModule.forward and type(self.loss_fct) is EdgeWeightBCELoss)

    def validation_step(self, batch, batch_idx: int = 0) -> dict[str, float]:
        """``training/ec.py:55-84``: the loss (``total``) and, for the pt cuts 0, 0.5, 0.9 and 1.5, the ROC
        AUCs (full, 0.01 and 0.001 FPR) and the maximised binary-classification stats - what the reference
        logs, returned as one dict.  The metrics run on the device (``metrics.ec_validation_metrics``: W is
        not scattered into ``edge_index`` order) and the host reads them once.  ``train()`` / ``eval()``
        is the caller's business, as in Lightning's loop."""
        from .metrics import ec_validation_metrics

        with torch.no_grad(), bf16_storage(self.bf16):
            batch = self.data_preproc(batch)
            out = self(batch, _preprocessed=True)
            loss = self.get_losses(out, batch)
            metrics = ec_validation_metrics(out["W"], batch.y, batch.pt, batch.edge_index, total=loss)
        return metrics

    def highlight_metric(self, metric: str) -> bool:
        return metric in ["max_mcc_pt0.9", "total", "tpr_eq_tnr_pt0.9"]


class TCModule(TrackingModule):
    """Object-condensation training and validation (``training/tc.py:20-114``): ``loss_fct`` is a
    ``MultiLossFct`` (``CondensationLossRG`` / ``CondensationLossTiger``), ``cluster_scanner`` an
    optional ``postprocessing.ClusterScanner`` (``DBSCANHyperParamScanner``) run on every validation
    batch."""

    def __init__(self, model: nn.Module, *, loss_fct: nn.Module, cluster_scanner=None, **kwargs):
        super().__init__(model, **kwargs)
        self.loss_fct = loss_fct
        self.cluster_scanner = cluster_scanner

    def get_losses(self, out: dict[str, Any], data, *, metrics: bool = True):
        losses = self.loss_fct(x=out["H"], particle_id=data.particle_id, beta=out["B"], pt=data.pt,
                               reconstructable=data.reconstructable, eta=data.eta,
                               ec_hit_mask=out.get("ec_hit_mask"), batch=getattr(data, "batch", None),
                               true_edge_index=getattr(data, "true_edges", None))
        if not metrics:  # (the float conversions below synchronise with the device)
            return losses.loss, {}
        return losses.loss, self._loss_metrics(losses)

    def training_step(self, data, batch_idx: int = 0, *, metrics: bool = False):
        data = self.data_preproc(data)
        out = self(data, _preprocessed=True)
        return self.get_losses(out, data, metrics=metrics)

    def validation_step(self, data, batch_idx: int = 0, *, last_batch: bool = False) -> dict[str, float]:
        """``training/tc.py:86-105``: the losses and, on the last validation batch, the cluster
        scanner's figures of merit (``trk.*``, ``best_dbscan_*``) - what the reference logs, as one
        dict.  The scanner sees every batch (``batch_idx == 0`` resets it).  Without a Lightning
        trainer the caller says which batch is the last one (``last_batch``, the reference's
        ``is_last_val_batch``)."""
        return self._scanned_validation_step(data, self.cluster_scanner,
                                             lambda d, out: self.cluster_scanner(d, out, batch_idx), last_batch)

    def highlight_metric(self, metric: str) -> bool:
        return metric in ["attractive", "repulsive", "trk.lhc_pt0.9", "trk.perfect_pt0.9",
                          "trk.double_majority_pt0.9"]


class MLModule(TrackingModule):
    """Metric-learning training and validation (``training/ml.py:25-110``): ``model(data) -> {"H": ...}``
    (e.g. ``GraphConstructionFCNN``), ``loss_fct`` a ``GraphConstructionHingeEmbeddingLoss``,
    ``gc_scanner`` an optional ``k_scanner.GraphConstructionKNNScanner`` run on the latent space of every
    validation batch (k-scan and its figures of merit, on the device)."""

    def __init__(self, model: nn.Module, *, loss_fct: nn.Module, gc_scanner=None, **kwargs):
        super().__init__(model, **kwargs)
        self.loss_fct = loss_fct
        self.gc_scanner = gc_scanner

    def get_losses(self, out: dict[str, Any], data, *, metrics: bool = True):
        if not hasattr(data, "true_edge_index"):
            # (ml.py:44-47: the point-cloud data saved the true edges as edge_index)
            data.true_edge_index = data.edge_index
        losses = self.loss_fct(x=out["H"], particle_id=data.particle_id, batch=getattr(data, "batch", None),
                               true_edge_index=data.true_edge_index, pt=data.pt, eta=data.eta,
                               reconstructable=data.reconstructable)
        if not metrics:
            return losses.loss, {}
        return losses.loss, self._loss_metrics(losses)

    def training_step(self, batch, batch_idx: int = 0, *, metrics: bool = False):
        batch = self.data_preproc(batch)
        out = self(batch, _preprocessed=True)
        return self.get_losses(out, batch, metrics=metrics)

    def validation_step(self, batch, batch_idx: int = 0, *, last_batch: bool = False) -> dict[str, float]:
        """``training/ml.py:77-96``: the losses and, on the last validation batch, the k-scanner's figures
        of merit (``on_validation_epoch_end``) - what the reference logs, as one dict.  The scanner sees
        the latent space ``out["H"]`` of every batch (``batch_idx == 0`` resets it).  Without a Lightning
        trainer the caller says which batch is the last one (``last_batch``)."""
        return self._scanned_validation_step(batch, self.gc_scanner,
                                             lambda d, out: self.gc_scanner(d, batch_idx, latent=out["H"]), last_batch)

    def highlight_metric(self, metric: str) -> bool:
        return metric in ["n_edges_frac_segment50_95", "total", "attractive", "repulsive", "max_frac_segment50"]
