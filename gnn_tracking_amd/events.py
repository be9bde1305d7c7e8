"""The events of a collated batch: everything the package knows about them.

A collated batch of B events keeps its hits sorted by event (PyG's convention) and names the events either by ``ptr``
(int64 ``[B + 1]`` row offsets, ``ptr[e]:ptr[e + 1]`` are the rows of event ``e``) or by ``batch`` (the event id of every
hit, ascending).  Every batched C entry takes the offsets, so this module turns whatever a caller has into them:

* ``event_ptr`` - the offsets of a ``Data``-like object (its ``ptr``, else its sorted ``batch``) or of ``batch=`` /
  ``ptr=`` given directly; ``None`` for at most one event, which is the caller's cue for the single-event C entry.
* ``unsorted`` - whether a ``batch`` breaks the convention, as a flag on the device.  ``event_ptr`` reads it and raises
  (one host read); a caller that reads the device anyway passes ``who=None`` and folds the flag into its own read.
* ``event_sizes`` - the hits per event, with the offsets checked on the host (one read): they ascend from 0 to ``n``.

An empty event in the middle stays an event (``batch = [0, 0, 2, 2, 2]`` gives ``[0, 2, 2, 5]``), and offsets derived
from a ``batch`` that lost rows to a mask are those of the rows that are left.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

__all__ = ["event_ptr", "offsets_of", "unsorted", "require_sorted", "event_sizes"]


def offsets_of(batch: Tensor) -> Tensor:
    """int64 ``[max(batch) + 2]`` row offsets of the events of a sorted ``batch``, one event included; no host read"""
    counts = torch.bincount(batch.long())
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=batch.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr


def unsorted(batch: Tensor) -> Tensor:
    """a bool scalar where ``batch`` lies: true if an event id is smaller than the one before it; no host read"""
    b = batch.long()
    return (b[1:] < b[:-1]).any()


def require_sorted(batch: Tensor, who: str) -> None:
    """``unsorted`` read on the host (one read; none for fewer than two hits)"""
    if batch.numel() > 1 and bool(unsorted(batch)):
        raise ValueError(f"{who}: `batch` must be sorted (PyG convention)")


def event_ptr(data=None, *, batch=None, ptr=None, who: str | None = "event_ptr") -> Tensor | None:
    """int64 ``[B + 1]`` row offsets of the events of ``data`` (its ``ptr``, else its ``batch``) or of ``ptr`` / ``batch``
    given directly (``ptr`` wins; a tensor, an array or a list); ``None`` for at most one event.  Offsets that come from
    a ``batch`` cost one host read for its order, with ``who`` in front of the refusal - none with ``who=None``, which
    leaves ``unsorted(batch)`` to the caller.  A ``ptr`` is handed through as it is: ``event_sizes`` checks it."""
    if data is not None:
        ptr, batch = getattr(data, "ptr", None), getattr(data, "batch", None)
    if ptr is None:
        if batch is None:
            return None
        ptr = offsets_of(batch)
        if who is not None:
            require_sorted(batch, who)
    elif not torch.is_tensor(ptr):
        ptr = torch.as_tensor(np.asarray(ptr))
    return ptr.long() if ptr.numel() > 2 else None


def event_sizes(ptr, n: int, who: str, rule: str = "ptr must ascend from 0 to the number of hits") -> list[int] | None:
    """The hits per event of ``ptr`` (``[B + 1]`` row offsets: a tensor, an array or a list), checked on the host in one
    read: they ascend from 0 to ``n``, or ``ValueError(who: rule)``.  ``None`` for ``ptr=None``."""
    if ptr is None:
        return None
    host = torch.as_tensor(np.asarray(ptr) if not torch.is_tensor(ptr) else ptr).cpu().long()
    sizes = torch.diff(host).tolist()
    if host.numel() < 1 or int(host[0]) != 0 or int(host[-1]) != n or any(s < 0 for s in sizes):
        raise ValueError(f"{who}: {rule}")
    return sizes
