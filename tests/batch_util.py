"""Helpers shared by the ``*_batch_cases.py`` modules: the events of a collated batch as row offsets, and the exact
comparison of result dicts and record lists (``==`` or both NaN: there is no tolerance here)."""

from __future__ import annotations

import contextlib

import numpy as np
import torch


def starts_of(sizes):
    return [0, *np.cumsum(sizes).tolist()]


def ptr_of(sizes, device):
    return torch.tensor(starts_of(sizes), dtype=torch.int64, device=device)


def assert_same(got: dict, want: dict, what: str, ordered=True):
    assert (list(got) == list(want)) if ordered else (sorted(got) == sorted(want)), f"{what}: keys {list(got)}"
    for k, v in want.items():
        g = float(got[k])
        assert g == v or (g != g and v != v), f"{what}: {k} = {got[k]!r}, want {v!r}"


def records_equal(got, want, what, skip=()):
    """record by record ``assert_same``, without the columns of ``skip``"""
    assert len(got) == len(want), f"{what}: {len(got)} records, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = ({c: v for c, v in r.items() if c not in skip} for r in (g, w))
        assert_same(g, w, f"{what}: record {i}")


def one_event_ptrs(n):
    """every way to say "one event of n hits": today's call"""
    return (None, torch.tensor([0, n]), [0, n])


@contextlib.contextmanager
def counted_calls(names):
    """wraps the entries ``names`` of the bound library while the block runs: {entry: number of calls}"""
    from gnn_tracking_amd import _capi

    lib = _capi.load()
    calls = dict.fromkeys(names, 0)
    real = {name: getattr(lib, name) for name in names}

    def wrapper(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    for name in names:
        setattr(lib, name, wrapper(name))
    try:
        yield calls
    finally:
        for name in names:
            setattr(lib, name, real[name])
