"""``MLGraphConstruction`` on a collated batch of events (``MLGraphConstruction.per_event``), shared by
tests/test_mlgc_batch_emul.py (CPU emulator) and tests/test_mlgc_batch_gpu.py.  Integers and copied coordinates only:
everything is compared bit for bit with the three single-event results, node offsets added, concatenated."""

from __future__ import annotations

import torch

import gnn_tracking_amd as G
import oc_cases as C

HITS = (90, 257, 64)
KS = (3, 100)            # 100 exceeds what the 90- and the 64-hit event can give
RADII = (1.0, 1e3)       # the default radius; one that cuts nothing, so that k alone limits the neighbours


def _events(device):
    out = []
    for n in HITS:
        ev = C.make_event(n, 20, 3)
        out.append(G.Data(x=ev.x.to(device), particle_id=ev.pid.to(device), pt=ev.pt.to(device), eta=ev.eta.to(device),
                          reconstructable=ev.reco.to(device), edge_index=torch.zeros(2, 0, dtype=torch.long, device=device)))
    return out


def case_batch_equals_events(device, k, radius, ratio_of_false):
    gc = G.MLGraphConstruction(ml=None, embedding_slice=(0, 3), max_num_neighbors=k, max_radius=radius,
                               ratio_of_false=ratio_of_false)
    gc.train(ratio_of_false is not None)
    events = _events(device)
    alone = [gc(ev) for ev in events]
    got = gc(G.collate(events))
    offs = [0, HITS[0], HITS[0] + HITS[1]]
    want_ei = torch.cat([a.edge_index + o for a, o in zip(alone, offs)], dim=1)
    assert want_ei.shape[1] > 0 and all(a.edge_index.shape[1] > 0 for a in alone)
    what = f"k {k} radius {radius} ratio_of_false {ratio_of_false}"
    assert got.edge_index.shape == want_ei.shape, f"{what}: {got.edge_index.shape[1]} edges, the events alone have {want_ei.shape[1]}"
    assert torch.equal(got.edge_index, want_ei), what + ": edge_index"
    assert got.y.dtype == alone[0].y.dtype and torch.equal(got.y, torch.cat([a.y for a in alone])), what + ": y"
    assert torch.equal(got.edge_attr.view(torch.int32), torch.cat([a.edge_attr for a in alone]).view(torch.int32)), what + ": edge_attr"
    ptr = torch.tensor(offs + [sum(HITS)], device=got.ptr.device)
    assert torch.equal(got.ptr, ptr) and torch.equal(got.batch, torch.repeat_interleave(torch.arange(3, device=ptr.device), ptr[1:] - ptr[:-1]))
    ev_of = torch.bucketize(got.edge_index, ptr[1:], right=True)
    assert torch.equal(ev_of[0], ev_of[1]), what + ": an edge crosses events"
    if ratio_of_false is not None:
        for a in alone:
            assert int((a.y == 0).sum()) <= int(int(a.y.sum()) * ratio_of_false)
        # (the ratio cuts in some event, or the case shows nothing)
        assert any(int((a.y == 0).sum()) == int(int(a.y.sum()) * ratio_of_false) for a in alone)
    elif radius > 10 and k == 100:
        assert alone[2].edge_index.shape[1] == 64 * 63 and alone[0].edge_index.shape[1] == 90 * 89


def case_reference_mixing(device):
    """``per_event = False`` restores the reference's search over all hits: what the concatenated hits give as ONE
    event"""
    gc = G.MLGraphConstruction(ml=None, embedding_slice=(0, 3), max_num_neighbors=100, max_radius=1e3).eval()
    events = _events(device)
    batch = G.collate(events)
    one = G.collate(events)
    del one.ptr, one.batch
    old = G.MLGraphConstruction.per_event
    G.MLGraphConstruction.per_event = False
    try:
        mixed = gc(batch)
    finally:
        G.MLGraphConstruction.per_event = old
    want = gc(one)
    assert torch.equal(mixed.edge_index, want.edge_index) and torch.equal(mixed.y, want.y)
    assert mixed.edge_index.shape[1] == sum(HITS) * 100
