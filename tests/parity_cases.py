"""Parity cases shared by the emulator tests (CPU, kernel sources on the wave64
emulator) and the GPU tests (real MI355X through libgnntrk.so).  Each case builds the
package's modules on ``device``, runs them, and compares with the committed golden
vectors (generated from the reference itself by oracle/make_golden.py) and/or the CPU
oracle.  Tolerances: outputs 1e-5 absolute-relative (north_star), gradients 1e-4."""

from __future__ import annotations

import pathlib

import math

import contextlib

import numpy as np
import torch

import gnn_tracking_amd as G
from gnn_tracking_amd import _capi, ops
import ref_cpu as O

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
TOL_OUT = 1e-5
TOL_GRAD = 1e-4


def load(name):
    return np.load(GOLD / name)


def tt(a, device=None):
    t = torch.from_numpy(np.asarray(a))
    return t if device is None else t.to(device)


def assert_close(a, b, tol, what):
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.numel() == 0:
        return
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, f"{what}: max|diff| {err:.3e} > {tol:.0e} * {scale:.3g}"


def assert_rows_close(a, b, tol, what, flips_per_rows=20000):
    """``assert_close`` for row-wise gradients of bf16 MLPs at large row counts: a ReLU whose
    pre-activation lies within fp32 summation noise of zero is gated differently by kernel and
    oracle (they sum in different orders), which changes ONE row's gradient by a whole term.
    At most one such row per ``flips_per_rows`` rows may exceed the tolerance (none below that
    size); everything must be finite."""
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape and torch.isfinite(a).all(), what
    bad = ((a - b).abs() > tol * max(1.0, b.abs().max().item())).reshape(a.shape[0], -1).any(dim=1)
    allowed = a.shape[0] // flips_per_rows
    assert int(bad.sum()) <= allowed, (f"{what}: {int(bad.sum())} rows beyond {tol:.0e} (allowed {allowed}), "
                                       f"max|diff| {(a - b).abs().max().item():.3e}")


def load_params(module, z, prefix):
    sd = {k[len(prefix):]: tt(z[k]) for k in z.files if k.startswith(prefix)}
    missing = module.load_state_dict(sd, strict=True)
    return sd


# --------------------------------------------------------------------- cases
def _check_graph_index(gi, eic, N, tag):
    order = torch.argsort(eic[1], stable=True)
    assert torch.equal(gi.perm.cpu().long(), order), tag + ": perm is the stable target sort"
    assert torch.equal(gi.tgt.cpu().long(), eic[1][order]), tag
    assert torch.equal(gi.src.cpu().long(), eic[0][order]), tag
    cnt = torch.bincount(eic[1], minlength=N)
    rp = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    assert torch.equal(gi.rowptr_t.cpu().long(), rp), tag
    so = torch.argsort(gi.src.cpu().long(), stable=True)
    assert torch.equal(gi.spos.cpu().long(), so), tag + ": spos is the stable source sort"
    inv = torch.empty_like(so)
    inv[so] = torch.arange(so.numel())
    assert torch.equal(gi.spos_inv.cpu().long(), inv), tag + ": spos_inv inverts spos"
    cnt = torch.bincount(eic[0], minlength=N)
    rp = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    assert torch.equal(gi.rowptr_s.cpu().long(), rp), tag


def case_graph_index(device, big=False):
    """Both forms of the build (own two-level counting sort / library radix sort) against torch's
    stable argsort: uniform random lists, a collated batch (disjoint id ranges, shuffled inside an
    event), hub nodes and a dense multigraph (buckets beyond the LDS capacity: the tiled ranking),
    an unsorted list wider than a chunk's LDS window of buckets (global-atomic counters)."""
    g = np.random.default_rng(0)
    cases = [("tiny", g.integers(0, 1, size=(2, 0)), 1), ("one", g.integers(0, 5, size=(2, 1)), 5),
             ("small", g.integers(0, 50, size=(2, 300)), 50), ("uniform", g.integers(0, 1000, size=(2, 20000)), 1000)]
    # collated events: ids of event i in [off_i, off_i + n_i), edges of an event contiguous
    offs, parts = 0, []
    for n, e in ((700, 5000), (300, 2500), (1, 3), (900, 9000)):
        parts.append(g.integers(0, n, size=(2, e)) + offs)
        offs += n
    cases.append(("collated", np.concatenate(parts, axis=1), offs))
    hub = g.integers(0, 600, size=(2, 30000))
    hub[1, ::2] = 17           # half of the edges end in one node (15 000 > the LDS capacity)
    hub[0, 1::3] = 300
    cases.append(("hub", hub, 600))
    hub2 = g.integers(0, 600, size=(2, 14000))
    hub2[1, ::2] = 333          # a 7 000-edge hub: just over the LDS capacity (the run walk; "hub" above takes the
    cases.append(("hub_small", hub2, 600))   # per-run bitmaps in the emulator build, the walk on the GPU)
    cases.append(("dense", g.integers(0, 7, size=(2, 12000)), 7))
    # more than 1024 touched buckets per chunk: several window slots per thread in the split's scans
    cases.append(("spread", g.integers(0, 300_000, size=(2, 20000)), 300_000))
    if big:   # more buckets than a chunk's LDS window (8192 x 256 nodes), ids unsorted
        cases.append(("wide", g.integers(0, 3_000_000, size=(2, 400_000)), 3_000_000))
        # a 300 000-edge hub (as target and, for a third of the edges, as source) spread over 37 chunks of the edge
        # list: the hub ranking through the chunk runs of the bucket's region
        hb = g.integers(0, 5000, size=(2, 600_000))
        hb[1, ::2] = 1234
        hb[0, 1::3] = 77
        cases.append(("hub_big", hb, 5000))
    for tag, arr, N in cases:
        ei = tt(arr, device).long()
        eic = ei.cpu()
        for flags in (0, 1, 2):   # default choice / library sort / own sort forced
            gi = ops.graph_index(ei, N, cache=False, flags=flags)
            _check_graph_index(gi, eic, N, f"{tag} flags={flags}")


def case_node_order(device, n_hits=10_000, n_edges=100_000, modes=("f32", "bf16")):
    """Node renumbering (locality.py, gnntrk_node_order, gnntrk_graph_index_carry.node_rank):
    (1) the order itself against torch's stable sorts - events keep their id ranges, ties keep the old order;
    (2) the index built through ``node_rank`` == the index of the relabelled edge list, all three build forms;
    (3) the edge classifier's training step with the renumbering ON against the CPU oracle in the caller's
        numbering (W, embeddings, pt-falsified loss, gradients, parameters after Adam: the fp32 bars), and
        ON against OFF: forward outputs bit for bit (a row's result does not depend on its tile), gradients to
        summation order."""
    from gnn_tracking_amd import synthetic

    g = np.random.default_rng(3)
    sizes = (700, 1, 300, 2049)
    batch = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes)])
    N = int(batch.numel())
    x = torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32))
    x[::7, 1] = 0.25           # ties
    x[5, 1] = -0.0
    x[6, 1] = 0.0
    def image(v):   # the order-preserving integer image of a float (gnntrk_node_order)
        u = v.contiguous().view(torch.int32).long() & 0xffffffff
        return torch.where(u >> 31 == 1, u ^ 0xffffffff, u ^ 0x80000000)

    def levels(v, ev):   # the quantised key of the counting-sort form (include/gnntrk.h: gnntrk_node_order), fp32 step by step
        out = torch.zeros(v.numel(), dtype=torch.int64)
        for e in ev.unique().tolist():   # (lo / hi per event)
            m = ev == e
            w = v[m]
            fin = w[~torch.isnan(w)]
            lo, hi = (fin.min(), fin.max()) if fin.numel() else (torch.tensor(0.0), torch.tensor(0.0))
            scale = torch.tensor(65535.0) / (hi - lo) if hi > lo else torch.tensor(0.0)
            t = ((w - lo) * scale).clamp_min(0.0)
            out[m] = torch.where(torch.isnan(w) | (t >= 65535.0), torch.tensor(65535), t.to(torch.int64))
        return out

    # (the own counting-sort form with 1 .. 64 stated events - no batch = one event -, the radix forms otherwise)
    for b, col, n_ev in ((batch, 1, 0), (None, 2, 0), (batch, 1, len(sizes)), (batch, 2, 200), (batch, 1, 1000)):
        perm, rank = ops.node_order(x.to(device), col, None if b is None else b.to(device), n_ev)
        if b is None or 1 <= n_ev <= 64:
            q = levels(x[:, col], torch.zeros_like(batch) if b is None else b)
        else:
            ebits = 32 if n_ev <= 0 else max(0, (n_ev - 1).bit_length())
            q = image(x[:, col]) >> (ebits if ebits <= 8 else 0)   # (up to eight event bits: the key keeps its top 32 - b bits)
        o = torch.argsort(q, stable=True)
        if b is not None:
            o = o[torch.argsort(b[o], stable=True)]
        assert torch.equal(perm.cpu().long(), o), f"node_order: perm is the stable (event, key) sort (n_events {n_ev})"
        inv = torch.empty_like(o)
        inv[o] = torch.arange(N)
        assert torch.equal(rank.cpu().long(), inv), "node_order: rank inverts perm"
    # the counting-sort form: 5 events of 900 .. 7000 nodes (two empty ones in between), ties, a NaN, infinities apart
    sizes2 = (900, 0, 7000, 1, 1200, 0)
    batch2 = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes2)])
    x2 = torch.from_numpy(g.uniform(-1, 1, (int(batch2.numel()), 3)).astype(np.float32))
    x2[::11, 1] = 0.125
    x2[17, 1] = float("nan")
    x2[:, 0] = 0.75          # a constant key: every node of an event on ONE level (a bucket far beyond the LDS capacity)
    x2[900:2500, 0] = -3.0   # ... and two levels, 1 600 + 5 400 nodes (the latter beyond the 5 120 records a bucket holds in LDS), in the second event
    for b, col, n_ev in ((batch2, 1, len(sizes2)), (None, 2, 0), (batch2, 2, 64), (batch2, 0, len(sizes2)), (None, 0, 1)):
        perm, rank = ops.node_order(x2.to(device), col, None if b is None else b.to(device), n_ev)
        o = torch.argsort(levels(x2[:, col], torch.zeros_like(batch2) if b is None else b), stable=True)
        if b is not None:
            o = o[torch.argsort(b[o], stable=True)]
        assert torch.equal(perm.cpu().long(), o), f"node_order (counting sort): perm is the stable (event, level) sort (n_events {n_ev})"
        inv = torch.empty_like(o)
        inv[o] = torch.arange(o.numel())
        assert torch.equal(rank.cpu().long(), inv), "node_order (counting sort): rank inverts perm"
    if device != "cpu":   # the headline's size: 32 events x 150 000 hits, azimuth-like keys (fp32 uniform: many shared levels)
        nb, ne = 150_000, 32
        xb = torch.from_numpy(g.uniform(-1, 1, (nb * ne, 2)).astype(np.float32))
        bb = torch.arange(ne).repeat_interleave(nb)
        perm, rank = ops.node_order(xb.to(device), 1, bb.to(device), ne)
        o = torch.argsort(levels(xb[:, 1], bb), stable=True)
        o = o[torch.argsort(bb[o], stable=True)]
        assert torch.equal(perm.cpu().long(), o), "node_order (counting sort, 4.8 M nodes): perm is the stable (event, level) sort"
        assert torch.equal(rank.cpu().long()[o], torch.arange(nb * ne)), "node_order (4.8 M nodes): rank inverts perm"
    offs, parts = 0, []
    for n in sizes:
        parts.append(g.integers(0, n, size=(2, 9 * n + 3)) + offs)
        offs += n
    eic = torch.from_numpy(np.concatenate(parts, axis=1)).long()
    xd, bd, ei = x.to(device), batch.to(device), eic.to(device)
    for flags in (0, 1, 2):
        gi = ops.graph_index(ei, N, cache=False, flags=flags, order_by=(xd, 1, bd))
        _check_graph_index(gi, gi.node_rank.cpu().long()[eic], N, f"node order flags={flags}")
        assert torch.equal(gi.node_perm.cpu().long()[gi.node_rank.cpu().long()], torch.arange(N))

    ev = synthetic.make_event(1, n_hits, n_edges, "cpu")
    d = ev.to(device)
    torch.manual_seed(0)
    model0 = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40)
    params = {k: v.detach().clone() for k, v in model0.state_dict().items()}
    ref, rloss, rgrads, rafter = O.ec_training_step(ev.x, ev.edge_index, ev.edge_attr, ev.y, params,
                                                    model_kwargs=dict(L_ec=3), pt=ev.pt, pt_thld=0.9)
    for mode in modes:
        runs = {}
        for order in ("off", 1):
            model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40)
            model.load_state_dict(params)
            model = model.to(device)
            ops.clear_graph_index_cache()
            with G.node_order(order), (G.bf16_storage() if mode == "bf16" else contextlib.nullcontext()):
                out = model(d)
                assert (ops.graph_index(d.edge_index, d.x.shape[0], order_by=(d.x, 1, None)).node_perm is not None) if order == 1 else True
                loss = G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=d.y, pt=d.pt, edge_index=d.edge_index)
                loss.backward()
            runs[order] = (torch.as_tensor(out["W"]).detach().float().cpu(), out["node_embedding"].detach().float().cpu(),
                           torch.as_tensor(out["edge_embedding"]).detach().float().cpu(), loss.detach().cpu(),
                           {k: v.grad.detach().cpu() for k, v in model.named_parameters()}, model)
        tag = f"node order {mode}"
        for i, nm in enumerate(("W", "node_embedding", "edge_embedding")):
            assert torch.equal(runs["off"][i], runs[1][i]), f"{tag}: {nm} differs between the numberings"
        # the loader-side form (io.renumber_nodes: the event renumbered ONCE, on the host, when it is read): the step
        # then does not renumber again, per-edge outputs are the original event's bit for bit, per-node outputs are
        # its rows in the new order
        from gnn_tracking_amd import io as gio
        ev2 = gio.renumber_nodes(ev)
        assert torch.equal(ev2.x[:, 1], ev.x[:, 1][ev2.node_perm]) and bool((ev2.x[1:, 1] >= ev2.x[:-1, 1]).all())
        assert torch.equal(ev2.node_perm[ev2.edge_index], ev.edge_index)
        d2 = G.collate([ev2]).to(device)
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40)
        model.load_state_dict(params)
        model = model.to(device)
        ops.clear_graph_index_cache()
        with G.node_order(1), (G.bf16_storage() if mode == "bf16" else contextlib.nullcontext()):
            out2 = model(d2)
            gi2 = ops.graph_index(d2.edge_index, d2.x.shape[0])
        assert gi2.node_perm is None, tag + ": an event ordered by the loader was renumbered again"
        assert torch.equal(torch.as_tensor(out2["W"]).detach().float().cpu(), runs["off"][0]), tag + " loader-ordered W"
        assert torch.equal(out2["node_embedding"].detach().float().cpu(), runs["off"][1][ev2.node_perm]), tag + " loader-ordered nodes"
        if mode == "f32":
            W, hn, en, loss, grads, model = runs[1]
            assert_close(W, ref["W"], TOL_OUT, tag + " W")
            assert_close(hn, ref["node_embedding"], TOL_OUT, tag + " node_embedding")
            assert_close(en, ref["edge_embedding"], TOL_OUT, tag + " edge_embedding")
            assert_close(loss, rloss, TOL_OUT, tag + " loss")
            for k, v in grads.items():
                assert_close(v, rgrads[k], TOL_GRAD, f"{tag} grad {k}")
            torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4).step()
            for k, v in model.state_dict().items():
                assert_close(v, rafter[k], 1e-6, f"{tag} after Adam {k}")
        else:
            assert abs(float(runs["off"][3]) - float(runs[1][3])) <= 1e-6, tag + " loss"
            for k in runs[1][4]:
                a, b = runs["off"][4][k], runs[1][4][k]
                assert (a - b).norm() <= 2e-2 * max(float(a.norm()), 1e-6) + 2e-3 * max(float(torch.cat([v.flatten() for v in runs["off"][4].values()]).norm()), 1e-6), f"{tag} grad {k}"


def case_graph_index_place(device, sizes=((700, 6301), (1, 3), (300, 2500), (2049, 18002), (64, 0)), order=True):
    """Cached per-event indices placed into a collated batch (gnntrk_graph_index_place, ops.place_graph_indices)
    against the index BUILT from the collated edge list: every array bit for bit - permutations, row pointers, the
    carried labels / edge features, the node order -, with edge offsets off the 16-byte grid, an event without edges
    and a one-node event; and the edge classifier finds the placed index (no second build) and returns the same W."""
    from gnn_tracking_amd import synthetic

    g = np.random.default_rng(5)
    events = []
    for i, (n, e) in enumerate(sizes):
        ev = G.Data(x=torch.from_numpy(g.standard_normal((n, 14)).astype(np.float32)),
                    edge_index=torch.from_numpy(g.integers(0, n, size=(2, e))).long(),
                    edge_attr=torch.from_numpy(g.standard_normal((e, 4)).astype(np.float32)),
                    y=torch.from_numpy(g.integers(0, 2, size=e).astype(bool)),
                    pt=torch.from_numpy(g.random(n).astype(np.float32)))
        events.append(ev.to(device))
    col = 1 if order else None
    parts = [ops.graph_index(ev.edge_index, ev.num_nodes, cache=False, carry_label=ev.y, carry_rows=ev.edge_attr,
                             order_by=None if col is None else (ev.x, col, None)) for ev in events]
    b = G.collate(events)
    ops.clear_graph_index_cache()
    gi = ops.place_graph_indices(parts, b)
    ref = ops.graph_index(b.edge_index, b.num_nodes, cache=False, carry_label=b.y, carry_rows=b.edge_attr,
                          order_by=None if col is None else (b.x, col, b.batch, len(sizes)))   # (event count stated, as the model does)
    for k in ("perm", "tgt", "src", "rowptr_t", "rowptr_s", "spos", "spos_inv") + (("node_perm", "node_rank") if order else ()):
        assert torch.equal(getattr(gi, k), getattr(ref, k)), f"placed index: {k} differs from the built one"
    assert torch.equal(ops.carried_label(gi, b.y), ops.carried_label(ref, b.y)), "placed index: carried labels"
    assert torch.equal(ops.carried_rows(gi, b.edge_attr).view(torch.int16), ops.carried_rows(ref, b.edge_attr).view(torch.int16))
    # the model takes the placed index from the cache (same object) and computes the same weights as on a built one
    torch.manual_seed(0)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=2, hidden_dim=40).to(device)
    with G.node_order(col if order else "off", min_nodes=0), G.bf16_storage():
        w1 = torch.as_tensor(model(b)["W"]).detach().float().cpu()
        hit = ops.graph_index(b.edge_index, b.num_nodes, order_by=None if col is None else (b.x, col, b.batch))
        assert hit is gi, "the edge classifier did not take the placed index"
        ops.clear_graph_index_cache()
        w2 = torch.as_tensor(model(b)["W"]).detach().float().cpu()
    assert torch.equal(w1, w2), "W on the placed index differs from W on the built index"


def case_resident_dataset(device, sizes=((700, 6301), (300, 2500), (1, 0), (2049, 18002), (1000, 9000), (50, 333))):
    """io.ResidentDataset: a static dataset on the device with one index per event; ``batches`` collates and PLACES.
    Against the same events collated and indexed inline: (1) every index array of every batch bit for bit,
    (2) one optimisation step per batch (bf16 storage and fp32): loss, W and the flat gradient bucket identical -
    the node-order policy says "off" for batches this small, the loader orders anyway (paid once) and the model takes
    the loader's index; (3) a second epoch reuses the per-event indices (no new build) in a new shuffle.  One event is a
    single hit without edges: the loader leaves it unordered and the placement gives it the identity order."""
    from gnn_tracking_amd import dist as gdist, io as gio, training

    g = np.random.default_rng(11)
    events = []
    for n, e in sizes:
        events.append(G.Data(x=torch.from_numpy(g.standard_normal((n, 14)).astype(np.float32)),
                             edge_index=torch.from_numpy(g.integers(0, n, size=(2, e))).long(),
                             edge_attr=torch.from_numpy(g.standard_normal((e, 4)).astype(np.float32)),
                             y=torch.from_numpy(g.integers(0, 2, size=e).astype(bool)),
                             pt=torch.from_numpy(g.random(n).astype(np.float32))))
    for bf16 in (True, False):
        ds = gio.ResidentDataset(events, device, bf16=bf16)
        assert len(ds) == len(events)
        seen = []
        for epoch in range(2):
            for b in ds.batches(2, shuffle=True, seed=epoch):
                gi = ops.placed_graph_index(b.edge_index, b.num_nodes)
                assert gi is not None and gi.node_perm is not None, "ResidentDataset: no placed, ordered index"
                ref = ops.graph_index(b.edge_index, b.num_nodes, cache=False, carry_label=b.y,
                                      carry_rows=b.edge_attr if bf16 else None,
                                      order_by=(b.x, 1, b.batch, int(b.ptr.numel()) - 1))   # (event count stated, as the model does)
                for k in ("perm", "tgt", "src", "rowptr_t", "rowptr_s", "spos", "spos_inv", "node_perm", "node_rank"):
                    assert torch.equal(getattr(gi, k), getattr(ref, k)), f"resident batch: {k} differs from the inline build"
                if b.num_edges:   # (a batch of nothing but the single-hit event carries nothing)
                    assert torch.equal(ops.carried_label(gi, b.y), ops.carried_label(ref, b.y))
                seen.append(int(b.num_edges))
        assert sum(seen) == 2 * sum(e for _, e in sizes), "every event once per epoch"
        parts = [ds.event(i)[1] for i in range(len(ds))]
        assert all(p is ds.event(i)[1] for i, p in enumerate(parts)), "per-event indices are kept"

        def run(resident: bool):
            torch.manual_seed(0)
            model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=2, hidden_dim=40).to(device)
            flat = gdist.FlatParameters(model)
            mod = training.ECModule(model, loss_fct=G.EdgeWeightBCELoss(), flat=flat, bf16=bf16, scheduler=None,
                                    optimizer=lambda p: torch.optim.SGD(p, lr=0.0))
            out = []
            for b in ds.batches(3, shuffle=True, seed=7):
                if not resident:   # the same events collated and indexed inside the step, renumbered there
                    ops.clear_graph_index_cache()
                with G.node_order("auto" if resident else 1, min_nodes=None if resident else 0):
                    loss = mod.optimisation_step(b)
                out.append((float(loss), flat.grad.detach().clone().cpu()))
            return out

        a, c = run(True), run(False)
        for (la, ga), (lc, gc) in zip(a, c):
            assert la == lc and torch.equal(ga, gc), "ResidentDataset step differs from the inline step"


def case_graph_index_carry(device):
    """Per-edge inputs carried into CSR order inside the build (gnntrk_graph_index_carry): identical to
    the gathers through perm, in both forms of the build, incl. buckets beyond the LDS capacity; and
    the fused CSR BCE (loss + unit gradient in one pass) against torch's BCE on the gathered labels."""
    from gnn_tracking_amd import ops_bf16
    g = np.random.default_rng(1)
    cases = [("small", g.integers(0, 50, size=(2, 300)), 50), ("uniform", g.integers(0, 1000, size=(2, 20000)), 1000)]
    hub = g.integers(0, 600, size=(2, 30000))
    hub[1, ::2] = 17
    cases.append(("hub", hub, 600))
    cases.append(("dense", g.integers(0, 7, size=(2, 12000)), 7))
    for tag, arr, N in cases:
        ei = tt(arr, device).long()
        E = ei.shape[1]
        y = tt(g.random(E) < 0.3, device)
        rows = tt(g.normal(size=(E, 4)).astype(np.float32) * 3, device)
        pt = tt(g.lognormal(size=N).astype(np.float32), device)
        for flags in (0, 1, 2):
            gi = ops.graph_index(ei, N, cache=False, flags=flags, carry_label=y, carry_rows=rows)
            _check_graph_index(gi, ei.cpu(), N, f"{tag} carry flags={flags}")
            lab, rc = ops.carried_label(gi, y), ops.carried_rows(gi, rows)
            assert lab is not None and rc is not None
            perm = gi.perm.long()
            assert torch.equal(lab.cpu(), y[perm].to(torch.uint8).cpu()), f"{tag} flags={flags}: carried labels"
            want = ops_bf16.to_rows16(rows, gi.perm)
            assert torch.equal(rc.cpu().view(torch.int16), want.cpu().view(torch.int16)), f"{tag} flags={flags}: carried rows"
            assert ops.carried_label(gi, y.clone()) is None, "another tensor must not match"
        # fused BCE on CSR-ordered weights
        for thld in (0.0, 0.9):
            w = tt(g.uniform(0.001, 0.999, size=E).astype(np.float32), device).requires_grad_(True)
            loss = ops._BCECsr.apply(w, lab, gi.src if thld > 0 else None, pt if thld > 0 else None, thld)
            (loss * 1.5).backward()
            wr = w.detach().clone().requires_grad_(True)
            t = y[perm].float()
            if thld > 0:
                t = t * (pt[gi.src.long()] > thld).float()
            ref = torch.nn.functional.binary_cross_entropy(wr, t)
            (ref * 1.5).backward()
            assert_close(loss, ref, 1e-6, f"{tag} fused BCE thld={thld}")
            assert_close(w.grad, wr.grad, 1e-6, f"{tag} fused BCE gradient thld={thld}")


def case_mlp(device, shapes=((14, 40, 4, 3), (9, 40, 5, 3), (14, 14, 5, 2), (26, 40, 1, 3),
                             (4, 2, 4, 2), (30, 33, 7, 3), (48, 64, 16, 3), (28, 40, 4, 2), (5, 40, 1, 3), (5, 40, 8, 3)), rows=77):
    torch.manual_seed(0)
    for (i, h, o, L) in shapes:
        for bias in (True, False):
            m = G.MLP(i, o, h, L=L, bias=bias)
            x = torch.randn(rows, i)
            r = torch.randn(rows, o)
            p = {"m." + k: v.detach().clone().requires_grad_(True)
                 for k, v in m.state_dict().items()}
            xo = x.clone().requires_grad_(True)
            yo = O.mlp(xo, p, "m", L, bias=bias)
            (yo * r).sum().backward()
            m = m.to(device)
            xd = x.to(device).requires_grad_(True)
            y = m(xd)
            (y * r.to(device)).sum().backward()
            tag = f"MLP {i}->{h}->{o} L={L} bias={bias}"
            assert_close(y, yo, TOL_OUT, tag + " y")
            assert_close(xd.grad, xo.grad, TOL_GRAD, tag + " gx")
            for k, v in m.named_parameters():
                assert_close(v.grad, p["m." + k].grad, TOL_GRAD, f"{tag} g {k}")


def case_in_layer(device, which=("std", "odd")):
    z = load("g3_in_layer.npz")
    for name in which:
        dn, de, dno, deo, hn, he = [int(v) for v in z[f"{name}/dims"]]
        m = G.InteractionNetwork(node_indim=dn, edge_indim=de, node_outdim=dno, edge_outdim=deo,
                                 node_hidden_dim=hn, edge_hidden_dim=he)
        load_params(m, z, f"{name}/p0/in.")
        m = m.to(device)
        x = tt(z[f"{name}/x"], device).requires_grad_(True)
        ea = tt(z[f"{name}/edge_attr"], device).requires_grad_(True)
        ei = tt(z[f"{name}/edge_index"], device)
        xt, et = m(x, ei, ea)
        assert_close(xt, z[f"{name}/x_tilde"], TOL_OUT, name + " x~")
        assert_close(et, z[f"{name}/e_tilde"], TOL_OUT, name + " e~")
        ((xt * tt(z[f"{name}/rx"], device)).sum() + (et * tt(z[f"{name}/re"], device)).sum()).backward()
        assert_close(x.grad, z[f"{name}/grad_x"], TOL_GRAD, name + " grad x")
        assert_close(ea.grad, z[f"{name}/grad_edge_attr"], TOL_GRAD, name + " grad edge_attr")
        for k, v in m.named_parameters():
            assert_close(v.grad, z[f"{name}/grad/in.{k}"], TOL_GRAD, f"{name} grad {k}")


def case_resin(device):
    z = load("g3b_resin.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    for name, kw in {
        "skip1": dict(n_layers=3, residual_type="skip1", alpha=0.5),
        "skip2": dict(n_layers=2, residual_type="skip2", alpha=0.3),
        "skip_top": dict(n_layers=3, residual_type="skip_top", alpha=0.7),
        "skip2_bn": dict(n_layers=2, residual_type="skip2", alpha=0.3, add_bn=True),
    }.items():
        kw = dict(kw)
        rk = {"collect_hidden_edge_embeds": True, **({"add_bn": True} if kw.pop("add_bn", False) else {})}
        m = G.ResIN(node_dim=5, edge_dim=4, object_hidden_dim=12, relational_hidden_dim=20,
                    residual_kwargs=rk, **kw)
        load_params(m, z, f"{name}/p0/r.")
        m = m.to(device)
        xo, eo, es = m(x, ei, ea)
        assert_close(xo, z[f"{name}/x_out"], TOL_OUT, name + " x")
        assert_close(eo, z[f"{name}/e_out"], TOL_OUT, name + " e")
        assert_close(torch.cat(es, 1), z[f"{name}/edge_attrs_cat"], TOL_OUT, name + " edge_attrs")


def case_ec_testgraph(device):
    """Row H of SURVEY.md section 8a: ECForGraphTCN(14,14,L_ec=1) on the reference's
    test graph: init == reference init under manual_seed(0), forward, BCE, grads, and
    the parameters after one Adam(lr=1e-4, weight_decay=1e-4) step."""
    z = load("g1_ec_testgraph.npz")
    torch.manual_seed(0)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=14, L_ec=1)
    for k, v in model.state_dict().items():
        assert torch.equal(v, tt(z["p0/" + k])), f"initial parameter {k} differs from reference"
    model = model.to(device)
    data = G.Data(x=tt(z["x"], device), edge_index=tt(z["edge_index"], device),
                  edge_attr=tt(z["edge_attr"], device), y=tt(z["y"], device), pt=tt(z["pt"], device))
    out = model(data)
    assert_close(out["W"], z["W"], TOL_OUT, "W")
    assert_close(out["node_embedding"], z["node_embedding"], TOL_OUT, "node_embedding")
    assert_close(out["edge_embedding"], z["edge_embedding"], TOL_OUT, "edge_embedding")
    loss = G.EdgeWeightBCELoss()(w=out["W"], y=data.y.float(), pt=data.pt,
                                 edge_index=data.edge_index)
    assert_close(loss, z["loss"], TOL_OUT, "BCE loss")
    loss.backward()
    for k, v in model.named_parameters():
        assert_close(v.grad, z["grad/" + k], TOL_GRAD, "grad " + k)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.step()
    for k, v in model.state_dict().items():
        assert_close(v, z["p1/" + k], 1e-6, "after Adam " + k)


EC_VARIANTS = {
    "skip1_L3_h40": dict(L_ec=3, hidden_dim=40),
    "skip1_L2_h2": dict(L_ec=2, hidden_dim=2),
    "skip2_L2": dict(L_ec=2, hidden_dim=8, residual_type="skip2"),
    "skiptop_L3": dict(L_ec=3, hidden_dim=8, residual_type="skip_top"),
    "no_inter": dict(L_ec=2, hidden_dim=8, use_intermediate_edge_embeddings=False),
    "no_inter_no_node": dict(L_ec=2, hidden_dim=8, use_intermediate_edge_embeddings=False,
                             use_node_embedding=False),
    "no_node": dict(L_ec=2, hidden_dim=8, use_node_embedding=False),
    "alpha0": dict(L_ec=2, hidden_dim=None, alpha=0.0),
    # hidden width 64: the widest the fp32 kernels hold; five hidden tiles (64 + the bias row) in bf16 storage
    "h64": dict(L_ec=2, hidden_dim=64),
    # hidden width 128: eight hidden tiles in bf16 storage (biases as accumulator initial values); library GEMMs in fp32
    "h128": dict(L_ec=1, hidden_dim=128),
    # widths beyond the fused kernels (hidden 128, 20-wide node / edge spaces): library-GEMM path
    "wide_h128": dict(L_ec=1, hidden_dim=128, interaction_node_dim=20, interaction_edge_dim=20),
}


def case_ec_variants(device, names=None):
    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, pt = tt(z["y"], device), tt(z["pt"], device)
    for name, kw in EC_VARIANTS.items():
        if names is not None and name not in names:
            continue
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **kw)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        out = model(G.Data(x=x, edge_index=ei, edge_attr=ea))
        assert_close(out["W"], z[f"{name}/W"], TOL_OUT, name + " W")
        assert_close(out["node_embedding"], z[f"{name}/node_embedding"], TOL_OUT, name + " node")
        assert_close(out["edge_embedding"], z[f"{name}/edge_embedding"], TOL_OUT, name + " edge")
        loss = G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=y.float(), pt=pt, edge_index=ei)
        assert_close(loss, z[f"{name}/loss"], TOL_OUT, name + " loss")
        loss.backward()
        for k, v in model.named_parameters():
            gk = v.grad if v.grad is not None else torch.zeros_like(v)
            assert_close(gk, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")


def case_edge_cases(device, modes=("f32",)):
    """Empty / ragged inputs: ZERO edges (an ``ec_threshold`` cut or a radius cut can leave
    none; the reference runs through), one edge, isolated nodes only, a tile-size multiple and
    +-1 row around it; forward and all parameter gradients."""
    torch.manual_seed(3)
    model = G.ECForGraphTCN(node_indim=6, edge_indim=3, L_ec=2, hidden_dim=8)
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(device)
    g = np.random.default_rng(9)
    for N, E in ((7, 0), (7, 1), (7, 2), (40, 15), (40, 16), (40, 17), (3, 64), (100, 63)):
        x = tt(g.normal(size=(N, 6)).astype(np.float32))
        ea = tt(g.normal(size=(E, 3)).astype(np.float32))
        ei = tt(g.integers(0, N, size=(2, E))).long()
        rn, rw = tt(g.normal(size=(N, 5)).astype(np.float32)), tt(g.normal(size=(E,)).astype(np.float32))
        ps = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        ref = O.ec_for_graph_tcn(x, ei, ea, ps, L_ec=2)
        rl = (ref["node_embedding"] * rn).sum() + (ref["W"].reshape(-1) * rw).sum()
        rg = torch.autograd.grad(rl, list(ps.values()), allow_unused=True)
        for mode in modes:
            model.zero_grad()
            d = G.Data(x=x.to(device), edge_index=ei.to(device), edge_attr=ea.to(device))
            if mode == "bf16":
                with G.bf16_storage():
                    out = model(d)
            else:
                out = model(d)
            tol_o, tol_g = (TOL_OUT, TOL_GRAD) if mode == "f32" else (0.05, 0.1)
            tag = f"N={N} E={E} {mode}"
            assert out["W"].reshape(-1).shape == (E,) and out["edge_embedding"].shape == (E, 4)
            assert_close(out["W"].reshape(-1), ref["W"].reshape(-1), tol_o, tag + " W")
            assert_close(out["node_embedding"].float(), ref["node_embedding"], tol_o, tag + " node")
            assert_close(out["edge_embedding"].float(), ref["edge_embedding"], tol_o, tag + " edge")
            loss = (out["node_embedding"].float() * rn.to(device)).sum() + (out["W"].reshape(-1) * rw.to(device)).sum()
            loss.backward()
            want_all = math.sqrt(sum(float(gk.double().pow(2).sum()) for gk in rg if gk is not None))
            err_all = 0.0
            for (k, v), gk in zip(model.named_parameters(), rg):
                got = v.grad if v.grad is not None else torch.zeros_like(v)
                want = gk if gk is not None else torch.zeros_like(v)
                assert torch.isfinite(got).all(), f"{tag} grad {k} not finite"
                if mode == "f32" or E == 0:
                    assert_close(got, want, tol_g, f"{tag} grad {k}")
                else:
                    # bf16 storage against the fp32 oracle.  On a handful of rows a single ReLU gate that
                    # rounds to the other side moves a small parameter gradient by tens of per cent, so
                    # the bound per parameter is relative to its own norm PLUS half a per cent of the
                    # whole gradient's; the whole gradient must agree to 5 % (measured: about 1 %).
                    wn = want.double().norm().item()
                    err = (got.detach().cpu().double() - want.double()).norm().item()
                    err_all += err * err
                    assert err <= 0.1 * wn + 0.005 * want_all + 1e-4, f"{tag} grad {k}: L2 error {err:.3e} of {wn:.3e}"
            assert math.sqrt(err_all) <= 0.05 * want_all + 1e-4, f"{tag}: gradient L2 error {math.sqrt(err_all):.3e} of {want_all:.3e}"


# ----------------------------------------------------------------- kNN / graphs
def case_knn_goldens(device, clouds=("tg3", "u2", "u8")):
    """knn_with_max_radius against the edge lists the reference produced (G4), bit-exact."""
    from gnn_tracking_amd.graph_construction import knn_with_max_radius

    z = load("g4_knn.npz")
    for cn in clouds:
        x = tt(z[f"{cn}/x"], device)
        for k in (1, 2, 3, 9):
            for r in (None, 1.0, 0.3):
                ei = knn_with_max_radius(x, k=k, max_radius=r)
                ref = tt(z[f"{cn}/k{k}_r{r}"])
                assert ei.dtype == torch.int64
                assert torch.equal(ei.cpu(), ref), f"kNN {cn} k={k} r={r} differs from reference"
        # the k-scan: ONE search at k = 9 reproduces the reference's per-k searches
        from gnn_tracking_amd.graph_construction import knn_scan
        for r in (None, 1.0, 0.3):
            scan = knn_scan(x, (1, 2, 3, 9), max_radius=r)
            for k in (1, 2, 3, 9):
                assert torch.equal(scan[k].cpu(), tt(z[f"{cn}/k{k}_r{r}"])), f"k-scan {cn} k={k} r={r}"


def case_knn_oracle(device, shapes=((300, 3, 4, None), (300, 8, 16, 0.9), (257, 2, 70, None),
                                    (130, 8, 3, 0.5), (65, 3, 100, 0.4), (1, 3, 4, None),
                                    (2, 3, 4, None))):
    """bit-exact against the C oracle incl. ties, k > n, buffer pruning and radius prefix."""
    g = np.random.default_rng(3)
    for (n, d, k, r) in shapes:
        x = tt(g.random((n, d)).astype(np.float32))
        ei = ops.knn_graph(x.to(device), k, r)
        ref = O.knn_graph_c(x, k, r) if n > 1 else torch.empty(2, 0, dtype=torch.int64)
        assert torch.equal(ei.cpu(), ref), f"kNN n={n} d={d} k={k} r={r}"
    x = tt(g.random((90, 4)).astype(np.float32))
    scan = ops.knn_scan(x.to(device), (1, 5, 200), 0.6)  # 200 > n - 1: clipped like a plain search
    for k in (1, 5, 200):
        assert torch.equal(scan[k].cpu(), O.knn_graph_c(x, k, 0.6)), f"k-scan k={k}"
    assert all(v.shape == (2, 0) for v in ops.knn_scan(x[:1].to(device), (1, 2)).values())
    x = torch.zeros(100, 3)
    x[50:] = 1.0  # massive ties: order must be by index
    assert torch.equal(ops.knn_graph(x.to(device), 5, None).cpu(), O.knn_graph_c(x, 5, None))


def case_ml_graph_construction(device):
    """MLGraphConstruction(ml=None, embedding_slice=(0,3)) vs the reference's output (G6)."""
    from gnn_tracking_amd.graph_construction import MLGraphConstruction

    z, g1 = load("g6_mlgc.npz"), load("g1_ec_testgraph.npz")
    for k, r in ((4, 1.0), (16, 0.5)):
        d = G.Data(x=tt(g1["x"], device), edge_index=tt(g1["edge_index"], device),
                   particle_id=tt(g1["particle_id"], device), pt=tt(g1["pt"], device),
                   eta=tt(g1["eta"], device), reconstructable=tt(g1["reconstructable"], device),
                   layer=tt(g1["layer"], device), sector=tt(g1["sector"], device))
        m = MLGraphConstruction(ml=None, embedding_slice=(0, 3), max_radius=r, max_num_neighbors=k)
        out = m(d)
        assert torch.equal(out.edge_index.cpu(), tt(z[f"k{k}_r{r}/edge_index"]))
        assert torch.equal(out.y.cpu(), tt(z[f"k{k}_r{r}/y"]))
        assert torch.equal(out.edge_attr.cpu(), tt(z[f"k{k}_r{r}/edge_attr"])), "edge features"
    # training mode with ``ratio_of_false``: the first int(n_true * ratio) false edges, then every true edge (G6, bit for bit);
    # in eval mode the ratio is ignored
    for k, r, rof in ((16, 0.5, 0.5), (4, 1.0, 2.0)):
        d = G.Data(x=tt(g1["x"], device), edge_index=tt(g1["edge_index"], device),
                   particle_id=tt(g1["particle_id"], device), pt=tt(g1["pt"], device),
                   eta=tt(g1["eta"], device), reconstructable=tt(g1["reconstructable"], device),
                   layer=tt(g1["layer"], device), sector=tt(g1["sector"], device))
        m = MLGraphConstruction(ml=None, embedding_slice=(0, 3), max_radius=r, max_num_neighbors=k, ratio_of_false=rof)
        m.train()
        out = m(d)
        tag = f"k{k}_r{r}_rof{rof}"
        assert torch.equal(out.edge_index.cpu(), tt(z[f"{tag}/edge_index"])), "ratio_of_false: edge list"
        assert torch.equal(out.y.cpu(), tt(z[f"{tag}/y"]).long()), "ratio_of_false: labels"
        assert torch.equal(out.edge_attr.cpu(), tt(z[f"{tag}/edge_attr"])), "ratio_of_false: edge features"
        m.eval()
        assert torch.equal(m(d).edge_index.cpu(), tt(z[f"k{k}_r{r}/edge_index"])), "ratio_of_false is a training-mode switch"
    # the edge features are differentiable w.r.t. the node features (graph_construction.py:386-393
    # is plain indexing + cat in the reference): gradient against torch autograd of that expression
    g = np.random.default_rng(4)
    x = tt(g.normal(size=(40, 5)).astype(np.float32))
    ei = tt(g.integers(0, 40, size=(2, 300))).long()
    r = tt(g.normal(size=(300, 10)).astype(np.float32))
    xo = x.clone().requires_grad_(True)
    (torch.cat([xo[ei[0]] - xo[ei[1]], xo[ei[0]] + xo[ei[1]]], dim=1) * r).sum().backward()
    xd = x.to(device).requires_grad_(True)
    f = ops.edge_features(xd, ei.to(device))
    (f * r.to(device)).sum().backward()
    assert_close(xd.grad, xo.grad, TOL_GRAD, "edge_features grad x")


# ------------------------------------------------------------ condensation losses
def case_condensation_losses(device, cases=("td1", "td2", "td3")):
    """CondensationLossRG / Tiger vs the reference (G5): the reference's pinned float64
    known-answer cases td1/td2 (tests/test_losses.py:112-123) are run here in fp32 and
    compared with the reference's own fp32 re-run, loss terms and gradients."""
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    z = load("g5_oc.npz")
    for cn in cases:
        t = {k: tt(z[f"{cn}/{k}"]) for k in ("beta", "x", "particle_id", "pt", "eta",
                                              "reconstructable")}
        if cn == "td3":
            pass  # x was already scaled when the golden was generated
        for strat, cls in (("tiger", CondensationLossTiger), ("rg", CondensationLossRG)):
            b = t["beta"].float().to(device).requires_grad_(True)
            x = t["x"].float().to(device).requires_grad_(True)
            ret = cls(lw_repulsive=2.0, lw_noise=0.5, lw_coward=0.25)(
                beta=b, x=x, particle_id=t["particle_id"].to(device),
                reconstructable=t["reconstructable"].float().to(device),
                pt=t["pt"].float().to(device), eta=t["eta"].float().to(device))
            for k in ("attractive", "repulsive", "coward", "noise"):
                assert_close(ret.loss_dct[k], z[f"{cn}/f32/{strat}/{k}"], TOL_OUT, f"{cn} {strat} {k}")
            assert_close(ret.loss, z[f"{cn}/f32/{strat}/total"], TOL_OUT, f"{cn} {strat} total")
            ret.loss.backward()
            assert_close(x.grad, z[f"{cn}/f32/{strat}/grad_x"], 2e-4, f"{cn} {strat} grad x")
            assert_close(b.grad, z[f"{cn}/f32/{strat}/grad_beta"], 2e-4, f"{cn} {strat} grad beta")


def case_oc_spatial(device, cases=("td1", "td2", "td3"), sampling=True, caps=(4, 256), cap_hits=None, n_cloud=3000):
    """The "spatial" passes of the condensation losses (sorted chunks + box culling, csrc/oc.hip) forced
    on for the small reference cases: the same golden values, sub-sampling switches and neighbour cap
    as the dense N x K passes; and dense == spatial directly on a clustered cloud with noise."""
    from gnn_tracking_amd import losses_oc, synthetic

    old = losses_oc.SPATIAL
    try:
        losses_oc.SPATIAL = "on"
        case_condensation_losses(device, cases=cases)
        if sampling:
            case_oc_sampling(device)
        if caps:
            case_rg_neighbor_cap(device, caps=caps, n_hits=cap_hits)
        res = {}
        for dim_c, scale in ((3, 0.6), (12, 0.35)):
          ev = synthetic.make_pileup_event(7, n_cloud, dim=dim_c, n_particles=n_cloud // 10)
          for mode in ("on", "off"):
              losses_oc.SPATIAL = mode
              for strat, cls in (("rg", losses_oc.CondensationLossRG), ("tiger", losses_oc.CondensationLossTiger)):
                  b = ev["beta"].to(device).requires_grad_(True)
                  x = (ev["x"] * scale).to(device).requires_grad_(True)
                  ret = cls(lw_repulsive=2.0, lw_noise=0.5, lw_coward=0.25)(
                      beta=b, x=x, particle_id=ev["particle_id"].to(device),
                      reconstructable=ev["reconstructable"].to(device), pt=ev["pt"].to(device), eta=ev["eta"].to(device))
                  ret.loss.backward()
                  res[mode, strat] = ({k: float(v.detach()) for k, v in ret.loss_dct.items()}, x.grad.cpu(), b.grad.cpu())
          for strat in ("rg", "tiger"):
              (la, gxa, gba), (lb, gxb, gbb) = res["on", strat], res["off", strat]
              for k in la:
                  assert abs(la[k] - lb[k]) <= 2e-6 * abs(lb[k]) + 1e-12, f"spatial vs dense {strat} {k}: {la[k]} {lb[k]}"
              assert la["repulsive"] > 0, "no repulsive pairs: the comparison is vacuous"
              assert_close(gxa, gxb, 1e-5, f"spatial vs dense {strat} grad x")
              assert_close(gba, gbb, 1e-5, f"spatial vs dense {strat} grad beta")
    finally:
        losses_oc.SPATIAL = old


def case_good_node_mask(device):
    from gnn_tracking_amd.graph_masks import get_good_node_mask_tensors

    z = load("g5_oc.npz")
    t = {k: tt(z[f"td3/{k}"]) for k in ("particle_id", "pt", "eta", "reconstructable")}
    ref = O.good_node_mask(t["pt"].float(), t["particle_id"], t["reconstructable"].float(),
                           t["eta"].float())
    got = get_good_node_mask_tensors(pt=t["pt"].float().to(device),
                                     particle_id=t["particle_id"].to(device),
                                     reconstructable=t["reconstructable"].float().to(device),
                                     eta=t["eta"].float().to(device))
    assert got.dtype == torch.bool and torch.equal(got.cpu(), ref)


def case_mlp_stress(device, rounds=3, seed=5, cases_per_round=12, row_choices=(1, 15, 16, 17, 77, 1000, 4099)):
    """Random MLP shapes / row counts / segmentations, forward + backward, repeated: the
    generic (run-time bound) kernels next to the static ones, tails, multi-segment inputs
    with and without gathers, alternating with and without parameter / input gradients."""
    g = np.random.default_rng(seed)
    torch.manual_seed(seed)
    for rnd in range(rounds):
        for _ in range(cases_per_round):
            L = int(g.integers(2, 4))
            n_seg = int(g.integers(1, 5))
            dims = [int(g.integers(1, 13)) for _ in range(n_seg)]
            while sum(dims) > 48:
                dims[int(np.argmax(dims))] -= 1
            hid, out = int(g.integers(1, 65)), int(g.integers(1, 17))
            rows = int(g.choice(list(row_choices)))
            src_rows = int(g.integers(3, 200))
            bias = bool(g.integers(0, 2))
            m = G.MLP(sum(dims), out, hid, L=L, bias=bias)
            p = {"m." + k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
            segs_cpu, idxs = [], []
            for d in dims:
                if g.random() < 0.5:
                    segs_cpu.append(torch.randn(src_rows, d))
                    idxs.append(torch.from_numpy(g.integers(0, src_rows, size=rows)).int())
                else:
                    segs_cpu.append(torch.randn(rows, d))
                    idxs.append(None)
            want_dx = bool(g.integers(0, 2))
            ref_in = [s.clone().requires_grad_(want_dx) for s in segs_cpu]
            cat = torch.cat([s if i is None else s[i.long()] for s, i in zip(ref_in, idxs)], dim=1)
            yo = O.mlp(cat, p, "m", L, bias=bias)
            r = torch.randn(rows, out)
            (yo * r).sum().backward()
            m = m.to(device)
            dev_in = [s.clone().to(device).requires_grad_(want_dx) for s in segs_cpu]
            # gathered segments fold their row gradients with torch's index_add here (the CSR
            # folds are covered by the interaction-network cases): give them reduce=None by
            # materialising the gather through autograd-aware indexing
            segs = []
            for s, i in zip(dev_in, idxs):
                segs.append(ops.Seg(s) if i is None else ops.Seg(s[i.to(device).long()]))
            y = m.fused(segs)
            (y * r.to(device)).sum().backward()
            tag = f"stress L={L} dims={dims} hid={hid} out={out} rows={rows} bias={bias}"
            assert_close(y, yo, TOL_OUT, tag + " y")
            for k, v in m.named_parameters():
                assert_close(v.grad, p["m." + k].grad, TOL_GRAD, f"{tag} g {k}")
            if want_dx:
                for a, b in zip(dev_in, ref_in):
                    assert_close(a.grad, b.grad, TOL_GRAD, tag + " gx")


# ------------------------------------------------------------------ bf16 storage mode
# Tolerances: the kernels and oracle/ref_cpu.py:mlp_bf16_* round at the same points; they
# differ by fp32 summation order only, which can move a value across a bf16 rounding
# boundary (1 ulp = 2^-8 relative).  TOL16 bounds that; fp32 outputs (sigmoid) are tight.
TOL16 = 2.0 ** -7
# fp32 sigmoid output: agreement is ~1e-6 unless ONE hidden activation lands on the other side of
# a bf16 rounding boundary (kernel and oracle sum in different orders): that moves the
# pre-activation by 2^-9 |h| |w| ~ 2e-4 and the weight by a quarter of it
TOL16_SIG = 1e-4


def _rand_rows16(rows, dim, device, gen, poison=True):
    from gnn_tracking_amd import ops_bf16 as B
    t = B.empty_rows(rows, dim, "cpu", zero=True)
    t.copy_(torch.randn(rows, dim, generator=gen))
    # poison the padding: the kernels must ignore it (poison=False: the buffer-addressed shapes read pads as stored -
    # every producer of padded rows in the library writes zeros, include/gnntrk.h)
    buf = t.as_strided((rows, B.pad4(dim)), (B.pad4(dim), 1))
    if B.pad4(dim) > dim and poison:
        buf[:, dim:] = float("nan")
    return t.to(device) if device != "cpu" else t


def case_mlp_bf16_forward(device, rows=75):
    from gnn_tracking_amd import _capi, ops_bf16 as B
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)  # (the layer initialisations use the global generator)
    cases = [
        # (segment dims, gathered?, relu?, hidden, out, L, bias, epilogue)
        ((5, 5, 4), (True, True, False), (True, True, True), 40, 4, 3, True, "none"),
        ((5, 4), (False, False), (False, False), 40, 5, 3, True, "residual"),
        ((14,), (False,), (False,), 40, 5, 2, False, "relu"),
        ((4,), (True,), (False,), 40, 4, 2, False, "relu"),
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, 40, 1, 3, True,
         "sigmoid"),
        ((3,), (False,), (False,), 7, 2, 3, True, "none"),
        ((8, 8, 8, 8), (False,) * 4, (False,) * 4, 16, 16, 3, True, "none"),   # no free pad slot
        ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, 62, 9, 3, True, "none"),  # KI=2, HT=4
        # hidden widths 64 .. 95: five / six hidden tiles (the plain instantiations)
        ((5, 5, 4), (True, True, False), (True, True, True), 64, 4, 3, True, "none"),      # HT=5 (64 + ones)
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, 64, 1, 3, True, "sigmoid"),
        ((5, 4), (False, False), (False, False), 95, 5, 3, True, "residual"),               # HT=6 (95 + ones)
        ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, 80, 9, 2, False, "relu"),              # KI=2, HT=5, no bias
        # hidden widths 96 .. 128: seven / eight hidden tiles, one k-step of inputs
        ((5, 5, 4), (True, True, False), (True, True, True), 127, 4, 3, True, "none"),     # HT=8 (127 + ones)
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, 100, 1, 3, True, "sigmoid"),
        ((14,), (False,), (False,), 128, 5, 3, False, "relu"),                             # HT=8 exactly, no bias
        # hidden 64 / 128 WITH biases: no constant-one row, biases as accumulator initial values
        ((5, 5, 4), (True, True, False), (True, True, True), 128, 4, 3, True, "none"),
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, 128, 1, 3, True, "sigmoid"),
        ((5, 4), (False, False), (False, False), 128, 5, 2, True, "residual"),
        ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, 64, 9, 3, True, "relu"),              # KI=2, hidden 64
        # outputs over 16 features: two / three output tiles (three hidden tiles)
        ((5, 5, 4), (True, True, False), (True, True, True), 40, 40, 3, True, "none"),
        ((14,), (False,), (False,), 40, 40, 2, False, "relu"),
        ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, 40, 33, 3, True, "residual"),         # KI=2, OT=3
        ((9, 4), (False, True), (False, False), 36, 17, 3, True, "none"),                  # OT=2, ragged
        # inputs over 64 slots: three / four k-steps (GraphConstructionResIN(hidden_dim=40): 120 -> 40 -> 40 -> 40)
        ((40, 40, 40), (True, True, False), (True, True, True), 40, 40, 3, True, "none"),  # KI=4, OT=3
        ((40, 40), (False, False), (True, False), 40, 40, 3, True, "residual"),            # KI=3 (20 chunks + ones)
        ((40, 31, 30), (True, False, True), (False, False, False), 37, 5, 2, False, "relu"),  # KI=4, OT=1, ragged
    ]
    epi_code = {"none": _capi.EPI_NONE, "relu": _capi.EPI_RELU, "residual": _capi.EPI_RESIDUAL,
                "sigmoid": _capi.EPI_SIGMOID}
    for dims, gath, relu, hid, out, L, bias, epi in cases:
        n_src = 31
        segs, idxs, xs = [], [], []
        for d, gflag in zip(dims, gath):
            t = _rand_rows16(n_src if gflag else rows, d, device, gen)
            idx = (torch.randint(0, n_src, (rows,), generator=gen).int().to(device) if gflag else None)
            segs.append(t)
            idxs.append(idx)
        in_dim = sum(dims)
        m = G.MLP(in_dim, out, hid, L=L, bias=bias)
        weights = [l.weight.detach() for l in m.layers if hasattr(l, "weight")]
        biases = [l.bias.detach() if bias else None for l in m.layers if hasattr(l, "weight")]
        res = B.rows16(_rand_rows16(rows, out, device, gen)) if epi == "residual" else None
        out_idx = torch.randperm(rows, generator=gen).int().to(device) if epi == "sigmoid" else None
        # oracle
        xin = []
        for t, idx, r in zip(segs, idxs, relu):
            v = t.float().cpu()
            if idx is not None:
                v = v[idx.cpu().long()]
            xin.append(torch.relu(v) if r else v)
        z, _ = O.mlp_bf16_forward(torch.cat(xin, 1), weights, biases)
        ca, cb = (0.6, 0.8) if epi == "residual" else ((0.001, 0.998) if epi == "sigmoid" else (0.0, 1.0))
        yo = O.mlp_bf16_epilogue(z, epi, ca, cb, None if res is None else res.float().cpu())
        if out_idx is not None:
            tmp = torch.empty_like(yo)
            tmp[out_idx.cpu().long()] = yo
            yo = tmp
        wd = [w.to(device).contiguous() for w in weights]
        bd = [None if b is None else b.to(device).contiguous() for b in biases]
        mlp = ops._fill_mlp(wd, bd)
        y = B.mlp_forward_raw([B.rows16(s) for s in segs], idxs, relu, wd, bd, n_rows=rows,
                              epilogue=epi_code[epi], ca=ca, cb=cb, res=res, out_idx=out_idx,
                              out_rows=rows, mlp=mlp)
        tag = f"bf16 MLP {dims}->{hid}->{out} L={L} bias={bias} {epi}"
        assert_close(y.float(), yo, TOL16_SIG if epi == "sigmoid" else TOL16, tag)
        if epi != "sigmoid" and B.pad4(out) > out:  # padding written as zeros
            buf = y.as_strided((rows, B.pad4(out)), (B.pad4(out), 1))
            assert (buf[:, out:] == 0).all(), tag + " padding"


def case_mlp_bf16_backward(device, rows=75, full=True, cases=None, seed=1):
    from gnn_tracking_amd import _capi, ops_bf16 as B
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)  # (the layer initialisations use the global generator)
    given = cases
    cases = [
        # (segment dims, gathered?, relu?, need grad?, hidden, out, L, bias, epilogue, n_gout)
        ((5, 5, 4), (True, True, False), (True, True, True), (True, True, True), 40, 4, 3, True, "none", 2),
        ((5, 4), (False, False), (False, False), (True, True), 40, 5, 3, True, "residual", 1),
        ((4,), (True,), (False,), (False,), 40, 4, 2, False, "relu", 1),
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, (True,) * 6, 40, 1, 3,
         True, "sigmoid", 1),
    ]
    if full:
        cases += [
            ((14,), (False,), (False,), (False,), 40, 5, 2, False, "relu", 1),
            ((3,), (False,), (True,), (True,), 7, 2, 3, True, "none", 1),
            ((8, 8, 8, 8), (False,) * 4, (False,) * 4, (True, False, True, False), 16, 16, 3, True, "none", 1),
            ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, (True,) * 5, 30, 9, 3, True, "none", 1),
            # hidden widths 64 .. 95 (five / six hidden tiles, one tile per iteration)
            ((5, 5, 4), (True, True, False), (True, True, True), (True, True, True), 64, 4, 3, True, "none", 2),
            ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, (True,) * 6, 64, 1, 3,
             True, "sigmoid", 1),
            ((5, 4), (False, False), (False, False), (True, True), 95, 5, 3, True, "residual", 1),
            ((4,), (True,), (False,), (False,), 72, 4, 2, False, "relu", 1),
            ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, (True,) * 5, 90, 9, 3, True, "none", 1),
            # hidden widths 96 .. 128 (seven / eight hidden tiles, one k-step of inputs)
            ((5, 5, 4), (True, True, False), (True, True, True), (True, True, True), 127, 4, 3, True, "none", 2),
            ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, (True,) * 6, 100, 1, 3,
             True, "sigmoid", 1),
            ((5, 4), (False, False), (False, False), (True, True), 112, 5, 3, True, "residual", 1),
            ((14,), (False,), (False,), (False,), 128, 5, 3, False, "relu", 1),
            # hidden 64 / 128 WITH biases: biases as accumulator initial values, bias gradients through ones tiles
            ((5, 5, 4), (True, True, False), (True, True, True), (True, True, True), 128, 4, 3, True, "none", 2),
            ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, (True,) * 6, 128, 1, 3,
             True, "sigmoid", 1),
            ((5, 4), (False, False), (False, False), (True, True), 128, 5, 3, True, "residual", 1),
            ((14,), (False,), (False,), (False,), 128, 5, 2, True, "relu", 1),
            ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, (True,) * 5, 64, 9, 3, True, "none", 1),
            # outputs over 16 features: two / three output tiles (three hidden tiles; NONE / RESIDUAL epilogues)
            ((5, 5, 4), (True, True, False), (True, True, True), (True, True, True), 40, 40, 3, True, "none", 2),
            ((14,), (False,), (False,), (False,), 40, 40, 2, False, "none", 1),
            ((8, 8, 8, 8, 3), (False,) * 5, (True,) * 5, (True, False, True, False, True), 40, 33, 3, True, "residual", 1),
            ((9, 4), (False, True), (False, False), (True, True), 36, 17, 3, True, "none", 2),
            # inputs over 64 slots: three / four k-steps
            ((40, 40, 40), (True, True, False), (True, True, True), (True, True, True), 40, 40, 3, True, "none", 2),
            ((40, 40), (False, False), (True, False), (True, True), 40, 40, 3, True, "residual", 1),
            ((40, 31, 30), (True, False, True), (False, False, False), (True, False, True), 37, 5, 2, False, "none", 1),
        ]
    if given is not None:
        cases = given
    epi_code = {"none": _capi.EPI_NONE, "relu": _capi.EPI_RELU, "residual": _capi.EPI_RESIDUAL,
                "sigmoid": _capi.EPI_SIGMOID}
    for dims, gath, relu, need, hid, out, L, bias, epi, n_gout in cases:
        n_src = 31
        segs, idxs = [], []
        for d, gflag in zip(dims, gath):
            segs.append(B.rows16(_rand_rows16(n_src if gflag else rows, d, device, gen)))
            idxs.append(torch.randint(0, n_src, (rows,), generator=gen).int().to(device) if gflag else None)
        m = G.MLP(sum(dims), out, hid, L=L, bias=bias)
        weights = [l.weight.detach() for l in m.linears()]
        biases = [l.bias.detach() if bias else None for l in m.linears()]
        ca, cb = (0.6, 0.8) if epi == "residual" else ((0.001, 0.998) if epi == "sigmoid" else (0.0, 1.0))
        # upstream gradient terms
        gout, g_sum = [], torch.zeros(rows, out)
        if epi == "sigmoid":
            perm = torch.randperm(rows, generator=gen)
            gfull = torch.randn(rows, out, generator=gen)
            gout.append((gfull.to(device), perm.int().to(device)))
            g_sum = gfull[perm]
        else:
            for t in range(n_gout):
                if t == 0:
                    gt = B.rows16(_rand_rows16(rows, out, device, gen))
                    gout.append((gt, None))
                    g_sum = g_sum + gt.float().cpu()
                else:
                    gt = B.rows16(_rand_rows16(n_src, out, device, gen))
                    gi = torch.randint(0, n_src, (rows,), generator=gen)
                    gout.append((gt, gi.int().to(device)))
                    g_sum = g_sum + gt.float().cpu()[gi]
        # oracle
        xin, raw = [], []
        for t, idx, r in zip(segs, idxs, relu):
            v = t.float().cpu()
            if idx is not None:
                v = v[idx.cpu().long()]
            raw.append(v)
            xin.append(torch.relu(v) if r else v)
        gin, dW, db = O.mlp_bf16_backward(torch.cat(xin, 1), weights, biases, g_sum, epi, ca, cb)
        wd = [w.to(device).contiguous() for w in weights]
        bd = [None if b is None else b.to(device).contiguous() for b in biases]
        # the second segment's gradient rows are written through a row permutation when it is
        # wanted (how source-ordered folds receive pre-sorted rows)
        gperm = torch.randperm(rows, generator=gen) if (len(dims) > 1 and need[1]) else None
        gidx = [gperm.int().to(device) if (j == 1 and gperm is not None) else None for j in range(len(dims))]
        slices, gW, gb = B.mlp_backward_raw(segs, idxs, relu, wd, bd, n_rows=rows, epilogue=epi_code[epi],
                                            ca=ca, cb=cb, gout=gout, need_seg=need, want_dw=True,
                                            mlp=ops._fill_mlp(wd, bd), gidx=gidx)
        if gperm is not None:
            slices[1] = slices[1][gperm.to(slices[1].device)]
        tag = f"bf16 MLP bwd {dims}->{hid}->{out} L={L} bias={bias} {epi}"
        col = 0
        for j, d in enumerate(dims):
            if need[j]:
                want = gin[:, col:col + d] * ((raw[j] > 0) if relu[j] else 1.0)
                assert_rows_close(slices[j].float(), want, TOL16, f"{tag} gseg{j}")
            else:
                assert slices[j] is None
            col += d
        for i in range(L):
            assert_close(gW[i], dW[i], TOL16, f"{tag} gW{i}")
            if bias:
                assert_close(gb[i], db[i], TOL16, f"{tag} gb{i}")


def case_mlp_bf16_fold(device, seed=5, sizes=(1, 31, 32, 33, 75, 640, 2050)):
    """The in-kernel target fold of the bf16 backward (include/gnntrk.h: gnntrk_gfold): the gradient of the segment
    gathered through SORTED ids leaves the kernel summed per node.  Relational shape (x_i | x_j | e, with and without
    the ReLU on load, two and three upstream terms) and the edge-weight head's shape (h[src] | h[tgt] | four edge
    tensors, fp32 upstream gradient), id patterns that exercise every arm of the unit logic: runs that cross units
    (carry rows), a hub node spanning several units (a carry chain), ids more than 16 apart inside a unit (the
    window loop), isolated nodes (rows the kernel never writes), row counts around the 32-row unit.  Against the
    oracle's per-row gradients summed per node, against the per-row form + segment sum of the same launch, and the
    parameter gradients of the two forms bit for bit."""
    from gnn_tracking_amd import _capi, ops_bf16 as B

    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    lib = _capi.load()
    shapes = [
        # (dims, gathered, relu, hidden, out, epilogue, n_gout, folded segment)
        ((5, 5, 4), (True, True, False), (True, True, True), 40, 4, "none", 2, 0),
        ((5, 5, 4), (True, True, False), (False, False, False), 40, 4, "none", 3, 0),
        ((5, 5, 4, 4, 4, 4), (True, True, False, False, False, False), (False,) * 6, 40, 1, "sigmoid", 1, 1),
    ]
    epi_code = {"none": _capi.EPI_NONE, "sigmoid": _capi.EPI_SIGMOID}

    def sorted_ids(rows, n_nodes, kind):
        if kind == "random":       # degrees ~ 6: most runs cross a 16-row half, many a 32-row unit
            ids = torch.sort(torch.randint(0, n_nodes, (rows,), generator=gen)).values
        elif kind == "hub":        # one node owns 100 consecutive rows (a chain of carries), the rest random
            ids = torch.sort(torch.cat([torch.randint(0, n_nodes, (max(rows - 100, 0),), generator=gen),
                                        torch.full((min(rows, 100),), n_nodes // 2)])).values
        elif kind == "sparse":     # ids 40 apart on average: windows beyond the first, isolated nodes everywhere
            ids = torch.sort(torch.randint(0, n_nodes, (rows,), generator=gen) // 40 * 40).values
        else:                      # "one": every row the same node
            ids = torch.full((rows,), n_nodes - 1)
        return ids.int()

    checked = 0
    for dims, gath, relu, hid, out, epi, n_gout, jf in shapes:
        for rows in sizes:
            for kind in ("random", "hub", "sparse", "one"):
                n_nodes = 977 if kind == "sparse" else max(rows // 6, 3)
                n_src = n_nodes
                segs, idxs = [], []
                for j, (d, gflag) in enumerate(zip(dims, gath)):
                    # (the two gathered segments read ONE node tensor - by target and by source - as in the models:
                    #  one descriptor with two id streams is what the buffer-addressed shapes are)
                    segs.append(segs[0] if gflag and j > 0 else B.rows16(_rand_rows16(n_src if gflag else rows, d, device, gen, poison=False)))
                    if not gflag:
                        idxs.append(None)
                    elif j == jf:
                        idxs.append(sorted_ids(rows, n_nodes, kind).to(device))
                    else:
                        idxs.append(torch.randint(0, n_src, (rows,), generator=gen).int().to(device))
                m = G.MLP(sum(dims), out, hid, L=3, bias=True)
                weights = [l.weight.detach() for l in m.linears()]
                biases = [l.bias.detach() for l in m.linears()]
                ca, cb = (0.001, 0.998) if epi == "sigmoid" else (0.0, 1.0)
                gout, g_sum = [], torch.zeros(rows, out)
                if epi == "sigmoid":
                    gfull = torch.randn(rows, out, generator=gen)
                    gout.append((gfull.to(device), None))
                    g_sum = gfull
                else:
                    for t in range(n_gout):
                        if t == 1:   # the aggregation's share, gathered through the sorted ids
                            gt = B.rows16(_rand_rows16(n_src, out, device, gen, poison=False))
                            gout.append((gt, idxs[jf]))
                            g_sum = g_sum + gt.float().cpu()[idxs[jf].cpu().long()]
                        else:
                            gt = B.rows16(_rand_rows16(rows, out, device, gen, poison=False))
                            gout.append((gt, None))
                            g_sum = g_sum + gt.float().cpu()
                xin, raw = [], []
                for t, idx, r in zip(segs, idxs, relu):
                    v = t.float().cpu()
                    if idx is not None:
                        v = v[idx.cpu().long()]
                    raw.append(v)
                    xin.append(torch.relu(v) if r else v)
                gin, dW, db = O.mlp_bf16_backward(torch.cat(xin, 1), weights, biases, g_sum, epi, ca, cb)
                wd = [w.to(device).contiguous() for w in weights]
                bd = [b.to(device).contiguous() for b in biases]
                need = [True] * len(dims)
                other = 1 - jf   # the source-gathered twin: its rows leave through a permutation, as in the step
                gperm = torch.randperm(rows, generator=gen)
                gidx = [gperm.int().to(device) if j == other else None for j in range(len(dims))]
                kw = dict(n_rows=rows, epilogue=epi_code[epi], ca=ca, cb=cb, gout=gout, need_seg=need, want_dw=True,
                          gidx=gidx)
                res = {}
                for mode in (True, False):
                    old, B.FOLD_IN_KERNEL = B.FOLD_IN_KERNEL, mode
                    try:
                        rowptr = torch.searchsorted(idxs[jf].cpu().long(), torch.arange(n_nodes + 1)).int().to(device)
                        slices, gW, gb = B.mlp_backward_raw(segs, idxs, relu, wd, bd, mlp=ops._fill_mlp(wd, bd),
                                                            fold=(jf, n_nodes, rowptr), **kw)
                    finally:
                        B.FOLD_IN_KERNEL = old
                    res[mode] = (slices, [g.clone() for g in gW], [g.clone() for g in gb])
                tag = f"bf16 fold {dims}->{hid}->{out} {epi} gout={n_gout} rows={rows} ids={kind}"
                sl_f, gW_f, gb_f = res[True]
                sl_p, gW_p, gb_p = res[False]
                assert jf in sl_f.folded, f"{tag}: the launch did not take the fold"
                assert not sl_p.folded and tuple(sl_p[jf].shape) == (rows, dims[jf])
                assert tuple(sl_f[jf].shape) == (n_nodes, dims[jf])
                col = sum(dims[:jf])
                want_rows = gin[:, col:col + dims[jf]] * ((raw[jf] > 0) if relu[jf] else 1.0)
                want = torch.zeros(n_nodes, dims[jf]).index_add_(0, idxs[jf].cpu().long(), want_rows.float())
                assert_rows_close(sl_f[jf].float(), want, 2 * TOL16, f"{tag} folded vs oracle")
                per_row = torch.zeros(n_nodes, dims[jf]).index_add_(0, idxs[jf].cpu().long(), sl_p[jf].float().cpu())
                assert_rows_close(sl_f[jf].float(), per_row, 2 * TOL16, f"{tag} folded vs per-row form")
                # everything else of the launch is the same arithmetic: identical bits
                for j in range(len(dims)):
                    if j != jf:
                        assert torch.equal(sl_f[j], sl_p[j]), f"{tag}: slice {j} differs between the two forms"
                for i in range(3):
                    assert torch.equal(gW_f[i], gW_p[i]) and torch.equal(gb_f[i], gb_p[i]), f"{tag}: parameter gradients differ"
                checked += 1
    return checked


# ---- the instantiations of the bf16 launchers: names, probes, launches ------------------------------------------
# (shape, segment dims, hidden, out, L, bias, epilogue, upstream terms, wanted gradients, debug_flags, mode) ->
# per row count (33, 1): kernel name, then max_terms, can_fold, bce_supported.  Shapes: "plain" own tensor per
# segment; "rel" x[tgt] | x[src] | e of one node tensor (the relational model), "obj" x | aggr, "head" h[src] |
# h[tgt] | four edge tensors with an fp32 upstream gradient, "enc" one tensor of the tile's rows - what the
# buffer-addressed classes take.  mode: "" / "fold" (in-kernel fold of the target-gathered segment) / "bce".
# THE LITERALS ARE THE PARENT COMMIT'S ANSWERS (recorded on the emulator build of the commit before the launchers
# were rewritten; names and probes are host code) - consumers key timers and profiles on the names.
BF16_FWD_INSTANTIATIONS = [
    # shared output tile (R = 4), wide and not, with and without the sigmoid; two and three layers
    (("rel", (5, 5, 4), 40, 4, 3, True, "none"), ("mlp16_fwd_kernel<1, 3, true, false, 4, true>", "mlp16_fwd_kernel<1, 3, true, false, 4, false>")),
    (("gath", (4,), 40, 4, 2, False, "relu"), ("mlp16_fwd_kernel<1, 3, false, false, 4, false>",) * 2),
    (("enc", (4,), 40, 4, 2, False, "relu"), ("mlp16_fwd_kernel<1, 3, false, false, 4, true>", "mlp16_fwd_kernel<1, 3, false, false, 4, false>")),
    (("head", (5, 5, 4, 4, 4, 4), 40, 1, 3, True, "sigmoid"), ("mlp16_fwd_kernel<1, 3, true, true, 4, false>",) * 2),
    (("enc", (8,), 40, 1, 2, True, "sigmoid"), ("mlp16_fwd_kernel<1, 3, false, true, 4, true>",) * 2),
    (("obj", (5, 4), 40, 5, 3, True, "residual"), ("mlp16_fwd_kernel<1, 3, true, false, 1, true>", "mlp16_fwd_kernel<1, 3, true, false, 1, false>")),
    (("plain", (8, 8, 8, 8, 3), 62, 9, 3, True, "none"), ("mlp16_fwd_kernel<2, 4, true, false, 1, true>", "mlp16_fwd_kernel<2, 4, true, false, 1, false>")),
    # plain forms, five to eight hidden tiles
    (("rel", (5, 5, 4), 70, 4, 3, True, "none"), ("mlp16_fwd_kernel<1, 5, true, false, 1, false>",) * 2),
    (("obj", (5, 4), 90, 5, 2, True, "residual"), ("mlp16_fwd_kernel<1, 6, false, false, 1, false>",) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 100, 1, 3, True, "sigmoid"), ("mlp16_fwd_kernel<1, 7, true, true, 1, false>",) * 2),
    (("enc", (14,), 120, 5, 3, True, "relu"), ("mlp16_fwd_kernel<1, 8, true, false, 1, false>",) * 2),
    # bias_init: hidden 64 / 128 with biases
    (("rel", (5, 5, 4), 64, 4, 3, True, "none"), ("mlp16_fwd_bi_kernel<1, 4, true, false>",) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 128, 1, 3, True, "sigmoid"), ("mlp16_fwd_bi_kernel<1, 8, true, true>",) * 2),
    # output tiles / wide inputs, one to four k-steps
    (("rel", (5, 5, 4), 40, 40, 3, True, "none"), ("mlp16_fwd_ot_kernel<1, 3, 3, true>",) * 2),
    (("plain", (8, 8, 8, 8, 3), 40, 33, 3, True, "residual"), ("mlp16_fwd_ot_kernel<2, 3, 3, true>",) * 2),
    (("plain", (40, 40), 40, 40, 3, True, "residual"), ("mlp16_fwd_ot_kernel<3, 3, 3, true>",) * 2),
    (("plain", (40, 31, 30), 37, 5, 2, False, "relu"), ("mlp16_fwd_ot_kernel<4, 3, 1, false>",) * 2),
]
BF16_BWD_INSTANTIATIONS = [
    # generic I/O: no / one / two input-gradient tiles, two tiles per iteration and one, the two A/B flags
    (("plain", (14,), 40, 5, 2, False, "relu", 1, (False,), 0, ""),
     (("mlp16_bwd_kernel<1, 3, 0, false, false, 2, IoNone>", 2, 0, 0),) * 2),
    (("plain", (3,), 7, 2, 3, True, "none", 1, (True,), 0, ""),
     (("mlp16_bwd_kernel<1, 1, 1, true, false, 2, IoNone>", 2, 0, 0),) * 2),
    (("plain", (8, 8, 8, 8), 16, 16, 3, True, "none", 1, (True, False, True, False), 0, ""),
     (("mlp16_bwd_kernel<2, 2, 1, true, false, 1, IoNone>", 2, 0, 0),) * 2),
    (("plain", (5, 4), 64, 5, 3, False, "residual", 1, (True, True), 0, ""),
     (("mlp16_bwd_kernel<1, 4, 1, true, false, 1, IoNone>", 2, 0, 0),) * 2),
    (("plain", (8, 8, 8, 8, 3), 30, 9, 3, True, "none", 1, (True,) * 5, 0, ""),
     (("mlp16_bwd_kernel<2, 2, 4, true, false, 1, IoNone>", 2, 0, 0),) * 2),
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 2, (True,) * 3, 64, ""),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 1, IoNone>", 2, 0, 0),) * 2),
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 2, (True,) * 3, 128, ""),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoNone>", 2, 0, 0),) * 2),
    # output tiles / wide inputs, bias_init (hidden 64 / 128 with biases)
    (("rel", (5, 5, 4), 40, 40, 3, True, "none", 2, (True,) * 3, 0, ""),
     (("mlp16_bwd_ot_kernel<1, 3, 3, true>", 2, 0, 0),) * 2),
    (("plain", (40, 40), 40, 40, 3, True, "residual", 1, (True, True), 0, ""),
     (("mlp16_bwd_ot_kernel<3, 3, 3, true>", 2, 0, 0),) * 2),
    (("rel", (5, 5, 4), 64, 4, 3, True, "none", 2, (True,) * 3, 0, ""),
     (("mlp16_bwd_bi_kernel<1, 4, 2, true, false>", 2, 0, 0),) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 128, 1, 3, True, "sigmoid", 1, (True,) * 6, 0, ""),
     (("mlp16_bwd_bi_kernel<1, 8, 2, true, true>", 2, 0, 0),) * 2),
    # the buffer-addressed classes
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 2, (True,) * 3, 0, ""),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<2, false> >", 3, 0, 0),) * 2),
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 3, (True,) * 3, 0, ""),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<3, false> >", 3, 0, 0),) * 2),
    (("rel", (5, 5, 4), 12, 4, 3, True, "none", 2, (True,) * 3, 0, ""),
     (("mlp16_bwd_kernel<1, 1, 2, true, false, 2, IoRelational<2, false> >", 3, 0, 0),) * 2),
    (("obj", (5, 4), 40, 5, 3, True, "residual", 1, (True, True), 0, ""),
     (("mlp16_bwd_kernel<1, 3, 1, true, false, 2, IoObject>", 2, 0, 0),) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 40, 1, 3, True, "sigmoid", 1, (True,) * 6, 0, ""),
     (("mlp16_bwd_kernel<1, 3, 2, true, true, 2, IoHeadT<false> >", 2, 0, 1),) * 2),
    (("enc", (4,), 40, 4, 2, False, "relu", 1, (False,), 0, ""),
     (("mlp16_bwd_kernel<1, 3, 0, false, false, 2, IoEncoder8<1> >", 2, 0, 0),) * 2),
    (("enc", (4,), 40, 4, 2, False, "relu", 2, (False,), 0, ""),
     (("mlp16_bwd_kernel<1, 3, 0, false, false, 2, IoEncoder8<2> >", 2, 0, 0),) * 2),
    # both fold classes, the BCE head with three hidden tiles and one
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 2, (True,) * 3, 0, "fold"),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<2, true> >", 3, 1, 0),) * 2),
    (("rel", (5, 5, 4), 40, 4, 3, True, "none", 3, (True,) * 3, 0, "fold"),
     (("mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<3, true> >", 3, 1, 0),) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 40, 1, 3, True, "sigmoid", 1, (True,) * 6, 0, "fold"),
     (("mlp16_bwd_kernel<1, 3, 2, true, true, 2, IoHeadT<true> >", 2, 1, 0),) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 40, 1, 3, True, "sigmoid", 1, (True,) * 6, 0, "bce"),
     (("mlp16_bwd_bce_kernel<3>", 2, 0, 1),) * 2),
    (("head", (5, 5, 4, 4, 4, 4), 10, 1, 3, True, "sigmoid", 1, (True,) * 6, 0, "bce"),
     (("mlp16_bwd_bce_kernel<1>", 2, 0, 1),) * 2),
]


def _rows16_on(device, n, d, gen, poison):
    """Kernel-ready random rows on ``device`` with the WHOLE padded buffer behind them: a device copy of the [1, d]
    view of a single row keeps the row stride but drops the padding after the row, which the buffer-addressed
    shapes read as stored."""
    from gnn_tracking_amd import ops_bf16 as B
    t = _rand_rows16(n, d, "cpu", gen, poison=poison)
    full = t.as_strided((n, B.pad4(d)), (B.pad4(d), 1))
    return B.rows16((full if device == "cpu" else full.to(device))[:, :d])


def _inst_inputs(shape, dims, rows, out, epi, n_gout, device, gen):
    """Segments, their id streams, the upstream terms and the gradient row permutations of one table entry."""
    from gnn_tracking_amd import ops_bf16 as B
    n_src = 31
    buf = shape != "plain" and shape != "gath"

    node = lambda d: _rows16_on(device, n_src, d, gen, not buf)
    tile = lambda d: _rows16_on(device, rows, d, gen, not buf)
    ids = lambda: torch.randint(0, n_src, (rows,), generator=gen).int().to(device)
    perm = lambda: torch.randperm(rows, generator=gen).int().to(device)
    segs, idxs, gidx = [], [], [None] * len(dims)
    if shape in ("rel", "head"):       # two gathers of ONE node tensor, then tensors of the tile's rows
        x = node(dims[0])
        tgt_first = shape == "rel"
        tgt = torch.sort(torch.randint(0, n_src, (rows,), generator=gen)).values.int().to(device)   # (CSR order)
        src = ids()
        segs, idxs = [x, x], ([tgt, src] if tgt_first else [src, tgt])
        for d in dims[2:]:
            segs.append(tile(d))
            idxs.append(None)
        gidx[1 if tgt_first else 0] = perm()    # the source-gathered slice leaves through a row permutation
    elif shape == "gath":
        segs, idxs = [node(d) for d in dims], [ids() for _ in dims]
    else:                              # "obj", "enc", "plain": rows of the tile
        segs, idxs = [tile(d) for d in dims], [None] * len(dims)
        if shape == "plain" and len(dims) > 1:
            gidx[1] = perm()
    gout = []
    if epi == "sigmoid":
        gout.append((torch.randn(rows, out, generator=gen).to(device), None))
    else:
        for t in range(n_gout):
            if t == 1 and shape == "rel":     # the aggregation's share, gathered through the target ids
                gout.append((_rows16_on(device, n_src, out, gen, False), idxs[0]))
            else:
                gout.append((_rows16_on(device, rows, out, gen, False), None))
    return segs, idxs, gidx, gout, n_src


class _LaunchSpy:
    """Stands in for the loaded library: every bf16 MLP launch is also asked for its kernel name and its probes,
    with exactly the arguments of the launch."""

    def __init__(self, lib, device):
        import ctypes as C
        from gnn_tracking_amd import _capi
        self._lib, self.seen = lib, []
        self._label = torch.zeros(64, dtype=torch.uint8, device=device)
        self._w = torch.zeros(64, dtype=torch.float32, device=device)

        def name(fn, *args):
            buf = C.create_string_buffer(160)
            _capi.check(fn(*args, buf, len(buf)), lib)
            return buf.value.decode()

        def fwd(a, stream):
            rc = lib.gnntrk_mlp_forward_bf16(a, stream)
            self.seen.append(("fwd", name(lib.gnntrk_mlp_forward_bf16_kernel_name, a), rc))
            return rc

        def probes(a, hb):
            return (int(lib.gnntrk_mlp_backward_bf16_max_terms(a)), int(lib.gnntrk_mlp_backward_bf16_can_fold(a)),
                    int(lib.gnntrk_mlp_backward_bf16_bce_supported(a, hb)))

        def bwd(a, ws, ws_bytes, stream):
            rc = lib.gnntrk_mlp_backward_bf16(a, ws, ws_bytes, stream)
            # (bce_supported is asked with a stand-in loss block: whether the SHAPE is the fused head's)
            hb = _capi.HeadBce(self._label.data_ptr(), self._w.data_ptr(), 1.0, 0, int(a._obj.n_rows))
            self.seen.append(("bwd", name(lib.gnntrk_mlp_backward_bf16_kernel_name, a), rc) + probes(a, C.byref(hb)))
            return rc

        def bwd_bce(a, hb, ws, ws_bytes, stream):
            rc = lib.gnntrk_mlp_backward_bf16_bce(a, hb, ws, ws_bytes, stream)
            self.seen.append(("bwd", name(lib.gnntrk_mlp_backward_bf16_bce_kernel_name, a, hb), rc) + probes(a, hb))
            return rc

        self._over = {"gnntrk_mlp_forward_bf16": fwd, "gnntrk_mlp_backward_bf16": bwd,
                      "gnntrk_mlp_backward_bf16_bce": bwd_bce}

    def __getattr__(self, key):
        return self._over.get(key) or getattr(self._lib, key)


def bf16_instantiation_answers(device, direction, spec, rows):
    """Runs one table entry; returns what the library answered (forward: the kernel name; backward: name, max_terms,
    can_fold, bce_supported).  The launch must succeed, and a backward launch's results must equal those of the same
    launch on the generic I/O (debug_flags = 128) by the rule of case_mlp_bf16_backward: rows within TOL16."""
    from gnn_tracking_amd import _capi, ops_bf16 as B
    epi_code = {"none": _capi.EPI_NONE, "relu": _capi.EPI_RELU, "residual": _capi.EPI_RESIDUAL,
                "sigmoid": _capi.EPI_SIGMOID}
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    if direction == "fwd":
        shape, dims, hid, out, L, bias, epi = spec
        n_gout, need, flags, mode = 1, None, 0, ""
    else:
        shape, dims, hid, out, L, bias, epi, n_gout, need, flags, mode = spec
    segs, idxs, gidx, gout, n_src = _inst_inputs(shape, dims, rows, out, epi, n_gout, device, gen)
    relu = [shape == "rel"] * len(dims)
    m = G.MLP(sum(dims), out, hid, L=L, bias=bias)
    W = [l.weight.detach().to(device).contiguous() for l in m.linears()]
    b = [l.bias.detach().to(device).contiguous() if bias else None for l in m.linears()]
    ca, cb = (0.6, 0.8) if epi == "residual" else ((0.001, 0.998) if epi == "sigmoid" else (0.0, 1.0))
    spy = _LaunchSpy(_capi.load(), device)
    saved = (_capi.load, B._DEBUG_FLAGS, B.FOLD_IN_KERNEL)
    _capi.load = lambda: spy
    try:
        if direction == "fwd":
            res = _rows16_on(device, rows, out, gen, True) if epi == "residual" else None
            B.mlp_forward_raw(segs, idxs, relu, W, b, n_rows=rows, epilogue=epi_code[epi], ca=ca, cb=cb, res=res,
                              out_idx=None, out_rows=rows, mlp=ops._fill_mlp(W, b))
            (_, name, rc), = spy.seen
            assert rc == 0, (spec, rows, rc)
            return name

        label = (torch.rand(rows + 8, generator=gen) < 0.5).to(torch.uint8).to(device)[:rows]

        def launch(flags_, fold_):
            B._DEBUG_FLAGS, B.FOLD_IN_KERNEL = flags_, fold_
            del spy.seen[:]
            kw, bce = {}, None
            if fold_:
                jf = 0 if shape == "rel" else 1
                rowptr = torch.searchsorted(idxs[jf].cpu().long(), torch.arange(n_src + 1)).int().to(device)
                kw["fold"] = (jf, n_src, rowptr)
            if mode == "bce":
                bce = kw["bce"] = B.HeadBce(label, torch.zeros(rows, dtype=torch.float32, device=device),
                                            torch.zeros(1, dtype=torch.float32, device=device), 0.5)
            sl, gW, gb = B.mlp_backward_raw(segs, idxs, relu, W, b, n_rows=rows, epilogue=epi_code[epi], ca=ca, cb=cb,
                                            gout=[] if mode == "bce" else gout, need_seg=need, want_dw=True,
                                            mlp=ops._fill_mlp(W, b), gidx=gidx, **kw)
            seen = [s for s in spy.seen if s[0] == "bwd"]
            assert len(seen) == 1 and seen[0][2] == 0, (spec, rows, spy.seen)
            return seen[0][1:2] + seen[0][3:], sl, [g.clone() for g in gW], [None if g is None else g.clone() for g in gb], bce

        got, sl, gW, gb, bce = launch(flags, mode == "fold")
        ref, sl_g, gW_g, gb_g, bce_g = launch(128, False)
        tag = f"bf16 instantiation {spec} rows={rows}"
        assert "IoNone" in ref[0] or "_ot_" in ref[0] or "_bi_" in ref[0], (tag, ref[0])
        for j in range(len(dims)):
            if sl[j] is None or j in sl.folded:   # (a folded slice is one row per node: case_mlp_bf16_fold checks it)
                continue
            assert_rows_close(sl[j].float(), sl_g[j].float().cpu(), TOL16, f"{tag} gseg{j} vs generic I/O")
        for i in range(L):
            assert_close(gW[i], gW_g[i].cpu(), TOL16, f"{tag} gW{i} vs generic I/O")
            if bias:
                assert_close(gb[i], gb_g[i].cpu(), TOL16, f"{tag} gb{i} vs generic I/O")
        if bce is not None:
            assert_close(bce.w, bce_g.w.cpu(), TOL16_SIG, f"{tag} W vs the forward launch")
        return got
    finally:
        _capi.load, B._DEBUG_FLAGS, B.FOLD_IN_KERNEL = saved


def case_bf16_instantiations(device, rows=(33, 1)):
    """Every branch of the bf16 launchers' selection (forward, generic / output-tile / bias_init backward, every
    buffer-addressed class, both fold classes, the BCE head): the name entry points and the probes answer the
    literals of the tables above, the launch runs, and its results are those of the generic I/O."""
    n = 0
    for spec, names in BF16_FWD_INSTANTIATIONS:
        for r, want in zip(rows, names):
            got = bf16_instantiation_answers(device, "fwd", spec, r)
            assert got == want, f"forward {spec} rows={r}: {got!r}, the table says {want!r}"
            n += 1
    for spec, answers in BF16_BWD_INSTANTIATIONS:
        for r, want in zip(rows, answers):
            got = bf16_instantiation_answers(device, "bwd", spec, r)
            assert got == want, f"backward {spec} rows={r}: {got!r}, the table says {want!r}"
            n += 1
    return n


def case_bf16_shape_rules_agree(device, hiddens=(1, 16, 31, 32, 33, 40, 47, 48, 63, 64, 65, 95, 96, 97, 112, 127, 128, 129),
                                outs=(1, 4, 16, 17, 40, 48, 49), min_ran=300):
    """What ``ops._fused_supported`` accepts in bf16 storage, the C launchers run - forward and backward - over a
    grid of widths around every tile boundary: a drift between the Python rule and ``make_slot_plan`` /
    the instantiation lists would otherwise surface as ``GNNTRK_EUNSUPPORTED`` in the middle of a training step."""
    from gnn_tracking_amd import _capi, ops_bf16 as B
    gen = torch.Generator().manual_seed(5)
    rows = 3
    dim_sets = ((5, 5, 4), (14,), (8, 8, 8, 8, 3), (40, 40, 40), (40, 40), (12, 12, 12, 12, 12, 4))
    ran = 0
    for dims in dim_sets:
        for hid in hiddens:
            for out in outs:
                for bias in (True, False):
                    for L, epi in ((3, _capi.EPI_NONE), (2, _capi.EPI_RESIDUAL), (3, _capi.EPI_RELU)):
                        segs = [B.rows16(_rand_rows16(rows, d, device, gen)) for d in dims]
                        m = G.MLP(sum(dims), out, hid, L=L, bias=bias)
                        W = [l.weight.detach().to(device).contiguous() for l in m.linears()]
                        b = [l.bias.detach().to(device).contiguous() if bias else None for l in m.linears()]
                        if not ops._fused_supported([ops.Seg(t) for t in segs], W, b, True, epi):
                            continue
                        tag = f"dims {dims} hidden {hid} out {out} bias {bias} L {L} epilogue {epi}"
                        mlp = ops._fill_mlp(W, b)
                        res = B.rows16(_rand_rows16(rows, out, device, gen)) if epi == _capi.EPI_RESIDUAL else None
                        try:
                            B.mlp_forward_raw(segs, [None] * len(dims), [False] * len(dims), W, b, n_rows=rows, epilogue=epi,
                                              ca=0.6, cb=0.8, res=res, out_idx=None, out_rows=rows, mlp=mlp)
                            g = B.rows16(_rand_rows16(rows, out, device, gen))
                            B.mlp_backward_raw(segs, [None] * len(dims), [False] * len(dims), W, b, n_rows=rows, epilogue=epi,
                                               ca=0.6, cb=0.8, gout=[(g, None)], need_seg=[True] * len(dims), want_dw=True,
                                               mlp=mlp)
                        except NotImplementedError as e:
                            raise AssertionError(f"Python accepts what the library refuses: {tag}: {e}") from e
                        ran += 1
    assert ran > min_ran, ran


def case_mlp_bf16_stress(device, rounds=3, seed=17, cases_per_round=8, row_choices=(1, 16, 17, 33, 100, 2050), wide=False,
                         wide_io=False):
    """Random shapes through the bf16 backward (and the forward recompute inside it): one to four
    segments with and without gathers / ReLU-on-load / wanted gradients, hidden widths on both
    sides of the tile boundaries (one k-step and up to three hidden tiles run the two-tile form,
    the rest the one-tile form; no wanted gradient at all runs the weight-gradient-only form),
    L = 2 / 3, with and without bias, all four epilogues, one or two upstream terms, row counts
    around the 16- and 32-row tile sizes.  ``wide``: also hidden widths 63 .. 127 (five to eight hidden
    tiles).  ``wide_io``: three hidden tiles with up to 32 input chunks and up to 48 outputs (NONE / RESIDUAL)."""
    g = np.random.default_rng(seed)
    for rnd in range(rounds):
        cases = []
        for _ in range(cases_per_round if not wide_io else 0):
            n_seg = int(g.integers(1, 5))
            dims = tuple(int(g.integers(1, 13)) for _ in range(n_seg))
            bias = bool(g.integers(0, 2))
            while sum((d + 3) // 4 for d in dims) + (1 if bias and all(d % 4 == 0 for d in dims) else 0) > 16:
                dims = dims[:-1]
            epi = ("none", "relu", "residual", "sigmoid")[int(g.integers(0, 4))]
            hid = int(g.choice([1, 7, 15, 16, 31, 40, 47, 48, 62] + ([63, 64, 65, 79, 80, 94, 95, 96, 111, 112, 126, 127, 128] if wide else [])))
            n_ch = sum((d + 3) // 4 for d in dims) + (1 if bias and all(d % 4 == 0 for d in dims) else 0)
            if hid + (1 if bias and hid != 128 else 0) > 96 and n_ch > 8:   # seven / eight hidden tiles: one k-step of inputs
                hid = 90
            out = int(g.integers(1, 17))
            cases.append((dims, tuple(bool(g.integers(0, 2)) for _ in dims), tuple(bool(g.integers(0, 2)) for _ in dims),
                          tuple(bool(g.integers(0, 3)) for _ in dims), hid, out, int(g.integers(2, 4)), bias, epi,
                          1 if epi == "sigmoid" else int(g.integers(1, 3))))
        for _ in range(cases_per_round if wide_io else 0):
            n_seg = int(g.integers(1, 5))
            dims = tuple(int(g.integers(1, 41)) for _ in range(n_seg))
            bias = bool(g.integers(0, 2))
            while sum((d + 3) // 4 for d in dims) + (1 if bias and all(d % 4 == 0 for d in dims) else 0) > 32:
                dims = dims[:-1]
            n_ch = sum((d + 3) // 4 for d in dims) + (1 if bias and all(d % 4 == 0 for d in dims) else 0)
            out = int(g.integers(17, 49)) if (n_ch <= 16 or g.integers(0, 2)) else int(g.integers(1, 17))
            hid = int(g.integers(33, 48 if not bias else 47))   # (hidden + bias row in 33 .. 48: three hidden tiles)
            epi = ("none", "residual")[int(g.integers(0, 2))]
            cases.append((dims, tuple(bool(g.integers(0, 2)) for _ in dims), tuple(bool(g.integers(0, 2)) for _ in dims),
                          tuple(bool(g.integers(0, 3)) for _ in dims), hid, out, int(g.integers(2, 4)), bias, epi,
                          int(g.integers(1, 3))))
        case_mlp_bf16_backward(device, rows=int(g.choice(row_choices)), cases=cases, seed=seed + rnd)


def case_ec_bf16(device, names=("skip1_L3_h40", "alpha0", "h64", "h128")):
    """ECForGraphTCN in bf16-storage mode on the golden inputs of g2: forward against the
    bf16 restatement (oracle/ref_cpu.py:ec_for_graph_tcn_bf16, same rounding points) and
    against the reference-pinned fp32 goldens with a bf16-sized tolerance; loss and
    parameter gradients against the fp32 goldens (bf16 noise bound)."""
    z = load("g2_ec_variants.npz")
    za = load("g2b_ec_bf16_autocast.npz")   # the reference's own modules under CPU bf16 autocast
    report = {}
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, pt = tt(z["y"], device), tt(z["pt"], device)
    for name in names:
        kw = EC_VARIANTS[name]
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **kw)
        p = load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        lib_path_before = set(ops._WIDE_WARNED)
        with G.bf16_storage():
            out = model(G.Data(x=x, edge_index=ei, edge_attr=ea))
            loss = G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=y.float(), pt=pt, edge_index=ei)
            loss.backward()
        assert out["W"].dtype == torch.float32 and out["node_embedding"].dtype == torch.bfloat16
        if name != "wide_h128":   # every MLP of the variant ran on the fused kernels (h64: five hidden tiles)
            assert set(ops._WIDE_WARNED) == lib_path_before, f"{name}: {set(ops._WIDE_WARNED) - lib_path_before} took the library path"
        plain = (kw.get("residual_type", "skip1") == "skip1" and kw.get("use_node_embedding", True)
                 and kw.get("use_intermediate_edge_embeddings", True))
        if plain:  # the bf16 restatement covers the default wiring
            ref = O.ec_for_graph_tcn_bf16(x.cpu(), ei.cpu(), ea.cpu(), p, L_ec=kw["L_ec"],
                                          alpha=kw.get("alpha", 0.5))
            # same rounding points: differences come from rare 1-ulp flips propagating
            # (measured: W 6e-8 .. 7e-7 on the fused kernels, 1.3e-4 on wide_h128's library GEMMs; embeddings equal)
            errW = (out["W"].detach().cpu() - ref["W"]).abs().max().item()
            assert errW <= BF16_ORACLE_W, f"{name}: |W - W_oracle16| {errW:.2e}"
            assert_close(out["node_embedding"].float(), ref["node_embedding"], TOL16, name + " node")
            assert_close(out["edge_embedding"].float(), ref["edge_embedding"], TOL16, name + " edge")
        # distance to the reference-pinned fp32 results
        assert_close(out["W"], z[f"{name}/W"], 0.03, name + " W vs fp32 golden")
        assert_close(loss, z[f"{name}/loss"], 0.01, name + " loss vs fp32 golden")
        for k, v in model.named_parameters():
            gref = tt(z[f"{name}/grad/{k}"]).double()
            if v.grad is None:  # parameter without a path to the loss in this variant
                assert gref.abs().max().item() == 0.0, f"{name} grad {k} missing"
                continue
            assert v.grad.dtype == torch.float32
            err = (v.grad.detach().cpu().double() - gref).norm() / max(gref.norm().item(), 1e-6)
            # (253 edges: a handful of bf16 roundings decide a gradient - measured 1.9 % on the headline shape,
            #  up to 6.0 % on the skip2 / skip-top / 128-wide variants of this graph; the full-size event: 1.2 %)
            bar = BF16_GRAD_REL_L2 if name in ("skip1_L3_h40", "skip1_L2_h2", "alpha0") else 0.07
            assert err < bar, f"{name} grad {k}: relative L2 error {err:.3f} vs fp32 golden (bar {bar})"
        # THE PIN AGAINST THE REFERENCE IN ITS OWN MIXED PRECISION (golden G2b): W within one
        # bf16 ulp of the reference's bf16-rounded W (2^-8 on [0.5, 1)), embeddings within
        # BF16_PIN_EMB of the largest reference entry, loss 5e-3 (the reference rounds W itself to bf16), parameter gradients 6 %
        # relative L2 bar 4 % (measured: W <= 2.9e-3, embeddings <= 3.1e-3, gradients <= 2.9 %; the reference's own scatter-add accumulates in bf16; ours in fp32).
        rep = report.setdefault(name, {})
        rep["W"] = (out["W"].detach().cpu() - tt(za[f"{name}/W"])).abs().max().item()
        for k in ("node_embedding", "edge_embedding"):
            ref_k = tt(za[f"{name}/{k}"])
            rep[k] = ((out[k].detach().float().cpu() - ref_k).abs().max() / max(1.0, ref_k.abs().max().item())).item()
        rep["loss"] = abs(float(loss) - float(za[f"{name}/loss"]))
        worst = 0.0
        for k, v in model.named_parameters():
            gref = tt(za[f"{name}/grad/{k}"]).double()
            if v.grad is None or gref.norm().item() < 1e-6:
                continue
            worst = max(worst, ((v.grad.detach().cpu().double() - gref).norm() / gref.norm()).item())
        rep["grad_rel_l2"] = worst
        assert rep["W"] <= BF16_PIN_W, f"{name}: |W - W_autocast| {rep['W']:.2e}"
        assert rep["node_embedding"] <= BF16_PIN_EMB and rep["edge_embedding"] <= BF16_PIN_EMB, (name, rep)
        assert rep["loss"] <= 5e-3 and rep["grad_rel_l2"] <= 0.04, (name, rep)
    return report


def case_ec_carry_equals_gather(device, name="skip1_L3_h40"):
    """The training step with the labels / edge features carried along by the graph-index build and the
    fused CSR BCE is BIT-IDENTICAL to the step with the gathers through perm and the two-pass BCE
    (bf16 storage, bool labels, pt falsification on and off)."""
    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, pt = tt(z["y"], device).bool(), tt(z["pt"], device)
    res = {}
    for thld in (0.0, 0.9):
        for carry in (True, False):
            ops.CARRY = carry
            try:
                model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
                load_params(model, z, f"{name}/p0/")
                model = model.to(device)
                ops.clear_graph_index_cache()
                with G.bf16_storage():
                    out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y))
                    gi = out["W"].graph_index
                    assert (ops.carried_label(gi, y) is not None) == carry and (ops.carried_rows(gi, ea) is not None) == carry
                    loss = G.EdgeWeightBCELoss(pt_thld=thld)(w=out["W"], y=y, pt=pt, edge_index=ei)
                    loss.backward()
                res[carry] = (loss.detach().clone(), out["W"].csr.detach().clone(),
                              {k: v.grad.clone() for k, v in model.named_parameters()})
            finally:
                ops.CARRY = True
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1]), f"thld={thld}"
        for k in res[True][2]:
            assert torch.equal(res[True][2][k], res[False][2][k]), f"thld={thld} grad {k}"
        assert_close(res[True][0], z[f"{name}/loss"], 0.01, "loss vs fp32 golden") if thld == 0.9 else None


def case_grad_sink(device, name="skip1_L3_h40"):
    """Parameters re-homed by ``dist.FlatParameters`` receive their weight / bias gradients straight from
    the backward launches (``accumulate_params``): BIT-IDENTICAL to the gradients autograd accumulates
    from returned tensors, in fp32 and bf16 storage, over one backward and over two accumulated ones."""
    from gnn_tracking_amd import dist as gdist
    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, pt = tt(z["y"], device).bool(), tt(z["pt"], device)
    for bf16 in (False, True):
        got = {}
        for sink in (True, False):
            model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
            load_params(model, z, f"{name}/p0/")
            model = model.to(device)
            flat = gdist.FlatParameters(model, grad_sink=sink)
            assert all(getattr(p_, "_gnntrk_grad_sink", False) == sink for p_ in flat.params)
            snaps = []
            for rep in range(2):   # (gradients ACCUMULATE over the two backward passes)
                ops.clear_graph_index_cache()
                with G.bf16_storage(bf16), ops.grad_sinks_armed():
                    out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y))
                    G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=y, pt=pt, edge_index=ei).backward()
                snaps.append(flat.grad.clone())
            for p_ in flat.params:   # the gradients still live in the bucket
                assert p_.grad.data_ptr() >= flat.grad.data_ptr() and p_.grad.untyped_storage().data_ptr() == flat.grad.untyped_storage().data_ptr()
            got[sink] = snaps
        for rep in range(2):
            assert torch.equal(got[True][rep], got[False][rep]), f"bf16={bf16} pass {rep}: sink != autograd accumulation"
        assert float(got[True][0].abs().sum()) > 0 and not torch.equal(got[True][0], got[True][1])
        if not bf16:   # (two accumulated passes = twice the reference's gradients)
            for k, v in model.named_parameters():
                assert_close(v.grad / 2, z[f"{name}/grad/{k}"], TOL_GRAD, f"sink grad {k} vs golden")
    # The shortcut bypasses AccumulateGrad, so it must step aside wherever that could be observed: a tensor
    # hook or a post-accumulate-grad hook on a marked parameter still fires (with the gradient autograd would
    # deliver), a backward() outside grad_sinks_armed() and torch.autograd.grad take the autograd path.
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
    load_params(model, z, f"{name}/p0/")
    model = model.to(device)
    flat = gdist.FlatParameters(model, grad_sink=True)
    names = dict((id(p_), k) for k, p_ in model.named_parameters())
    fired, post = {}, []
    hooked = [p_ for p_ in flat.params if p_.dim() == 2][:2]
    handles = [hooked[0].register_hook(lambda g, k=names[id(hooked[0])]: fired.__setitem__(k, g.clone()))]
    handles.append(hooked[1].register_post_accumulate_grad_hook(lambda p_: post.append(names[id(p_)])))

    def loss_of():
        ops.clear_graph_index_cache()
        out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y))
        return G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=y, pt=pt, edge_index=ei)

    flat.zero_grad()
    with ops.grad_sinks_armed():
        loss_of().backward()
    assert list(fired) == [names[id(hooked[0])]] and post == [names[id(hooked[1])]], (fired.keys(), post)
    for k, v in model.named_parameters():
        assert_close(v.grad, z[f"{name}/grad/{k}"], TOL_GRAD, f"grad {k} with hooks on two parameters")
    assert_close(fired[names[id(hooked[0])]], z[f"{name}/grad/{names[id(hooked[0])]}"], TOL_GRAD, "gradient seen by the tensor hook")
    for h in handles:
        h.remove()
    before = flat.grad.clone()
    gs = torch.autograd.grad(loss_of(), flat.params)   # (not armed: returned, .grad untouched)
    assert torch.equal(flat.grad, before), "torch.autograd.grad wrote into .grad"
    for (k, _), g in zip(model.named_parameters(), gs):
        assert_close(g, z[f"{name}/grad/{k}"], TOL_GRAD, f"autograd.grad {k}")


BF16_PIN_W = 2.0 ** -8       # one ulp of the reference's bf16 W on [0.5, 1)
#: against OUR restatement of the rounding contract (oracle.ec_for_graph_tcn_bf16: same rounding points, so only rare
#: one-ulp flips of a hidden activation propagate): measured 6e-8 on the golden graph, 6.4e-6 at 20 k edges, 1.1e-4
#: at 2 M edges - the bar is 5e-4, not the bf16 ulp of W (3.9e-3) that rounds 2-5 accepted
BF16_ORACLE_W = 5e-4
#: parameter gradients of a bf16-storage run against the fp32 oracle, relative L2 of the worst parameter: 1.2 % measured
#: on the headline shape from 20 k edges on (the bf16 rounding of activations and activation gradients; fp32 accumulation)
BF16_GRAD_REL_L2 = 0.03
BF16_PIN_EMB = 2.0 ** -6     # four bf16 ulps relative to the largest entry


def case_bf16_reproducible(device):
    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y = tt(z["y"], device)
    name = "skip1_L3_h40"
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
    load_params(model, z, f"{name}/p0/")
    model = model.to(device)
    grads = []
    for _ in range(2):
        model.zero_grad()
        with G.bf16_storage():
            out = model(G.Data(x=x, edge_index=ei, edge_attr=ea))
            G.EdgeWeightBCELoss()(w=out["W"], y=y.float()).backward()
        grads.append({k: v.grad.clone() for k, v in model.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), f"{k}: run-to-run difference"


def case_rows_bf16(device):
    """bf16 helper kernels: conversion (+gather), CSR segment sums (both orders, dims that are
    not multiples of 4), row permutations - against torch on the same bf16 values."""
    from gnn_tracking_amd import ops_bf16 as B
    g = np.random.default_rng(4)
    for N, E, D in ((1, 0, 4), (7, 20, 5), (300, 4000, 4), (1000, 9000, 9), (50, 333, 4), (5, 1, 3), (9, 2, 2),
                    (300, 4000, 40), (50, 333, 33),   # (rows wider than 16 features: 16-column passes)
                    (300, 4000, 8), (3, 2000, 7), (17, 5000, 6), (1, 700, 8), (1000, 1500, 5)):   # (16-byte rows: streaming)
        ei = tt(g.integers(0, N, size=(2, E)), device).long()
        gi = ops.graph_index(ei, N, cache=False)
        x32 = tt(g.normal(size=(E, D)).astype(np.float32), device)
        rows = B.to_rows16(x32)
        assert rows.dtype == torch.bfloat16 and rows.stride(0) == B.pad4(D)
        assert torch.equal(rows.float().cpu(), x32.cpu().to(torch.bfloat16).float()), "RNE conversion"
        if E:
            perm = gi.perm
            got = B.to_rows16(x32, perm)
            assert torch.equal(got.float().cpu(), x32.cpu()[perm.cpu().long()].to(torch.bfloat16).float())
            back = B.permute_raw(got, perm, scatter=True)
            assert torch.equal(back.float().cpu(), rows.float().cpu()), "permute scatter inverts gather"
        csr = rows  # treat the rows as already CSR ordered
        for by, ids in (("tgt", gi.tgt), ("src", None)):
            out = ops.segment_sum(csr, gi, by)
            ref = torch.zeros(N, D)
            if E:
                node = gi.tgt.cpu().long() if by == "tgt" else gi.src.cpu().long()
                ref.index_add_(0, node, csr.float().cpu())
            assert_close(out.float(), ref.to(torch.bfloat16).float(), TOL16, f"segment_sum16 {by} N={N} D={D}")
            if E:
                # one more term per segment before the single rounding (gnntrk_segment_sum_bf16_add)
                rowptr_a, pos_a = (gi.rowptr_t, None) if by == "tgt" else (gi.rowptr_s, gi.spos)
                add32 = tt(g.normal(size=(N, D)).astype(np.float32), device)
                addend = B.to_rows16(add32)
                got = B.segment_sum_raw(csr, rowptr_a, pos_a, N, addend=addend)
                want = (ref.double() + addend.float().cpu().double()).float().to(torch.bfloat16).float()
                assert_close(got.float(), want, TOL16, f"segment_sum16 + addend {by} N={N} D={D}")
            if E and B.pad4(D) == 8:
                # contiguous 16-byte rows take the LDS-staged streaming kernel, rows at a 32-byte stride the
                # plain four-lane walk: the same sums in the same order, bit for bit
                padded = torch.zeros(E, 16, dtype=torch.bfloat16, device=csr.device)
                padded[:, :csr.shape[1]] = csr
                strided = padded[:, :csr.shape[1]]
                rowptr, pos = (gi.rowptr_t, None) if by == "tgt" else (gi.rowptr_s, gi.spos)
                a = B.segment_sum_raw(csr, rowptr, None, N)
                b = B.segment_sum_raw(strided, rowptr, None, N)
                assert strided.stride(0) == 16 and torch.equal(a.view(torch.int16).cpu(), b.view(torch.int16).cpu()), \
                    f"streaming and walking segment sums differ: {by} N={N} D={D}"


def case_segment_sum_f32(device):
    """fp32 CSR segment sums (PyG ``aggr="add"``, interaction_network.py:36): every row-width class of the
    kernels (scalar, the 4-wide edge rows, 16-byte rows for widths that are multiples of four) against
    index_add in fp64, both orders, with and without accumulation; the 16-byte kernel and the scalar kernel -
    reached through a row stride that is not a multiple of four - agree bit for bit."""
    g = np.random.default_rng(14)
    for N, E, D in ((1, 0, 4), (7, 20, 5), (300, 4000, 4), (300, 4000, 40), (1000, 9000, 8), (50, 333, 12),
                    (5, 1, 3), (9, 2, 1), (64, 5000, 48)):
        ei = tt(g.integers(0, N, size=(2, E)), device).long()
        gi = ops.graph_index(ei, N, cache=False)
        wide = tt(g.normal(size=(E, D + 1)).astype(np.float32), device)
        rows_strided = wide[:, :D]                     # row stride D + 1
        rows = rows_strided.contiguous()
        for by in ("tgt", "src"):
            out = ops.segment_sum(rows, gi, by)
            node = (gi.tgt if by == "tgt" else gi.src).cpu().long()
            ref = torch.zeros(N, D, dtype=torch.float64)
            if E:
                ref.index_add_(0, node, rows.cpu().double())
            assert_close(out, ref.float(), TOL_OUT, f"segment_sum {by} N={N} D={D}")
            rowptr, pos = (gi.rowptr_t, None) if by == "tgt" else (gi.rowptr_s, gi.spos)
            if E:
                out_s = ops._segment_sum_raw(rows_strided, rowptr, pos, N)
                assert torch.equal(out.cpu(), out_s.cpu()), f"row-width classes differ: {by} N={N} D={D}"
            base = tt(g.normal(size=(N, D)).astype(np.float32), device)
            acc = base.clone()
            ops._segment_sum_raw(rows, rowptr, pos, N, out=acc, accumulate=True)
            assert_close(acc, (base.cpu().double() + ref).float(), TOL_OUT, f"segment_sum accumulate {by} D={D}")


def case_node_tap(device):
    """bf16 storage: the fused gradient plumbing of one interaction-network layer (ops_bf16.node_tap, the folds of
    a tensor gathered twice, the residual pass-through joining its identity segment) against plain autograd
    accumulation of the same kernels' gradients (flags off): all gradients within bf16 rounding of each other, for
    a whole backward, for ``torch.autograd.grad`` w.r.t. the node embedding only, with frozen relational weights,
    with an input that needs no gradient, and for two backward passes over a retained graph."""
    from gnn_tracking_amd import ops_bf16 as B
    from gnn_tracking_amd.interaction_network import InteractionNetwork
    gen = torch.Generator().manual_seed(31)
    N, E = 200, 2600
    net = InteractionNetwork(node_indim=5, edge_indim=4, node_outdim=5, edge_outdim=4).to(device)
    enc = G.MLP(5, 5, hidden_dim=8, L=2).to(device)   # (kernel outputs are padded rows, as inside a stack)
    taps = []
    inner_apply = B._NodeTap.apply
    ei = torch.randint(0, N, (2, E), generator=gen).to(device)
    gi = ops.graph_index(ei, N, cache=False)
    x0 = torch.randn(N, 5, generator=gen)
    e0 = torch.randn(E, 4, generator=gen)
    rx, re = torch.randn(N, 5, generator=gen).to(device), torch.randn(E, 4, generator=gen).to(device)

    def run(flags_on, mode):
        B.TAP = B.FOLD_ADD = flags_on
        try:
            net.zero_grad()
            enc.zero_grad()
            for p_ in net.parameters():
                p_.requires_grad_(not (mode == "frozen_rel" and p_ in set(net.relational_model.parameters())))
            with G.bf16_storage(True):
                xin = B.to_rows16(x0.to(device)).requires_grad_(mode != "no_x_grad")
                ein = B.to_rows16(e0.to(device)).requires_grad_(True)
                with torch.set_grad_enabled(mode != "no_x_grad"):
                    x1 = enc(xin)
                xo, eo = net.forward_csr(gi, x1, ein, relu_in=True, residue=x1, alpha_residue=0.5)
                loss = (xo.float() * rx).sum() + (eo.float() * re).sum()
                if mode == "grad_x_only":
                    (gx,) = torch.autograd.grad(loss, [xin])
                    return {"x": gx.float().clone()}
                if mode == "twice":
                    loss.backward(retain_graph=True)
                    loss.backward()
                else:
                    loss.backward()
            out = {"e": ein.grad.float().clone()}
            if mode != "no_x_grad":
                out["x"] = xin.grad.float().clone()
            for k, v in list(net.named_parameters()) + [("enc." + k_, v_) for k_, v_ in enc.named_parameters()]:
                if v.grad is not None:
                    out[k] = v.grad.float().clone()
            return out
        finally:
            B.TAP = B.FOLD_ADD = True
            for p_ in net.parameters():
                p_.requires_grad_(True)

    def counting(*a):
        taps.append(1)
        return inner_apply(*a)

    for mode in ("all", "grad_x_only", "frozen_rel", "no_x_grad", "twice"):
        taps.clear()
        B._NodeTap.apply = counting
        try:
            on = run(True, mode)
        finally:
            B._NodeTap.apply = inner_apply
        assert len(taps) == (0 if mode == "no_x_grad" else 1), f"node_tap {mode}: tap taken {len(taps)} times"
        off = run(False, mode)
        assert on.keys() == off.keys(), f"node_tap {mode}: different gradients present {on.keys()} vs {off.keys()}"
        for k in on:
            scale = max(1.0, float(off[k].abs().max()))
            err = float((on[k] - off[k]).abs().max())
            # (both sides round bf16 sums; the fused side rounds once where autograd rounds two or three times)
            assert err <= 2.0 ** -6 * scale, f"node_tap {mode}: {k} differs by {err:.3e} (scale {scale:.3g})"


def case_fold_alias(device):
    """Gradient folds only merge gradients of ONE autograd tensor: two distinct autograd tensors that alias the same
    memory (``x`` and ``x.detach().requires_grad_()``) gathered by target and by source keep separate gradients, equal
    to the run in which the second one is a copy."""
    from gnn_tracking_amd import ops_bf16 as B
    gen = torch.Generator().manual_seed(7)
    N, E = 120, 900
    ei = torch.randint(0, N, (2, E), generator=gen).to(device)
    gi = ops.graph_index(ei, N, cache=False)
    mlp = G.MLP(14, 4, hidden_dim=40, L=3).to(device)
    lin = mlp.linears()
    x0 = torch.randn(N, 5, generator=gen).to(device)
    e0 = torch.randn(E, 4, generator=gen).to(device)
    grads = {}
    for alias in (True, False):
        with G.bf16_storage(True):
            xa = B.to_rows16(x0).requires_grad_(True)
            xb = (xa.detach() if alias else xa.detach().clone()).requires_grad_(True)
            ee = B.to_rows16(e0).requires_grad_(True)
            segs = [ops.Seg(xa, gi.tgt, False, ("tgt", gi)), ops.Seg(xb, gi.src, False, ("src", gi)), ops.Seg(ee)]
            out = ops.fused_mlp(segs, [m.weight for m in lin], [m.bias for m in lin], n_rows=E)
            out.float().square().sum().backward()
        assert xa.grad is not None and xb.grad is not None, "an aliased input lost its gradient"
        grads[alias] = (xa.grad.float().cpu(), xb.grad.float().cpu())
    assert torch.equal(grads[True][0], grads[False][0]) and torch.equal(grads[True][1], grads[False][1]), \
        "gradients of two aliasing autograd tensors were merged"


def case_hipgraph_capture(device):
    """The training step is capturable as a HIP graph (every gnntrk_* call is stream
    ordered, allocation- and sync-free); a replay reproduces the eager gradients bit for bit."""
    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y = tt(z["y"], device).float()
    name = "skip1_L3_h40"
    for bf16 in (False, True):
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        data = G.Data(x=x, edge_index=ei, edge_attr=ea)

        def step():
            ops.clear_graph_index_cache()
            for p_ in model.parameters():
                if p_.grad is not None:
                    p_.grad.zero_()
            with G.bf16_storage(bf16):
                out = model(data)
                loss = G.EdgeWeightBCELoss()(w=out["W"], y=y)
                loss.backward()
            return loss

        for _ in range(2):
            step()
        eager = {k: v.grad.clone() for k, v in model.named_parameters()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for p_ in model.parameters():
            p_.grad.fill_(7.0)  # must be overwritten by the replay
        g.replay()
        torch.cuda.synchronize()
        for k, v in model.named_parameters():
            assert torch.equal(v.grad, eager[k]), f"hipGraph replay differs from eager: {k} (bf16={bf16})"


# ------------------------------------------------ graph track-condensation network (8f-1)
GTCN_VARIANTS = {
    "test_cfg": dict(h_dim=2, hidden_dim=2, L_ec=2, L_hc=2),
    "default": dict(),
    "orphans_ecfeed": dict(L_ec=2, L_hc=2, hidden_dim=16, mask_orphan_nodes=True,
                           use_ec_embeddings_for_hc=True, feed_edge_weights=True),
    "latent": dict(L_ec=1, L_hc=2, hidden_dim=8, h_outdim=4, alpha_latent=0.4, n_embedding_coords=3),
    "hetero": dict(L_ec=1, L_hc=1, hidden_dim=12, mask_orphan_nodes=True, heterogeneous_node_encoder=True),
    "perfect_ec": dict(_cls="PerfectECGraphTCN", L_hc=2, hidden_dim=10, mask_orphan_nodes=True),
    "mlgc": dict(_cls="GraphTCNForMLGCPipeline", L_hc=1, hidden_dim=10),
    "all_cut": dict(L_ec=1, L_hc=2, hidden_dim=8, _thr=0.9995),  # threshold above every weight: no edge left
}


def make_gtcn(kw, thr):
    """(model, class name) of a G7 variant."""
    kw = dict(kw)
    cls = kw.pop("_cls", "GraphTCN")
    kw.pop("_thr", None)
    if cls == "GraphTCN":
        return G.GraphTCN(14, 4, ec_threshold=thr, **kw), cls
    return getattr(G, cls)(node_indim=14, edge_indim=4, ec_threshold=thr, **kw), cls


def gtcn_oracle_kwargs(kw, thr, y=None):
    okw = dict(L_ec=kw.get("L_ec", 3), L_hc=kw.get("L_hc", 3), ec_threshold=thr)
    if kw.get("_cls") == "PerfectECGraphTCN":
        okw.update(ec_kind="perfect", y=y)
    elif kw.get("_cls") == "GraphTCNForMLGCPipeline":
        okw.update(ec_kind="none")
    for k in ("mask_orphan_nodes", "feed_edge_weights", "use_ec_embeddings_for_hc", "alpha_latent",
              "n_embedding_coords", "heterogeneous_node_encoder"):
        if k in kw:
            okw[k] = kw[k]
    return okw


def case_graph_tcn(device, names=None):
    """GraphTCN (EC -> threshold cut -> orphan masking -> encoders -> ResIN -> beta / cluster
    heads) against the reference-generated golden G7: masks bit-exact, W/H/B 1e-5, gradients
    of sum(H rH) + sum(B rB) + BCE(W, y) 1e-4."""
    z = load("g7_graph_tcn.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y = tt(z["y"], device)
    for name, kw in GTCN_VARIANTS.items():
        if names is not None and name not in names:
            continue
        thr = float(z[f"{name}/ec_threshold"])
        model, cls = make_gtcn(kw, thr)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y, layer=tt(z["layer"], device)))
        if cls == "GraphTCNForMLGCPipeline":
            assert out["W"] is None and out["ec_edge_mask"] is None and out["ec_hit_mask"] is None
        else:
            assert torch.equal(out["ec_edge_mask"].cpu(), tt(z[f"{name}/ec_edge_mask"])), name + " edge mask"
            assert torch.equal(out["ec_hit_mask"].cpu(), tt(z[f"{name}/ec_hit_mask"])), name + " hit mask"
            assert_close(out["W"], z[f"{name}/W"], TOL_OUT, name + " W")
        assert_close(out["H"], z[f"{name}/H"], TOL_OUT, name + " H")
        assert_close(out["B"], z[f"{name}/B"], TOL_OUT, name + " B")
        loss = (out["H"] * tt(z[f"{name}/rH"], device)).sum() + (out["B"] * tt(z[f"{name}/rB"], device)).sum()
        if cls == "GraphTCN":
            loss = loss + G.EdgeWeightBCELoss()(w=out["W"], y=y.float())
        assert_close(loss, z[f"{name}/loss"], TOL_OUT, name + " loss")
        loss.backward()
        for k, v in model.named_parameters():
            gk = v.grad if v.grad is not None else torch.zeros_like(v)
            assert_close(gk, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")


def case_graph_tcn_bf16(device):
    """bf16 storage through the whole GraphTCN: runs, fp32 outputs, finite, every parameter
    with a path to the loss gets an fp32 gradient.  (No value comparison: the threshold cut
    can differ from the fp32 golden once W moves by a bf16-sized amount.)"""
    z = load("g7_graph_tcn.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y = tt(z["y"], device)
    for name, kw in GTCN_VARIANTS.items():
        if "_cls" in kw:
            continue  # (the wrappers without a learned edge classifier add nothing in this mode)
        all_cut = "_thr" in kw
        model, _ = make_gtcn(kw, float(z[f"{name}/ec_threshold"]))
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        with G.bf16_storage():
            out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y, layer=tt(z["layer"], device)))
            loss = out["H"].square().sum() + out["B"].sum() + G.EdgeWeightBCELoss()(w=out["W"], y=y.float())
            loss.backward()
        for k in ("W", "H", "B"):
            assert out[k].dtype == torch.float32 and torch.isfinite(out[k]).all(), f"{name} {k}"
        # (the golden thresholds sit inside a dense cluster of weights, so the kept fraction
        # itself moves with bf16 noise; it only has to stay a genuine cut)
        kept = out["ec_edge_mask"].float().mean().item()
        assert (kept == 0.0) if all_cut else (0.02 < kept < 0.98), f"{name}: cut keeps {kept:.2f} of the edges"
        for k, v in model.named_parameters():
            gref = tt(z[f"{name}/grad/{k}"])
            if gref.abs().max() > 0:
                assert v.grad is not None and v.grad.dtype == torch.float32 and torch.isfinite(v.grad).all(), k


GTCN_AUTOCAST_VARIANTS = {
    "default_nocut": dict(ec_threshold=0.0),
    "ecfeed_nocut": dict(L_ec=2, L_hc=2, hidden_dim=16, mask_orphan_nodes=True, use_ec_embeddings_for_hc=True,
                         feed_edge_weights=True, ec_threshold=0.0),
    "latent_nocut": dict(L_ec=1, L_hc=2, hidden_dim=8, h_outdim=4, alpha_latent=0.4, n_embedding_coords=3,
                         ec_threshold=0.0),
    "perfect_ec": dict(_cls="PerfectECGraphTCN", L_hc=2, hidden_dim=10, mask_orphan_nodes=True, ec_threshold=0.5),
    "mlgc": dict(_cls="GraphTCNForMLGCPipeline", L_hc=1, hidden_dim=10, ec_threshold=0.5),
}
GTCN16_PIN_H = 2.0 ** -6    # of the largest |H| entry
GTCN16_PIN_B = 2.0 ** -7    # beta in (0, 1): two bf16 ulps on [0.5, 1)
GTCN16_PIN_GRAD = 0.08      # relative L2 of a parameter gradient


def case_graph_tcn_bf16_autocast(device, names=None):
    """The bf16-storage GraphTCN PINNED AGAINST THE REFERENCE IN ITS OWN MIXED PRECISION (golden G7b:
    the reference's GraphTCN / PerfectECGraphTCN / GraphTCNForMLGCPipeline under CPU bf16 autocast;
    the learned threshold cut is off or replaced by the truth, so both sides see the same edges):
    masks equal, H within 2^-6 of the largest entry, beta within 2^-7, W within one bf16 ulp, every
    parameter gradient within 8 % relative L2 + 1.25 x the distance of the reference's autocast
    gradient to its own fp32 gradient (on 300 hits and hidden widths of 8 - 16 a single rounding
    moves a small gradient by tens of per cent; measured: the kernels sit at 1 - 3 % from the
    autocast reference where autocast itself sits at 6 - 20 % from fp32) + half a per cent of the
    whole gradient's norm.  Returns the measured distances."""
    z = load("g7b_graph_tcn_bf16_autocast.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, layer = tt(z["y"], device), tt(z["layer"], device)
    report = {}
    for name, kw in GTCN_AUTOCAST_VARIANTS.items():
        if names is not None and name not in names:
            continue
        kw = dict(kw)
        thr = kw.pop("ec_threshold")
        model, cls = make_gtcn(kw, thr)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        with G.bf16_storage():
            out = model(G.Data(x=x, edge_index=ei, edge_attr=ea, y=y, layer=layer))
            loss = (out["H"].float() * tt(z[f"{name}/rH"], device)).sum() + (out["B"].float() * tt(z[f"{name}/rB"], device)).sum()
            if cls == "GraphTCN":
                loss = loss + G.EdgeWeightBCELoss()(w=out["W"], y=y.float())
            loss.backward()
        rep = report.setdefault(name, {})
        for k in ("ec_hit_mask", "ec_edge_mask"):
            if f"{name}/{k}" in z.files:
                assert torch.equal(out[k].cpu(), tt(z[f"{name}/{k}"])), f"{name} {k}"
        href = tt(z[f"{name}/H"])
        rep["H"] = ((out["H"].detach().float().cpu() - href).abs().max() / max(1.0, href.abs().max().item())).item()
        rep["B"] = (out["B"].detach().float().cpu() - tt(z[f"{name}/B"])).abs().max().item()
        if cls == "GraphTCN":
            rep["W"] = (out["W"].detach().float().cpu() - tt(z[f"{name}/W"])).abs().max().item()
            assert rep["W"] <= BF16_PIN_W, (name, rep)
        want_all = math.sqrt(sum(float(tt(z[f"{name}/grad/{k}"]).double().pow(2).sum()) for k, _ in model.named_parameters()))
        worst = 0.0
        for k, v in model.named_parameters():
            gref = tt(z[f"{name}/grad/{k}"]).double()
            if v.grad is None:
                assert gref.abs().max().item() == 0.0, f"{name} grad {k} missing"
                continue
            err = (v.grad.detach().cpu().double() - gref).norm().item()
            own = (gref - tt(z[f"{name}/grad_fp32/{k}"]).double()).norm().item()   # autocast's own distance to fp32
            assert err <= GTCN16_PIN_GRAD * gref.norm().item() + 1.25 * own + 0.005 * want_all, \
                f"{name} grad {k}: {err:.3e} of {gref.norm().item():.3e} (autocast - fp32: {own:.3e})"
            if gref.norm().item() > 0.02 * want_all:
                worst = max(worst, err / gref.norm().item())
        rep["grad_rel_l2"] = worst
        assert rep["H"] <= GTCN16_PIN_H and rep["B"] <= GTCN16_PIN_B, (name, rep)
    return report


def case_hinge_loss(device, cases=("td1", "td4")):
    """GraphConstructionHingeEmbeddingLoss vs the reference (G8: the reference's pinned td1
    values re-run in fp32, and a two-event case), loss terms, edge counts and grad wrt x."""
    z = load("g8_hinge.npz")
    for cn in cases:
        t = {k: tt(z[f"{cn}/{k}"]) for k in ("x", "particle_id", "pt", "eta", "reconstructable", "batch",
                                              "true_edge_index")}
        for norm in ("n_hits_oi", "n_rep_edges"):
            x = t["x"].float().to(device).requires_grad_(True)
            ret = G.GraphConstructionHingeEmbeddingLoss(rep_normalization=norm, lw_repulsive=0.7)(
                x=x, particle_id=t["particle_id"].to(device), batch=t["batch"].to(device),
                true_edge_index=t["true_edge_index"].to(device), pt=t["pt"].float().to(device),
                eta=t["eta"].float().to(device), reconstructable=t["reconstructable"].float().to(device))
            assert ret.extra_metrics["n_edges_rep"] == int(z[f"{cn}/{norm}/n_edges_rep"]), f"{cn} edge count"
            for k in ("attractive", "repulsive"):
                assert_close(ret.loss_dct[k], z[f"{cn}/f32/{norm}/{k}"], TOL_OUT, f"{cn} {norm} {k}")
            assert_close(ret.loss, z[f"{cn}/f32/{norm}/total"], TOL_OUT, f"{cn} {norm} total")
            ret.loss.backward()
            assert_close(x.grad, z[f"{cn}/f32/{norm}/grad_x"], 2e-4, f"{cn} {norm} grad x")


def case_gc_fcnn(device, names=("d1_h40", "d4_h96")):
    """GraphConstructionFCNN vs the reference (G9): depth 1 on the fused kernel, depth 4 /
    hidden 96 on the library GEMM path."""
    z = load("g9_gc_fcnn.npz")
    x = tt(z["x"], device)
    for name, kw in {"d1_h40": dict(hidden_dim=40, depth=1, out_dim=8),
                     "d4_h96": dict(hidden_dim=96, depth=4, out_dim=8, alpha=0.6)}.items():
        if name not in names:
            continue
        model = G.GraphConstructionFCNN(in_dim=14, **kw)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        out = model(G.Data(x=x))["H"]
        assert_close(out, z[f"{name}/H"], TOL_OUT, name + " H")
        (out * tt(z[f"{name}/r"], device)).sum().backward()
        for k, v in model.named_parameters():
            assert_close(v.grad, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")


def case_res_fcnn(device, shapes=None, rows=(1, 16, 45, 130)):
    """``ops_ml.res_fcnn`` (gnntrk_resfcnn_forward / _backward: the whole residual FCNN of models/mlp.py:65-120
    in one launch each) against the reference's formula in float64, over depths 1 .. 6, hidden widths on both
    sides of every tile count (10 .. 128), with and without biases, the output scale, the ReLU epilogue, row
    counts off the tile size, and the gradient w.r.t. the (normalised) input."""
    from gnn_tracking_amd import ops_ml
    gen = torch.Generator().manual_seed(7)
    shapes = shapes or [(14, 10, 8, 2, 0.6, False), (14, 40, 8, 1, 0.6, True), (7, 64, 12, 3, 0.3, True),
                        (30, 33, 5, 2, 0.0, False), (14, 96, 8, 4, 0.6, False), (64, 128, 32, 6, 0.5, True),
                        (3, 17, 1, 2, 1.0, True), (20, 80, 24, 3, 0.7, False),
                        (19, 16, 5, 1, 0.6, True), (64, 12, 32, 2, 0.5, False), (40, 30, 20, 3, 0.4, True)]
    worst = 0.0
    for (din, hid, dout, depth, alpha, bias) in shapes:
        for n in rows:
            for out_relu, use_scale in ((False, True), (True, False)):
                ws = [torch.randn(hid, din, generator=gen) / din ** 0.5] + \
                     [torch.randn(hid, hid, generator=gen) * (2 / hid) ** 0.5 for _ in range(depth - 1)] + \
                     [torch.randn(dout, hid, generator=gen) * (2 / hid) ** 0.5]
                bs = [torch.randn(w.shape[0], generator=gen) * 0.3 if bias else None for w in ws]
                x = torch.randn(n, din, generator=gen) * 2
                if n > 2:
                    x[1] = 0   # a zero row: the eps branch of the normalisation
                scale = torch.tensor([1.7]) if use_scale else None
                r = torch.randn(n, dout, generator=gen)

                def ref():
                    xs = x.double().requires_grad_(True)
                    W = [w.double().requires_grad_(True) for w in ws]
                    B = [None if b is None else b.double().requires_grad_(True) for b in bs]
                    sc = None if scale is None else scale.double().requires_grad_(True)
                    lin = lambda h, i: h @ W[i].t() + (0 if B[i] is None else B[i])  # noqa: E731
                    h = lin(torch.nn.functional.normalize(xs, p=2.0, dim=1, eps=1e-12), 0)
                    for i in range(1, depth):
                        h = math.sqrt(alpha) * h + math.sqrt(1 - alpha) * lin(torch.relu(h), i)
                    y = lin(torch.relu(h), depth)
                    if sc is not None:
                        y = y * sc
                    if out_relu:
                        y = torch.relu(y)
                    (y * r.double()).sum().backward()
                    return y, xs.grad, [w.grad for w in W], [None if b is None else b.grad for b in B], None if sc is None else sc.grad

                xd = x.clone().to(device).requires_grad_(True)
                Wd = [w.clone().to(device).requires_grad_(True) for w in ws]
                Bd = [None if b is None else b.clone().to(device).requires_grad_(True) for b in bs]
                sd = None if scale is None else scale.clone().to(device).requires_grad_(True)
                y = ops_ml.res_fcnn(xd, Wd, Bd, alpha=alpha, normalize=True, out_relu=out_relu, scale=sd)
                (y * r.to(device)).sum().backward()
                yr, gxr, gWr, gBr, gsr = ref()
                tag = f"res_fcnn in {din} hidden {hid} out {dout} depth {depth} alpha {alpha} bias {bias} rows {n} relu {out_relu}"
                assert_close(y, yr, TOL_OUT, tag + " y")
                assert_close(xd.grad, gxr, TOL_GRAD, tag + " grad x")
                for i, (a, b) in enumerate(zip(Wd, gWr)):
                    assert_close(a.grad, b, TOL_GRAD, tag + f" grad W{i}")
                    worst = max(worst, float((a.grad.cpu().double() - b).abs().max() / max(1.0, float(b.abs().max()))))
                for i, (a, b) in enumerate(zip(Bd, gBr)):
                    if a is not None:
                        assert_close(a.grad, b, TOL_GRAD, tag + f" grad b{i}")
                if sd is not None:
                    assert_close(sd.grad, gsr, TOL_GRAD, tag + " grad scale")
    # two runs are bit-identical (fixed-order partial sums)
    y2 = ops_ml.res_fcnn(xd.detach().requires_grad_(True), Wd, Bd, alpha=alpha, normalize=True, out_relu=out_relu, scale=sd)
    assert torch.equal(y2, y)
    return worst


def case_mlp_wide(device, rows=(1, 16, 45, 130), shapes=None):
    """``ops.fused_mlp`` on the wide fp32 kernels (gnntrk_mlp_forward_wide / _backward_wide: in <= 128, hidden <= 128,
    out <= 48) against the reference's MLP (models/mlp.py:18-62) on the gathered concatenation in float64: gathered
    and identity segments, ReLU on load, two and three layers, with and without biases, the three epilogues,
    every tile count on both sides of the limits."""
    gen = torch.Generator().manual_seed(13)
    shapes = shapes or [((40, 40, 40), 40, 40, 3, True), ((40, 40), 40, 40, 3, True), ((14,), 40, 40, 2, False),
                        ((20, 20, 9), 64, 17, 3, True), ((50, 50, 28), 128, 48, 3, True), ((5, 5, 4), 100, 4, 3, False),
                        ((64, 64), 16, 33, 2, True), ((30,), 96, 1, 3, True)]
    for dims, hid, dout, L, bias in shapes:
        din = sum(dims)
        for n in rows:
            for epi in (_capi.EPI_NONE, _capi.EPI_RELU, _capi.EPI_RESIDUAL):
                n_src = max(7, n // 3)
                srcs = [torch.randn(n_src if j < len(dims) - 1 else n, d, generator=gen) for j, d in enumerate(dims)]
                idxs = [torch.randint(0, n_src, (n,), generator=gen).int() if j < len(dims) - 1 else None
                        for j in range(len(dims))]
                relu = [bool((j + n) % 2) for j in range(len(dims))]
                sizes = [din] + [hid] * (L - 1) + [dout]
                ws = [torch.randn(sizes[i + 1], sizes[i], generator=gen) / sizes[i] ** 0.5 for i in range(L)]
                bs = [torch.randn(sizes[i + 1], generator=gen) * 0.3 if bias else None for i in range(L)]
                res = torch.randn(n, dout, generator=gen)
                r = torch.randn(n, dout, generator=gen)
                ca, cb = 0.6, 0.8

                def run(dev, dt):
                    S = [t.clone().to(dev, dt).requires_grad_(True) for t in srcs]
                    W = [w.clone().to(dev, dt).requires_grad_(True) for w in ws]
                    B = [None if b is None else b.clone().to(dev, dt).requires_grad_(True) for b in bs]
                    R = res.clone().to(dev, dt).requires_grad_(True)
                    if dt == torch.float64:
                        cols = []
                        for t, ix, rl in zip(S, idxs, relu):
                            t2 = torch.relu(t) if rl else t
                            cols.append(t2 if ix is None else t2[ix.long()])
                        h = torch.cat(cols, dim=1)
                        for i in range(L):
                            h = h @ W[i].t() + (0 if B[i] is None else B[i])
                            if i < L - 1:
                                h = torch.relu(h)
                        y = torch.relu(h) if epi == _capi.EPI_RELU else (ca * R + cb * h if epi == _capi.EPI_RESIDUAL else h)
                    else:
                        segs = [ops.Seg(t, None if ix is None else ix.to(dev), rl,
                                        None if ix is None else _IndexReduce(ix.to(dev), int(t.shape[0])))
                                for t, ix, rl in zip(S, idxs, relu)]
                        y = ops.fused_mlp(segs, W, B, n_rows=n, epilogue=epi, ca=ca, cb=cb,
                                          res=R if epi == _capi.EPI_RESIDUAL else None)
                    (y * r.to(dev, dt)).sum().backward()
                    return y, S, W, B, R

                ops._WIDE_WARNED.clear()
                y, S, W, B, R = run(device, torch.float32)
                assert not ops._WIDE_WARNED, f"library path taken: {ops._WIDE_WARNED}"
                yr, Sr, Wr, Br, Rr = run("cpu", torch.float64)
                tag = f"mlp_wide in {dims} hidden {hid} out {dout} L {L} bias {bias} rows {n} epilogue {epi}"
                assert_close(y, yr, TOL_OUT, tag + " y")
                for j, (a, b) in enumerate(zip(S, Sr)):
                    assert_close(a.grad, b.grad, TOL_GRAD, tag + f" grad seg {j}")
                for i, (a, b) in enumerate(zip(W, Wr)):
                    assert_close(a.grad, b.grad, TOL_GRAD, tag + f" grad W{i}")
                for i, (a, b) in enumerate(zip(B, Br)):
                    if a is not None:
                        assert_close(a.grad, b.grad, TOL_GRAD, tag + f" grad b{i}")
                if epi == _capi.EPI_RESIDUAL:
                    assert_close(R.grad, Rr.grad, TOL_GRAD, tag + " grad res")


def case_in_edge_wide(device, sizes=((60, 700), (9, 1), (300, 4000))):
    """One interaction-network layer (interaction_network.py:67-89) at the widths of the wide fp32 kernels - the
    relational model and its sum aggregation as one autograd node (ops.in_edge_wide) - against the same layer
    in float64 torch: node and edge outputs, and all gradients with the edge embedding read by a second
    consumer, by the aggregation only, and by neither the aggregation's consumer (upstream terms: both / the
    gathered one / the direct one)."""
    from gnn_tracking_amd.interaction_network import InteractionNetwork
    gen = torch.Generator().manual_seed(21)
    calls, inner = [], ops.in_edge_wide

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    ops.in_edge_wide = counted
    try:
        _in_edge_wide_body(device, sizes, gen)
    finally:
        ops.in_edge_wide = inner
    assert len(calls) == 6 * len(sizes), "the fused relational + aggregation node was not the path taken"


def _in_edge_wide_body(device, sizes, gen):
    from gnn_tracking_amd.interaction_network import InteractionNetwork
    for (N, E), (dn, de, eo, no) in [(sz, w) for sz in sizes for w in ((40, 40, 40, 40), (24, 17, 33, 8))]:
        net = InteractionNetwork(node_indim=dn, edge_indim=de, node_outdim=no, edge_outdim=eo)
        ref = InteractionNetwork(node_indim=dn, edge_indim=de, node_outdim=no, edge_outdim=eo).double()
        ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        net = net.to(device)
        ei = torch.randint(0, N, (2, E), generator=gen)
        x0, e0 = torch.randn(N, dn, generator=gen), torch.randn(E, de, generator=gen)
        rx, re = torch.randn(N, no, generator=gen), torch.randn(E, eo, generator=gen)
        for use_x, use_e in ((True, True), (True, False), (False, True)):
            net.zero_grad()
            ref.zero_grad()
            x = x0.clone().to(device).requires_grad_(True)
            e = e0.clone().to(device).requires_grad_(True)
            ops._WIDE_WARNED.clear()
            xo, eo_ = net(x, ei.to(device), e)
            assert not ops._WIDE_WARNED, f"library path taken: {ops._WIDE_WARNED}"
            xr_in, er_in = x0.clone().double().requires_grad_(True), e0.clone().double().requires_grad_(True)
            src, tgt = ei[0], ei[1]

            def chain(m, h):   # models/mlp.py:18-62 as torch ops
                lin = m.linears()
                for i, l in enumerate(lin):
                    h = torch.nn.functional.linear(h, l.weight, l.bias)
                    if i < len(lin) - 1:
                        h = torch.relu(h)
                return h

            er = chain(ref.relational_model, torch.cat([xr_in[tgt], xr_in[src], er_in], dim=1))
            aggr = torch.zeros(N, eo, dtype=torch.float64).index_add(0, tgt, er)
            xr = chain(ref.object_model, torch.cat([xr_in, aggr], dim=1))
            tag = f"in_edge_wide N={N} E={E} widths {(dn, de, eo, no)} x {use_x} e {use_e}"
            assert_close(xo, xr, TOL_OUT, tag + " x~")
            assert_close(eo_, er, TOL_OUT, tag + " e~")
            loss = 0
            loss_r = 0
            if use_x:
                loss, loss_r = loss + (xo * rx.to(device)).sum(), loss_r + (xr * rx.double()).sum()
            if use_e:
                loss, loss_r = loss + (eo_ * re.to(device)).sum(), loss_r + (er * re.double()).sum()
            loss.backward()
            loss_r.backward()
            assert_close(x.grad, xr_in.grad, TOL_GRAD, tag + " grad x")
            assert_close(e.grad, er_in.grad, TOL_GRAD, tag + " grad e")
            pr = dict(ref.named_parameters())
            for k, v in net.named_parameters():
                if use_x or k.startswith("relational_model"):
                    assert_close(v.grad, pr[k].grad, TOL_GRAD, tag + f" grad {k}")


class _IndexReduce(tuple):
    """A ``("tgt", index)`` reduce rule for a plain row gather (test helper): row pointers of the stable sort of
    ``idx`` stand in for a graph index, so that the fold is the package's own segment sum."""

    def __new__(cls, idx, n_src):
        order = torch.argsort(idx.long(), stable=True)
        rowptr = torch.zeros(n_src + 1, dtype=torch.int32, device=idx.device)
        rowptr[1:] = torch.cumsum(torch.bincount(idx.long(), minlength=n_src), 0).int()

        class _GI:
            pass
        gi = _GI()
        gi.rowptr_s, gi.spos, gi.rowptr_t = rowptr, order.int().contiguous(), None
        return super().__new__(cls, ("src", gi))


def case_hinge_terms(device, n=400, dim=8, n_edges=3000):
    """``ops_ml.hinge_terms`` (gnntrk_hinge_forward / _backward) against the reference's expressions
    (metric_learning.py:14-55 with the edge selection of :88-110) in torch: every selection mode, powers 1 / 2 /
    0.5 / 3, the three normalisations, an empty selection, duplicate and self edges."""
    from gnn_tracking_amd import ops_ml
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(n, dim, generator=gen) * 0.4)
    pid = torch.randint(0, 40, (n,), generator=gen)
    mask = torch.rand(n, generator=gen) > 0.3
    edges = torch.randint(0, n, (2, n_edges), generator=gen)
    edges[:, :5] = edges[:, 5:10]          # duplicates
    edges[1, 10:14] = edges[0, 10:14]      # self edges: d = 0
    norm_t = torch.tensor(123.0)
    for rep in (False, True):
        for p in (1.0, 2.0, 0.5, 3.0):
            for use_mask, use_pid, norm in ((True, False, None), (False, True, norm_t), (True, True, None), (False, False, None)):
                xr = x.double().requires_grad_(True)
                keep = torch.ones(n_edges, dtype=torch.bool)
                if use_mask:
                    keep &= mask[edges[0]]
                if use_pid:
                    keep &= pid[edges[0]] != pid[edges[1]]
                e = edges[:, keep]
                d = torch.linalg.norm(xr[e[0]] - xr[e[1]], dim=-1)
                terms = torch.relu(0.9 - torch.pow(d, p)) if rep else torch.pow(d, p)
                den = (float(norm) if norm is not None else e.shape[1]) + 1e-9
                lr = terms.sum() / den
                lr.backward()
                xd = x.clone().to(device).requires_grad_(True)
                l, cnt, dn = ops_ml.hinge_terms(xd, edges.to(device), node_mask=mask.to(device) if use_mask else None,
                                                particle_id=pid.to(device) if use_pid else None,
                                                norm=None if norm is None else norm.to(device), r_emb=0.9, p=p, repulsive=rep)
                tag = f"hinge rep {rep} p {p} mask {use_mask} pid {use_pid}"
                assert int(cnt) == e.shape[1], tag
                assert_close(l, lr, TOL_OUT, tag + " loss")
                (l * 1.5).backward()
                g_ref = xr.grad * 1.5
                if p < 1.0:   # (d^(p-1) is unbounded near d = 0: compare where the reference itself is finite)
                    ok = torch.isfinite(g_ref).all(dim=1)
                    assert_close(xd.grad.cpu()[ok], g_ref[ok], TOL_GRAD, tag + " grad")
                else:
                    assert_close(xd.grad, g_ref, TOL_GRAD, tag + " grad")
    # other dtypes of the selection inputs (the reference's indexing takes any integer ids / any mask): int32 particle
    # ids and a float mask select the same edges as int64 / bool; wrong sizes and float ids are refused
    xd = x.clone().to(device)
    ref_l, ref_c, _ = ops_ml.hinge_terms(xd, edges.to(device), node_mask=mask.to(device), particle_id=pid.to(device),
                                         r_emb=0.9, repulsive=True)
    for pid_t, mask_t in ((pid.to(torch.int32), mask), (pid, mask.float()), (pid.to(torch.int16), mask.to(torch.uint8))):
        l, cnt, _ = ops_ml.hinge_terms(xd, edges.to(device), node_mask=mask_t.to(device), particle_id=pid_t.to(device),
                                       r_emb=0.9, repulsive=True)
        assert int(cnt) == int(ref_c) and float(l) == float(ref_l), f"hinge: dtypes {pid_t.dtype} / {mask_t.dtype}"
    for bad in (dict(particle_id=pid[:-1].to(device)), dict(node_mask=mask[:-1].to(device)),
                dict(particle_id=pid.float().to(device))):
        try:
            ops_ml.hinge_terms(xd, edges.to(device), **bad)
        except (ValueError, TypeError):
            pass
        else:
            raise AssertionError(f"hinge: accepted {list(bad)} of the wrong size / dtype")
    # nothing selected: 0 / 1e-9 = 0, zero gradient
    xd = x.clone().to(device).requires_grad_(True)
    l, cnt, _ = ops_ml.hinge_terms(xd, edges.to(device), node_mask=torch.zeros(n, dtype=torch.bool, device=device))
    l.backward()
    assert float(l) == 0.0 and int(cnt) == 0 and float(xd.grad.abs().max()) == 0.0
    l, cnt, _ = ops_ml.hinge_terms(xd, edges[:, :0].to(device))
    assert float(l) == 0.0 and int(cnt) == 0


HETERO_CASES = {
    "hetero_d2": ("GraphConstructionHeteroResFCNN", dict(hidden_dim=40, depth=2, out_dim=8, alpha=0.0)),
    "hetero_d3": ("GraphConstructionHeteroResFCNN", dict(hidden_dim=48, depth=3, out_dim=6, alpha=0.6)),
    "heteroenc": ("GraphConstructionHeteroEncResFCNN",
                  dict(hidden_dim_enc=24, hidden_dim=32, out_dim=8, depth_enc=2, depth=3, alpha=0.6)),
}


def case_pc_transformer(device):
    """MLPCTransformer(GraphConstructionFCNN): data.x becomes the reference's latent space H
    (G9), optionally followed by the original features; the model is frozen."""
    z = load("g9_gc_fcnn.npz")
    x = tt(z["x"], device)
    ml = G.GraphConstructionFCNN(in_dim=14, hidden_dim=40, depth=1, out_dim=8)
    load_params(ml, z, "d1_h40/p0/")
    for orig in (False, True):
        tr = G.MLPCTransformer(ml.to(device), original_features=orig)
        assert all(not p.requires_grad for p in tr.parameters())
        d = tr(G.Data(x=x.clone()))
        assert d.x.shape[1] == (8 + 14 if orig else 8)
        assert_close(d.x[:, :8], z["d1_h40/H"], TOL_OUT, "latent space")
        if orig:
            assert torch.equal(d.x[:, 8:], x)


def case_hetero_fcnn(device, names=None):
    """Pixel / strip embedding networks vs the reference (G10): depth 2 with alpha 0 is one
    fused three-layer launch per detector part, the others run on the library GEMM path."""
    z = load("g10_hetero_fcnn.npz")
    x, layer = tt(z["x"], device), tt(z["layer"], device)
    for name, (cls, kw) in HETERO_CASES.items():
        if names is not None and name not in names:
            continue
        model = getattr(G, cls)(in_dim=14, **kw)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        out = model(G.Data(x=x, layer=layer))["H"]
        assert_close(out, z[f"{name}/H"], TOL_OUT, name + " H")
        (out * tt(z[f"{name}/r"], device)).sum().backward()
        for k, v in model.named_parameters():
            assert_close(v.grad, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")


def case_graph_cut(device, sizes=(0, 1, 63, 2048, 2049, 5000), big=0):
    """gnntrk_threshold_compact / gnntrk_connected_nodes vs the oracle (bit-exact): empty,
    single, tile-boundary and ragged sizes, all / none kept, NaN weights, isolated nodes,
    self loops and duplicate edges; ``big`` adds a size that needs a multi-chunk count scan."""
    from gnn_tracking_amd import graph_cut

    g = np.random.default_rng(21)
    for n in tuple(sizes) + ((big,) if big else ()):
        w = torch.from_numpy(g.random(n).astype(np.float32))
        if n > 10:
            w[3] = float("nan")
            w[n - 1] = 0.5  # exactly the threshold: not kept (strict >)
        for thr in (0.5, -1.0, 2.0):
            mask, idx = graph_cut.threshold_compact(w.to(device), thr)
            om, oi = O.threshold_compact(w, thr)
            assert torch.equal(mask.cpu(), om), f"mask n={n} thr={thr}"
            assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), oi), f"idx n={n} thr={thr}"
        if n > 1:  # a view that is not 16-byte aligned takes the item-by-item loads
            mask, idx = graph_cut.threshold_compact(w.to(device)[1:], 0.5)
            om, oi = O.threshold_compact(w[1:], 0.5)
            assert torch.equal(mask.cpu(), om) and torch.equal(idx.cpu().long(), oi), f"unaligned view n={n}"
    for n_nodes, n_edges in ((1, 0), (5, 3), (300, 150), (2049, 700), (6000, 9000)) + (((big, big // 3),) if big else ()):
        ei = torch.from_numpy(g.integers(0, max(1, n_nodes // 2 * 2 - n_nodes // 3), size=(2, n_edges))).long()
        if n_edges > 2:
            ei[:, 1] = ei[:, 0]          # duplicate edge
            ei[1, 2] = ei[0, 2]          # self loop
        hit, node_idx, ei2 = graph_cut.connected_nodes(ei.to(device), n_nodes)
        oh, oc, oe = O.connected_nodes(ei, n_nodes)
        assert torch.equal(hit.cpu(), oh), f"hit mask N={n_nodes}"
        assert torch.equal(node_idx.cpu().long(), oc), f"connected nodes N={n_nodes}"
        assert ei2.dtype == torch.int64 and torch.equal(ei2.cpu(), oe), f"relabelled edge_index N={n_nodes}"
    try:
        graph_cut.connected_nodes(torch.tensor([[0, 7], [1, 2]], device=device), 5)
    except ValueError:
        pass
    else:
        raise AssertionError("out-of-range node id not reported")
    # the container-level operations against Data.edge_subgraph / Data.subgraph
    n_nodes, n_edges = 400, 1500
    ei = torch.from_numpy(g.integers(0, 250, size=(2, n_edges))).long()
    d = G.Data(x=torch.randn(n_nodes, 3), edge_index=ei, edge_attr=torch.randn(n_edges, 2),
               y=torch.randint(0, 2, (n_edges,)), edge_weights=torch.rand(n_edges, 1),
               particle_id=torch.arange(n_nodes)).to(device)
    cut, mask = graph_cut.edge_cut(d, d.edge_weights, 0.6)
    ref = d.edge_subgraph((d.edge_weights > 0.6).squeeze())
    for k in ("edge_index", "edge_attr", "y", "edge_weights"):
        assert torch.equal(getattr(cut, k), getattr(ref, k)), k
    assert torch.equal(cut.x, d.x)
    sub, hit = graph_cut.drop_orphans(cut)
    ref2 = ref.subgraph(ref.edge_index.flatten().unique())
    for k in ("edge_index", "edge_attr", "y", "x", "particle_id"):
        assert torch.equal(getattr(sub, k), getattr(ref2, k)), k
    assert int(hit.sum()) == sub.num_nodes


DBSCAN_TRIALS = ((1.0, 1), (0.5, 2), (0.3, 3), (0.2, 5), (0.11, 4), (0.45, 6))


def case_dbscan(device, clouds=("d2", "d3", "d8"), trials=DBSCAN_TRIALS, extras=True):
    """DBSCANFastRescan vs the labels of the reference's own class (G11, bit-exact) and the
    neighbourhood graph vs the oracle (ids exact, fp64 distances exact); rescan beyond
    max_eps; empty / single-point / all-noise inputs."""
    from gnn_tracking_amd.postprocessing import DBSCANFastRescan, dbscan

    z = load("g11_dbscan.npz")
    for cn in clouds:
        x = z[f"{cn}/x"]
        fr = DBSCANFastRescan(tt(x, device), max_eps=1.0)
        off, nbr, dist = O.radius_neighbors(x, 1.0)
        assert np.array_equal(fr._off.cpu().numpy(), off), cn + " offsets"
        assert np.array_equal(fr._nbr.cpu().numpy()[:len(nbr)].astype(np.int64), nbr), cn + " neighbours"
        assert np.array_equal(fr._dist.cpu().numpy()[:len(dist)], dist), cn + " distances (fp64)"
        for eps, mp in trials:
            lab = fr.cluster(eps, mp)
            assert lab.dtype == np.intp
            assert np.array_equal(lab, z[f"{cn}/eps{eps}_mp{mp}"]), f"DBSCAN {cn} eps={eps} min_pts={mp}"
        assert np.array_equal(fr.cluster(1.3, 3), z[f"{cn}/eps1.3_mp3"]), cn + " rescan beyond max_eps"
    if not extras:
        return
    one = torch.zeros(1, 3)
    assert dbscan(one.to(device), 0.5, 1).tolist() == [0] and dbscan(one.to(device), 0.5, 2).tolist() == [-1]
    assert dbscan(torch.zeros(0, 3).to(device), 0.5, 1).shape == (0,)
    # a long chain: the component's lowest index has to travel along every link
    chain = torch.stack([torch.arange(300, dtype=torch.float32).flip(0) * 0.9, torch.zeros(300)], 1)
    assert np.array_equal(dbscan(chain.to(device), 1.0, 2), O.dbscan_labels(chain.numpy(), 1.0, 1.0, 2))


def case_dbscan_pruned(device, clouds=("d2", "d3", "d8"), trials=DBSCAN_TRIALS, n_big=0, extras=True):
    """The pruned radius graph (sorted chunks, box-to-box bound, lists re-ordered) forced on: the same
    golden / oracle comparisons as the brute-force graph, and (n_big) pruned == brute force on a
    clustered cloud with noise incl. a list longer than the ordering kernel's LDS path."""
    from gnn_tracking_amd import postprocessing, synthetic

    old = postprocessing.RADIUS_FLAGS
    try:
        postprocessing.RADIUS_FLAGS = 1
        case_dbscan(device, clouds=clouds, trials=trials, extras=extras)
        for dim_c in ((8, 12) if n_big else ()):
            x = synthetic.make_pileup_cloud(3, n_big, dim_c)
            x[:1500] = x[0] + 0.001 * torch.randn(1500, dim_c)      # one neighbourhood of > 1024 points
            res = {}
            for flags in (1, 2):
                postprocessing.RADIUS_FLAGS = flags
                fr = postprocessing.DBSCANFastRescan(x.to(device), max_eps=0.4)
                res[flags] = (fr._off.cpu(), fr._nbr[:fr._n_edges].cpu(), fr._dist[:fr._n_edges].cpu(),
                              fr.cluster(0.3, 3))
            assert torch.equal(res[1][0], res[2][0]), "pruned radius graph: offsets"
            assert torch.equal(res[1][1], res[2][1]), "pruned radius graph: neighbours"
            assert torch.equal(res[1][2], res[2][2]), "pruned radius graph: distances"
            assert np.array_equal(res[1][3], res[2][3]), "pruned radius graph: labels"
    finally:
        postprocessing.RADIUS_FLAGS = old


def case_workspace_exact(device):
    """Every workspace of the sorted-chunk units (csrc/knn.hip, dbscan.hip, oc.hip) at exactly the size its
    gnntrk_*_workspace_bytes function states, through the raw C entries: the results equal those of a call with a
    megabyte to spare bit for bit, 4096 guard bytes behind the stated size stay as they were, and one byte less is
    refused with GNNTRK_EINVAL before anything is launched (the outputs keep their fill).  Shapes: the smallest with
    more than one chunk of 64 and a partial last one, one per padded width."""
    import ctypes as C

    lib = _capi.load()
    EINVAL, GUARD, ROOM = 1, 4096, 1 << 20
    gen = torch.Generator().manual_seed(11)

    def fresh(shape, dtype):   # an output no kernel has written: every byte 0xEE
        numel = int(np.prod(shape)) if shape else 1
        return torch.full((numel * torch.empty((), dtype=dtype).element_size(),), 0xEE, dtype=torch.uint8,
                          device=device).view(dtype).reshape(shape)

    def raw(t):
        return t.contiguous().view(torch.uint8).cpu()

    def check(what, sizes, run):
        """run([(buffer, stated bytes), ...]) -> (return code, outputs made by fresh())"""
        assert all(s > 0 for s in sizes), f"{what}: workspace sizes {sizes}"

        def buffers(extra, short=None):
            return [(torch.full((s + extra,), 0xA5, dtype=torch.uint8, device=device), s - (1 if i == short else 0))
                    for i, s in enumerate(sizes)]

        rc, want = run([(t, t.numel()) for t, _ in buffers(ROOM)])
        assert rc == 0, f"{what} (roomy): {lib.gnntrk_last_error()}"
        exact = buffers(GUARD)
        rc, got = run(exact)
        assert rc == 0, f"{what} (exact): {lib.gnntrk_last_error()}"
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(raw(a), raw(b)), f"{what}: output {i} differs between the exact and the roomy workspace"
        for (t, s) in exact:
            assert bool((t[s:] == 0xA5).all()), f"{what}: wrote behind its {s} bytes"
        for i in range(len(sizes)):
            rc, outs = run(buffers(GUARD, short=i))
            assert rc == EINVAL, f"{what}: workspace {i} one byte short returned {rc}"
            for o in outs:
                assert bool((raw(o) == 0xEE).all()), f"{what}: an output was written although the call was refused"
        return want

    # ---- pruned k-NN search (flag 1: pruned form forced)
    n = 130
    for dim, k in ((3, 4), (8, 16), (12, 4)):
        x = torch.randn(n, dim, generator=gen).to(device)
        st = ops._stream(x)

        def run_knn(ws):
            nbr, cnt = fresh((n, k), torch.int32), fresh((n,), torch.int32)
            return lib.gnntrk_knn_search_ws(ops._p(x), n, dim, dim, k, 0.0, None, 0, ops._p(nbr), ops._p(cnt),
                                            ops._p(ws[0][0]), ws[0][1], 1, st), (nbr, cnt)

        _, cnt = check(f"knn_search_ws dim={dim} k={k}", [int(lib.gnntrk_knn_workspace_bytes(n, dim, k))], run_knn)
        assert int(cnt.min()) == k, "fewer than k neighbours found"

    # ---- pruned radius graph (points and edges workspaces) and the DBSCAN labels on it
    for dim in (3, 8, 12):
        x = (0.5 * torch.randn(n, dim, generator=gen)).to(device)
        st = ops._stream(x)
        radius = 0.5 * math.sqrt(dim)   # (about 0.7 of the typical distance of two points: a few neighbours each)
        nbp = int(lib.gnntrk_radius_points_workspace_bytes(n, dim))

        def count(ws_p, stated, cnt, off):
            return lib.gnntrk_radius_count_ws(ops._p(x), n, dim, dim, radius, ops._p(cnt), ops._p(off), ops._p(ws_p),
                                              stated, 1, st)

        def run_count(ws):
            cnt, off = fresh((n,), torch.int32), fresh((n + 1,), torch.int64)
            return count(ws[0][0], ws[0][1], cnt, off), (cnt, off)

        _, off = check(f"radius_count_ws dim={dim}", [nbp], run_count)
        m = int(off[n])
        assert m > n, "the radius graph has no edges beside the points themselves"

        def run_fill(ws):   # (the count pass, which fills the chunks the fill pass reads, always gets the full size)
            nbr, dist = fresh((m,), torch.int32), fresh((m,), torch.float64)
            cnt2, off2 = fresh((n,), torch.int32), fresh((n + 1,), torch.int64)
            rc = count(ws[0][0], nbp, cnt2, off2)
            assert rc == 0, lib.gnntrk_last_error()
            return lib.gnntrk_radius_fill_ws(ops._p(x), n, dim, dim, radius, ops._p(off), m, ops._p(nbr), ops._p(dist),
                                             ops._p(ws[0][0]), ws[0][1], ops._p(ws[1][0]), ws[1][1], 1, st), (nbr, dist)

        nbr, dist = check(f"radius_fill_ws dim={dim}", [nbp, int(lib.gnntrk_radius_edges_workspace_bytes(m))], run_fill)
        assert bool((nbr >= 0).all()) and bool((nbr < n).all())

        eps, min_pts = 0.9 * radius, 3
        core, root = fresh((n,), torch.uint8), fresh((n,), torch.int32)
        changed = torch.ones(1, dtype=torch.int32, device=device)
        _capi.check(lib.gnntrk_dbscan_init(ops._p(off), ops._p(dist), n, eps, min_pts, ops._p(core), ops._p(root), st), lib)
        for _ in range(n):
            _capi.check(lib.gnntrk_dbscan_propagate(ops._p(off), ops._p(nbr), ops._p(dist), n, eps, ops._p(core),
                                                    ops._p(root), 8, ops._p(changed), st), lib)
            if int(changed.item()) == 0:
                break
        assert int(changed.item()) == 0

        def run_labels(ws):
            labels, n_clusters = fresh((n,), torch.int64), fresh((1,), torch.int64)
            return lib.gnntrk_dbscan_labels(ops._p(off), ops._p(nbr), ops._p(dist), n, eps, ops._p(core), ops._p(root),
                                            ops._p(labels), ops._p(n_clusters), ops._p(ws[0][0]), ws[0][1], st), \
                (labels, n_clusters)

        labels, n_clusters = check(f"dbscan_labels dim={dim}", [int(lib.gnntrk_dbscan_workspace_bytes(n))], run_labels)
        assert int(n_clusters) >= 1 and int(labels.max()) == int(n_clusters) - 1

    # ---- condensation losses: point selection, spatial forward and backward
    def oc_inputs(n, dim):
        x = (0.5 * torch.randn(n, dim, generator=gen)).to(device)
        beta = (0.01 + 0.98 * torch.rand(n, generator=gen)).to(device)
        pid = torch.randint(0, 12, (n,), generator=gen).to(device)   # (0: noise)
        mask = ((pid > 0).cpu() & (torch.rand(n, generator=gen) < 0.8)).to(torch.uint8).to(device)
        return x, beta, pid, mask

    def select(ws, n, beta, pid, mask):
        alphas, gid, n_cp = fresh((n,), torch.int32), fresh((n,), torch.int32), fresh((1,), torch.int32)
        return lib.gnntrk_oc_select_cps(ops._p(beta), ops._p(pid), ops._p(mask), n, 0, ops._p(alphas), ops._p(gid),
                                        ops._p(n_cp), ops._p(ws[0][0]), ws[0][1], ops._stream(beta)), (alphas, gid, n_cp)

    n = 65
    x, beta, pid, mask = oc_inputs(n, 3)
    check("oc_select_cps", [int(lib.gnntrk_oc_select_workspace_bytes(n))], lambda ws: select(ws, n, beta, pid, mask))

    n = 200
    for dim in (3, 8):
        x, beta, pid, mask = oc_inputs(n, dim)
        st = ops._stream(x)
        sel = torch.empty(int(lib.gnntrk_oc_select_workspace_bytes(n)), dtype=torch.uint8, device=device)
        rc, (alphas, gid, n_cp) = select([(sel, sel.numel())], n, beta, pid, mask)
        assert rc == 0 and int(n_cp) > 1
        a = _capi.OcArgs(ops._p(x), ops._p(beta), ops._p(pid), ops._p(mask), ops._p(gid), ops._p(alphas), ops._p(n_cp),
                         n, dim, dim, 0.01, 1.0, 1e-9, 0, 1.0, 0, 0, None)
        nbs = int(lib.gnntrk_oc_spatial_workspace_bytes(n, dim))

        def run_forward(ws):
            out = fresh((9,), torch.float32)
            return lib.gnntrk_oc_forward_spatial(C.byref(a), ops._p(out), ops._p(ws[0][0]), ws[0][1], st), (out,)

        (fwd,) = check(f"oc_forward_spatial dim={dim}", [nbs], run_forward)
        assert float(fwd[7]) > 0, "no repulsive pairs: the comparison is vacuous"
        g = torch.tensor([1.0, 2.0, 0.25, 0.5], device=device)

        def run_backward(ws):   # (the forward, which fills the buffer the backward reads, always gets the full size)
            out = fresh((9,), torch.float32)
            rc = lib.gnntrk_oc_forward_spatial(C.byref(a), ops._p(out), ops._p(ws[0][0]), nbs, st)
            assert rc == 0, lib.gnntrk_last_error()
            gx, gbeta = fresh((n, dim), torch.float32), fresh((n,), torch.float32)
            return lib.gnntrk_oc_backward_spatial(C.byref(a), ops._p(g), ops._p(fwd), ops._p(gx), ops._p(gbeta), n,
                                                  ops._p(ws[0][0]), ws[0][1], st), (gx, gbeta)

        gx, gbeta = check(f"oc_backward_spatial dim={dim}", [nbs], run_backward)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gbeta).all()) and float(gx.abs().max()) > 0


def case_full_size_properties(device, n_events=32, n_nodes=150_000, n_edges=2_000_000, n_hits=200_000):
    """BASELINE.json's full sizes (cfg3: 32 events x 150 k hits x 2 M edges collated; cfg5:
    200 k hits), checked through properties that do not need an oracle run of that size:
    sortedness / permutation / row-pointer consistency of the graph index, EVENT INDEPENDENCE
    (an event's edge weights inside the collated batch are bit-identical to the event run
    alone, fp32 and bf16 storage), the compaction invariants, the kNN ordering / prefix
    properties and the DBSCAN label invariants."""
    from gnn_tracking_amd import graph_cut, synthetic
    from gnn_tracking_amd.postprocessing import DBSCANFastRescan

    events = [synthetic.make_event(100 + i, n_nodes, n_edges, device) for i in range(n_events)]
    batch = G.collate(events)
    N, E = batch.num_nodes, batch.edge_index.shape[1]
    gi = ops.graph_index(batch.edge_index, N, cache=False)
    tgt, src, perm = gi.tgt.long(), gi.src.long(), gi.perm.long()
    assert bool((tgt[1:] >= tgt[:-1]).all()), "CSR targets not sorted"
    assert torch.equal(batch.edge_index[1][perm], tgt) and torch.equal(batch.edge_index[0][perm], src)
    seen = torch.zeros(E, dtype=torch.bool, device=device)
    seen[perm] = True
    assert bool(seen.all()), "perm is not a permutation"
    same_t = tgt[1:] == tgt[:-1]
    assert bool((perm[1:][same_t] > perm[:-1][same_t]).all()), "target sort not stable"
    assert int(gi.rowptr_t[-1]) == E and int(gi.rowptr_s[-1]) == E
    assert torch.equal(gi.rowptr_t[1:].long() - gi.rowptr_t[:-1].long(), torch.bincount(tgt, minlength=N))
    s_sorted = src[gi.spos.long()]
    assert bool((s_sorted[1:] >= s_sorted[:-1]).all()), "source view not sorted"
    assert torch.equal(gi.spos_inv.long()[gi.spos.long()], torch.arange(E, device=device))
    del seen, same_t, s_sorted, tgt, src, perm, gi

    torch.manual_seed(0)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40).to(device)
    for mode in ("f32", "bf16"):
        def run(d):
            with torch.no_grad():
                if mode == "bf16":
                    with G.bf16_storage():
                        return model(d)["W"]
                return model(d)["W"]
        w_batch = run(batch)
        assert w_batch.shape == (E,) and bool(torch.isfinite(w_batch).all())
        assert 0.001 <= float(w_batch.min()) and float(w_batch.max()) <= 0.999
        for i in (0, n_events - 1):
            w_one = run(events[i])
            assert torch.equal(w_batch[i * n_edges:(i + 1) * n_edges], w_one), f"event {i} ({mode}) depends on its batch"
        # the cut on the full edge list: ascending kept positions, count and threshold respected
        mask, idx = graph_cut.threshold_compact(w_batch, 0.5)
        assert idx.numel() == int(mask.sum()) and bool((idx[1:] > idx[:-1]).all())
        assert bool((w_batch[idx.long()] > 0.5).all()) and bool((w_batch[~mask] <= 0.5).all())
        del w_batch, mask, idx
    del batch, events, model

    # cfg5: kNN ordering / prefix properties and DBSCAN invariants on 200 k hits in 8 dimensions
    g = torch.Generator(device=device)
    g.manual_seed(5)
    centers = torch.randn(6000, 8, generator=g, device=device)
    x = centers[torch.randint(0, 6000, (n_hits,), generator=g, device=device)] \
        + 0.05 * torch.randn(n_hits, 8, generator=g, device=device)
    scan = ops.knn_scan(x, (4, 16), 1.0)
    ei = scan[16]
    assert bool((ei[1][1:] >= ei[1][:-1]).all()), "edges not grouped by query"
    assert bool((ei[0] != ei[1]).all()), "self loop"
    d = (x[ei[0]] - x[ei[1]]).norm(dim=1)
    assert float(d.max()) < 1.0
    same_q = ei[1][1:] == ei[1][:-1]
    assert bool((d[1:][same_q] >= d[:-1][same_q] - 1e-6).all()), "neighbours not in ascending distance"
    assert int(torch.bincount(ei[1], minlength=n_hits).max()) <= 16
    rank = torch.arange(ei.shape[1], device=device) - torch.searchsorted(ei[1], ei[1])  # position within the query
    assert torch.equal(ei[:, rank < 4], scan[4]), "k = 4 is not the prefix of k = 16"
    fr = DBSCANFastRescan(x, max_eps=0.3)
    eps, mp = 0.2, 3
    lab = fr.cluster_device(eps, mp)
    off, nbr, dist = fr._off, fr._nbr.long()[:fr._n_edges], fr._dist[:fr._n_edges]
    srcn = torch.repeat_interleave(torch.arange(n_hits, device=device), off[1:] - off[:-1])
    keep = dist <= eps
    deg = torch.bincount(srcn[keep], minlength=n_hits)
    core = deg >= mp
    assert bool((lab[core] >= 0).all()), "core point without a cluster"
    cc = keep & core[srcn] & core[nbr]
    assert torch.equal(lab[srcn[cc]], lab[nbr[cc]]), "core neighbours in different clusters"
    reach = torch.zeros(n_hits, dtype=torch.bool, device=device)
    reach[srcn[keep & core[nbr]]] = True
    assert torch.equal(lab >= 0, core | reach), "noise / border assignment"
    n_cl = int(lab.max()) + 1
    assert torch.unique(lab[lab >= 0]).numel() == n_cl, "cluster numbers not dense"
    first_core = torch.full((n_cl,), n_hits, dtype=torch.long, device=device)
    first_core.scatter_reduce_(0, lab[core], torch.arange(n_hits, device=device)[core], reduce="amin")
    assert bool((first_core[1:] > first_core[:-1]).all()), "clusters not numbered by their lowest core index"


def case_full_size_backward(device, n_events=32, n_nodes=150_000, n_edges=2_000_000, modes=("f32", "bf16")):
    """The BACKWARD of BASELINE config 3 at its full size (32 events x 150 k hits x 2 M edges collated, the
    bench's model and loss), through properties that need no oracle run of that size:

    * the parameter gradients of the collated batch equal the edge-weighted sum of the 32 single-event
      gradients (the loss is a mean over all edges; per-row arithmetic is identical in both runs, only
      the fp32 summation order of the weight-gradient partials differs): fp32 1e-5, bf16 storage 1e-4 of
      the largest entry of each parameter's gradient;
    * two backward runs are bit-identical;
    * gradients added in place by the backward launches (``dist.FlatParameters(grad_sink=True)``) equal
      autograd's accumulation bit for bit at this size."""
    from gnn_tracking_amd import dist as gdist
    from gnn_tracking_amd import synthetic

    events = [synthetic.make_event(100 + i, n_nodes, n_edges, device) for i in range(n_events)]
    batch = G.collate(events)
    E = batch.edge_index.shape[1]
    loss_fct = G.EdgeWeightBCELoss()
    report = {}

    def make_model():
        torch.manual_seed(0)
        return G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40).to(device)

    def backward(model, d, mode, scale=1.0):
        ops.clear_graph_index_cache()
        with G.bf16_storage(mode == "bf16"):
            out = model(d)
            loss = loss_fct(w=out["W"], y=d.y, pt=d.pt, edge_index=d.edge_index)
            (loss * scale).backward()
        return float(loss.detach())

    for mode in modes:
        model = make_model()
        names = [k for k, _ in model.named_parameters()]
        runs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            loss_b = backward(model, batch, mode)
            runs.append([p.grad.clone() for p in model.parameters()])
        assert math.isfinite(loss_b)
        for k, a, b in zip(names, *runs):
            assert torch.equal(a, b), f"{mode} {k}: two full-size backward runs differ"
        g_batch = runs[0]
        assert all(bool(torch.isfinite(g).all()) for g in g_batch) and sum(float(g.abs().sum()) for g in g_batch) > 0
        # in-place parameter gradients at this size
        sink_model = make_model()
        flat = gdist.FlatParameters(sink_model, grad_sink=True)
        flat.zero_grad()
        with ops.grad_sinks_armed():
            backward(sink_model, batch, mode)
        for k, p_, g in zip(names, flat.params, g_batch):
            assert torch.equal(p_.grad, g), f"{mode} {k}: grad sink != autograd accumulation at full size"
        del sink_model, flat
        # sum of the single-event gradients (fp64 accumulation of the 32 terms on the host side of the sum)
        model.zero_grad(set_to_none=True)
        acc = [torch.zeros_like(g, dtype=torch.float64) for g in g_batch]
        loss_sum = 0.0
        for ev in events:
            model.zero_grad(set_to_none=True)
            e_ev = ev.edge_index.shape[1]
            # (the event's share of the batch mean enters as the upstream gradient of its loss, so that every
            #  per-row value is what it is inside the batch - exactly for power-of-two shares; scaling the
            #  finished gradients instead would round the bf16 activation gradients at another scale)
            loss_sum += backward(model, ev, mode, scale=e_ev / E) * e_ev / E
            for a, p in zip(acc, model.parameters()):
                a += p.grad.double()
        tol = 1e-5 if mode == "f32" else 1e-4
        worst = 0.0
        for k, a, g in zip(names, acc, g_batch):
            err = float((a - g.double()).abs().max()) / max(float(a.abs().max()), 1e-30)
            worst = max(worst, err)
            assert err <= tol, f"{mode} {k}: batch gradient vs sum of event gradients {err:.2e} > {tol}"
        assert abs(loss_sum - loss_b) <= 1e-5 * abs(loss_b), f"{mode}: loss {loss_b} vs {loss_sum}"
        report[mode] = worst
        del model, runs, g_batch, acc
    return report


GC_RESIN_CASES = {"h12_l2": dict(h_outdim=6, hidden_dim=12, n_layers=2, alpha=0.5, alpha_fcnn=0.5),
                  "h16_l1": dict(h_outdim=8, hidden_dim=16, n_layers=1, alpha=0.3, alpha_fcnn=0.7),
                  # the reference's defaults: 120-wide relational input, 40-wide outputs -> library-GEMM path
                  "default_h40": dict(h_outdim=8, hidden_dim=40, n_layers=1, alpha=0.5, alpha_fcnn=0.5)}


def case_graph_tcn_wide_hidden_bf16(device, hiddens=(64, 100, 128), n_hits=400, n_edges=3000):
    """GraphTCN (edge classifier + track condenser + heads) with hidden widths beyond four hidden tiles in bf16
    storage: every MLP runs on the fused kernels (no library launch), H and the parameter gradients sit at a
    bf16-sized distance from the fp32 run of the same model (which takes library GEMMs above hidden 64)."""
    from gnn_tracking_amd import synthetic
    ev = synthetic.make_event(3, n_hits, n_edges, device)
    for hd in hiddens:
        torch.manual_seed(0)
        model = G.GraphTCN(node_indim=14, edge_indim=4, h_dim=5, e_dim=4, h_outdim=4, hidden_dim=hd, L_ec=2, L_hc=2).to(device)
        res = {}
        for bf16 in (False, True):
            model.zero_grad()
            ops._WIDE_WARNED.clear()
            ops.clear_graph_index_cache()
            with G.bf16_storage(bf16):
                out = model(G.Data(x=ev.x, edge_index=ev.edge_index, edge_attr=ev.edge_attr, y=ev.y))
                (out["H"].float().square().mean() + out["B"].float().mean()).backward()
            if bf16:
                assert not ops._WIDE_WARNED, f"hidden {hd}: library path taken for {sorted(ops._WIDE_WARNED)}"
            res[bf16] = (out["H"].float().detach().clone(),
                         torch.cat([p_.grad.reshape(-1).float() for p_ in model.parameters() if p_.grad is not None]).clone())
        dh = float((res[True][0] - res[False][0]).abs().max()) / max(float(res[False][0].abs().max()), 1e-6)
        dg = float((res[True][1] - res[False][1]).norm()) / max(float(res[False][1].norm()), 1e-12)
        assert 0 < dh < 0.05 and dg < 0.05, f"hidden {hd}: bf16 vs fp32 H {dh:.3e} gradients {dg:.3e}"


def case_gc_resin(device, names=None):
    """GraphConstructionResIN vs the reference (G12): encoders, ResIN with node = edge width =
    hidden_dim (relational input 3 x hidden_dim), decoder, latent mix."""
    z = load("g12_gc_resin.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    for name, kw in GC_RESIN_CASES.items():
        if names is not None and name not in names:
            continue
        model = G.GraphConstructionResIN(node_indim=14, edge_indim=4, **kw)
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        ops._WIDE_WARNED.clear()
        out = model(G.Data(x=x, edge_index=ei, edge_attr=ea))["H"]
        assert_close(out, z[f"{name}/H"], TOL_OUT, name + " H")
        (out * tt(z[f"{name}/r"], device)).sum().backward()
        for k, v in model.named_parameters():
            assert_close(v.grad, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")
        # (fp32 - the reference's own precision - at the reference's default width runs on the wide fused kernels,
        #  csrc/mlp_wide.hip: no library GEMM)
        assert not ops._WIDE_WARNED, f"{name}: library path taken in fp32: {ops._WIDE_WARNED}"
    # bf16 storage at the reference's default width: the 120 -> 40 -> 40 -> 40 relational model, the 80-wide object
    # model and the 40-wide encoder outputs run on the fused kernels (output tiles, three / four k-steps of inputs),
    # not on library GEMMs; H and the parameter gradients against the fp32 goldens with bf16-sized bounds
    kw = GC_RESIN_CASES["default_h40"]
    if names is None or "default_h40" in names:
        model = G.GraphConstructionResIN(node_indim=14, edge_indim=4, **kw)
        load_params(model, z, "default_h40/p0/")
        model = model.to(device)
        ops._WIDE_WARNED.clear()
        with G.bf16_storage():
            out16 = model(G.Data(x=x, edge_index=ei, edge_attr=ea))["H"]
            (out16.float() * tt(z["default_h40/r"], device)).sum().backward()
        assert not ops._WIDE_WARNED, f"library path taken: {ops._WIDE_WARNED}"
        assert float((out16.float() - tt(z["default_h40/H"], device)).abs().max()) > 0, "bf16 storage was not engaged"
        assert_close(out16.float(), z["default_h40/H"], 0.02, "default_h40 H (bf16 storage)")
        tot = math.sqrt(sum(float(tt(z[f"default_h40/grad/{k}"]).double().pow(2).sum()) for k, _ in model.named_parameters()))
        err2 = 0.0
        for k, v in model.named_parameters():
            assert v.grad is not None and torch.isfinite(v.grad).all(), k
            gref = tt(z[f"default_h40/grad/{k}"]).double()
            d = float((v.grad.detach().cpu().double() - gref).norm())
            err2 += d * d
            assert d <= 0.10 * float(gref.norm()) + 0.01 * tot, f"default_h40 bf16 grad {k}: {d:.3e} vs |g| {float(gref.norm()):.3e}"
        assert math.sqrt(err2) <= 0.05 * tot, f"default_h40 bf16 gradients: relative L2 {math.sqrt(err2) / tot:.3f}"


FOCAL_CASES = {"ew_default": ("EdgeWeightFocalLoss", dict()),
               "ew_pt": ("EdgeWeightFocalLoss", dict(alpha=0.4, gamma=1.5, pos_weight=2.0, pt_thld=0.9)),
               "ew_g0": ("EdgeWeightFocalLoss", dict(alpha=0.5, gamma=0.0)),
               "haughty": ("HaughtyFocalLoss", dict(alpha=0.3, gamma=2.0, pt_thld=0.9)),
               "haughty0": ("HaughtyFocalLoss", dict(alpha=0.25, gamma=3.0))}


def case_focal_losses(device):
    """EdgeWeightFocalLoss / HaughtyFocalLoss vs the reference (G13): loss 1e-6, gradient wrt w
    1e-6 relative; the reference's own check focal(alpha=.5, gamma=0) = BCE / 2."""
    z = load("g13_focal.npz")
    y, ei, pt = tt(z["y"], device), tt(z["edge_index"], device), tt(z["pt"], device)
    for name, (cls, kw) in FOCAL_CASES.items():
        w = tt(z["w"], device).requires_grad_(True)
        loss = getattr(G, cls)(**kw)(w=w, y=y, edge_index=ei, pt=pt)
        assert_close(loss, z[f"{name}/loss"], 1e-6, name + " loss")
        loss.backward()
        assert_close(w.grad, z[f"{name}/grad_w"], 1e-5, name + " grad")
    w = tt(z["w"], device)
    half = G.binary_focal_loss(inpt=w, target=y, alpha=0.5, gamma=0.0)
    assert_close(half, 0.5 * float(G.EdgeWeightBCELoss()(w=w, y=y)), 1e-6, "focal(.5, 0) = BCE / 2")


# ------------------------------------------------- BASELINE configs on their stated workloads
def case_cfg12_event(device):
    """BASELINE.json configs[0] and configs[1] on THEIR event (seed 1,
    10 000 hits, 100 000 edges): ``ECForGraphTCN(14, 4, L_ec=1)`` (hidden_dim None) and
    ``(L_ec=3, hidden_dim=40)`` in fp32 against the CPU oracle's training step: W and the
    embeddings <= 1e-5, loss <= 1e-5, every parameter gradient <= 1e-4, parameters after one
    Adam(lr=1e-4, weight_decay=1e-4) step <= 1e-6."""
    from gnn_tracking_amd import synthetic

    ev = synthetic.make_event(1, 10_000, 100_000, "cpu")
    d = ev.to(device)
    for kw in (dict(L_ec=1), dict(L_ec=3, hidden_dim=40)):
        torch.manual_seed(0)
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **kw)
        params = {k: v.detach().clone() for k, v in model.state_dict().items()}
        ref, rloss, rgrads, rafter = O.ec_training_step(ev.x, ev.edge_index, ev.edge_attr, ev.y, params,
                                                        model_kwargs=dict(L_ec=kw["L_ec"]), pt=ev.pt,
                                                        pt_thld=0.9)
        model = model.to(device)
        out = model(d)
        tag = f"cfg event L_ec={kw['L_ec']}"
        assert out["W"].shape == (100_000,)
        assert_close(out["W"], ref["W"], TOL_OUT, tag + " W")
        assert_close(out["node_embedding"], ref["node_embedding"], TOL_OUT, tag + " node_embedding")
        assert_close(out["edge_embedding"], ref["edge_embedding"], TOL_OUT, tag + " edge_embedding")
        loss = G.EdgeWeightBCELoss(pt_thld=0.9)(w=out["W"], y=d.y.float(), pt=d.pt, edge_index=d.edge_index)
        assert_close(loss, rloss, TOL_OUT, tag + " loss")
        loss.backward()
        for k, v in model.named_parameters():
            assert_close(v.grad, rgrads[k], TOL_GRAD, f"{tag} grad {k}")
        torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4).step()
        for k, v in model.state_dict().items():
            assert_close(v, rafter[k], 1e-6, f"{tag} after Adam {k}")


def case_cfg3_event(device, n_hits=150_000, n_edges=2_000_000, modes=("f32", "bf16"), seed=100, pt_thld=0.0):
    """ONE event of BASELINE.json configs[2] at its full size (seed 100: event 0 of the bench's batch; 150 000 hits,
    2 000 000 edges) against the CPU oracle - the size the headline number is measured at, compared value for
    value, not through properties: fp32 against ``oracle.ec_training_step`` (W / embeddings / loss 1e-5, every
    parameter gradient 1e-4, parameters after Adam(lr=1e-4, weight_decay=1e-4) 1e-6); bf16 storage against the
    oracle's restatement of the rounding contract ``ec_for_graph_tcn_bf16`` (``BF16_ORACLE_W`` = 5e-4: 1.1e-4
    measured; loss 1e-4) and its gradients against the fp32 oracle's (relative L2 3 %: 1.2 % measured).
    Runs with the package's default node order (renumbered from 65 536 hits on).  ``seed`` / ``pt_thld``: another
    event of the batch, and the loss with ``falsify_low_pt_edges`` on (losses/ec.py:71-92)."""
    from gnn_tracking_amd import synthetic

    ev = synthetic.make_event(seed, n_hits, n_edges, "cpu")
    d = ev.to(device)
    torch.manual_seed(0)
    model0 = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40)
    params = {k: v.detach().clone() for k, v in model0.state_dict().items()}
    ref, rloss, rgrads, rafter = O.ec_training_step(ev.x, ev.edge_index, ev.edge_attr, ev.y, params,
                                                    model_kwargs=dict(L_ec=3), pt=ev.pt, pt_thld=pt_thld)
    report = {}
    for mode in modes:
        model = G.ECForGraphTCN(node_indim=14, edge_indim=4, L_ec=3, hidden_dim=40)
        model.load_state_dict(params)
        model = model.to(device)
        ops.clear_graph_index_cache()
        with (G.bf16_storage() if mode == "bf16" else contextlib.nullcontext()):
            out = model(d)
            loss = G.EdgeWeightBCELoss(pt_thld=pt_thld)(w=out["W"], y=d.y, pt=d.pt, edge_index=d.edge_index)
            loss.backward()
        W = torch.as_tensor(out["W"]).detach().float().cpu()
        tag = f"cfg3 event {mode}"
        assert W.shape == (n_edges,)
        if mode == "f32":
            assert_close(W, ref["W"], TOL_OUT, tag + " W")
            assert_close(out["node_embedding"], ref["node_embedding"], TOL_OUT, tag + " node_embedding")
            assert_close(torch.as_tensor(out["edge_embedding"]), ref["edge_embedding"], TOL_OUT, tag + " edge_embedding")
            assert_close(loss, rloss, TOL_OUT, tag + " loss")
            for k, v in model.named_parameters():
                assert_close(v.grad, rgrads[k], TOL_GRAD, f"{tag} grad {k}")
            torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4).step()
            # (Adam normalises g + weight_decay * p: where that sum is below 1e-6 - the mean over 2 M edges leaves
            #  gradient elements of that size, and on this event one of them cancels its decay term to 4e-9 - rounding
            #  noise becomes a step of up to lr in either direction: _check_after_adam on the EFFECTIVE gradient)
            geff = {k: rgrads[k] + 1e-4 * params[k] for k in rgrads}
            _check_after_adam(model, geff, rafter, tag, lr_step=1e-4)
            report[mode] = {"W": (W - ref["W"]).abs().max().item()}
        else:
            with torch.no_grad():
                ref16 = O.ec_for_graph_tcn_bf16(ev.x, ev.edge_index, ev.edge_attr, params, L_ec=3)
            errW = (W - ref16["W"]).abs().max().item()
            assert errW <= BF16_ORACLE_W, f"{tag}: |W - W_oracle16| {errW:.2e}"
            loss16 = O.edge_weight_bce_loss(ref16["W"], ev.y.float(), ev.edge_index, ev.pt, pt_thld)
            assert abs(float(loss) - float(loss16)) <= 1e-4, tag + " loss"
            assert_close(W, ref["W"], 2e-3, tag + " W vs fp32 oracle")   # (3.9e-4 measured)
            worst = 0.0
            for k, v in model.named_parameters():
                g = rgrads[k].double()
                if g.norm().item() < 1e-6:
                    continue
                worst = max(worst, ((v.grad.detach().cpu().double() - g).norm() / g.norm()).item())
            assert worst <= BF16_GRAD_REL_L2, f"{tag}: parameter gradients {worst:.3f} relative L2 from the fp32 oracle"
            report[mode] = {"W": errW, "grad_rel_l2": worst}
    return report


#: the reference's five training configs (tests/test_configs/*.yml) with this package's class paths: the YAML swap
#: of INTEGRATION.md, written as the dicts LightningCLI hands to the modules.  (tc.yml:5-10 leaves out the
#: pre-trained edge classifier its model requires - track_condensation_networks.py:460 -: the ec.yml model is
#: nested in, which also exercises the nested {class_path, init_args} form.)
REFERENCE_CONFIGS = {
    "ec": dict(   # ec.yml:4-12
        module="ECModule",
        model={"class_path": "gnn_tracking_amd.edge_classifier.ECForGraphTCN",
               "init_args": {"node_indim": 14, "edge_indim": 14, "L_ec": 1}},
        loss_fct={"class_path": "gnn_tracking_amd.losses_ec.EdgeWeightBCELoss", "init_args": {}}),
    "tc": dict(   # tc.yml:4-13
        module="TCModule",
        model={"class_path": "gnn_tracking_amd.track_condensation_networks.PreTrainedECGraphTCN",
               "init_args": {"ec": {"class_path": "gnn_tracking_amd.edge_classifier.ECForGraphTCN",
                                    "init_args": {"node_indim": 14, "edge_indim": 14, "L_ec": 1}},
                             "node_indim": 14, "edge_indim": 14, "hidden_dim": 3, "L_hc": 2}},
        loss_fct={"class_path": "gnn_tracking_amd.losses_oc.CondensationLossTiger", "init_args": {}}),
    "ml": dict(   # ml.yml:4-15
        module="MLModule",
        model={"class_path": "gnn_tracking_amd.track_condensation_networks.GraphConstructionFCNN",
               "init_args": {"in_dim": 14, "out_dim": 8, "hidden_dim": 10, "depth": 2}},
        loss_fct={"class_path": "gnn_tracking_amd.losses_ml.GraphConstructionHingeEmbeddingLoss",
                  "init_args": {"max_num_neighbors": 1, "lw_repulsive": 0.3}}),
    "ml_hetero": dict(   # ml_hetero.yml:4-15
        module="MLModule",
        model={"class_path": "gnn_tracking_amd.track_condensation_networks.GraphConstructionHeteroResFCNN",
               "init_args": {"in_dim": 14, "out_dim": 8, "hidden_dim": 10, "depth": 2}},
        loss_fct={"class_path": "gnn_tracking_amd.losses_ml.GraphConstructionHingeEmbeddingLoss",
                  "init_args": {"max_num_neighbors": 1, "lw_repulsive": 0.3}}),
    "ml_heteroenc": dict(   # ml_heteroenc.yml:4-17
        module="MLModule",
        model={"class_path": "gnn_tracking_amd.track_condensation_networks.GraphConstructionHeteroEncResFCNN",
               "init_args": {"in_dim": 14, "out_dim": 8, "hidden_dim": 10, "hidden_dim_enc": 8, "depth": 2,
                             "depth_enc": 2}},
        loss_fct={"class_path": "gnn_tracking_amd.losses_ml.GraphConstructionHingeEmbeddingLoss",
                  "init_args": {"max_num_neighbors": 1, "lw_repulsive": 0.3}}),
}


def case_class_path_configs(device, names=None):
    """The drop-in boundary as the reference enters it (utils/lightning.py:59-94; tests/
    test_lightning_from_config_training.py:25-53 runs ``fit`` for one step on every tests/test_configs/*.yml): each
    config's model and loss are built from ``{class_path, init_args}`` through ``hparams.obj_from_or_to_hparams`` /
    ``get_object_from_path``, the dict is found again in the holder's ``hparams`` (and an OBJECT handed to the
    holder is recorded as the same class path with init_args that rebuild an identical module), and one
    optimisation step (the yml's Adam) runs on the reference's own ``test_graph.pt`` on the fused kernels
    (no library-GEMM fallback)."""
    import copy

    from gnn_tracking_amd import hparams as H, io, training

    data0 = io.load_graph(GOLD / "test_graph.pt")
    for name, cfg in REFERENCE_CONFIGS.items():
        if names is not None and name not in names:
            continue

        class Holder(H.HyperparametersMixin):   # (what TrackingModule.__init__ does with its arguments, base.py:86-92)
            pass

        hold = Holder()
        torch.manual_seed(0)
        model = H.obj_from_or_to_hparams(hold, "model", copy.deepcopy(cfg["model"]))
        loss_fct = H.obj_from_or_to_hparams(hold, "loss_fct", copy.deepcopy(cfg["loss_fct"]))
        assert hold.hparams["model"] == cfg["model"] and hold.hparams["loss_fct"] == cfg["loss_fct"], name
        assert type(model).__module__ + "." + type(model).__name__ == cfg["model"]["class_path"]
        for k, v in cfg["model"]["init_args"].items():   # the module's own hparams carry its init_args
            if k != "ec":
                assert model.hparams[k] == v, (name, k)
        # the other direction: an object -> its class path + init_args, which rebuild the same module
        hold2 = Holder()
        assert H.obj_from_or_to_hparams(hold2, "model", model) is model
        rec = hold2.hparams["model"]
        assert rec["class_path"] == cfg["model"]["class_path"], name
        for k, v in cfg["model"]["init_args"].items():
            assert rec["init_args"][k] == v, (name, k)
        twin = H.get_object_from_path(rec["class_path"], copy.deepcopy(rec["init_args"]))
        assert {k: tuple(v.shape) for k, v in twin.state_dict().items()} == \
               {k: tuple(v.shape) for k, v in model.state_dict().items()}, name
        assert dict(twin.hparams) == dict(model.hparams), name

        data = copy.copy(data0).to(device)
        if name == "tc":
            # (test_graph.pt has no noise hit: the loss's noise term - a mean over none, oc.py:158 - is NaN there in
            #  the reference as well and takes the gradients with it; the condensation step gets five noise hits)
            data.particle_id = data.particle_id.clone()
            data.particle_id[:5] = 0
        model = model.to(device)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        warned = set(ops._WIDE_WARNED)
        mod = getattr(training, cfg["module"])(
            model, loss_fct=loss_fct, scheduler=None,
            optimizer=lambda p: torch.optim.Adam(p, lr=1e-4, weight_decay=1e-4))   # *.yml: optimizer
        loss = mod.optimisation_step(data)
        assert torch.isfinite(loss).all(), name
        assert set(ops._WIDE_WARNED) == warned, f"{name}: {set(ops._WIDE_WARNED) - warned} took the library-GEMM path"
        moved = sum(int(not torch.equal(v, before[k])) for k, v in model.state_dict().items())
        assert moved > 0, f"{name}: the optimisation step changed no parameter"


def case_cfg5_condensation(device, n_hits=200_000, chunk=4096):
    """BASELINE.json configs[4] loss leg at full size (seed 500, 200 000 hits in 8 latent
    dimensions, several thousand particles of interest): CondensationLossRG and
    CondensationLossTiger, the four terms, the weighted total (rel <= 1e-5) and the gradients
    w.r.t. x and beta (<= 1e-4 of the largest entry) against the blocked float64 oracle
    (oracle/ref_cpu.py: condensation_loss_chunked, itself pinned on the reference's G5 values)."""
    from gnn_tracking_amd import synthetic
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    ev = synthetic.make_pileup_event(500, n_hits)
    mask = O.good_node_mask(ev["pt"], ev["particle_id"], ev["reconstructable"], ev["eta"])
    d = {k: v.to(device) for k, v in ev.items()}
    w = dict(lw_repulsive=2.0, lw_noise=0.5, lw_coward=0.25)
    report = {}
    for strat, cls in (("rg", CondensationLossRG), ("tiger", CondensationLossTiger)):
        b = d["beta"].clone().requires_grad_(True)
        x = d["x"].clone().requires_grad_(True)
        ret = cls(**w)(beta=b, x=x, particle_id=d["particle_id"], reconstructable=d["reconstructable"],
                       pt=d["pt"], eta=d["eta"])
        ret.loss.backward()
        od = O.condensation_loss_chunked(beta=ev["beta"], x=ev["x"], particle_id=ev["particle_id"], mask=mask,
                                         mode=strat, weights=(1.0, 2.0, 0.25, 0.5), chunk=chunk)
        assert od["K"] > 1000 and od["n_rep"] > 0, "workload degenerate"
        for k in ("attractive", "repulsive", "coward", "noise"):
            rel = abs(float(ret.loss_dct[k]) - od[k]) / abs(od[k])
            report[f"{strat}/{k}"] = rel
            assert rel <= 1e-5, f"cfg5 {strat} {k}: rel err {rel:.2e}"
        rel = abs(float(ret.loss) - od["total"]) / abs(od["total"])
        assert rel <= 1e-5, f"cfg5 {strat} total: rel err {rel:.2e}"
        if strat == "tiger":
            assert abs(int(ret.extra_metrics["n_rep"]) - od["n_rep"]) <= 2, "number of repulsive pairs"  # fp32 vs fp64 d < 1 at the boundary
        for name, got, want in (("grad_x", x.grad, od["grad_x"]), ("grad_beta", b.grad, od["grad_beta"])):
            err = (got.double().cpu() - want).abs().max().item() / want.abs().max().item()
            report[f"{strat}/{name}"] = err
            assert err <= 1e-4, f"cfg5 {strat} {name}: {err:.2e}"
    return report


def case_cfg5_knn(device, n_hits=200_000, n_slice=20_000):
    """BASELINE.json configs[4] graph-build leg: ``knn_with_max_radius(k, max_radius=1)`` for
    k = 16 and k = 64 on the 200 000-hit cloud: ordering / radius / degree / k-prefix
    properties at full size and bit-exact edge lists against the C oracle on a 20 000-hit
    slice (k = 64 included)."""
    from gnn_tracking_amd import synthetic
    from gnn_tracking_amd.graph_construction import knn_with_max_radius

    xc = synthetic.make_pileup_cloud(500, n_hits)
    x = xc.to(device)
    lists = {k: knn_with_max_radius(x, k=k, max_radius=1.0) for k in (16, 64)}
    for k, ei in lists.items():
        assert ei.dtype == torch.int64 and ei.shape[0] == 2
        assert bool((ei[1][1:] >= ei[1][:-1]).all()), "edges not grouped by query"
        assert bool((ei[0] != ei[1]).all()), "self loop"
        dist = (x[ei[0]] - x[ei[1]]).norm(dim=1)
        assert float(dist.max()) < 1.0, "radius"
        same_q = ei[1][1:] == ei[1][:-1]
        assert bool((dist[1:][same_q] >= dist[:-1][same_q] - 1e-6).all()), "neighbours not in ascending distance"
        assert int(torch.bincount(ei[1], minlength=n_hits).max()) <= k
    ei = lists[64]
    rank = torch.arange(ei.shape[1], device=device) - torch.searchsorted(ei[1], ei[1])
    assert torch.equal(ei[:, rank < 16], lists[16]), "k = 16 is not the prefix of k = 64"
    for k in (16, 64):
        got = knn_with_max_radius(x[:n_slice], k=k, max_radius=1.0)
        assert torch.equal(got.cpu(), O.knn_graph_c(xc[:n_slice], k, 1.0)), f"kNN k={k} differs from the C oracle"


def case_edge_ordered(device, name="skip1_L3_h40"):
    """``W`` / ``edge_embedding`` are handed out as ``EdgeOrdered`` (held in CSR order, behaving
    like ``edge_index``-ordered tensors): metadata without a scatter, every other use
    materialises the reference's ordering, the package's losses take the CSR fast path and
    agree with torch's own loss on the materialised tensor, gradients included."""
    from gnn_tracking_amd.edge_order import EdgeOrdered

    z = load("g2_ec_variants.npz")
    x, ei, ea = tt(z["x"], device), tt(z["edge_index"], device), tt(z["edge_attr"], device)
    y, pt = tt(z["y"], device).float(), tt(z["pt"], device)
    model = G.ECForGraphTCN(node_indim=14, edge_indim=4, **EC_VARIANTS[name])
    load_params(model, z, f"{name}/p0/")
    model = model.to(device)
    out = model(G.Data(x=x, edge_index=ei, edge_attr=ea))
    w, e = out["W"], out["edge_embedding"]
    assert isinstance(w, EdgeOrdered) and isinstance(e, EdgeOrdered)
    E = ei.shape[1]
    assert w.shape == (E,) and e.shape == (E, 4) and w.dtype == torch.float32 and w.dim() == 1
    assert len(w) == E and w.numel() == E and w.device == x.device and w.requires_grad
    assert w._coo is None and e._coo is None, "metadata queries must not trigger the scatter"
    # fast path (CSR) vs torch's own BCE on the materialised, edge_index-ordered weights
    fast = G.EdgeWeightBCELoss(pt_thld=0.9)(w=w, y=y, pt=pt, edge_index=ei)
    assert w._coo is None, "the package's loss must not materialise W"
    yf = (y.bool() & (pt[ei[0]] > 0.9)).float()
    slow = torch.nn.functional.binary_cross_entropy(w, yf)
    assert w._coo is not None
    assert_close(fast, slow, 1e-6, "CSR fast path vs torch BCE")
    assert_close(fast, z[f"{name}/loss"], TOL_OUT, "loss vs reference")
    g_fast = torch.autograd.grad(fast, list(model.parameters()), retain_graph=True)
    g_slow = torch.autograd.grad(slow, list(model.parameters()), retain_graph=True)
    for (k, _), a, b in zip(model.named_parameters(), g_fast, g_slow):
        assert_close(a, b, 1e-5, f"fast vs materialised grad {k}")
        assert_close(a, z[f"{name}/grad/{k}"], TOL_GRAD, f"grad {k} vs reference")
    # ordinary tensor behaviour in the reference's ordering
    assert_close(w, z[f"{name}/W"], TOL_OUT, "W")
    assert_close(w.detach().cpu(), z[f"{name}/W"], TOL_OUT, "W.cpu()")
    assert_close(e, z[f"{name}/edge_embedding"], TOL_OUT, "edge_embedding")
    w_ref = tt(z[f"{name}/W"])
    clear = (w_ref - 0.5).abs() > 1e-4   # (weights within the output tolerance of 0.5 may flip)
    assert int(clear.sum()) > 0.9 * E and torch.equal((w > 0.5).cpu()[clear], (w_ref > 0.5)[clear]), "comparison"
    assert_close(w[5:9], z[f"{name}/W"][5:9], TOL_OUT, "slice")
    assert_close(torch.cat([w, w])[E:], z[f"{name}/W"], TOL_OUT, "torch.cat")
    assert_close(w * 2 + 1, 2 * z[f"{name}/W"] + 1, TOL_OUT, "arithmetic")
    assert abs(float(w[0]) - float(z[f"{name}/W"][0])) < 1e-5 and "EdgeOrdered" in repr(w)
    import copy
    import pickle
    assert_close(pickle.loads(pickle.dumps(w.detach().cpu())), z[f"{name}/W"], TOL_OUT, "pickle")
    # a caller that hands the loss ANOTHER edge_index tensor (here: edges and labels permuted together)
    # gets the reference's elementwise semantics - falsification through the edge_index it passed
    pi = torch.randperm(E, generator=torch.Generator().manual_seed(5)).to(ei.device)
    ei2, y2 = ei[:, pi].contiguous(), y[pi].contiguous()
    w2 = model(G.Data(x=x, edge_index=ei, edge_attr=ea))["W"]
    got = G.EdgeWeightBCELoss(pt_thld=0.9)(w=w2, y=y2, pt=pt, edge_index=ei2)
    want = torch.nn.functional.binary_cross_entropy(w2.in_edge_index_order(), (y2.bool() & (pt[ei2[0]] > 0.9)).float())
    assert_close(got, want, 1e-6, "loss with a foreign edge_index")
    # autograd attributes are those of the materialised tensor
    w3 = model(G.Data(x=x, edge_index=ei, edge_attr=ea))["W"]
    assert w3.grad_fn is not None and not w3.is_leaf
    w3.retain_grad()
    (w3 * 2).sum().backward()
    assert w3.grad is not None and bool((w3.grad == 2).all())
    # what a training loop does to an output dict: torch.save / load round trip
    import io
    buf = io.BytesIO()
    torch.save({"W": out["W"].detach(), "edge_embedding": out["edge_embedding"].detach()}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert_close(back["W"], z[f"{name}/W"], TOL_OUT, "torch.save round trip")
    # haughty focal loss needs raw and falsified labels: it materialises and still agrees
    hl = G.HaughtyFocalLoss(pt_thld=0.9)(w=model(G.Data(x=x, edge_index=ei, edge_attr=ea))["W"], y=y, pt=pt,
                                          edge_index=ei)
    assert torch.isfinite(hl)


# ------------------------------------------------------------- TC training step (row H)
TC_STEP_CASES = {
    "rg_feedw": dict(loss="rg", gtcn=dict(L_ec=2, L_hc=2, hidden_dim=16, h_outdim=3, feed_edge_weights=True)),
    "tiger_orphans": dict(loss="tiger", gtcn=dict(L_ec=1, L_hc=2, hidden_dim=12, h_outdim=2, mask_orphan_nodes=True,
                                                   use_ec_embeddings_for_hc=True)),
}
TC_MLGC = dict(embedding_slice=(0, 3), max_radius=1.0, max_num_neighbors=6)
TC_LOSS_W = (2.0, 0.25, 0.5)   # lw_repulsive, lw_coward, lw_noise


def case_tc_step(device, names=None):
    """SURVEY.md section 8a row H, object-condensation half: one optimisation step as the
    reference's ``TCModule`` runs it (training/tc.py:50-84; golden G14 from the reference's own
    module): ``MLGraphConstruction(ml=None)`` -> ``GraphTCN`` -> condensation loss with the
    post-EC hit mask -> backward -> Adam under the default ConstantLR scheduler.  Built graph and
    masks bit-exact, W / H / B and the loss terms 1e-5, gradients 1e-4, parameters after the
    step 1e-6."""
    from gnn_tracking_amd import training
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    z = load("g14_tc_step.npz")
    for name, cfg in TC_STEP_CASES.items():
        if names is not None and name not in names:
            continue
        model = G.GraphTCN(14, 28, ec_threshold=float(z[f"{name}/ec_threshold"]), **cfg["gtcn"])
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        lw_rep, lw_cow, lw_noise = TC_LOSS_W
        loss_cls = CondensationLossTiger if cfg["loss"] == "tiger" else CondensationLossRG
        mod = training.TCModule(model, loss_fct=loss_cls(lw_repulsive=lw_rep, lw_coward=lw_cow, lw_noise=lw_noise),
                                preproc=G.MLGraphConstruction(ml=None, **TC_MLGC))
        data = G.Data(x=tt(z["x"], device), edge_index=tt(z["edge_index_in"], device),
                      particle_id=tt(z["particle_id"], device), pt=tt(z["pt"], device), eta=tt(z["eta"], device),
                      reconstructable=tt(z["reconstructable"], device), layer=tt(z["layer"], device),
                      sector=tt(z["sector"], device))
        data = mod.data_preproc(data)
        assert torch.equal(data.edge_index.cpu(), tt(z[f"{name}/edge_index"])), name + " built edge_index"
        assert torch.equal(data.y.cpu(), tt(z[f"{name}/y"])), name + " edge labels"
        assert torch.equal(data.edge_attr.cpu(), tt(z[f"{name}/edge_attr"])), name + " edge features"
        out = mod(data, _preprocessed=True)
        assert torch.equal(out["ec_edge_mask"].cpu(), tt(z[f"{name}/ec_edge_mask"])), name + " edge mask"
        assert torch.equal(out["ec_hit_mask"].cpu(), tt(z[f"{name}/ec_hit_mask"])), name + " hit mask"
        for k in ("W", "H", "B"):
            assert_close(out[k], z[f"{name}/{k}"], TOL_OUT, f"{name} {k}")
        loss, metrics = mod.get_losses(out, data)
        for k in ("attractive", "repulsive", "coward", "noise"):
            assert_close(metrics[k], z[f"{name}/{k}"], TOL_OUT, f"{name} {k}")
        assert_close(loss, z[f"{name}/loss"], TOL_OUT, name + " loss")
        mod.zero_grad()
        loss.backward()
        for k, v in model.named_parameters():
            gk = v.grad if v.grad is not None else torch.zeros_like(v)
            assert_close(gk, z[f"{name}/grad/{k}"], TOL_GRAD, f"{name} grad {k}")
        mod.configure_optimizers().step()
        for k, v in model.state_dict().items():
            # Adam's first step is lr * g / (|g| + 1e-8): where a gradient ELEMENT vanishes (dead
            # ReLU units; the bias of the last cluster layer - the potentials are translation
            # invariant) rounding noise of 1e-9 becomes a step of up to lr in EITHER direction, in the
            # reference's run and in ours.  Those elements are only required to stay within two steps of
            # each other (a step is lr / 3 under the default ConstantLR).
            ref1 = tt(z[f"{name}/p1/{k}"]).double()
            got = v.detach().cpu().double()
            tol = torch.full_like(ref1, 1e-6)
            if f"{name}/grad/{k}" in z.files:
                tol[tt(z[f"{name}/grad/{k}"]).abs() < 1e-6] = 2 * 3.4e-4
            bad = (got - ref1).abs() > tol * torch.clamp_min(ref1.abs(), 1.0)
            assert not bool(bad.any()), f"{name} after Adam {k}: max|diff| {(got - ref1).abs().max().item():.3e}"
        # and the same through the one-call form (a second step from the updated parameters)
        assert torch.isfinite(mod.optimisation_step(G.Data(
            x=tt(z["x"], device), edge_index=tt(z["edge_index_in"], device), particle_id=tt(z["particle_id"], device),
            pt=tt(z["pt"], device), eta=tt(z["eta"], device), reconstructable=tt(z["reconstructable"], device),
            layer=tt(z["layer"], device), sector=tt(z["sector"], device))))


# ---- the same step at built-graph scale (golden G14b, generated by the reference's own TCModule)
TC_STEP_B_CASES = {
    "cfg5_rg": dict(loss="rg", gtcn=dict(h_outdim=8, hidden_dim=40, L_ec=3, L_hc=3, alpha_latent=0.9,
                                         n_embedding_coords=8), loss_w=(1.0, 0.1, 0.1)),
    "tiger_orphans_h24": dict(loss="tiger", gtcn=dict(h_outdim=4, hidden_dim=24, L_ec=2, L_hc=2,
                                                      mask_orphan_nodes=True, feed_edge_weights=True),
                              loss_w=(2.0, 0.25, 0.5)),
}
TC_B_MLGC = dict(embedding_slice=(0, 8), max_radius=1.0, max_num_neighbors=16)


def _check_after_adam(model, grads_ref: dict, p1_ref: dict, tag: str, lr_step: float = 3.4e-4):
    """Parameters after the step within 1e-6; where a gradient ELEMENT vanishes analytically (dead
    ReLU units, the translation-invariant last cluster bias) Adam turns rounding noise into a step
    of up to lr in EITHER direction - the sign of the noise is arbitrary in the reference's run and in ours -
    so those elements only have to stay within two steps of each other."""
    for k, v in model.state_dict().items():
        ref1 = tt(p1_ref[k]).double()
        got = v.detach().cpu().double()
        tol = torch.full_like(ref1, 1e-6)
        if k in grads_ref:
            tol[tt(grads_ref[k]).abs() < 1e-6] = 2 * lr_step
        bad = (got - ref1).abs() > tol * torch.clamp_min(ref1.abs(), 1.0)
        assert not bool(bad.any()), f"{tag} after Adam {k}: max|diff| {(got - ref1).abs().max().item():.3e}"


def case_tc_step_event(device, names=None):
    """Row H at built-graph scale (golden G14b: the reference's own ``TCModule`` on a 1500-hit event
    of the cfg5 generator - 21 617 kNN edges, about 1 600 kept by the cut - with the cfg5 model of
    bench.py and a Tiger / orphan-masking variant): built graph and both masks bit-exact (the
    golden's threshold sits in a gap of the weights of 2e-6), W / H / B and the loss terms 1e-5,
    all gradients 1e-4, parameters after the module's own Adam step 1e-6."""
    from gnn_tracking_amd import training
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    z = load("g14b_tc_step_event.npz")
    raw = {k: tt(z[k], device) for k in ("x", "particle_id", "pt", "eta", "reconstructable", "layer", "sector")}
    for name, cfg in TC_STEP_B_CASES.items():
        if names is not None and name not in names:
            continue
        model = G.GraphTCN(14, 28, ec_threshold=float(z[f"{name}/ec_threshold"]), **cfg["gtcn"])
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        lw_rep, lw_cow, lw_noise = cfg["loss_w"]
        loss_cls = CondensationLossTiger if cfg["loss"] == "tiger" else CondensationLossRG
        mod = training.TCModule(model, loss_fct=loss_cls(lw_repulsive=lw_rep, lw_coward=lw_cow, lw_noise=lw_noise),
                                preproc=G.MLGraphConstruction(ml=None, **TC_B_MLGC))
        data = mod.data_preproc(G.Data(edge_index=torch.zeros(2, 0, dtype=torch.long, device=raw["x"].device), **raw))
        assert torch.equal(data.edge_index.cpu(), tt(z[f"{name}/edge_index"])), name + " built edge_index"
        assert torch.equal(data.y.cpu(), tt(z[f"{name}/y"])), name + " edge labels"
        assert torch.equal(data.edge_attr[:64].cpu(), tt(z[f"{name}/edge_attr_head"])), name + " edge features"
        assert_close(data.edge_attr.double().sum(0), z[f"{name}/edge_attr_colsum"], 1e-9, name + " edge feature sums")
        out = mod(data, _preprocessed=True)
        margin = float(z[f"{name}/threshold_margin"])
        w_err = (out["W"].detach().cpu() - tt(z[f"{name}/W"])).abs().max().item()
        assert w_err < 0.25 * margin, f"{name}: |W - W_ref| {w_err:.1e} against a threshold margin of {margin:.1e}"
        assert torch.equal(out["ec_edge_mask"].cpu(), tt(z[f"{name}/ec_edge_mask"])), name + " edge mask"
        assert torch.equal(out["ec_hit_mask"].cpu(), tt(z[f"{name}/ec_hit_mask"])), name + " hit mask"
        assert int(out["ec_edge_mask"].sum()) > 1000
        for k in ("W", "H", "B"):
            assert_close(out[k], z[f"{name}/{k}"], TOL_OUT, f"{name} {k}")
        loss, metrics = mod.get_losses(out, data)
        for k in ("attractive", "repulsive", "coward", "noise"):
            assert_close(metrics[k], z[f"{name}/{k}"], TOL_OUT, f"{name} {k}")
        assert_close(loss, z[f"{name}/loss"], TOL_OUT, name + " loss")
        mod.zero_grad()
        loss.backward()
        grads_ref = {}
        for k, v in model.named_parameters():
            gk = v.grad if v.grad is not None else torch.zeros_like(v)
            grads_ref[k] = z[f"{name}/grad/{k}"]
            assert_close(gk, grads_ref[k], TOL_GRAD, f"{name} grad {k}")
        mod.configure_optimizers().step()
        _check_after_adam(model, grads_ref, {k: z[f"{name}/p1/{k}"] for k in model.state_dict()}, name)


def case_tc_step_oracle(device, n_hits=6000, loss="rg"):
    """The HIP ``TCModule`` step on the first ``n_hits`` hits of the cfg5 event (bench.py's own
    generator, model, kNN and loss settings; above the row thresholds of the pruned kNN search?
    no - 6 000 hits run the brute-force search; the spatial loss passes start at 16 384) against
    ``oracle.tc_training_step``: built graph bit-exact, EC cut identical (threshold placed in a gap
    of the ORACLE's weights, stated below), loss terms 1e-5, all gradients 1e-4, parameters after
    Adam 1e-6."""
    from gnn_tracking_amd import synthetic, training
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    ev = synthetic.make_pileup_event(500, 200_000, 8)
    g = np.random.default_rng(500)
    extra = torch.from_numpy(g.uniform(0, 1.5, size=(200_000, 6)).astype(np.float32))
    raw = {"x": torch.cat([ev["x"], extra], dim=1)[:n_hits].contiguous()}
    raw.update({k: ev[k][:n_hits].contiguous() for k in ("particle_id", "pt", "eta", "reconstructable")})
    gt = dict(h_outdim=8, hidden_dim=40, L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=8)
    mlgc = dict(embedding_slice=(0, 8), max_radius=1.0, max_num_neighbors=16)
    lw = (1.0, 0.1, 0.1)   # lw_repulsive, lw_coward, lw_noise
    torch.manual_seed(0)
    model = G.GraphTCN(14, 28, **gt)
    p0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    okw = dict(L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=8)
    # threshold: in a gap (>= 2e-6) of the oracle's own edge weights nearest to the median
    ei = O.knn_with_max_radius(raw["x"][:, :8], 16, 1.0)
    _, ea = O.ml_graph_construction_edges(raw["x"], raw["particle_id"], ei)
    pe = {k[len("_gtcn.ec."):]: v for k, v in p0.items() if k.startswith("_gtcn.ec.")}
    w0 = O.ec_for_graph_tcn(raw["x"], ei, ea, pe, L_ec=3)["W"].double().sort().values
    gaps = w0[1:] - w0[:-1]
    ok = torch.nonzero(gaps >= 2e-6).flatten()
    j = int(ok[(ok - len(w0) // 2).abs().argmin()])
    thr, margin = float((w0[j] + w0[j + 1]) / 2), float(gaps[j] / 2)
    graph, oo, terms, total, og, op = O.tc_training_step(raw, p0, mlgc=mlgc, gtcn=dict(okw, ec_threshold=thr),
                                                        loss_kind=loss, loss_weights=lw)
    model = G.GraphTCN(14, 28, ec_threshold=thr, **gt)
    model.load_state_dict(p0)
    model = model.to(device)
    loss_cls = CondensationLossTiger if loss == "tiger" else CondensationLossRG
    mod = training.TCModule(model, loss_fct=loss_cls(lw_repulsive=lw[0], lw_coward=lw[1], lw_noise=lw[2]),
                            preproc=G.MLGraphConstruction(ml=None, **mlgc))
    dev = torch.device(device)
    data = mod.data_preproc(G.Data(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev),
                                   **{k: v.to(dev) for k, v in raw.items()}))
    tag = f"TC step {n_hits} hits"
    assert torch.equal(data.edge_index.cpu(), graph["edge_index"]), tag + ": built graph"
    assert torch.equal(data.y.cpu(), graph["y"]) and torch.equal(data.edge_attr.cpu(), graph["edge_attr"]), tag
    out = mod(data, _preprocessed=True)
    w_err = (out["W"].detach().cpu() - oo["W"]).abs().max().item()
    assert w_err < 0.25 * margin, f"{tag}: |W - W_oracle| {w_err:.1e}, threshold margin {margin:.1e}"
    assert torch.equal(out["ec_edge_mask"].cpu(), oo["ec_edge_mask"]), tag + ": EC cut"
    assert torch.equal(out["ec_hit_mask"].cpu(), oo["ec_hit_mask"])
    for k in ("W", "H", "B"):
        assert_close(out[k], oo[k], TOL_OUT, f"{tag} {k}")
    l, metrics = mod.get_losses(out, data)
    for k in ("attractive", "repulsive", "coward", "noise"):
        assert_close(metrics[k], terms[k], TOL_OUT, f"{tag} {k}")
    assert_close(l, total, TOL_OUT, tag + " loss")
    mod.zero_grad()
    l.backward()
    for k, v in model.named_parameters():
        assert_close(v.grad if v.grad is not None else torch.zeros_like(v), og[k], TOL_GRAD, f"{tag} grad {k}")
    mod.configure_optimizers().step()
    _check_after_adam(model, og, op, tag)
    return {"hits": n_hits, "edges": int(graph["edge_index"].shape[1]), "kept": int(oo["ec_edge_mask"].sum()),
            "threshold_margin": margin, "w_err": w_err}


# ------------------------------------------------------------- ML training step (golden G15)
ML_STEP_CASES = {
    "d3_h64": dict(model=dict(in_dim=14, hidden_dim=64, out_dim=8, depth=3), loss=dict(max_num_neighbors=256),
                   lw_repulsive=0.5),
    "d1_h40_nrep": dict(model=dict(in_dim=14, hidden_dim=40, out_dim=8, depth=1, alpha=0.5),
                        loss=dict(max_num_neighbors=64, rep_normalization="n_rep_edges", r_emb=0.8), lw_repulsive=1.0),
}


def case_ml_step(device, names=None):
    """The metric-learning training step (golden G15: the reference's own ``MLModule`` on the 1500-hit
    event, two events through ``batch``): ``GraphConstructionFCNN`` -> hinge loss (radius graph
    inside the event, repulsion from hits of interest) -> backward -> Adam under the default
    ConstantLR: H 1e-5, edge counts exact, loss terms 1e-5, gradients 1e-4, parameters 1e-6."""
    from gnn_tracking_amd import training
    from gnn_tracking_amd.losses_ml import GraphConstructionHingeEmbeddingLoss

    z = load("g15_ml_step.npz")
    raw = {k: tt(z[k], device) for k in ("x", "particle_id", "pt", "eta", "reconstructable", "batch", "true_edge_index")}
    for name, cfg in ML_STEP_CASES.items():
        if names is not None and name not in names:
            continue
        model = G.GraphConstructionFCNN(**cfg["model"])
        load_params(model, z, f"{name}/p0/")
        model = model.to(device)
        mod = training.MLModule(model, loss_fct=GraphConstructionHingeEmbeddingLoss(lw_repulsive=cfg["lw_repulsive"],
                                                                                   **cfg["loss"]))
        data = G.Data(edge_index=raw["true_edge_index"], **raw)
        out = mod(data)
        assert_close(out["H"], z[f"{name}/H"], TOL_OUT, name + " H")
        loss, metrics = mod.get_losses(out, data)
        assert int(metrics["n_edges_rep"]) == int(z[f"{name}/n_edges_rep"]), name + " repulsive edge count"
        assert int(metrics["n_edges_att"]) == int(z[f"{name}/n_edges_att"]), name + " attractive edge count"
        for k in ("attractive", "repulsive"):
            assert_close(metrics[k], z[f"{name}/{k}"], TOL_OUT, f"{name} {k}")
        assert_close(loss, z[f"{name}/loss"], TOL_OUT, name + " loss")
        mod.zero_grad()
        loss.backward()
        grads_ref = {}
        for k, v in model.named_parameters():
            grads_ref[k] = z[f"{name}/grad/{k}"]
            assert_close(v.grad if v.grad is not None else torch.zeros_like(v), grads_ref[k], TOL_GRAD, f"{name} grad {k}")
        mod.configure_optimizers().step()
        _check_after_adam(model, grads_ref, {k: z[f"{name}/p1/{k}"] for k in model.state_dict()}, name)


def case_oc_sampling(device):
    """The reference's random sub-sampling switches of the condensation losses (oc.py:222-226,
    :322-328): ``max_n_rep`` keeps about that many repulsive pairs and rescales the normalisation
    (an unbiased estimate of the full term; the same pairs in forward and backward - checked by a
    directional finite difference; reproducible under ``torch.manual_seed``; ``n_rep`` reported
    before the sampling), ``sample_pids`` thins the hits of interest."""
    from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

    z = load("g5_oc.npz")
    t = {k: tt(z[f"td3/{k}"]) for k in ("beta", "x", "particle_id", "pt", "eta", "reconstructable")}
    kw = dict(particle_id=t["particle_id"].to(device), reconstructable=t["reconstructable"].float().to(device),
              pt=t["pt"].float().to(device), eta=t["eta"].float().to(device))
    beta = t["beta"].float().to(device)
    x0 = t["x"].float().to(device)
    full = CondensationLossTiger(lw_repulsive=1.0)(beta=beta, x=x0, **kw)
    n_rep = int(full.extra_metrics["n_rep"])
    assert n_rep > 300, "case needs repulsive pairs"
    sub = CondensationLossTiger(lw_repulsive=1.0, max_n_rep=n_rep // 3)

    def run(x):
        torch.manual_seed(123)
        return sub(beta=beta, x=x, **kw)

    r1, r2 = run(x0), run(x0)
    assert int(r1.extra_metrics["n_rep"]) == n_rep, "n_rep is the count before the sub-sampling"
    assert float(r1.loss_dct["repulsive"]) == float(r2.loss_dct["repulsive"]), "same seed, same pairs"
    assert_close(r1.loss_dct["attractive"], full.loss_dct["attractive"], 1e-6, "attractive is not sampled")
    rel = abs(float(r1.loss_dct["repulsive"]) - float(full.loss_dct["repulsive"])) / float(full.loss_dct["repulsive"])
    assert rel < 0.3, f"sub-sampled repulsive term off by {rel:.2f} (a third of {n_rep} pairs)"
    torch.manual_seed(7)
    assert float(sub(beta=beta, x=x0, **kw).loss_dct["repulsive"]) != float(r1.loss_dct["repulsive"]), "seed ignored"
    # forward and backward use the same pairs: directional derivative of the sampled repulsive term at a
    # FIXED keep probability and seed (through the loss class the probability itself moves with x)
    from gnn_tracking_amd.losses_oc import _CondensationPotentials
    from gnn_tracking_amd.graph_masks import get_good_node_mask_tensors

    mask = get_good_node_mask_tensors(pt=kw["pt"], particle_id=kw["particle_id"], reconstructable=kw["reconstructable"],
                                      eta=kw["eta"])

    def rep(x, b):
        return _CondensationPotentials.apply(b, x, kw["particle_id"], mask, 0.01, 1.0, 0.0, 1, 0.4, 99)[1]

    xg = x0.clone().requires_grad_(True)
    bg = beta.clone().requires_grad_(True)
    rep(xg, bg).backward()
    g = np.random.default_rng(2)
    d = tt(g.normal(size=tuple(x0.shape)).astype(np.float32), device)
    eps = 2e-3
    fd = (float(rep(x0 + eps * d, beta)) - float(rep(x0 - eps * d, beta))) / (2 * eps)
    an = float((xg.grad * d).sum())
    assert abs(fd - an) <= 0.05 * max(abs(an), abs(fd)) + 1e-7, f"finite difference {fd:.4e} vs autograd {an:.4e}"
    assert torch.isfinite(bg.grad).all()
    full_rep = _CondensationPotentials.apply(beta, x0, kw["particle_id"], mask, 0.01, 1.0, 0.0, 1)[1]
    assert abs(float(rep(x0, beta)) - float(full_rep)) < 0.3 * float(full_rep)
    # sample_pids: fewer hits of interest, still a valid loss; reproducible
    for cls in (CondensationLossRG, CondensationLossTiger):
        torch.manual_seed(5)
        a = cls(sample_pids=0.5)(beta=beta, x=x0, **kw)
        torch.manual_seed(5)
        b = cls(sample_pids=0.5)(beta=beta, x=x0, **kw)
        assert torch.isfinite(a.loss) and float(a.loss) == float(b.loss)
        assert float(a.loss_dct["attractive"]) != float(cls()(beta=beta, x=x0, **kw).loss_dct["attractive"])


def case_knn_batched(device, sizes=(1, 5, 70, 130, 2, 64)):
    """One batched search (``seg_ptr`` = torch_cluster's ``batch``) == the per-event searches,
    bit for bit: events smaller than k, single-hit events, waves that straddle two events."""
    g = np.random.default_rng(8)
    n = sum(sizes)
    for d, k, r in ((3, 4, None), (8, 16, 0.9), (2, 100, 0.5)):
        x = tt(g.random((n, d)).astype(np.float32), device)
        seg_ptr = torch.tensor([0, *np.cumsum(sizes)], dtype=torch.int64, device=device)
        got = ops.knn_graph(x, k, r, seg_ptr=seg_ptr)
        parts, off = [], 0
        for s_ in sizes:
            if s_ > 1:
                parts.append(ops.knn_graph(x[off:off + s_].contiguous(), k, r) + off)
            off += s_
        want = torch.cat(parts, dim=1)
        assert torch.equal(got, want), f"batched kNN d={d} k={k} r={r}"
    from gnn_tracking_amd.losses_ml import radius_graph
    batch = torch.repeat_interleave(torch.arange(len(sizes), device=device), torch.tensor(sizes, device=device))
    assert torch.equal(radius_graph(x, 0.5, batch, 100), want)


def case_knn_pruned(device, shapes=((700, 8, 16, 1.0), (300, 3, 4, None), (513, 2, 70, 0.3), (200, 5, 100, None),
                                    (64, 4, 5, 0.5), (65, 8, 3, None), (400, 3, 256, 0.8), (600, 12, 16, 1.0),
                                    (300, 16, 70, None)), with_oracle=True,
                    batched_sizes=(1, 5, 70, 130, 2, 64)):
    """The pruned search (sorted chunks + bounding-box lower bounds, ``gnntrk_knn_search_ws``) against
    the brute-force kernel and the C oracle, bit for bit: clustered clouds with noise (boxes that
    prune), plain uniform ones (nothing to prune), no radius (thresholds start at infinity), ties
    (duplicated points), k beyond the first buffer size, events of a collated batch."""
    g = np.random.default_rng(12)
    old = ops._KNN_FLAGS

    def search(x, k, r, seg_ptr, flags):
        ops._KNN_FLAGS = flags
        try:
            return ops.knn_graph(x, k, r, seg_ptr=seg_ptr)
        finally:
            ops._KNN_FLAGS = old

    for (n, d, k, r) in shapes:
        centres = g.uniform(-2, 2, size=(max(n // 30, 1), d))
        x = centres[g.integers(0, len(centres), size=n)] + 0.05 * g.normal(size=(n, d))
        x[::11] = g.uniform(-2, 2, size=(len(x[::11]), d))      # noise hits
        x[5::50] = x[4::50][:len(x[5::50])]                     # exact duplicates: ties by index
        x = tt(x.astype(np.float32))
        pruned, brute = search(x.to(device), k, r, None, 1), search(x.to(device), k, r, None, 2)
        assert torch.equal(pruned, brute), f"pruned kNN != brute force: n={n} d={d} k={k} r={r}"
        if with_oracle:
            assert torch.equal(pruned.cpu(), O.knn_graph_c(x, k, r)), f"pruned kNN vs oracle n={n} d={d} k={k} r={r}"
    x = torch.zeros(200, 3)
    x[100:] = 1.0  # two points only: every box is degenerate
    assert torch.equal(search(x.to(device), 5, None, None, 1), search(x.to(device), 5, None, None, 2))
    if batched_sizes:
        n = sum(batched_sizes)
        seg_ptr = torch.tensor([0, *np.cumsum(batched_sizes)], dtype=torch.int64, device=device)
        for d, k, r in ((3, 4, None), (8, 16, 0.9)):
            x = tt(g.random((n, d)).astype(np.float32), device)
            assert torch.equal(search(x, k, r, seg_ptr, 1), search(x, k, r, seg_ptr, 2)), f"batched pruned d={d} k={k}"


def case_rg_neighbor_cap(device, caps=(4, 16, 256), n_hits=None):
    """``CondensationLossRG.neighbor_cap = "nearest"``: the radius graph's ``max_num_neighbors`` cap
    applied nearest first, against the oracle (whose radius graph truncates nearest first) where the
    cap binds hard (4 and 16 neighbours on hits with dozens inside the radius): loss terms and
    gradients; and unchanged results where it does not bind (256)."""
    from gnn_tracking_amd.losses_oc import CondensationLossRG

    z = load("g5_oc.npz")
    t = {k: tt(z[f"td3/{k}"])[:n_hits] for k in ("beta", "x", "particle_id", "pt", "eta", "reconstructable")}
    beta32, x32 = t["beta"].float(), t["x"].float()
    mask = O.good_node_mask(t["pt"].float(), t["particle_id"], t["reconstructable"].float(), t["eta"].float())
    kw = dict(particle_id=t["particle_id"].to(device), reconstructable=t["reconstructable"].float().to(device),
              pt=t["pt"].float().to(device), eta=t["eta"].float().to(device))
    old = CondensationLossRG.neighbor_cap
    try:
        CondensationLossRG.neighbor_cap = "nearest"
        small = None
        for cap in caps:
            bo, xo = beta32.clone().requires_grad_(True), x32.clone().requires_grad_(True)
            od = O.condensation_loss_rg(beta=bo, x=xo, particle_id=t["particle_id"], mask=mask, max_num_neighbors=cap)
            (od["attractive"] + 2.0 * od["repulsive"]).backward()
            b, x = beta32.clone().to(device).requires_grad_(True), x32.clone().to(device).requires_grad_(True)
            ret = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=cap)(beta=b, x=x, **kw)
            (ret.loss_dct["attractive"] + 2.0 * ret.loss_dct["repulsive"]).backward()
            for k in ("attractive", "repulsive"):
                assert_close(ret.loss_dct[k], od[k], TOL_OUT, f"cap {cap} {k}")
            assert_close(x.grad, xo.grad, 2e-4, f"cap {cap} grad x")
            assert_close(b.grad, bo.grad, 2e-4, f"cap {cap} grad beta")
            if cap == 256:   # does not bind on this cloud: must equal the uncapped sum
                CondensationLossRG.neighbor_cap = "off"
                off = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=4)(
                    beta=beta32.clone().to(device), x=x32.clone().to(device), **kw)
                CondensationLossRG.neighbor_cap = "nearest"
                assert_close(off.loss_dct["repulsive"], float(ret.loss_dct["repulsive"]), 1e-6, "cap off == cap that does not bind")
            else:
                small = float(ret.loss_dct["repulsive"].detach())
        CondensationLossRG.neighbor_cap = "off"
        off = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=4)(beta=beta32.clone().to(device),
                                                                        x=x32.clone().to(device), **kw)
        assert small < 0.9 * float(off.loss_dct["repulsive"]), "the cap should have removed repulsive pairs in this case"
        # "auto" (the default): one count pass decides - nearest first where a hit has more neighbours than the cap,
        # the plain sum (= the reference) where none has
        CondensationLossRG.neighbor_cap = "auto"
        for cap, want in ((caps[0], small if len(caps) > 1 and caps[0] != 256 else None), (100000, float(off.loss_dct["repulsive"]))):
            m = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=cap)
            ret = m(beta=beta32.clone().to(device), x=x32.clone().to(device), **kw)
            if cap == 100000:
                assert m._cap_binds is False if x32.shape[0] - 1 > cap else getattr(m, "_cap_binds", None) is None
                assert_close(ret.loss_dct["repulsive"], want, 1e-6, "auto == off where the cap cannot bind")
            else:
                assert m._cap_binds is True, "auto must notice that the cap binds"
                CondensationLossRG.neighbor_cap = "nearest"
                ref = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=cap)(
                    beta=beta32.clone().to(device), x=x32.clone().to(device), **kw)
                CondensationLossRG.neighbor_cap = "auto"
                assert float(ret.loss_dct["repulsive"]) == float(ref.loss_dct["repulsive"]), "auto == nearest where it binds"
        m = CondensationLossRG(lw_repulsive=2.0, max_num_neighbors=min(256, x32.shape[0] - 2))
        ret = m(beta=beta32.clone().to(device), x=x32.clone().to(device), **kw)
        assert m._cap_binds is False
        assert_close(ret.loss_dct["repulsive"], float(off.loss_dct["repulsive"]), 1e-6, "auto == off at the default cap on this cloud")
    finally:
        CondensationLossRG.neighbor_cap = old
