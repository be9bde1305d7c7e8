"""The object-condensation training step on a collated batch of events, end to end on the device:
``TCModule.training_step(collate(events))`` (``MLGraphConstruction`` per event -> ``GraphTCN`` -> condensation loss
per event, mean over the events -> backward) against ``oracle.ref_cpu.tc_training_step`` run on every event alone and
averaged - three events of 1500, 1100 and 700 hits from the cfg5 generator, cfg5's model and loss settings, as
``parity_cases.case_tc_step_oracle`` does for one event: built graph and both masks exact, loss terms 1e-5, all
parameter gradients 1e-4.  Under bf16 storage the batch is compared with its own three single-event bf16 runs
(1e-4 of the largest entry of each parameter's gradient, the bar of ``parity_cases.case_full_size_backward``)."""

import functools

import numpy as np
import pytest
import torch

import gnn_tracking_amd as G
import parity_cases as P
import ref_cpu as O
from gnn_tracking_amd import ops, synthetic, training
from gnn_tracking_amd.losses_oc import CondensationLossRG, CondensationLossTiger

pytestmark = pytest.mark.gpu
DEVICE = "cuda"
HITS = (1500, 1100, 700)
GT = dict(h_outdim=8, hidden_dim=40, L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=8)
OKW = dict(L_ec=3, L_hc=3, alpha_latent=0.9, n_embedding_coords=8)
MLGC = dict(embedding_slice=(0, 8), max_radius=1.0, max_num_neighbors=16)
LW = (1.0, 0.1, 0.1)   # lw_repulsive, lw_coward, lw_noise
LOSSES = {"rg": (CondensationLossRG, {}), "tiger": (CondensationLossTiger, dict(mask_orphan_nodes=True))}


@functools.lru_cache(maxsize=None)
def _events():
    out = []
    for i, n in enumerate(HITS):
        # (cfg5's cloud at a tenth of its size: ids of 2000 particles, so that they repeat inside and across events)
        ev = synthetic.make_pileup_event(600 + i, 20_000, 8, n_particles=2000, n_clusters=600)
        g = np.random.default_rng(600 + i)
        extra = torch.from_numpy(g.uniform(0, 1.5, size=(20_000, 6)).astype(np.float32))
        raw = {"x": torch.cat([ev["x"], extra], dim=1)[:n].contiguous()}
        raw.update({k: ev[k][:n].contiguous() for k in ("particle_id", "pt", "eta", "reconstructable")})
        out.append(raw)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _setup():
    """initial parameters and an EC threshold in a gap (>= 2e-6) of the ORACLE's edge weights over all three events,
    nearest to their median"""
    torch.manual_seed(0)
    p0 = {k: v.detach().clone() for k, v in G.GraphTCN(14, 28, **GT).state_dict().items()}
    pe = {k[len("_gtcn.ec."):]: v for k, v in p0.items() if k.startswith("_gtcn.ec.")}
    ws = []
    for raw in _events():
        ei = O.knn_with_max_radius(raw["x"][:, :8], 16, 1.0)
        _, ea = O.ml_graph_construction_edges(raw["x"], raw["particle_id"], ei)
        ws.append(O.ec_for_graph_tcn(raw["x"], ei, ea, pe, L_ec=3)["W"].double())
    w0 = torch.cat(ws).sort().values
    gaps = w0[1:] - w0[:-1]
    ok = torch.nonzero(gaps >= 2e-6).flatten()
    j = int(ok[(ok - len(w0) // 2).abs().argmin()])
    return p0, float((w0[j] + w0[j + 1]) / 2), float(gaps[j] / 2)


@functools.lru_cache(maxsize=None)
def _oracle(loss):
    p0, thr, _ = _setup()
    return tuple(O.tc_training_step(raw, p0, mlgc=MLGC, gtcn=dict(OKW, ec_threshold=thr, **LOSSES[loss][1]),
                                    loss_kind=loss, loss_weights=LW) for raw in _events())


def _module(loss):
    p0, thr, _ = _setup()
    model = G.GraphTCN(14, 28, ec_threshold=thr, **GT, **LOSSES[loss][1])
    model.load_state_dict(p0)
    model = model.to(DEVICE)
    mod = training.TCModule(model, loss_fct=LOSSES[loss][0](lw_repulsive=LW[0], lw_coward=LW[1], lw_noise=LW[2]),
                            preproc=G.MLGraphConstruction(ml=None, **MLGC))
    return model, mod


def _data(raw):
    dev = torch.device(DEVICE)
    return G.Data(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev), **{k: v.to(dev) for k, v in raw.items()})


@pytest.mark.parametrize("loss", tuple(LOSSES))
def test_batched_step_against_the_oracle_per_event(loss):
    _, _, margin = _setup()
    per_event = _oracle(loss)
    model, mod = _module(loss)
    data = mod.data_preproc(G.collate([_data(raw) for raw in _events()]))
    offs = np.cumsum((0,) + HITS)
    tag = f"batched TC step {loss}"
    assert torch.equal(data.edge_index.cpu(), torch.cat([r[0]["edge_index"] + int(o) for r, o in zip(per_event, offs)], dim=1)), tag + ": built graph"
    assert torch.equal(data.y.cpu(), torch.cat([r[0]["y"] for r in per_event])), tag
    assert torch.equal(data.edge_attr.cpu(), torch.cat([r[0]["edge_attr"] for r in per_event])), tag
    assert torch.equal(data.batch.cpu(), torch.repeat_interleave(torch.arange(3), torch.tensor(HITS)))
    out = mod(data, _preprocessed=True)
    w_err = (out["W"].detach().cpu() - torch.cat([r[1]["W"] for r in per_event])).abs().max().item()
    assert w_err < 0.25 * margin, f"{tag}: |W - W_oracle| {w_err:.1e}, threshold margin {margin:.1e}"
    for k in ("ec_edge_mask", "ec_hit_mask"):
        assert torch.equal(out[k].cpu(), torch.cat([r[1][k] for r in per_event])), f"{tag}: {k}"
    if loss == "tiger":
        assert not bool(out["ec_hit_mask"].all()), "no orphan node: the hit mask does nothing"
    l, metrics = mod.get_losses(out, data)
    for k in ("attractive", "repulsive", "coward", "noise"):
        P.assert_close(metrics[k], sum(r[2][k] for r in per_event) / 3, P.TOL_OUT, f"{tag} {k}")
    P.assert_close(l, sum(r[3] for r in per_event) / 3, P.TOL_OUT, tag + " loss")
    mod.zero_grad()
    l.backward()
    for k, v in model.named_parameters():
        want = sum(r[4][k] for r in per_event) / 3
        P.assert_close(v.grad if v.grad is not None else torch.zeros_like(v), want, P.TOL_GRAD, f"{tag} grad {k}")


def test_batched_step_in_bf16_storage_against_its_single_event_runs():
    """(the events' share 1/3 enters as the upstream gradient of their loss, as in ``case_full_size_backward``: the
    bf16 activation gradients are then rounded at the scale they have inside the batch).  Measured on an MI355X: every
    parameter at 1e-6 or below except ``p_cluster.layers.4.bias`` at 5.2e-5 - the bias of the cluster coordinates, whose
    exact gradient is 0 (the potentials depend on coordinate differences only): its entries are the rounding residue of
    the sum over the hits, and so is the difference."""
    model, mod = _module("rg")
    names = [k for k, _ in model.named_parameters()]

    def backward(d, scale):
        ops.clear_graph_index_cache()
        model.zero_grad(set_to_none=True)
        with G.bf16_storage(True):
            loss, _ = mod.training_step(d)
            (loss * scale).backward()
        return float(loss.detach()), [p.grad.double() if p.grad is not None else torch.zeros_like(p, dtype=torch.float64)
                                      for p in model.parameters()]

    loss_b, g_batch = backward(G.collate([_data(raw) for raw in _events()]), 1.0)
    acc, loss_sum = [torch.zeros_like(g) for g in g_batch], 0.0
    for raw in _events():
        l, gs = backward(_data(raw), 1.0 / 3.0)
        loss_sum += l / 3.0
        for a, g in zip(acc, gs):
            a += g
    assert abs(loss_b - loss_sum) <= 1e-5 * abs(loss_sum), f"loss {loss_b!r}, mean of the events {loss_sum!r}"
    for k, a, g in zip(names, acc, g_batch):
        err = float((a - g).abs().max()) / max(float(a.abs().max()), 1e-30)
        print(f"bf16 {k}: {err:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= 1e-4, f"bf16 grad {k}: {err:.2e} of the largest entry"
