"""Parity tests proper: the HIP path (libgnntrk.so through the C ABI) on a real MI355X
against the golden vectors generated from the reference, and against the CPU oracle."""

import pytest
import torch

import parity_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnn_tracking_amd import _capi

    lib = _capi.load()  # fails loudly if the extension is missing
    assert lib.gnntrk_version() == 600
    return "cuda"


def test_graph_index(dev):
    P.case_graph_index(dev, big=True)


def test_node_order(dev):
    P.case_node_order(dev)


def test_graph_index_placed_from_cached_events(dev):
    P.case_graph_index_place(dev)
    P.case_graph_index_place(dev, order=False)
    P.case_graph_index_place(dev, sizes=((150_000, 2_000_000), (70_001, 1_000_002), (150_000, 2_000_000)))


def test_resident_dataset(dev):
    P.case_resident_dataset(dev)


def test_graph_index_carry_and_fused_bce(dev):
    P.case_graph_index_carry(dev)
    P.case_ec_carry_equals_gather(dev)


def test_gradient_folds_need_one_autograd_tensor(dev):
    P.case_fold_alias(dev)


def test_parameter_gradients_added_in_place_equal_autograd_accumulation(dev):
    P.case_grad_sink(dev)


def test_fused_mlp_forward_backward(dev):
    P.case_mlp(dev)
    P.case_mlp(dev, shapes=((14, 40, 4, 3), (26, 40, 1, 3)), rows=40001)


def test_fused_mlp_stress(dev):
    P.case_mlp_stress(dev, rounds=4)


def test_interaction_network_layer(dev):
    P.case_in_layer(dev)


def test_resin_variants(dev):
    P.case_resin(dev)


def test_ec_testgraph_training_step(dev):
    P.case_ec_testgraph(dev)


def test_ec_variants(dev):
    P.case_ec_variants(dev)


def test_edge_cases(dev):
    P.case_edge_cases(dev, modes=("f32", "bf16"))


def test_knn_goldens_and_oracle(dev):
    P.case_knn_goldens(dev)
    P.case_knn_oracle(dev)
    P.case_knn_oracle(dev, shapes=((5000, 8, 64, 1.0), (4097, 3, 256, None), (3000, 24, 16, 2.0)))
    P.case_knn_batched(dev)
    P.case_knn_batched(dev, sizes=(3000, 1, 2500, 40, 4000))


def test_knn_pruned_equals_brute_force(dev):
    P.case_knn_pruned(dev)
    # above the row threshold (the pruned form is what knn_graph runs by default there): many
    # batches of boxes, both buffer sizes, events
    P.case_knn_pruned(dev, shapes=((20000, 8, 16, 1.0), (9000, 3, 64, None), (12000, 6, 100, 0.5), (8200, 2, 9, None),
                                   (10000, 8, 256, 1.0), (9000, 12, 16, 1.5), (8500, 16, 100, None)),
                      with_oracle=False, batched_sizes=(3000, 1, 9000, 40, 4500))
    P.case_knn_pruned(dev, shapes=((9000, 8, 16, 1.0),), batched_sizes=())


def test_ml_graph_construction(dev):
    P.case_ml_graph_construction(dev)


def test_condensation_losses(dev):
    P.case_good_node_mask(dev)
    P.case_condensation_losses(dev)
    P.case_oc_sampling(dev)
    P.case_rg_neighbor_cap(dev)


def test_condensation_losses_spatial_passes(dev):
    P.case_oc_spatial(dev)


def test_cpu_tensor_is_rejected(dev):
    import gnn_tracking_amd as G

    m = G.MLP(4, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        m(torch.zeros(3, 4))


# ---- bf16-storage mode (BASELINE configs 3/4) ------------------------------------------
def test_bf16_mlp_forward(dev):
    P.case_mlp_bf16_forward(dev, rows=1000)
    P.case_mlp_bf16_forward(dev, rows=16 * 4 * 8 * 5 + 3)  # several tile groups per wave


def test_bf16_mlp_backward(dev):
    P.case_mlp_bf16_backward(dev, rows=1000)
    P.case_mlp_bf16_backward(dev, rows=100_000, full=False)


def test_graph_tcn_wide_hidden_bf16(dev):
    P.case_graph_tcn_wide_hidden_bf16(dev)
    P.case_graph_tcn_wide_hidden_bf16(dev, hiddens=(64, 127), n_hits=20_000, n_edges=200_000)


def test_bf16_mlp_stress(dev):
    P.case_mlp_bf16_stress(dev, rounds=6)
    P.case_mlp_bf16_stress(dev, rounds=6, seed=29, wide=True)   # + hidden widths 63 .. 128
    P.case_mlp_bf16_stress(dev, rounds=4, seed=31, wide_io=True)   # output tiles / three - four k-steps of inputs


def test_bf16_edge_classifier(dev):
    # all residual layouts / head inputs; includes the pin against the reference's own modules
    # under bf16 autocast (golden G2b) - the report holds the measured distances
    for name, rep in P.case_ec_bf16(dev, names=tuple(P.EC_VARIANTS)).items():
        print("bf16 vs reference autocast:", name, {k: float(f"{v:.3g}") for k, v in rep.items()})


def test_bf16_backward_is_reproducible(dev):
    """Fixed-order partial reduction: two runs give bit-identical parameter gradients."""
    P.case_bf16_reproducible(dev)


def test_bf16_row_helpers(dev):
    P.case_rows_bf16(dev)


def test_training_step_is_hipgraph_capturable(dev):
    P.case_hipgraph_capture(dev)


def test_graph_tcn(dev):
    P.case_graph_tcn(dev)


def test_graph_tcn_bf16_storage(dev):
    P.case_graph_tcn_bf16(dev)
    # the pin against the reference's own GraphTCN under bf16 autocast (golden G7b)
    for name, rep in P.case_graph_tcn_bf16_autocast(dev).items():
        print("GraphTCN bf16 vs reference autocast:", name, {k: float(f"{v:.3g}") for k, v in rep.items()})


def test_hinge_embedding_loss(dev):
    P.case_hinge_loss(dev)


def test_graph_construction_fcnn(dev):
    P.case_gc_fcnn(dev)


def test_res_fcnn_and_hinge_kernels(dev):
    print("res_fcnn worst weight-gradient error:", P.case_res_fcnn(dev))
    P.case_hinge_terms(dev)
    P.case_hinge_terms(dev, n=20_000, dim=12, n_edges=300_000)


def test_mlp_wide(dev):
    P.case_mlp_wide(dev)


def test_node_tap(dev):
    P.case_node_tap(dev)


def test_segment_sum_f32(dev):
    P.case_segment_sum_f32(dev)


def test_in_edge_wide(dev):
    P.case_in_edge_wide(dev)


def test_hetero_fcnn(dev):
    P.case_hetero_fcnn(dev)


def test_graph_cut(dev):
    P.case_graph_cut(dev, big=3_000_000)


def test_workspace_exact(dev):
    P.case_workspace_exact(dev)


def test_dbscan(dev):
    P.case_dbscan(dev)
    P.case_dbscan_pruned(dev, n_big=30000)


def test_full_size_properties(dev):
    P.case_full_size_properties(dev)


def test_full_size_backward_properties(dev):
    """cfg3's backward at its full size (64 M rows), fp32 and bf16 storage: batch gradient == sum of the
    single-event gradients, run-to-run bit-identity, in-place parameter gradients == autograd's."""
    print(P.case_full_size_backward(dev))


def test_graph_construction_resin(dev):
    P.case_gc_resin(dev)


def test_focal_losses(dev):
    P.case_focal_losses(dev)


def test_pc_transformer(dev):
    P.case_pc_transformer(dev)


def test_edge_ordered_outputs(dev):
    P.case_edge_ordered(dev)


def test_tc_training_step(dev):
    P.case_tc_step(dev)


def test_ml_training_step(dev):
    """golden G15: the reference's own MLModule (GraphConstructionFCNN + hinge loss + Adam)"""
    P.case_ml_step(dev)


def test_tc_training_step_event_scale(dev):
    """golden G14b: the reference's own TCModule on a 1500-hit event, cfg5 model + Tiger variant"""
    P.case_tc_step_event(dev)


def test_tc_training_step_vs_oracle_6k_hits(dev):
    """the cfg5 step (bench.py's event, model, kNN, loss) on 6000 hits against oracle.tc_training_step,
    every value compared; and on 20 000 hits (pruned kNN search + spatial loss passes in the path)"""
    print(P.case_tc_step_oracle(dev, n_hits=6000))
    print(P.case_tc_step_oracle(dev, n_hits=20000))


# ---- BASELINE.json configs on their own workloads ---------------------------------------
def test_cfg1_cfg2_event_vs_oracle(dev):
    P.case_cfg12_event(dev)


def test_cfg5_condensation_losses_200k(dev):
    print(P.case_cfg5_condensation(dev))


def test_cfg5_knn_200k(dev):
    P.case_cfg5_knn(dev)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_bench_cfg4_two_ranks_match_one_rank(dev, dtype):
    """BASELINE config 4 on its own workload - ALL 256 events (hits ~ U(100 k, 200 k), 8 size-balanced
    shards of 32 events): bench.py's own launcher starts two ranks (gloo, both on this GPU - RCCL
    needs one GPU per rank), each runs its four of the eight shards as micro-batches, gradients are
    all-reduced; the parameters after the run must equal the one-rank run's (same arithmetic: the
    mean over all eight shards).  The line names the backend and only claims RCCL under nccl.
    ``bf16`` is the precision BASELINE.md states for this config (bf16 storage, fp32 accumulation and
    parameters: every micro-batch's gradient is bit-reproducible, the two runs differ in the fp32 order
    in which the eight micro-batch gradients are summed); ``f32`` is the reference's precision."""
    import json
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    outs = {}
    for n in (1, 2):
        cmd = [sys.executable, str(root / "bench.py"), "--gpus", str(n), "--workload", "cfg4",
               "--steps", "2", "--warmup", "1", "--full", "--no-extra", "--no-cpu-baseline", "--dtype", dtype]
        if n > 1:
            cmd += ["--backend", "gloo"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[n] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    a, b = outs[1], outs[2]
    assert a["dtype"] == b["dtype"] == dtype
    assert a["backend"] == "none" and "rccl_ranks" not in a
    assert b["n_gpus"] == 2 and b["backend"] == "gloo" and "rccl_ranks" not in b and b["self_launched"] is True
    assert "RCCL" not in b["config"]["parallelism"]
    assert a["scaling"] == b["scaling"] == "strong"
    assert a["config"]["events"] == b["config"]["events"] == 256
    assert a["config"]["global_edges_per_step"] == b["config"]["global_edges_per_step"] > 4e8
    assert a["config"]["micro_batches_per_rank"] == 8 and b["config"]["micro_batches_per_rank"] == 4
    assert a["config"]["shard_edges_max_over_mean"] < 1.01 and b["config"]["rank_edges_max_over_mean"] < 1.01
    rel = abs(a["param_checksum"] - b["param_checksum"]) / a["param_checksum"]
    print(f"cfg4 {dtype}: |checksum(1 rank) - checksum(2 ranks)| / checksum = {rel:.2e}")
    assert rel < 1e-6, f"parameters after the run differ between 1 and 2 ranks: {rel:.2e}"


def test_bench_cfg5_step_runs_in_both_storage_modes(dev):
    """bench.py --workload cfg5 end to end (the object-condensation step: pruned kNN graph build ->
    GraphTCN -> spatial condensation-loss passes -> backward -> Adam) on a reduced event, fp32 and bf16
    storage: one JSON line with the stage times, a finite loss that the two modes agree on to bf16
    accuracy, the same graph."""
    import json
    import math
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    outs = {}
    for dt in ("f32", "bf16"):
        cmd = [sys.executable, str(root / "bench.py"), "--workload", "cfg5", "--events", "30000", "--dtype", dt,
               "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[dt] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for dt, o in outs.items():
        assert o["dtype"] == dt and o["config"]["workload"].startswith("cfg5")
        assert set(o["stages"]) >= {"graph_build", "model_forward", "oc_loss_forward", "backward"}
        assert math.isfinite(o["final_loss"]) and o["value"] > 0
    assert outs["f32"]["config"]["edges_built"] == outs["bf16"]["config"]["edges_built"]
    assert abs(outs["f32"]["final_loss"] - outs["bf16"]["final_loss"]) <= 0.02 * abs(outs["f32"]["final_loss"])


def test_pruned_paths_random_stress(dev):
    """tools/gpu_stress_pruned.py, a short run: the sorted-chunk kNN search, the DBSCAN radius graph
    and the spatial condensation-loss passes against their exhaustive forms on random sizes around
    the chunk / batch boundaries, 1..16 dimensions, k up to 448, event splits."""
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "tools" / "gpu_stress_pruned.py"), "5", "10"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "pruned stress ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


def test_mlp_bf16_in_kernel_fold(dev):
    """gnntrk_gfold: the target-gathered segment's gradient summed per node inside the backward kernel - relational
    and head shapes, carries / carry chains / id windows / isolated nodes / the tail unit (60 + 24 configurations)."""
    assert P.case_mlp_bf16_fold(dev) == 3 * 7 * 4


def test_bf16_instantiations(dev):
    """Every branch of the bf16 launchers' selection: kernel names and probe answers are the recorded literals, the
    launches run and agree with the generic I/O (17 forward + 23 backward entries, 33 rows and 1)."""
    assert P.case_bf16_instantiations(dev) == 2 * (17 + 23)


def test_cfg3_full_size_event_against_oracle(dev):
    rep = P.case_cfg3_event(dev)
    print("cfg3 event:", rep)


def test_cfg3_full_size_event_second_seed_low_pt_falsified(dev):
    """Another event of the bench's batch (seed 117) with ``EdgeWeightBCELoss(pt_thld=0.9)`` - the labels of edges
    whose source hit is below the pt threshold falsified inside the loss kernel (losses/ec.py:71-92) - in the
    headline's precision, value for value against the oracle."""
    rep = P.case_cfg3_event(dev, modes=("bf16",), seed=117, pt_thld=0.9)
    print("cfg3 event, seed 117, pt_thld 0.9:", rep)


def test_bench_default_line_is_one_small_json_line(dev):
    """``python bench.py --full`` (here: two events, no side runs) prints exactly ONE stdout line, well below the size the
    driver's parser lost in round 5, carrying ``roofline`` (with the live access floors), ``cpu_baseline`` and
    ``parity_check``; the full record goes to ``bench_extra.json`` and stderr."""
    import json
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--events", "2", "--steps", "3", "--warmup", "2",
                        "--full", "--cpu-iters", "1", "--no-extra"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(out) == 1 and len(out[0].encode()) < 8192, (len(out), [len(o) for o in out])
    d = json.loads(out[0])
    assert d["metric"] == "edges_per_sec_fwd_bwd" and d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "bf16"
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and 0 < roof["frac"] < 1 and roof["peak"] == 8000.0 and "IoRelational" in roof["kernel"]
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1
    assert d["parity_check"]["ok"] is True and d["parity_check"]["max_abs_W"] <= d["parity_check"]["bound"] <= 5e-4
    full = json.loads((root / "bench_extra.json").read_text())
    assert full["ms_per_step"] == __import__("pytest").approx(d["ms_per_step"], rel=1e-4) and len(full["kernels"]) >= 8


def test_bench_plain_run_dumps_its_last_step(dev, tmp_path):
    """A plain ``python bench.py`` times the steps and nothing else (no roofline, CPU baseline or parity check),
    and ``--dump-outputs`` writes what the last timed step computed: the edge weights in edge_index order (a seeded
    sample of the rows), the embeddings, loss, parameters and gradients, float32 / float64, within 64 MB."""
    import json
    import math
    import pathlib
    import subprocess
    import sys

    import numpy as np

    root = pathlib.Path(__file__).resolve().parent.parent
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--events", "2", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] == "edges_per_sec_fwd_bwd" and d["steps"] == 2 and d["dtype"] == "bf16" and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] == __import__("pytest").approx(
        d["config"]["global_edges_per_step"] / (d["ms_per_step"] * 1e-3), rel=1e-4)
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["parity_check"] is None and d["kernels"] is None
    a = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert set(a) == {"out_W", "out_node_embedding", "out_edge_embedding", "loss", "params", "grads"}, sorted(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(f.stat().st_size for f in out.glob("*.npy")) <= 64 << 20
    w = a["out_W"]
    assert w.ndim == 1 and 0 < w.size <= 4_000_000 and np.all((w > 0) & (w < 1))
    assert math.isclose(float(a["loss"][0]), d["final_loss"], rel_tol=1e-5)   # (the line carries six digits)
    assert a["params"].shape == a["grads"].shape and np.isfinite(a["grads"]).all() and np.abs(a["grads"]).max() > 0


def test_reference_configs_from_class_path(dev):
    P.case_class_path_configs(dev)
