// Forward launchers and C entries of the bf16-storage fused MLP kernels (mlp_bf16_kernels.h).  Own translation
// unit: the forward kernels are compiled with -amdgpu-sched-strategy=max-ilp (_build.py), which
// suits their load-heavy tile loop (edge-weight head 1.58 -> 1.39 ms) but not the backward.
#include "mlp_bf16_kernels.h"

namespace gnntrk {

// The instantiation a forward launch takes, resolved ONCE: the launcher below lifts these values over its
// instantiation lists, the name entry point prints them.
struct Fwd16Sel {
    enum Kind { kOt, kBi8, kBi, kMain } kind;   // output tiles / wide inputs | hidden 128 with biases | hidden 64 with biases | the rest
    int KI, HT, OT, R;   // R: tiles sharing one output tile (4 / 1)
    bool three, sig, wide;
    int per_cu;          // workgroups per CU the grid is sized for (kMain with up to four hidden tiles: what is resident)
};
static Fwd16Sel fwd16_select(const gnntrk_mlp_fwd_args *a, const SlotPlan &P) {
    Fwd16Sel S{};
    S.KI = P.KI;
    S.HT = P.HT;
    S.OT = (a->mlp.out_dim + 15) / 16;
    S.R = 1;
    S.three = a->mlp.n_layers == 3;
    S.sig = a->epilogue == GNNTRK_EPI_SIGMOID;
    if (a->mlp.out_dim > 16 || P.KI > 2) {
        S.kind = Fwd16Sel::kOt;
        S.per_cu = P.KI > 2 ? 1 : 2;
    } else if (P.bias_init) {
        S.kind = P.HT == 8 ? Fwd16Sel::kBi8 : Fwd16Sel::kBi;
        S.per_cu = P.HT == 8 ? 1 : 3;
    } else {
        // hidden widths 64 .. 127 (five to eight hidden tiles): the plain forms only (own output tile per tile, 8-byte
        // loads) - four instantiations per shape instead of sixteen
        const bool plain = P.HT >= 5;
        S.kind = Fwd16Sel::kMain;
        S.R = (a->mlp.out_dim <= 4 && !plain) ? 4 : 1;       // four tiles share one output tile and one store
        S.wide = !plain && wide_ok(P, a->seg, a->n_rows);   // one 16-byte load per lane and k-step
        // (five / six hidden tiles: 230 .. 330 registers per lane - two workgroups per CU are resident with one
        //  k-step, one with two; the grid of the persistent tile schedule matches what is resident)
        S.per_cu = plain ? ((P.KI == 1 && P.HT <= 6) ? 2 : 1) : kFwd16BlocksPerCu;
    }
    return S;
}

static int fwd16_grid(int64_t n_rows, int per_cu) {
    const int grid = tile_grid(n_rows, per_cu);
    return grid > kFwdMaxBlocks ? kFwdMaxBlocks - kFwdMaxBlocks % 8 : grid;   // (the store-redirect slots: g_fwd_trash)
}
// The persistent grid of an instantiation of up to four hidden tiles = the workgroups of it that are RESIDENT at once
// (tile_mlp.h: resident_blocks), not a fixed five per CU: a larger grid runs in rounds whose last one leaves CUs idle
// (round 5: the hot instantiations hold 164-230 registers = two, not five, workgroups per CU).
template <auto Kfn> static void fwd16_launch_resident(const gnntrk_mlp_fwd_args *a, hipStream_t stream) {
    launch(Kfn, fwd16_grid(a->n_rows, resident_blocks<Kfn>(kFwd16BlocksPerCu)), kBlock, stream, *a);
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

// exact forward instantiation
int gnntrk_mlp_forward_bf16_kernel_name(const gnntrk_mlp_fwd_args *args, char *buf, size_t len) {
    if (!args || !buf || len == 0) return fail(GNNTRK_EINVAL, "mlp_kernel_name: bad argument");
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, nullptr);
    const Fwd16Sel S = fwd16_select(args, P);
    const char *three = S.three ? "true" : "false", *sig = S.sig ? "true" : "false";
    if (S.kind == Fwd16Sel::kOt)
        snprintf(buf, len, "mlp16_fwd_ot_kernel<%d, %d, %d, %s>", S.KI, S.HT, S.OT, three);
    else if (S.kind != Fwd16Sel::kMain)
        snprintf(buf, len, "mlp16_fwd_bi_kernel<%d, %d, %s, %s>", S.KI, S.HT, three, sig);
    else
        snprintf(buf, len, "mlp16_fwd_kernel<%d, %d, %s, %s, %d, %s>", S.KI, S.HT, three, sig, S.R, S.wide ? "true" : "false");
    return GNNTRK_OK;
}

int gnntrk_mlp_forward_bf16(const gnntrk_mlp_fwd_args *args, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!args) return fail(GNNTRK_EINVAL, "mlp_forward_bf16: NULL args");
    int rc = check_bf16_mlp(args->mlp, args->n_seg, args->seg, "mlp_forward_bf16", args->n_rows);
    if (rc) return rc;
    if (args->epilogue < 0 || args->epilogue > 3) return fail(GNNTRK_EINVAL, "mlp_forward_bf16: bad epilogue");
    if (args->n_rows == 0) return GNNTRK_OK;  // nothing to write: NULL row pointers are fine
    const int out_pad = (args->mlp.out_dim + 3) / 4 * 4;
    if (args->epilogue == GNNTRK_EPI_SIGMOID) {
        if (!args->out || args->out_stride < args->mlp.out_dim)
            return fail(GNNTRK_EINVAL, "mlp_forward_bf16: bad (fp32) output");
    } else if (!args->out || args->out_stride < out_pad || args->out_stride % 4 != 0 ||
               ((uintptr_t)args->out & 7) != 0) {
        return fail(GNNTRK_EINVAL,
                    "mlp_forward_bf16: output rows must be 8-byte aligned bf16, stride a multiple of 4 >= "
                    "out_dim rounded up to 4");
    }
    if (args->epilogue == GNNTRK_EPI_RESIDUAL &&
        (!args->res || args->res_stride < out_pad || args->res_stride % 4 != 0 || ((uintptr_t)args->res & 7) != 0))
        return fail(GNNTRK_EINVAL, "mlp_forward_bf16: residual epilogue needs padded bf16 res rows");
    if (args->n_rows < 0 || args->n_rows > 0x7fffffff) return fail(GNNTRK_EINVAL, "mlp_forward_bf16: bad n_rows");
    if (args->n_rows == 0) return GNNTRK_OK;
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, nullptr);
    if (!P.ok || P.KI > kMaxChunks16 / 8)
        return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: shape outside the instantiations (include/gnntrk.h)");
    const Fwd16Sel S = fwd16_select(args, P);
    const int grid = fwd16_grid(args->n_rows, S.per_cu);
    bool found = false;
    switch (S.kind) {
    case Fwd16Sel::kOt:   // outputs of 17 .. 48 features / inputs of 65 .. 128 slots (three hidden tiles): the plain output-tile kernels
        if (S.sig) return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: SIGMOID epilogue with a wide input / output");
        found = S.HT == 3 &&
                lift_int2<int2_c<1, 2>, int2_c<1, 3>, int2_c<2, 2>, int2_c<2, 3>, int2_c<3, 1>, int2_c<3, 2>, int2_c<3, 3>,
                          int2_c<4, 1>, int2_c<4, 2>, int2_c<4, 3>>(S.KI, S.OT, [&](auto p) {
                    lift_bools([&](auto three) {
                        launch(mlp16_fwd_ot_kernel<decltype(p)::a, 3, decltype(p)::b, decltype(three)::value>, grid,
                               kBlock, stream, *args);
                    }, S.three);
                });
        if (!found) return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: no instantiation (output tiles)");
        break;
    case Fwd16Sel::kBi8:
        return launch_fwd16_bi8(args, P, grid, stream);
    case Fwd16Sel::kBi:   // hidden width 64 with biases (SlotPlan::bias_init): plain forms of the accumulator-initialised kernels
        found = lift_int2<int2_c<1, 4>, int2_c<2, 4>>(S.KI, S.HT, [&](auto p) {
            lift_bools([&](auto three, auto sig) {
                launch(mlp16_fwd_bi_kernel<decltype(p)::a, decltype(p)::b, decltype(three)::value, decltype(sig)::value>, grid,
                       kBlock, stream, *args);
            }, S.three, S.sig);
        });
        if (!found) return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: no instantiation (bias_init)");
        break;
    case Fwd16Sel::kMain:
        // the I/O skeleton of the two large forward shapes (three hidden tiles, shared output tile): debug_flags & 4096
        if ((args->debug_flags & 4096) && S.KI == 1 && S.HT == 3 && S.three && S.R == 4 && S.sig != S.wide) {
            if (S.wide) fwd16_launch_resident<mlp16_fwd_skel_kernel<1, 3, true, false, 4, true>>(args, stream);   // relational / object-shaped: bf16 output, 16-byte loads
            else fwd16_launch_resident<mlp16_fwd_skel_kernel<1, 3, true, true, 4, false>>(args, stream);          // the edge-weight head: fp32 sigmoid output, 8-byte loads
            break;
        }
        found = lift_int2<int2_c<1, 1>, int2_c<1, 2>, int2_c<1, 3>, int2_c<1, 4>, int2_c<2, 1>, int2_c<2, 2>, int2_c<2, 3>,
                          int2_c<2, 4>>(S.KI, S.HT, [&](auto p) {
            lift_bools([&](auto three, auto sig, auto share, auto wide) {
                fwd16_launch_resident<mlp16_fwd_kernel<decltype(p)::a, decltype(p)::b, decltype(three)::value, decltype(sig)::value,
                                                       decltype(share)::value ? 4 : 1, decltype(wide)::value>>(
                    args, stream);
            }, S.three, S.sig, S.R == 4, S.wide);
        });
        found = found || lift_int2<int2_c<1, 5>, int2_c<1, 6>, int2_c<2, 5>, int2_c<2, 6>, int2_c<1, 7>, int2_c<1, 8>>(
                             S.KI, S.HT, [&](auto p) {
            lift_bools([&](auto three, auto sig) {
                launch(mlp16_fwd_kernel<decltype(p)::a, decltype(p)::b, decltype(three)::value, decltype(sig)::value, 1, false>, grid,
                       kBlock, stream, *args);
            }, S.three, S.sig);
        });
        if (!found) return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: no instantiation");
        break;
    }
    return check_launch("mlp_forward_bf16");
}

}  // extern "C"
