// Backward launchers and C entries of the bf16-storage fused MLP kernels (mlp_bf16_kernels.h).  The
// instantiations with an fp32 upstream gradient (EPI_SIGMOID: the edge-weight head) are
// compiled in mlp_bf16_g32.hip, the forward kernels in mlp_bf16_fwd.hip (own scheduling
// strategy, see _build.py), so the three parts also build in parallel.
#include "mlp_bf16_kernels.h"

namespace gnntrk {

int launch_bwd16_g32(const gnntrk_mlp_bwd_args *a, const SlotPlan &P, float *part, uint8_t *trash, hipStream_t stream,
                     const gnntrk_head_bce *bce, int *grid_out);  // mlp_bf16_g32.hip

int mlp16_kernel_name(const gnntrk_mlp *m, int n_seg, const gnntrk_seg *seg, int backward, char *buf,
                      size_t len) {
    if (!m || !seg || !buf || len == 0) return fail(GNNTRK_EINVAL, "mlp_kernel_name: bad argument");
    SlotPlan P;
    make_slot_plan(P, *m, n_seg, seg, nullptr);
    // (the backward instantiation also depends on how many input gradients are wanted:
    // GT = 1 or 2 KI gradient tiles; the name reports the k-step and hidden-tile counts)
    snprintf(buf, len, "mlp16_%s_kernel<%d, %d, %s>", backward ? "bwd" : "fwd", P.KI, P.HT,
             m->n_layers == 3 ? "true" : "false");  // (forward: + the sigmoid flag, see ops_bf16.py)
    return GNNTRK_OK;
}

// workspace = one partial block per wave | one 8-byte trash slot per lane
static size_t bwd16_partial_bytes(const gnntrk_mlp *m) {
    return align_up((size_t)cu_count() * kBwd16BlocksPerCuMax * kWaves * (size_t)part_total(*m) * sizeof(float), 256);
}
// the launch of gnntrk_mlp_backward_bf16_bce as the shared launcher takes it: the upstream term is a stand-in that
// describes w_out (fp32 [n_rows]) - the buffer plan is the fp32-upstream head's, and the kernel stores W through
// the term's descriptor
static bool bce_args(const gnntrk_mlp_bwd_args *a, const gnntrk_head_bce *bce, gnntrk_mlp_bwd_args &b) {
    if (!a || !bce || !bce->label || !bce->w_out || ((uintptr_t)bce->label & 3) != 0 || ((uintptr_t)bce->w_out & 3) != 0 ||
        a->n_rows < 1 || a->n_rows > 0x7fffffff || bce->n_total < 1)
        return false;
    b = *a;
    b.n_gout = 1;
    b.gout[0].ptr = bce->w_out;
    b.gout[0].idx = nullptr;
    b.gout[0].stride = 1;
    b.gout[0].rows = (int32_t)a->n_rows;
    return true;
}

// what gnntrk_mlp_backward_bf16 (bce == NULL) and gnntrk_mlp_backward_bf16_bce share
static int bwd16_launch(const gnntrk_mlp_bwd_args *a, void *ws, size_t ws_bytes, hipStream_t stream,
                        const gnntrk_head_bce *bce) {
    if (!a) return fail(GNNTRK_EINVAL, "mlp_backward_bf16: NULL args");
    int rc = check_bf16_mlp(a->mlp, a->n_seg, a->seg, "mlp_backward_bf16", a->n_rows);
    if (rc) return rc;
    if (a->epilogue < 0 || a->epilogue > 3) return fail(GNNTRK_EINVAL, "mlp_backward_bf16: bad epilogue");
    const bool empty = a->n_rows == 0;  // no rows: only the parameter gradients are written (zeros)
    if (a->n_gout < 1 || a->n_gout > 3)
        return fail(GNNTRK_EINVAL, "mlp_backward_bf16: bad upstream gradient terms");
    for (int t = 0; t < a->n_gout && !empty; ++t)
        if (!a->gout[t].ptr) return fail(GNNTRK_EINVAL, "mlp_backward_bf16: bad upstream gradient terms");
    const int out_pad = (a->mlp.out_dim + 3) / 4 * 4;
    if (a->epilogue == GNNTRK_EPI_SIGMOID) {
        if (a->n_gout != 1 || a->gout[0].stride < a->mlp.out_dim)
            return fail(GNNTRK_EINVAL, "mlp_backward_bf16: SIGMOID takes one fp32 upstream gradient term");
    } else {
        for (int t = 0; t < a->n_gout; ++t)
            if (a->gout[t].stride < out_pad || a->gout[t].stride % 4 != 0 || ((uintptr_t)a->gout[t].ptr & 7) != 0)
                return fail(GNNTRK_EINVAL, "mlp_backward_bf16: upstream gradient rows must be padded bf16 rows");
    }
    for (int j = 0; j < a->n_seg; ++j) {
        const gnntrk_gseg &gs = a->gseg[j];
        if (!gs.ptr) continue;
        if (gs.accumulate) return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16: gseg.accumulate is reserved");
        if (gs.stride < (a->seg[j].dim + 3) / 4 * 4 || gs.stride % 4 != 0 || ((uintptr_t)gs.ptr & 7) != 0)
            return fail(GNNTRK_EINVAL, "mlp_backward_bf16: gradient slices must be padded bf16 rows");
    }
    if (a->n_rows < 0 || a->n_rows > 0x7fffffff) return fail(GNNTRK_EINVAL, "mlp_backward_bf16: bad n_rows");
    if (a->fold.ids && !empty) {
        const gnntrk_gfold &f = a->fold;
        if (f.seg < 0 || f.seg >= a->n_seg || !a->gseg[f.seg].ptr || a->gseg[f.seg].idx || a->seg[f.seg].idx != f.ids ||
            f.n_nodes <= 0 || a->gseg[f.seg].stride != 8 || ((uintptr_t)a->gseg[f.seg].ptr & 15) != 0 ||
            false)
            return fail(GNNTRK_EINVAL, "mlp_backward_bf16: bad fold block (include/gnntrk.h: gnntrk_gfold)");
        if (!gnntrk_mlp_backward_bf16_can_fold(a))
            return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16: this launch does not take a fold (gnntrk_mlp_backward_bf16_can_fold)");
    }
    if (a->n_gout == 3 && a->n_rows > 0 && gnntrk_mlp_backward_bf16_max_terms(a) < 3)
        return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16: three upstream terms only on the buffer-addressed shapes "
                                         "(gnntrk_mlp_backward_bf16_max_terms)");
    const bool want_dw = a->gW[0] != nullptr;
    if (want_dw)
        for (int i = 0; i < a->mlp.n_layers; ++i)
            if (!a->gW[i]) return fail(GNNTRK_EINVAL, "mlp_backward_bf16: gW must be all set or all NULL");
    if (!ws || ws_bytes < gnntrk_mlp_backward_bf16_workspace_bytes(&a->mlp))
        return fail(GNNTRK_EINVAL, "mlp_backward_bf16: workspace too small (always required)");
    SlotPlan P;
    make_slot_plan(P, a->mlp, a->n_seg, a->seg, a->gseg);
    if (!P.ok || P.KI > kMaxChunks16 / 8)
        return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16: shape outside the instantiations (include/gnntrk.h)");
    int grid = 0;
    if (a->n_rows > 0) {
        float *part = reinterpret_cast<float *>(ws);
        uint8_t *trash = reinterpret_cast<uint8_t *>(ws) + bwd16_partial_bytes(&a->mlp);
        rc = (a->epilogue == GNNTRK_EPI_SIGMOID) ? launch_bwd16_g32(a, P, part, trash, stream, bce, &grid)
                                                 : launch_bwd16<false>(a, P, part, trash, stream, nullptr, &grid);
        if (rc) return rc;
    }
    if (want_dw) {
        // one partial block per workgroup when the parameters fit the kernel's LDS image
        const bool via_lds = part_total(a->mlp) <= bwd16_img_dwords(P.KI, P.HT, bwd16_gt(a, P), a->mlp.n_layers == 3) &&
                             P.HT <= 4 && !(a->debug_flags & 2048);
        rc = reduce_partials_launch(reinterpret_cast<const float *>(ws), via_lds ? grid : grid * kWaves, &a->mlp,
                                    a->gW, a->gb, a->accumulate_params, stream);
    }
    return rc;
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

// exact backward instantiation (needs the gradient slices and the epilogue): the selection of the launcher, printed
int gnntrk_mlp_backward_bf16_kernel_name(const gnntrk_mlp_bwd_args *args, char *buf, size_t len) {
    if (!args || !buf || len == 0) return fail(GNNTRK_EINVAL, "mlp_kernel_name: bad argument");
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, args->gseg);
    BufPlan B;
    const Bwd16Sel S = bwd16_select(args, P, B);
    const char *three = S.three ? "true" : "false", *g32 = S.g32 ? "true" : "false";
    if (S.kind == Bwd16Sel::kOt)
        snprintf(buf, len, "mlp16_bwd_ot_kernel<%d, %d, %d, %s>", S.KI, S.HT, S.OT, three);
    else if (S.kind == Bwd16Sel::kBi8 || S.kind == Bwd16Sel::kBi)
        snprintf(buf, len, "mlp16_bwd_bi_kernel<%d, %d, %d, %s, %s>", S.KI, S.HT, S.GT, three, g32);
    else   // (as rocprofv3 prints the instantiation: a template argument that itself ends in '>' is followed by a space)
        snprintf(buf, len, "mlp16_bwd_kernel<%d, %d, %d, %s, %s, %d, %s%s>", S.KI, S.HT, S.GT, three, g32, S.D, S.io_name,
                 S.io_name[strlen(S.io_name) - 1] == '>' ? " " : "");
    return GNNTRK_OK;
}

// the number of upstream terms (2 or 3) the launch described by `args` can take: 3 where it runs
// buffer-addressed with a further term on the tile's rows
int gnntrk_mlp_backward_bf16_max_terms(const gnntrk_mlp_bwd_args *args) {
    if (!args || args->epilogue == GNNTRK_EPI_SIGMOID || args->n_rows <= 0 || args->n_gout < 1 || args->n_gout > 3)
        return 2;
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, args->gseg);
    if (!P.ok || P.KI != 1) return 2;
    gnntrk_mlp_bwd_args b = *args;
    while (b.n_gout < 3) {   // probe with stand-in terms: rows of the tile, sized like the first term
        b.gout[b.n_gout] = b.gout[0];
        b.gout[b.n_gout].idx = nullptr;
        b.gout[b.n_gout].rows = (int32_t)(args->n_rows < 0x7fffffff ? args->n_rows : 0x7fffffff);
        b.n_gout += 1;
    }
    BufPlan B;
    const Bwd16Sel S = bwd16_select(&b, P, B);
    return (S.kind == Bwd16Sel::kBuf && S.terms == 3) ? 3 : 2;
}

// 1 if the launch described by `args` (fold block filled in) runs on an instantiation that folds inside the kernel
int gnntrk_mlp_backward_bf16_can_fold(const gnntrk_mlp_bwd_args *args) {
    if (!args || !args->fold.ids || args->fold.seg < 0 || args->fold.seg >= args->n_seg || args->n_rows <= 0 ||
        args->n_rows > 0x7fffffff || args->n_gout < 1 || args->n_gout > 3)
        return 0;
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, args->gseg);
    if (!P.ok) return 0;
    BufPlan B;
    const Bwd16Sel S = bwd16_select(args, P, B);
    return (S.kind == Bwd16Sel::kBuf && S.fold) ? 1 : 0;
}

size_t gnntrk_mlp_backward_bf16_workspace_bytes(const gnntrk_mlp *mlp) {
    if (!mlp) return 0;
    return bwd16_partial_bytes(mlp) + (size_t)cu_count() * kBwd16BlocksPerCuMax * kWaves * 64 * 8;
}

int gnntrk_mlp_backward_bf16_bce_supported(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce) {
    gnntrk_mlp_bwd_args b;
    if (!bce_args(args, bce, b) || b.n_seg < 1 || b.n_seg > GNNTRK_MAX_SEGS) return 0;
    SlotPlan P;
    make_slot_plan(P, b.mlp, b.n_seg, b.seg, b.gseg);
    if (!P.ok) return 0;
    BufPlan B;
    return bwd16_select(&b, P, B).bce ? 1 : 0;
}

int gnntrk_mlp_backward_bf16_bce_kernel_name(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce, char *buf,
                                             size_t len) {
    if (!buf || len == 0) return fail(GNNTRK_EINVAL, "mlp_kernel_name: bad argument");
    if (!gnntrk_mlp_backward_bf16_bce_supported(args, bce))
        return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16_bce: not the buffer-addressed head shape");
    SlotPlan P;
    make_slot_plan(P, args->mlp, args->n_seg, args->seg, args->gseg);
    snprintf(buf, len, "mlp16_bwd_bce_kernel<%d>", P.HT);
    return GNNTRK_OK;
}

int gnntrk_mlp_backward_bf16(const gnntrk_mlp_bwd_args *args, void *workspace, size_t workspace_bytes, void *stream) {
    return bwd16_launch(args, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

int gnntrk_mlp_backward_bf16_bce(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce, void *workspace,
                                 size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    gnntrk_mlp_bwd_args b;
    if (!bce_args(args, bce, b)) return fail(GNNTRK_EINVAL, "mlp_backward_bf16_bce: bad argument");
    if (b.epilogue != GNNTRK_EPI_SIGMOID || b.fold.ids)
        return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16_bce: the SIGMOID epilogue, no fold");
    return bwd16_launch(&b, workspace, workspace_bytes, stream, bce);
}

}  // extern "C"
