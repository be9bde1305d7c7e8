// Hidden width 128 with biases in bf16 storage: eight hidden tiles with accumulator-initialised biases
// (SlotPlan::bias_init; with a constant-one row it would be nine tiles - 81 weight-gradient tiles for the
// middle layer alone).  Own translation unit because it is compiled WITHOUT -amdgpu-mfma-vgpr-form (see
// _build.py): with the MFMA results forced into VGPRs the compiler's AGPR-copy rewrite crashes on the
// eight-tile backward with two gradient tiles (ROCm 7.2).  The three-layer backward instantiations spill
// 117-133 registers (388 accumulators + the tile state in 512 registers) - still two orders of magnitude
// faster than the library-GEMM path these models took before.
#include "mlp_bf16_kernels.h"

namespace gnntrk {

int launch_fwd16_bi8(const gnntrk_mlp_fwd_args *a, const SlotPlan &P, int grid, hipStream_t stream) {
    if (P.KI != 1 || P.HT != 8) return fail(GNNTRK_EUNSUPPORTED, "mlp_forward_bf16: no instantiation (hidden 128)");
    lift_bools([&](auto three, auto sig) {
        launch(mlp16_fwd_bi_kernel<1, 8, decltype(three)::value, decltype(sig)::value>, grid, kBlock, stream, *a);
    }, a->mlp.n_layers == 3, a->epilogue == GNNTRK_EPI_SIGMOID);
    return check_launch("mlp_forward_bf16");
}

int launch_bwd16_bi8(const gnntrk_mlp_bwd_args *a, const SlotPlan &P, int GT, int grid, float *part, uint8_t *trash,
                     hipStream_t stream) {
    BufPlan B;
    make_buf_plan(B, P, a, GT);
    const bool found = P.KI == 1 && P.HT == 8 && lift_int<0, 1, 2>(GT, [&](auto gt) {
        lift_bools([&](auto three, auto g32) {
            launch(mlp16_bwd_bi_kernel<1, 8, decltype(gt)::value, decltype(three)::value, decltype(g32)::value>, grid, kBlock,
                   stream, *a, part, trash, B);
        }, a->mlp.n_layers == 3, a->epilogue == GNNTRK_EPI_SIGMOID);
    });
    if (!found) return fail(GNNTRK_EUNSUPPORTED, "mlp_backward_bf16: no instantiation (hidden 128)");
    return check_launch("mlp_backward_bf16");
}

}  // namespace gnntrk
