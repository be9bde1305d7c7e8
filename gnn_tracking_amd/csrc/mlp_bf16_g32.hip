// Backward instantiations of the bf16-storage fused MLP with an fp32 upstream gradient
// (GNNTRK_EPI_SIGMOID: the edge-weight head feeds the fp32 BCE loss) and the head's launch that forms
// that gradient itself (bce != NULL: mlp16_bwd_bce_kernel).  Separate
// translation unit only to halve the build time of mlp_bf16.hip.
#include "mlp_bf16_kernels.h"

namespace gnntrk {

int launch_bwd16_g32(const gnntrk_mlp_bwd_args *a, const SlotPlan &P, float *part, uint8_t *trash, hipStream_t stream,
                     const gnntrk_head_bce *bce, int *grid_out) {
    return launch_bwd16<true>(a, P, part, trash, stream, bce, grid_out);
}

}  // namespace gnntrk
