// Device-side helpers of one wave (64 lanes), for any unit: nothing here needs the counting units' table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnntrk {

// orders the wave's LDS / memory accesses before the call against those after it (no s_barrier: one wave)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// wave sum by butterfly (every lane of the wave calls it and gets the total; for floating point the
// order of the additions is fixed, lane distance 32 first)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

}  // namespace gnntrk
