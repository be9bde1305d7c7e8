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

// segment (event of a collated batch) of row q: the last s with seg_ptr[s] <= q (seg_ptr: n_seg + 1 ascending
// offsets, seg_ptr[0] = 0; empty segments hold no row, so none of them is ever returned for a row)
__device__ __forceinline__ int segment_of(const int64_t *__restrict__ seg_ptr, int n_seg, int64_t q) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_ptr[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
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
