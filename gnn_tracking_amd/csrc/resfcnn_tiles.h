// Building blocks the residual-network kernels share (resfcnn.hip: the embedding networks on hits;
// edge_filter.hip: the same network on gathered edge rows): the fragment packing, the LDS staging of one
// layer's fragments, the wave-private images of the K = rows contractions, the in-block sum of the weight-
// gradient tiles and the fixed-order reduction of the per-block partial sums.  Orientation and fragment
// layout: see the head of resfcnn.hip.  Everything is internal to the including unit (anonymous namespace:
// each unit carries its own copy of the two small kernels).
#pragma once

#include "host_util.h"
#include "tile_mlp.h"

namespace gnntrk {
namespace {

constexpr int kRfMaxL = GNNTRK_RESFCNN_MAX_HIDDEN + 2;   // encoder, hidden layers, decoder
constexpr int kRfMaxKTI = GNNTRK_RESFCNN_MAX_IN / 16;     // input tiles
constexpr int kRfMaxOT = GNNTRK_RESFCNN_MAX_OUT / 16;     // output tiles
constexpr int kRfLd = 20;                                 // leading dim of a [feature][row] staging image

__host__ __device__ inline int rf_tiles(int d) { return (d + 15) / 16; }

// ---- fragment packing --------------------------------------------------------------------------
// dst[(to * KS + ks) * 64 + lane] = Mat[16 to + c][16 (ks >> 2) + 4 g + (ks & 3)]   (0 outside the matrix)
// Mat = W (rows = out features, k = in features) or W^T, W in nn.Linear storage [out][in].
struct RfPackJob {
    const float *W;
    float *dst;
    int32_t rows, cols;   // of Mat
    int32_t rt, kt;       // row tiles / k tiles of the fragment image (the kernel's padded counts)
    int32_t ld;           // leading dim of W
    int32_t transposed;
};
struct RfPackArgs {
    RfPackJob job[2 * kRfMaxL + 1];
    int32_t n_jobs;
};

__global__ __launch_bounds__(256) void resfcnn_pack_kernel(const RfPackArgs a) {
    const RfPackJob j = a.job[blockIdx.y];
    if ((int)blockIdx.y >= a.n_jobs) return;
    const int RT = j.rt, KS = 4 * j.kt;
    const int n = RT * KS * 64;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int fr = i >> 6, l = i & 63;
        const int to = fr / KS, ks = fr - to * KS;
        const int g = l >> 4, c = l & 15;
        const int r = 16 * to + c, k = 16 * (ks >> 2) + 4 * g + (ks & 3);
        float v = 0.f;
        if (r < j.rows && k < j.cols) v = j.transposed ? j.W[(int64_t)k * j.ld + r] : j.W[(int64_t)r * j.ld + k];
        j.dst[i] = v;
    }
}

__device__ __forceinline__ void rf_stage(float *s_frag, const float *src, int n_floats, float *s_bias, const float *bias,
                                         int n_bias, int n_bias_pad, int tid) {
    __syncthreads();   // every wave is done with the previous layer's fragments
    const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
    f32x4 *d4 = reinterpret_cast<f32x4 *>(s_frag);
    for (int i = tid; i < n_floats / 4; i += kBlock) d4[i] = s4[i];
    for (int i = tid; i < n_bias_pad; i += kBlock) s_bias[i] = (bias != nullptr && i < n_bias) ? bias[i] : 0.f;
    __syncthreads();
}

// wave-private staging images [feature][row] (leading dim kRfLd): operands of the K = rows contractions
template <int NT>
__device__ __forceinline__ void rf_stage_tiles(float *img, const f32x4 (&v)[NT], int nt, int g, int c) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) img[(16 * t + 4 * g + r) * kRfLd + c] = v[t][r];
        }
}
// k-step s of the K = rows contraction pairs lane group g with row 4g + s: both operands are 16-byte
// reads of feature (16 t + c), rows 4g .. 4g + 3
__device__ __forceinline__ f32x4 rf_read_k(const float *img, int t, int g, int c) {
    return *reinterpret_cast<const f32x4 *>(img + (16 * t + c) * kRfLd + 4 * g);
}

// sums the four waves' accumulator tiles in wave order through LDS and writes the block's partial:
// acc[to][ti] register r of lane (g, c) = dW[16 to + 4g + r][16 ti + c]
template <int NO, int NI>
__device__ __forceinline__ void rf_emit_dw(float *s_red, float *dst, const f32x4 (&acc)[NO][NI], int no, int ni, int O,
                                           int K, int wv, int tid, int g, int c) {
    __syncthreads();   // the fragments are no longer needed
    for (int w = 0; w < kWaves; ++w) {
        if (wv == w) {
#pragma unroll
            for (int to = 0; to < NO; ++to)
#pragma unroll
                for (int ti = 0; ti < NI; ++ti)
                    if (to < no && ti < ni) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int o = 16 * to + 4 * g + r, i = 16 * ti + c;
                            if (o < O && i < K) {
                                float *p = s_red + o * K + i;
                                *p = (w == 0) ? acc[to][ti][r] : *p + acc[to][ti][r];
                            }
                        }
                    }
        }
        __syncthreads();
    }
    for (int i = tid; i < O * K; i += kBlock) dst[i] = s_red[i];
}
// bias gradients: dbacc[to] register r of lane (g, c) = sum over this wave's tiles of g[16 to + 4g + r][row c]
template <int NO>
__device__ __forceinline__ void rf_emit_db(float *s_redb, float *dst, const f32x4 (&dbacc)[NO], int no, int O, int wv,
                                           int tid, int g, int c) {
    for (int w = 0; w < kWaves; ++w) {
        if (wv == w) {
#pragma unroll
            for (int to = 0; to < NO; ++to)
                if (to < no) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = dbacc[to][r];
                        v += __shfl_xor(v, 1);
                        v += __shfl_xor(v, 2);
                        v += __shfl_xor(v, 4);
                        v += __shfl_xor(v, 8);
                        const int o = 16 * to + 4 * g + r;
                        if (c == 0 && o < O) s_redb[o] = (w == 0) ? v : s_redb[o] + v;
                    }
                }
        }
        __syncthreads();
    }
    for (int i = tid; i < O; i += kBlock) dst[i] = s_redb[i];
    // (the caller's next rf_stage starts with a barrier)
}

// ---- final reduction of the per-block partials ---------------------------------------------------
struct RfReduceArgs {
    const float *part;
    int32_t n_part, part_total, n_seg, accumulate;
    int32_t off[2 * kRfMaxL + 1];   // first float of segment j inside a partial block (+ the end)
    float *dst[2 * kRfMaxL];        // destination or NULL
    int32_t scaled[2 * kRfMaxL];    // segment is multiplied by out_scale (decoder W / b)
    const float *out_scale;
    float *raw;                     // [n_raw] unscaled sums of the first n_raw entries (decoder W, b), or NULL
    int32_t n_raw, _pad;
};

// 32 parameters x 8 slices of the partial blocks per workgroup: a slice adds its blocks in order, the eight slice
// sums are added in slice order - a fixed association, and 256 instead of 32 workgroups in flight (the one-thread-
// per-parameter walk over 256 blocks was a 90 us latency chain for 32 KB of sums)
__global__ __launch_bounds__(256) void resfcnn_reduce_kernel(const RfReduceArgs a) {
    __shared__ float s_part[8][32];
    const int pl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + pl;
    const int per = (a.n_part + 7) / 8, b0 = sl * per, b1 = b0 + per < a.n_part ? b0 + per : a.n_part;
    float acc = 0.f;
    if (i < a.part_total)
        for (int b = b0; b < b1; ++b) acc += a.part[(int64_t)b * a.part_total + i];
    s_part[sl][pl] = acc;
    __syncthreads();
    if (sl != 0 || i >= a.part_total) return;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += s_part[q][pl];
    if (a.raw != nullptr && i < a.n_raw) a.raw[i] = s;
    int j = 0;
    while (j + 1 < a.n_seg && i >= a.off[j + 1]) ++j;
    if (a.dst[j] == nullptr) return;
    if (a.scaled[j] && a.out_scale != nullptr) s *= a.out_scale[0];
    float *p = a.dst[j] + (i - a.off[j]);
    *p = a.accumulate ? *p + s : s;
}

int rf_ht(int hidden) {
    const int t = rf_tiles(hidden);
    return t <= 4 ? t : t <= 6 ? 6 : 8;
}

}  // namespace
}  // namespace gnntrk
