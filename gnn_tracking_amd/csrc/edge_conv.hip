// Dynamic edge convolution (models/dynamic_edge_conv.py:14-64) on a k-nearest-neighbour table:
//     h_i = aggr_{j in kNN(i)} nn(cat[x_i, x_j - x_i]),  nn = Linear(2D, H) -> ReLU -> Linear(H, O),  aggr in {add, mean, max}
// (see include/gnntrk.h for the operator and the C ABI).  Orientation, fragment layout and the K = rows
// contractions are those of resfcnn.hip (shared through resfcnn_tiles.h).  What differs:
//  * a 16-row tile is 16 NODES at one neighbour slot and the kernel loops over the slots: every query has its
//    neighbours contiguous in the table, so the sum / mean / max of a node stays in that lane's accumulator
//    registers - no edge-sized message tensor, no second pass, no graph index, no cross-lane step;
//  * W1 is packed as two fragment images, W1a = W1[:, :D] (on x_i) and W1b = W1[:, D:] (on x_j - x_i), each
//    padded to whole 16-feature tiles: the two gradients of one input feature then sit in the same lane and
//    register, and W1a x_i + b1 is formed once per node instead of once per slot.  The difference x_j - x_i
//    is formed in fp32 from the loaded rows BEFORE it is contracted (the reference's rounding; the algebraic
//    split x_i (W1a - W1b) + x_j W1b cancels catastrophically between nearest neighbours);
//  * the backward recomputes the hidden layer per (node, slot) and keeps nothing edge-sized from the forward.
//    Weight and bias gradients: per-workgroup partials, fixed-order final reduction.  Target side of the input
//    gradient: in registers.  Source side: per-slot rows g_b, which the caller folds by source with the
//    graph index's deterministic segment sums.  No floating-point atomics.
#include <cmath>
#include <cstring>

#include "resfcnn_tiles.h"

namespace gnntrk {
namespace {

constexpr int kEcAdd = 0, kEcMean = 1, kEcMax = 2;
constexpr int kEcMaxHidden = GNNTRK_RESFCNN_MAX_WIDTH;
constexpr int kEcMaxOut = GNNTRK_RESFCNN_MAX_OUT, kEcMaxSlots = 64;

struct EcArgs {
    const float *x;
    const int32_t *nbr, *cnt;
    int64_t n;
    int32_t x_stride, dim, k, k_stride, include_self, hidden, out_dim, aggr, relu, part_total;
    const float *fw1a, *fw1b, *fw2;      // forward fragments
    const float *fw2t, *fw1at, *fw1bt;   // transposed fragments (backward)
    const float *b1, *b2;
    float *h;           // [n, out_dim]: forward writes, backward reads (the ReLU gate)
    int32_t *win;       // [n, out_dim] winning slot (max), -1: none; forward writes, backward reads
    const float *gout;  // [n, out_dim]
    float *gx_tgt;      // [n, dim] or NULL: no input gradient wanted
    float *gx_slot;     // [n, k + include_self, dim]: row (i, s) is written for s < count[i] (and for some beyond)
    float *part;        // [grid][part_total]
};

__device__ __forceinline__ void ec_copy(float *dst, const float *src, int n_floats, int tid) {
    const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
    f32x4 *d4 = reinterpret_cast<f32x4 *>(dst);
    for (int i = tid; i < n_floats / 4; i += kBlock) d4[i] = s4[i];
}
__device__ __forceinline__ void ec_bias(float *dst, const float *b, int n, int n_pad, int tid) {
    for (int i = tid; i < n_pad; i += kBlock) dst[i] = (b != nullptr && i < n) ? b[i] : 0.f;
}

// what a lane knows of its node: the row, the number of present slots, x_i in accumulator layout
template <int DT> struct EcNode {
    int64_t row;
    int count;
    bool valid;
    f32x4 xi[DT];
};
template <int DT>
__device__ __forceinline__ void ec_load_node(const EcArgs &a, int64_t tile, int g, int c, EcNode<DT> &nd) {
    const int64_t node = tile * 16 + c;
    nd.valid = node < a.n;
    nd.row = nd.valid ? node : a.n - 1;
    int cn = a.cnt[nd.row];
    cn = cn < 0 ? 0 : (cn > a.k ? a.k : cn);
    nd.count = nd.valid ? cn + a.include_self : 0;
    const float *xr = a.x + nd.row * a.x_stride;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * t + 4 * g + r;
            if (f < a.dim) v[r] = xr[f];
        }
        nd.xi[t] = v;
    }
}
// x_j - x_i of slot s (0 where the slot is absent); ids outside [0, n) are clamped: a bad table reads a
// wrong hit, never foreign memory
template <int DT>
__device__ __forceinline__ bool ec_load_diff(const EcArgs &a, const EcNode<DT> &nd, int s, int g, f32x4 (&d)[DT]) {
    const bool present = s < nd.count;
    int64_t j = nd.row;
    if (present && !(a.include_self && s == 0)) {
        j = a.nbr[nd.row * a.k_stride + (s - a.include_self)];
        j = j < 0 ? 0 : (j >= a.n ? a.n - 1 : j);
    }
    const float *xr = a.x + j * a.x_stride;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * t + 4 * g + r;
            if (present && f < a.dim) v[r] = xr[f] - nd.xi[t][r];
        }
        d[t] = v;
    }
    return present;
}
// acc[to] += Mat in[.]: `frag` is a fragment image of RT row tiles and KT k tiles.  Every bound is static: the
// padding of a fragment image is zero, and a run-time guard around an MFMA costs far more than the MFMA
template <int RT, int KT>
__device__ __forceinline__ void ec_gemm(const float *frag, const f32x4 (&in)[KT], f32x4 (&acc)[RT], int lane) {
#pragma unroll
    for (int ti = 0; ti < KT; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int to = 0; to < RT; ++to) acc[to] = mfma4(frag[(to * 4 * KT + 4 * ti + r) * 64 + lane], in[ti][r], acc[to]);
}
template <int NT>
__device__ __forceinline__ void ec_init_bias(const float *s_b, f32x4 (&v)[NT], int g) {
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = *reinterpret_cast<const f32x4 *>(s_b + 16 * t + 4 * g);
}

// ================================================================================ forward
template <int HT, int DT, int OT>
__global__ __launch_bounds__(kBlock) void edge_conv_fwd_kernel(const EcArgs a) {
    constexpr int kW1 = HT * 4 * DT * 64, kW2 = OT * 4 * HT * 64;
    __shared__ __attribute__((aligned(16))) float s_w1a[kW1];
    __shared__ __attribute__((aligned(16))) float s_w1b[kW1];
    __shared__ __attribute__((aligned(16))) float s_w2[kW2];
    __shared__ __attribute__((aligned(16))) float s_b1[16 * HT];
    __shared__ __attribute__((aligned(16))) float s_b2[16 * OT];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.k + a.include_self;
    ec_copy(s_w1a, a.fw1a, kW1, tid);
    ec_copy(s_w1b, a.fw1b, kW1, tid);
    ec_copy(s_w2, a.fw2, kW2, tid);
    ec_bias(s_b1, a.b1, a.hidden, 16 * HT, tid);
    ec_bias(s_b2, a.b2, a.out_dim, 16 * OT, tid);
    __syncthreads();
    const int64_t n_tiles = (a.n + 15) / 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wv; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
        EcNode<DT> nd;
        ec_load_node<DT>(a, tile, g, c, nd);
        f32x4 ha[HT];   // W1a x_i + b1: the same for every slot
        ec_init_bias<HT>(s_b1, ha, g);
        ec_gemm<HT, DT>(s_w1a, nd.xi, ha, lane);
        f32x4 acc[OT];
        int win[OT][4];
#pragma unroll
        for (int to = 0; to < OT; ++to) {
            acc[to] = zero;
#pragma unroll
            for (int r = 0; r < 4; ++r) win[to][r] = -1;
        }
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            f32x4 d[DT], p[HT], o[OT];
            if (__ballot(s < nd.count) == 0ull) break;   // no node of the tile has this slot, nor a later one
            lds_wave_order();   // (the fragments are read again per slot, not kept in registers across the loop)
            const bool present = ec_load_diff<DT>(a, nd, s, g, d);
#pragma unroll
            for (int t = 0; t < HT; ++t) p[t] = ha[t];
            ec_gemm<HT, DT>(s_w1b, d, p, lane);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) p[t][r] = fmaxf(p[t][r], 0.f);
            ec_init_bias<OT>(s_b2, o, g);
            ec_gemm<OT, HT>(s_w2, p, o, lane);
            if (present) {
#pragma unroll
                for (int to = 0; to < OT; ++to)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (a.aggr != kEcMax) acc[to][r] += o[to][r];
                        else if (win[to][r] < 0 || o[to][r] > acc[to][r]) {   // ties: the lowest slot
                            acc[to][r] = o[to][r];
                            win[to][r] = s;
                        }
                    }
            }
        }
        if (nd.valid) {
            // (a query without a slot: 0 for every aggregation)
            const float inv = (a.aggr == kEcMean && nd.count > 0) ? 1.f / (float)nd.count : 1.f;
#pragma unroll
            for (int to = 0; to < OT; ++to)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * to + 4 * g + r;
                    if (f < a.out_dim) {
                        float v = acc[to][r];
                        if (a.aggr == kEcMean) v = v * inv;
                        if (a.relu) v = fmaxf(v, 0.f);
                        a.h[nd.row * a.out_dim + f] = v;
                        if (a.win != nullptr) a.win[nd.row * a.out_dim + f] = win[to][r];
                    }
                }
        }
    }
}

// ================================================================================ backward
// the block's partial of dW1 [H][2D] from its two halves (layout of rf_emit_dw per half)
template <int HT, int DT>
__device__ __forceinline__ void ec_emit_dw1(float *s_red, float *dst, const f32x4 (&da)[HT][DT], const f32x4 (&db)[HT][DT],
                                            int H, int D, int wv, int tid, int g, int c) {
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) {
        if (wv == w) {
#pragma unroll
            for (int to = 0; to < HT; ++to)
#pragma unroll
                for (int ti = 0; ti < DT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * to + 4 * g + r, i = 16 * ti + c;
                        if (o < H && i < D) {
                            float *p = s_red + o * 2 * D + i;
                            p[0] = (w == 0) ? da[to][ti][r] : p[0] + da[to][ti][r];
                            p[D] = (w == 0) ? db[to][ti][r] : p[D] + db[to][ti][r];
                        }
                    }
        }
        __syncthreads();
    }
    for (int i = tid; i < H * 2 * D; i += kBlock) dst[i] = s_red[i];
    __syncthreads();
}

// dW[to][ti] += sum over the tile's rows of A[16 to + .][row] B[16 ti + .][row] (both staged as images)
template <int NO, int NI>
__device__ __forceinline__ void ec_outer(const float *imgA, const float *imgB, f32x4 (&dW)[NO][NI], int g, int c) {
#pragma unroll
    for (int ti = 0; ti < NI; ++ti) {
        const f32x4 b4 = rf_read_k(imgB, ti, g, c);
#pragma unroll
        for (int to = 0; to < NO; ++to) {
            const f32x4 a4 = rf_read_k(imgA, to, g, c);
#pragma unroll
            for (int s = 0; s < 4; ++s) dW[to][ti] = mfma4(a4[s], b4[s], dW[to][ti]);
        }
    }
}

template <int HT, int DT, int OT>
__global__ __launch_bounds__(kBlock, 1) void edge_conv_bwd_kernel(const EcArgs a) {
    constexpr int kW1 = HT * 4 * DT * 64, kW2 = OT * 4 * HT * 64;
    constexpr int kFrag = 4 * kW1 + 2 * kW2;
    constexpr int kRed = (16 * HT) * (32 * DT) > (16 * OT) * (16 * HT) ? (16 * HT) * (32 * DT) : (16 * OT) * (16 * HT);
    constexpr int kMem = kFrag > kRed ? kFrag : kRed;
    constexpr int kST = OT > DT ? OT : DT;
    __shared__ __attribute__((aligned(16))) float s_mem[kMem];
    __shared__ __attribute__((aligned(16))) float s_big[kWaves][16 * HT * kRfLd];
    __shared__ __attribute__((aligned(16))) float s_small[kWaves][16 * kST * kRfLd];
    __shared__ __attribute__((aligned(16))) float s_b1[16 * HT];
    __shared__ __attribute__((aligned(16))) float s_redb[16 * HT];
    float *s_w1a = s_mem, *s_w1b = s_w1a + kW1, *s_w1at = s_w1b + kW1, *s_w1bt = s_w1at + kW1;
    float *s_w2 = s_w1bt + kW1, *s_w2t = s_w2 + kW2;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.k + a.include_self;
    const bool want_dx = a.gx_tgt != nullptr;
    ec_copy(s_w1a, a.fw1a, kW1, tid);
    ec_copy(s_w1b, a.fw1b, kW1, tid);
    ec_copy(s_w1at, a.fw1at, kW1, tid);
    ec_copy(s_w1bt, a.fw1bt, kW1, tid);
    ec_copy(s_w2, a.fw2, kW2, tid);
    ec_copy(s_w2t, a.fw2t, kW2, tid);
    ec_bias(s_b1, a.b1, a.hidden, 16 * HT, tid);
    __syncthreads();
    float *imgBig = s_big[wv], *imgSmall = s_small[wv];
    const int64_t n_tiles = (a.n + 15) / 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 dW2[OT][HT], dW1a[HT][DT], dW1b[HT][DT], db1[HT], db2[OT];
#pragma unroll
    for (int to = 0; to < OT; ++to) {
        db2[to] = zero;
#pragma unroll
        for (int ti = 0; ti < HT; ++ti) dW2[to][ti] = zero;
    }
#pragma unroll
    for (int to = 0; to < HT; ++to) {
        db1[to] = zero;
#pragma unroll
        for (int ti = 0; ti < DT; ++ti) dW1a[to][ti] = dW1b[to][ti] = zero;
    }

    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wv; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
        EcNode<DT> nd;
        ec_load_node<DT>(a, tile, g, c, nd);
        // upstream gradient of the aggregated row: through the ReLU epilogue, and g / count for the mean
        f32x4 gq[OT];
        int win[OT][4];
        const float inv = (a.aggr == kEcMean && nd.count > 0) ? 1.f / (float)nd.count : 1.f;
#pragma unroll
        for (int to = 0; to < OT; ++to)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * to + 4 * g + r;
                float v = 0.f;
                int w = -1;
                if (nd.valid && f < a.out_dim) {
                    v = a.gout[nd.row * a.out_dim + f];
                    if (a.relu && !(a.h[nd.row * a.out_dim + f] > 0.f)) v = 0.f;
                    if (a.aggr == kEcMean) v = v * inv;
                    if (a.aggr == kEcMax) w = a.win[nd.row * a.out_dim + f];
                }
                gq[to][r] = v;
                win[to][r] = w;
            }
        f32x4 ha[HT], gzsum[HT], gbsum[DT];
        ec_init_bias<HT>(s_b1, ha, g);
        ec_gemm<HT, DT>(s_w1a, nd.xi, ha, lane);
#pragma unroll
        for (int t = 0; t < HT; ++t) gzsum[t] = zero;
#pragma unroll
        for (int t = 0; t < DT; ++t) gbsum[t] = zero;

#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            f32x4 d[DT], p[HT], gm[OT];
            if (__ballot(s < nd.count) == 0ull) break;   // (the rows of gx_slot past a node's count stay unwritten)
            const bool present = ec_load_diff<DT>(a, nd, s, g, d);
#pragma unroll
            for (int t = 0; t < HT; ++t) p[t] = ha[t];
            ec_gemm<HT, DT>(s_w1b, d, p, lane);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) p[t][r] = fmaxf(p[t][r], 0.f);
            // the slot's share of the upstream gradient: all of it (add, mean), or where the slot won (max)
#pragma unroll
            for (int to = 0; to < OT; ++to)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool on = present && (a.aggr != kEcMax || win[to][r] == s);
                    gm[to][r] = on ? gq[to][r] : 0.f;
                    db2[to][r] += gm[to][r];
                }
            rf_stage_tiles<HT>(imgBig, p, HT, g, c);
            rf_stage_tiles<OT>(imgSmall, gm, OT, g, c);
            lds_wave_order();
            ec_outer<OT, HT>(imgSmall, imgBig, dW2, g, c);
            lds_wave_order();
            // through W2 and the hidden ReLU (p > 0 exactly where the pre-activation is)
            f32x4 gz[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) gz[t] = zero;
            ec_gemm<HT, OT>(s_w2t, gm, gz, lane);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gz[t][r] = p[t][r] > 0.f ? gz[t][r] : 0.f;
                    gzsum[t][r] += gz[t][r];
                }
            rf_stage_tiles<HT>(imgBig, gz, HT, g, c);
            rf_stage_tiles<DT>(imgSmall, d, DT, g, c);
            lds_wave_order();
            ec_outer<HT, DT>(imgBig, imgSmall, dW1b, g, c);
            lds_wave_order();
            if (want_dx) {   // g_b = W1b^T gz: the slot's row for the source, and minus it for the target
                f32x4 gb[DT];
#pragma unroll
                for (int t = 0; t < DT; ++t) gb[t] = zero;
                ec_gemm<DT, HT>(s_w1bt, gz, gb, lane);
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * t + 4 * g + r;
                        gbsum[t][r] += gb[t][r];
                        if (nd.valid && f < a.dim) a.gx_slot[(nd.row * S + s) * a.dim + f] = gb[t][r];
                    }
            }
        }
        // what is the same for every slot: dW1a = (sum_s gz) (x) x_i, db1, g_a = W1a^T sum_s gz
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) db1[t][r] += gzsum[t][r];
        rf_stage_tiles<HT>(imgBig, gzsum, HT, g, c);
        rf_stage_tiles<DT>(imgSmall, nd.xi, DT, g, c);
        lds_wave_order();
        ec_outer<HT, DT>(imgBig, imgSmall, dW1a, g, c);
        lds_wave_order();
        if (want_dx) {
            f32x4 ga[DT];
#pragma unroll
            for (int t = 0; t < DT; ++t) ga[t] = zero;
            ec_gemm<DT, HT>(s_w1at, gzsum, ga, lane);
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * t + 4 * g + r;
                    if (nd.valid && f < a.dim) a.gx_tgt[nd.row * a.dim + f] = ga[t][r] - gbsum[t][r];
                }
        }
    }

    // the block's partial: dW2 [O][H], db2 [O], dW1 [H][2D], db1 [H]
    const int H = a.hidden, O = a.out_dim, D = a.dim;
    float *part = a.part + (int64_t)blockIdx.x * a.part_total;
    rf_emit_dw<OT, HT>(s_mem, part, dW2, OT, HT, O, H, wv, tid, g, c);
    rf_emit_db<OT>(s_redb, part + O * H, db2, OT, O, wv, tid, g, c);
    ec_emit_dw1<HT, DT>(s_mem, part + O * H + O, dW1a, dW1b, H, D, wv, tid, g, c);
    rf_emit_db<HT>(s_redb, part + O * H + O + H * 2 * D, db1, HT, H, wv, tid, g, c);
}

// ---- host -----------------------------------------------------------------------------------------
struct EcShape {
    int HT, DT, OT;
};
EcShape ec_shape(int dim, int hidden, int out_dim) {
    const int t = rf_tiles(hidden);
    return {t <= 2 ? 2 : t <= 4 ? 4 : t <= 7 ? 7 : 8, rf_tiles(dim), rf_tiles(out_dim)};
}
int ec_part_total(int dim, int hidden, int out_dim) { return out_dim * hidden + out_dim + hidden * 2 * dim + hidden; }
int ec_grid(int64_t n, bool backward) {
    const int64_t tiles = (n + 15) / 16;
    int64_t g = (tiles + kWaves - 1) / kWaves;
    const int64_t cap = (int64_t)cu_count() * (backward ? 1 : 2);
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}
struct EcWs {
    float *w1a, *w1b, *w2, *w2t, *w1at, *w1bt, *part;
    size_t total;
};
EcWs ec_ws(int dim, int hidden, int out_dim, int64_t n, bool backward, void *base) {
    const EcShape s = ec_shape(dim, hidden, out_dim);
    const size_t w1 = (size_t)s.HT * 4 * s.DT * 64, w2 = (size_t)s.OT * 4 * s.HT * 64;
    Carver ws{(char *)base};
    EcWs w{};
    w.w1a = ws.take<float>(w1);
    w.w1b = ws.take<float>(w1);
    w.w2 = ws.take<float>(w2);
    if (backward) {
        w.w2t = ws.take<float>(w2);
        w.w1at = ws.take<float>(w1);
        w.w1bt = ws.take<float>(w1);
        w.part = ws.take<float>((size_t)ec_grid(n, true) * ec_part_total(dim, hidden, out_dim));
    }
    w.total = ws.off;
    return w;
}

int ec_check_shape(const char *who, int dim, int hidden, int out_dim) {
    (void)who;
    if (dim < 1 || hidden < 1 || out_dim < 1) return fail(GNNTRK_EINVAL, "edge_conv: dim, hidden and out_dim must be positive");
    if (2 * dim > GNNTRK_RESFCNN_MAX_IN || hidden > kEcMaxHidden || out_dim > kEcMaxOut)
        return fail(GNNTRK_EUNSUPPORTED, "edge_conv: limits are 2 dim <= 64, hidden <= 128, out_dim <= 32");
    return GNNTRK_OK;
}

int ec_check(const char *who, const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
             const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *W1, const float *W2,
             int32_t hidden, int32_t out_dim, int32_t aggr) {
    if (n < 0) return fail(GNNTRK_EINVAL, "edge_conv: negative node count");
    if (k < 1 || k_stride < k) return fail(GNNTRK_EINVAL, "edge_conv: k must be at least 1 and at most k_stride");
    if (aggr < kEcAdd || aggr > kEcMax) return fail(GNNTRK_EINVAL, "edge_conv: aggr must be 0 (add), 1 (mean) or 2 (max)");
    if (!W1 || !W2) return fail(GNNTRK_EINVAL, "edge_conv: NULL weight pointer");
    int rc = ec_check_shape(who, dim, hidden, out_dim);
    if (rc) return rc;
    if (k + (include_self ? 1 : 0) > kEcMaxSlots)
        return fail(GNNTRK_EUNSUPPORTED, "edge_conv: at most 64 slots per query (k + include_self)");
    if (n >= ((int64_t)1 << 30)) return fail(GNNTRK_EUNSUPPORTED, "edge_conv: at most 2^30-1 nodes");
    if (n > 0 && (!x || !nbr || !cnt)) return fail(GNNTRK_EINVAL, "edge_conv: NULL rows or neighbour table");
    if (n > 0 && x_stride < dim) return fail(GNNTRK_EINVAL, "edge_conv: x_stride smaller than dim");
    return GNNTRK_OK;
}

int ec_pack(const EcWs &w, const float *W1, const float *W2, int dim, int hidden, int out_dim, bool backward,
            hipStream_t stream) {
    const EcShape s = ec_shape(dim, hidden, out_dim);
    RfPackArgs pa;
    memset(&pa, 0, sizeof(pa));
    int n = 0;
    auto job = [&](const float *W, float *dst, int rows, int cols, int rt, int kt, int ld, int transposed) {
        RfPackJob &j = pa.job[n++];
        j.W = W, j.dst = dst, j.rows = rows, j.cols = cols, j.rt = rt, j.kt = kt, j.ld = ld, j.transposed = transposed;
    };
    job(W1, w.w1a, hidden, dim, s.HT, s.DT, 2 * dim, 0);
    job(W1 + dim, w.w1b, hidden, dim, s.HT, s.DT, 2 * dim, 0);
    job(W2, w.w2, out_dim, hidden, s.OT, s.HT, hidden, 0);
    if (backward) {
        job(W2, w.w2t, hidden, out_dim, s.HT, s.OT, hidden, 1);
        job(W1, w.w1at, dim, hidden, s.DT, s.HT, 2 * dim, 1);
        job(W1 + dim, w.w1bt, dim, hidden, s.DT, s.HT, 2 * dim, 1);
    }
    pa.n_jobs = n;
    hipLaunchKernelGGL(resfcnn_pack_kernel, dim3(8, n), dim3(256), 0, stream, pa);
    return check_launch("edge_conv_pack");
}

template <class F> void ec_dispatch(const EcShape &s, F &&f) {
#define GNNTRK_EC_CASE(HT_, DT_, OT_) \
    if (s.HT == HT_ && s.DT == DT_ && s.OT == OT_) f(int_c<HT_>{}, int_c<DT_>{}, int_c<OT_>{});
    GNNTRK_EC_CASE(2, 1, 1) GNNTRK_EC_CASE(2, 1, 2) GNNTRK_EC_CASE(2, 2, 1) GNNTRK_EC_CASE(2, 2, 2)
    GNNTRK_EC_CASE(4, 1, 1) GNNTRK_EC_CASE(4, 1, 2) GNNTRK_EC_CASE(4, 2, 1) GNNTRK_EC_CASE(4, 2, 2)
    GNNTRK_EC_CASE(7, 1, 1) GNNTRK_EC_CASE(7, 1, 2) GNNTRK_EC_CASE(7, 2, 1) GNNTRK_EC_CASE(7, 2, 2)
    GNNTRK_EC_CASE(8, 1, 1) GNNTRK_EC_CASE(8, 1, 2) GNNTRK_EC_CASE(8, 2, 1) GNNTRK_EC_CASE(8, 2, 2)
#undef GNNTRK_EC_CASE
}

void ec_fill(EcArgs &a, const EcWs &w, const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
             const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *b1, const float *b2,
             int32_t hidden, int32_t out_dim, int32_t aggr, int32_t relu) {
    memset(&a, 0, sizeof(a));
    a.x = x, a.nbr = nbr, a.cnt = cnt, a.n = n;
    a.x_stride = x_stride, a.dim = dim, a.k = k, a.k_stride = k_stride, a.include_self = include_self ? 1 : 0;
    a.hidden = hidden, a.out_dim = out_dim, a.aggr = aggr, a.relu = relu ? 1 : 0;
    a.part_total = ec_part_total(dim, hidden, out_dim);
    a.fw1a = w.w1a, a.fw1b = w.w1b, a.fw2 = w.w2, a.fw2t = w.w2t, a.fw1at = w.w1at, a.fw1bt = w.w1bt;
    a.b1 = b1, a.b2 = b2;
}

}  // namespace
}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_edge_conv_workspace_bytes(int32_t dim, int32_t hidden, int32_t out_dim, int64_t n, int32_t backward) {
    if (n < 0 || ec_check_shape("edge_conv_workspace_bytes", dim, hidden, out_dim)) return 0;
    return ec_ws(dim, hidden, out_dim, n, backward != 0, nullptr).total;
}

int gnntrk_edge_conv_forward(const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
                             const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *W1,
                             const float *b1, const float *W2, const float *b2, int32_t hidden, int32_t out_dim,
                             int32_t aggr, int32_t relu, float *h, int32_t *win, void *workspace, size_t workspace_bytes,
                             void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ec_check("edge_conv_forward", x, x_stride, n, dim, nbr, cnt, k, k_stride, include_self, W1, W2, hidden, out_dim,
                      aggr);
    if (rc || n == 0) return rc;
    if (!h || (aggr == kEcMax && !win)) return fail(GNNTRK_EINVAL, "edge_conv_forward: NULL output");
    const EcWs w = ec_ws(dim, hidden, out_dim, n, false, workspace);
    rc = check_workspace("edge_conv", workspace, workspace_bytes, w.total);
    if (rc) return rc;
    if ((uintptr_t)workspace & 15) return fail(GNNTRK_EINVAL, "edge_conv_forward: workspace misaligned");
    rc = ec_pack(w, W1, W2, dim, hidden, out_dim, false, stream);
    if (rc) return rc;
    EcArgs a;
    ec_fill(a, w, x, x_stride, n, dim, nbr, cnt, k, k_stride, include_self, b1, b2, hidden, out_dim, aggr, relu);
    a.h = h;
    a.win = aggr == kEcMax ? win : nullptr;
    const int grid = ec_grid(n, false);
    ec_dispatch(ec_shape(dim, hidden, out_dim), [&](auto HT, auto DT, auto OT) {
        hipLaunchKernelGGL((edge_conv_fwd_kernel<decltype(HT)::value, decltype(DT)::value, decltype(OT)::value>), dim3(grid), dim3(kBlock), 0, stream, a);
    });
    return check_launch("edge_conv_forward");
}

int gnntrk_edge_conv_backward(const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
                              const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *W1,
                              const float *b1, const float *W2, const float *b2, int32_t hidden, int32_t out_dim,
                              int32_t aggr, int32_t relu, const float *h, const int32_t *win, const float *gout, float *gW1,
                              float *gb1, float *gW2, float *gb2, float *gx_tgt, float *gx_slot, int32_t accumulate,
                              void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ec_check("edge_conv_backward", x, x_stride, n, dim, nbr, cnt, k, k_stride, include_self, W1, W2, hidden, out_dim,
                      aggr);
    if (rc || n == 0) return rc;
    if (!gout || (relu && !h) || (aggr == kEcMax && !win)) return fail(GNNTRK_EINVAL, "edge_conv_backward: NULL pointer");
    if ((gx_tgt == nullptr) != (gx_slot == nullptr))
        return fail(GNNTRK_EINVAL, "edge_conv_backward: gx_tgt and gx_slot come together");
    const EcWs w = ec_ws(dim, hidden, out_dim, n, true, workspace);
    rc = check_workspace("edge_conv", workspace, workspace_bytes, w.total);
    if (rc) return rc;
    if ((uintptr_t)workspace & 15) return fail(GNNTRK_EINVAL, "edge_conv_backward: workspace misaligned");
    rc = ec_pack(w, W1, W2, dim, hidden, out_dim, true, stream);
    if (rc) return rc;
    EcArgs a;
    ec_fill(a, w, x, x_stride, n, dim, nbr, cnt, k, k_stride, include_self, b1, b2, hidden, out_dim, aggr, relu);
    a.h = const_cast<float *>(h);
    a.win = const_cast<int32_t *>(win);
    a.gout = gout;
    a.gx_tgt = gx_tgt;
    a.gx_slot = gx_slot;
    a.part = w.part;
    const int grid = ec_grid(n, true);
    ec_dispatch(ec_shape(dim, hidden, out_dim), [&](auto HT, auto DT, auto OT) {
        hipLaunchKernelGGL((edge_conv_bwd_kernel<decltype(HT)::value, decltype(DT)::value, decltype(OT)::value>), dim3(grid), dim3(kBlock), 0, stream, a);
    });
    rc = check_launch("edge_conv_backward");
    if (rc) return rc;
    // segments of a partial block in the kernel's order
    RfReduceArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.part = w.part;
    ra.part_total = a.part_total;
    ra.n_part = grid;
    ra.accumulate = accumulate;
    int ns = 0, off = 0;
    auto seg = [&](float *dst, int len) {
        ra.off[ns] = off;
        ra.dst[ns] = dst;
        off += len;
        ++ns;
    };
    seg(gW2, out_dim * hidden);
    seg(gb2, out_dim);
    seg(gW1, hidden * 2 * dim);
    seg(gb1, hidden);
    ra.off[ns] = off;
    ra.n_seg = ns;
    hipLaunchKernelGGL(resfcnn_reduce_kernel, dim3((a.part_total + 31) / 32), dim3(256), 0, stream, ra);
    return check_launch("edge_conv_reduce");
}

}  // extern "C"
