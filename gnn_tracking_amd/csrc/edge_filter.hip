// Edge filters (models/edge_filter.py) on the device (see include/gnntrk.h for the operators and the C ABI).
//
// EFMLP (:68-141) is the residual network of resfcnn.hip on EDGE rows: orientation, fragment layout, LDS
// staging and the layer-outer backward are those of resfcnn.hip (shared through resfcnn_tiles.h).  What
// differs:
//  * the input row of edge e is gathered as [x[i], x[j], edge_attr[e]] (i = edge_index[0][e], j =
//    edge_index[1][e]) straight into the accumulator layout; in the DERIVED mode there is no edge_attr array
//    and the third segment is [x[i] - x[j], x[i] + x[j]] formed in registers (the arithmetic of
//    edge_features_kernel, knn.hip: MLGraphConstruction scores its kNN edges before writing their features);
//  * no biases, no L2 normalisation, and a 1-wide decoder: a VALU dot product per lane and a cross-lane sum
//    over the four lane groups, then W = 0.001 + 0.998 sigmoid(z);
//  * rows are edges (millions): the backward keeps no edge-sized activations.  It walks the edges in chunks
//    sized by a workspace cap; per chunk the forward is re-run into the chunk's `acts`, the backward runs on
//    it, and the chunk's reduced partial sums are added to the gradients in chunk order (deterministic for a
//    given chunk size, no atomics).
//
// EFDeepSet (:22-65) needs one kernel of its own between its two MLPs: the per-edge invariants
// [|h_i - h_j|, h_i + h_j] of the encoded hits, with the per-edge gradients of its backward.
#include <cmath>
#include <cstring>

#include "resfcnn_tiles.h"

namespace gnntrk {
namespace {

struct EfArgs {
    const float *x;
    const int64_t *ei0, *ei1;      // the chunk's first edge in both rows of edge_index
    const float *edge_attr;        // the chunk's first row, or NULL (no edge features, or derived)
    int64_t n_nodes, n_rows;       // n_rows: edges of this launch
    const float *frag[kRfMaxL];    // forward fragments: 0 encoder, 1 .. n_hidden hidden
    const float *fragT[kRfMaxL];   // transposed fragments of the hidden layers (backward)
    const float *wdec;             // [hidden]
    float *out;                    // W [n_rows] or NULL
    float *z;                      // logits [n_rows] (forward of a backward chunk: written; backward: read) or NULL
    float *acts;                   // [n_hidden + 1][n_rows][HP]; forward: written (or NULL); backward: read
    const float *gout;             // dL/dW [n_rows]
    float *gstream;                // [n_rows][HP] gradient of the residual stream
    float *part;                   // [grid][part_total]
    int32_t x_stride, ea_stride, node_dim, edge_dim, in_dim, hidden, n_hidden, derived, part_total;
    float sa, sb;
};

// the gathered input rows of one tile in accumulator layout
__device__ __forceinline__ void ef_load_input(const EfArgs &a, int64_t row, bool valid, int g, int kti,
                                              f32x4 (&xin)[kRfMaxKTI]) {
    // (ids outside [0, n_nodes) are clamped: a bad edge list reads a wrong hit, never foreign memory)
    int64_t i = a.ei0[row], j = a.ei1[row];
    i = i < 0 ? 0 : (i >= a.n_nodes ? a.n_nodes - 1 : i);
    j = j < 0 ? 0 : (j >= a.n_nodes ? a.n_nodes - 1 : j);
    const float *xi = a.x + i * a.x_stride, *xj = a.x + j * a.x_stride;
    const float *ea = a.edge_attr != nullptr ? a.edge_attr + row * a.ea_stride : nullptr;
    const int nd = a.node_dim;
#pragma unroll
    for (int t = 0; t < kRfMaxKTI; ++t) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < kti) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * t + 4 * g + r;
                float u = 0.f;
                if (valid && f < a.in_dim) {
                    if (f < nd) u = xi[f];
                    else if (f < 2 * nd) u = xj[f - nd];
                    else if (!a.derived) u = ea[f - 2 * nd];
                    else if (f < 3 * nd) u = xi[f - 2 * nd] - xj[f - 2 * nd];
                    else u = xi[f - 3 * nd] + xj[f - 3 * nd];
                }
                v[r] = u;
            }
        }
        xin[t] = v;
    }
}

// ================================================================================ forward
template <int HT, int T>
__global__ __launch_bounds__(kBlock) void efmlp_fwd_kernel(const EfArgs a) {
    constexpr int KSH = 4 * HT;
    constexpr int kFragFloats = HT * (KSH > 4 * kRfMaxKTI ? KSH : 4 * kRfMaxKTI) * 64;
    __shared__ __attribute__((aligned(16))) float s_frag[kFragFloats];
    __shared__ __attribute__((aligned(16))) float s_wd[16 * HT];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    const int kti = rf_tiles(a.in_dim), ksi = 4 * kti;
    const int HP = 16 * HT;
    const int64_t n_tiles = (a.n_rows + 15) / 16;
    const int64_t n_batches = (n_tiles + kWaves * T - 1) / (kWaves * T);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        f32x4 h[T][HT];
        int64_t row[T];
        bool valid[T];
        {   // ---- encoder: h = W_enc [x_i, x_j, edge_attr]
            f32x4 xin[T][kRfMaxKTI];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t r0 = ((b * kWaves + wv) * T + t) * 16 + c;
                valid[t] = r0 < a.n_rows;
                row[t] = valid[t] ? r0 : a.n_rows - 1;
                ef_load_input(a, row[t], valid[t], g, kti, xin[t]);
            }
            rf_stage(s_frag, a.frag[0], HT * ksi * 64, s_wd, nullptr, 0, 0, tid);
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int to = 0; to < HT; ++to) h[t][to] = zero;
#pragma unroll
            for (int ti = 0; ti < kRfMaxKTI; ++ti)
                if (ti < kti) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int to = 0; to < HT; ++to) {
                            const float fa = s_frag[(to * ksi + 4 * ti + r) * 64 + lane];
#pragma unroll
                            for (int t = 0; t < T; ++t) h[t][to] = mfma4(fa, xin[t][ti][r], h[t][to]);
                        }
                }
        }
        if (a.acts != nullptr) {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (valid[t]) {
#pragma unroll
                    for (int to = 0; to < HT; ++to)
                        *reinterpret_cast<f32x4 *>(a.acts + row[t] * HP + 16 * to + 4 * g) = h[t][to];
                }
        }
        // ---- hidden layers: h = sa h + sb W relu(h)
        for (int l = 1; l <= a.n_hidden; ++l) {
            rf_stage(s_frag, a.frag[l], HT * KSH * 64, s_wd, nullptr, 0, 0, tid);
            f32x4 p[T][HT], acc[T][HT];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int to = 0; to < HT; ++to) {
                    acc[t][to] = zero;
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[t][to][r] = fmaxf(h[t][to][r], 0.f);
                }
#pragma unroll
            for (int ti = 0; ti < HT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int to = 0; to < HT; ++to) {
                        const float fa = s_frag[(to * KSH + 4 * ti + r) * 64 + lane];
#pragma unroll
                        for (int t = 0; t < T; ++t) acc[t][to] = mfma4(fa, p[t][ti][r], acc[t][to]);
                    }
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int to = 0; to < HT; ++to)
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[t][to][r] = a.sa * h[t][to][r] + a.sb * acc[t][to][r];
            if (a.acts != nullptr) {
                float *dst = a.acts + (int64_t)l * a.n_rows * HP;
#pragma unroll
                for (int t = 0; t < T; ++t)
                    if (valid[t]) {
#pragma unroll
                        for (int to = 0; to < HT; ++to)
                            *reinterpret_cast<f32x4 *>(dst + row[t] * HP + 16 * to + 4 * g) = h[t][to];
                    }
            }
        }
        // ---- decoder: z = w_dec . relu(h): every lane over its own features, then over the four lane groups
        rf_stage(s_frag, nullptr, 0, s_wd, a.wdec, a.hidden, HP, tid);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            float z = 0.f;
#pragma unroll
            for (int to = 0; to < HT; ++to) {
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(s_wd + 16 * to + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) z += w4[r] * fmaxf(h[t][to][r], 0.f);
            }
            z += __shfl_xor(z, 16);
            z += __shfl_xor(z, 32);
            if (valid[t] && g == 0) {
                if (a.z != nullptr) a.z[row[t]] = z;
                if (a.out != nullptr) a.out[row[t]] = 0.001f + 0.998f * sigmoidf_(z);
            }
        }
    }
}

// ================================================================================ backward (one chunk)
template <int HT>
__global__ __launch_bounds__(kBlock, HT > 4 ? 1 : 2) void efmlp_bwd_kernel(const EfArgs a) {
    constexpr int KSH = 4 * HT;
    constexpr int kFragFloats = HT * (KSH > 4 * kRfMaxKTI ? KSH : 4 * kRfMaxKTI) * 64;   // >= hidden^2, hidden * in
    constexpr int kImgTiles = HT > kRfMaxKTI ? HT : kRfMaxKTI;
    constexpr int kImg = 16 * kImgTiles * kRfLd;
    __shared__ __attribute__((aligned(16))) float s_frag[kFragFloats];
    __shared__ __attribute__((aligned(16))) float s_img[kWaves][2][kImg];
    __shared__ __attribute__((aligned(16))) float s_wd[16 * HT];
    __shared__ __attribute__((aligned(16))) float s_redb[16 * HT];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    const int kti = rf_tiles(a.in_dim);
    const int HP = 16 * HT, H = a.hidden;
    const int64_t n_tiles = (a.n_rows + 15) / 16;
    // the block's tiles: one contiguous range (the gradient stream of a row is written and read by the same lane)
    const int64_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tb0 = per * blockIdx.x, tb1 = (tb0 + per < n_tiles) ? tb0 + per : n_tiles;
    float *imgG = s_img[wv][0], *imgP = s_img[wv][1];
    float *part = a.part + (int64_t)blockIdx.x * a.part_total;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int poff = 0;   // running offset inside the partial block: dec W, hidden n_hidden .. 1, enc W

    {   // ---------------------------------------------------------------- decoder and the output map
        rf_stage(s_frag, nullptr, 0, s_wd, a.wdec, H, HP, tid);
        const float *xl = a.acts + (int64_t)a.n_hidden * a.n_rows * HP;
        f32x4 dwd[HT];   // register r of lane (g, c): sum over this wave's tiles of gz[row c] relu(h)[16 t + 4g + r][row c]
#pragma unroll
        for (int t = 0; t < HT; ++t) dwd[t] = zero;
        for (int64_t tile = tb0 + wv; tile < tb1; tile += kWaves) {
            const int64_t r0 = tile * 16 + c;
            const bool valid = r0 < a.n_rows;
            const int64_t row = valid ? r0 : a.n_rows - 1;
            // W = 0.001 + 0.998 s(z):  dL/dz = dL/dW 0.998 s (1 - s)
            const float s = sigmoidf_(a.z[row]);
            const float gz = valid ? a.gout[row] * (0.998f * (s * (1.f - s))) : 0.f;
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xl + row * HP + 16 * t + 4 * g);
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(s_wd + 16 * t + 4 * g);
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = fmaxf(xv[r], 0.f);
                    dwd[t][r] += gz * p;
                    v[r] = p > 0.f ? w4[r] * gz : 0.f;
                }
                if (valid) *reinterpret_cast<f32x4 *>(a.gstream + row * HP + 16 * t + 4 * g) = v;
            }
        }
        rf_emit_db<HT>(s_redb, part + poff, dwd, HT, H, wv, tid, g, c);
        poff += H;
    }

    // ---------------------------------------------------------------- hidden layers, last to first
    for (int l = a.n_hidden; l >= 1; --l) {
        rf_stage(s_frag, a.fragT[l], HT * KSH * 64, s_wd, nullptr, 0, 0, tid);
        const float *xl = a.acts + (int64_t)(l - 1) * a.n_rows * HP;
        f32x4 dW[HT][HT];
#pragma unroll
        for (int to = 0; to < HT; ++to)
#pragma unroll
            for (int ti = 0; ti < HT; ++ti) dW[to][ti] = zero;
        for (int64_t tile = tb0 + wv; tile < tb1; tile += kWaves) {
            const int64_t r0 = tile * 16 + c;
            const bool valid = r0 < a.n_rows;
            const int64_t row = valid ? r0 : a.n_rows - 1;
            // (gz = sb gy is staged straight into its image and re-derived per use, as in resfcnn_bwd_kernel)
            f32x4 gy[HT], p[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                gy[t] = valid ? *reinterpret_cast<const f32x4 *>(a.gstream + row * HP + 16 * t + 4 * g) : zero;
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xl + row * HP + 16 * t + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[t][r] = fmaxf(xv[r], 0.f);
                    imgG[(16 * t + 4 * g + r) * kRfLd + c] = a.sb * gy[t][r];
                    imgP[(16 * t + 4 * g + r) * kRfLd + c] = p[t][r];
                }
            }
            f32x4 gp[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) gp[t] = zero;
            lds_wave_order();
            // W^T gz (a run-time loop over the k-steps: fully unrolled it spills at eight tiles)
#pragma unroll 4
            for (int ks = 0; ks < KSH; ++ks) {
                const float gzv = imgG[(16 * (ks >> 2) + 4 * g + (ks & 3)) * kRfLd + c];
#pragma unroll
                for (int t = 0; t < HT; ++t) gp[t] = mfma4(s_frag[(t * KSH + ks) * 64 + lane], gzv, gp[t]);
            }
            if (valid) {
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = a.sa * gy[t][r] + (p[t][r] > 0.f ? gp[t][r] : 0.f);
                    *reinterpret_cast<f32x4 *>(a.gstream + row * HP + 16 * t + 4 * g) = v;
                }
            }
#pragma unroll
            for (int ti = 0; ti < HT; ++ti) {
                const f32x4 b4 = rf_read_k(imgP, ti, g, c);
#pragma unroll
                for (int to = 0; to < HT; ++to) {
                    const f32x4 a4 = rf_read_k(imgG, to, g, c);
#pragma unroll
                    for (int s = 0; s < 4; ++s) dW[to][ti] = mfma4(a4[s], b4[s], dW[to][ti]);
                }
                __builtin_amdgcn_sched_barrier(0);   // (keeps the operand reads of the next column tile from being hoisted)
            }
            lds_wave_order();
        }
        rf_emit_dw<HT, HT>(s_frag, part + poff, dW, HT, HT, H, H, wv, tid, g, c);
        poff += H * H;
    }

    {   // ---------------------------------------------------------------- encoder (weights only)
        f32x4 dW[HT][kRfMaxKTI];
#pragma unroll
        for (int to = 0; to < HT; ++to)
#pragma unroll
            for (int ti = 0; ti < kRfMaxKTI; ++ti) dW[to][ti] = zero;
        for (int64_t tile = tb0 + wv; tile < tb1; tile += kWaves) {
            const int64_t r0 = tile * 16 + c;
            const bool valid = r0 < a.n_rows;
            const int64_t row = valid ? r0 : a.n_rows - 1;
            f32x4 gy[HT], xin[kRfMaxKTI];
#pragma unroll
            for (int t = 0; t < HT; ++t)
                gy[t] = valid ? *reinterpret_cast<const f32x4 *>(a.gstream + row * HP + 16 * t + 4 * g) : zero;
            ef_load_input(a, row, valid, g, kti, xin);
            rf_stage_tiles<HT>(imgG, gy, HT, g, c);
            rf_stage_tiles<kRfMaxKTI>(imgP, xin, kti, g, c);
            lds_wave_order();
#pragma unroll
            for (int ti = 0; ti < kRfMaxKTI; ++ti)
                if (ti < kti) {
                    const f32x4 b4 = rf_read_k(imgP, ti, g, c);
#pragma unroll
                    for (int to = 0; to < HT; ++to) {
                        const f32x4 a4 = rf_read_k(imgG, to, g, c);
#pragma unroll
                        for (int s = 0; s < 4; ++s) dW[to][ti] = mfma4(a4[s], b4[s], dW[to][ti]);
                    }
                }
            lds_wave_order();
        }
        rf_emit_dw<HT, kRfMaxKTI>(s_frag, part + poff, dW, HT, kti, H, a.in_dim, wv, tid, g, c);
    }
}

// ================================================================================ EFDeepSet: pair invariants
// out[e] = [|h_i - h_j|, h_i + h_j]; one thread per (edge, feature)
__global__ __launch_bounds__(256) void pair_invariants_fwd_kernel(const float *__restrict__ h, int dim, int stride,
                                                                  const int64_t *__restrict__ ei0,
                                                                  const int64_t *__restrict__ ei1, int64_t n_nodes,
                                                                  int64_t m, float *__restrict__ out) {
    const int64_t total = m * dim;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t e = t / dim;
        const int f = (int)(t - e * dim);
        int64_t i = ei0[e], j = ei1[e];
        i = i < 0 ? 0 : (i >= n_nodes ? n_nodes - 1 : i);
        j = j < 0 ? 0 : (j >= n_nodes ? n_nodes - 1 : j);
        const float u = h[i * stride + f], v = h[j * stride + f];
        out[e * 2 * dim + f] = fabsf(u - v);
        out[e * 2 * dim + dim + f] = u + v;
    }
}
// per-edge gradients at the two ends: gi[e] = sign(h_i - h_j) g_abs + g_sum, gj[e] = -sign(h_i - h_j) g_abs + g_sum
// (sign(0) = 0: the subgradient torch.abs uses); the caller sums them per hit over its graph index
__global__ __launch_bounds__(256) void pair_invariants_bwd_kernel(const float *__restrict__ h, int dim, int stride,
                                                                  const int64_t *__restrict__ ei0,
                                                                  const int64_t *__restrict__ ei1, int64_t n_nodes,
                                                                  int64_t m, const float *__restrict__ gout,
                                                                  float *__restrict__ gi, float *__restrict__ gj) {
    const int64_t total = m * dim;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t e = t / dim;
        const int f = (int)(t - e * dim);
        int64_t i = ei0[e], j = ei1[e];
        i = i < 0 ? 0 : (i >= n_nodes ? n_nodes - 1 : i);
        j = j < 0 ? 0 : (j >= n_nodes ? n_nodes - 1 : j);
        const float d = h[i * stride + f] - h[j * stride + f];
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float ga = sg * gout[e * 2 * dim + f], gs = gout[e * 2 * dim + dim + f];
        gi[t] = ga + gs;
        gj[t] = gs - ga;
    }
}

// ---- host -----------------------------------------------------------------------------------------
int ef_in_dim(const gnntrk_efmlp *m) { return 2 * m->node_dim + m->edge_dim; }

int ef_check(const gnntrk_efmlp *m) {
    if (!m) return fail(GNNTRK_EINVAL, "efmlp: NULL model");
    if (m->node_dim < 1 || m->edge_dim < 0 || ef_in_dim(m) > GNNTRK_RESFCNN_MAX_IN || m->hidden < 1 ||
        m->hidden > GNNTRK_RESFCNN_MAX_WIDTH || m->n_hidden < 0 || m->n_hidden > GNNTRK_RESFCNN_MAX_HIDDEN)
        return fail(GNNTRK_EUNSUPPORTED, "efmlp: limits are 2 node_dim + edge_dim <= 64, hidden <= 128, depth - 1 <= 16");
    if (m->derived && m->edge_dim != 2 * m->node_dim)
        return fail(GNNTRK_EINVAL, "efmlp: derived edge features need edge_dim = 2 node_dim");
    if (!m->W_enc || !m->W_dec) return fail(GNNTRK_EINVAL, "efmlp: NULL weight pointer");
    for (int l = 0; l < m->n_hidden; ++l)
        if (!m->W_hid[l]) return fail(GNNTRK_EINVAL, "efmlp: NULL weight pointer");
    if (!(m->beta >= 0.f && m->beta <= 1.f)) return fail(GNNTRK_EINVAL, "efmlp: beta must be in [0, 1]");
    return GNNTRK_OK;
}

int ef_check_graph(const gnntrk_efmlp *m, const gnntrk_edge_rows *d, const char *who) {
    if (!d) return fail(GNNTRK_EINVAL, "efmlp: NULL edge rows");
    if (d->n_edges < 0 || d->n_edges > 0x7fffffff) return fail(GNNTRK_EINVAL, "efmlp: bad n_edges");
    if (d->n_edges == 0) return GNNTRK_OK;
    if (!d->x || !d->edge_index || d->n_nodes < 1 || d->x_stride < m->node_dim || d->edge_stride < d->n_edges)
        return fail(GNNTRK_EINVAL, "efmlp: bad hits or edge_index");
    const bool wants_attr = m->edge_dim > 0 && !m->derived;
    if (wants_attr && (!d->edge_attr || d->ea_stride < m->edge_dim)) return fail(GNNTRK_EINVAL, "efmlp: bad edge_attr");
    (void)who;
    return GNNTRK_OK;
}

// floats of the packed fragments: encoder and hidden layers forward, then the hidden layers transposed
struct EfLayout {
    size_t fwd[kRfMaxL], bwd[kRfMaxL], total;
};
EfLayout ef_layout(const gnntrk_efmlp *m, bool with_bwd) {
    EfLayout L;
    const size_t HT = rf_ht(m->hidden), KTI = rf_tiles(ef_in_dim(m));
    size_t off = 0;
    for (int l = 0; l <= m->n_hidden; ++l) {
        L.fwd[l] = off;
        off += HT * 4 * (l == 0 ? KTI : HT) * 64;
    }
    for (int l = 0; l <= m->n_hidden; ++l) {
        L.bwd[l] = off;
        if (with_bwd && l > 0) off += HT * 4 * HT * 64;
    }
    L.total = off;
    return L;
}

int ef_pack(const gnntrk_efmlp *m, float *frag, const EfLayout &L, bool with_bwd, hipStream_t stream) {
    RfPackArgs pa;
    memset(&pa, 0, sizeof(pa));
    const int HT = rf_ht(m->hidden), KTI = rf_tiles(ef_in_dim(m));
    int n = 0;
    for (int pass = 0; pass < (with_bwd ? 2 : 1); ++pass)
        for (int l = pass; l <= m->n_hidden; ++l) {
            RfPackJob &j = pa.job[n++];
            j.W = l == 0 ? m->W_enc : m->W_hid[l - 1];
            j.ld = l == 0 ? ef_in_dim(m) : m->hidden;
            j.transposed = pass;
            j.rows = m->hidden;
            j.cols = j.ld;
            j.rt = HT;
            j.kt = l == 0 ? KTI : HT;
            j.dst = frag + (pass ? L.bwd[l] : L.fwd[l]);
        }
    pa.n_jobs = n;
    hipLaunchKernelGGL(resfcnn_pack_kernel, dim3(8, n), dim3(256), 0, stream, pa);
    return check_launch("efmlp_pack");
}

void ef_fill_args(EfArgs &a, const gnntrk_efmlp *m, const gnntrk_edge_rows *d, const float *frag, const EfLayout &L,
                  int64_t e0, int64_t rows) {
    memset(&a, 0, sizeof(a));
    for (int l = 0; l <= m->n_hidden; ++l) {
        a.frag[l] = frag + L.fwd[l];
        a.fragT[l] = frag + L.bwd[l];
    }
    a.wdec = m->W_dec;
    a.x = d->x;
    a.x_stride = d->x_stride;
    a.n_nodes = d->n_nodes;
    a.ei0 = d->edge_index + e0;
    a.ei1 = d->edge_index + d->edge_stride + e0;
    const bool wants_attr = m->edge_dim > 0 && !m->derived;
    a.edge_attr = wants_attr ? d->edge_attr + e0 * d->ea_stride : nullptr;
    a.ea_stride = d->ea_stride;
    a.n_rows = rows;
    a.node_dim = m->node_dim;
    a.edge_dim = m->edge_dim;
    a.in_dim = ef_in_dim(m);
    a.hidden = m->hidden;
    a.n_hidden = m->n_hidden;
    a.derived = m->derived;
    // np.sqrt(beta) * layer(relu(x)) + np.sqrt(1 - beta) * x: doubles, rounded when they meet the fp32 tensor
    a.sa = (float)sqrt(1.0 - (double)m->beta);
    a.sb = (float)sqrt((double)m->beta);
}

int ef_launch_fwd(const EfArgs &a, hipStream_t stream) {
    const int HT = rf_ht(a.hidden);
    const int64_t tiles = (a.n_rows + 15) / 16;
#define GNNTRK_EF_FWD(HT_, T_)                                                                          \
    if (HT == HT_) {                                                                                    \
        int64_t grid = (tiles + kWaves * T_ - 1) / (kWaves * T_);                                       \
        const int64_t cap = (int64_t)cu_count() * (HT_ > 4 ? 1 : 2);                                    \
        if (grid > cap) grid = cap;                                                                     \
        hipLaunchKernelGGL((efmlp_fwd_kernel<HT_, T_>), dim3((int)grid), dim3(kBlock), 0, stream, a);   \
    }
    GNNTRK_EF_FWD(1, 2) GNNTRK_EF_FWD(2, 2) GNNTRK_EF_FWD(3, 2) GNNTRK_EF_FWD(4, 2) GNNTRK_EF_FWD(6, 1) GNNTRK_EF_FWD(8, 1)
#undef GNNTRK_EF_FWD
    return check_launch("efmlp_forward");
}

int ef_part_total(const gnntrk_efmlp *m) {
    return m->hidden + m->n_hidden * m->hidden * m->hidden + m->hidden * ef_in_dim(m);
}

int ef_bwd_grid(int64_t n_rows) {
    const int64_t tiles = (n_rows + 15) / 16;
    int64_t g = (tiles + kWaves - 1) / kWaves;
    if (g > cu_count()) g = cu_count();
    return (int)(g < 1 ? 1 : g);
}

// bytes a row of a backward chunk holds: its residual stream after every layer, its gradient stream, its logit
size_t ef_row_bytes(const gnntrk_efmlp *m) {
    return ((size_t)(m->n_hidden + 2) * 16 * rf_ht(m->hidden) + 1) * sizeof(float);
}

int64_t ef_chunk_rows(const gnntrk_efmlp *m, int64_t n_edges, size_t cap_bytes) {
    int64_t rows = (int64_t)(cap_bytes / ef_row_bytes(m));
    rows -= rows % 64;   // whole tiles for every wave of a block
    if (rows < 64) rows = 64;
    return rows < n_edges ? rows : (n_edges > 0 ? n_edges : 1);
}

struct EfBwdWs {
    float *frag, *acts, *gstream, *z, *part;
    size_t total;
};
EfBwdWs ef_bwd_ws(const gnntrk_efmlp *m, int64_t chunk, void *base) {
    Carver ws{(char *)base};
    EfBwdWs w;
    const size_t HP = 16 * rf_ht(m->hidden);
    w.frag = ws.take<float>(ef_layout(m, true).total);
    w.acts = ws.take<float>((size_t)(m->n_hidden + 1) * chunk * HP);
    w.gstream = ws.take<float>((size_t)chunk * HP);
    w.z = ws.take<float>((size_t)chunk);
    w.part = ws.take<float>((size_t)ef_bwd_grid(chunk) * ef_part_total(m));
    w.total = ws.off;
    return w;
}

int pair_check(const float *h, int dim, int stride, const int64_t *ei, int64_t edge_stride, int64_t n_nodes, int64_t m) {
    if (dim < 1 || stride < dim || m < 0 || m > 0x7fffffff) return fail(GNNTRK_EINVAL, "pair_invariants: bad argument");
    if (m > 0 && (!h || !ei || n_nodes < 1 || edge_stride < m)) return fail(GNNTRK_EINVAL, "pair_invariants: NULL pointer");
    return GNNTRK_OK;
}

}  // namespace
}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_efmlp_forward_workspace_bytes(const gnntrk_efmlp *m) {
    if (!m || ef_check(m)) return 0;
    return ef_layout(m, false).total * sizeof(float);
}

int gnntrk_efmlp_forward(const gnntrk_efmlp *m, const gnntrk_edge_rows *rows, float *W, void *workspace,
                         size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ef_check(m);
    if (rc) return rc;
    rc = ef_check_graph(m, rows, "efmlp_forward");
    if (rc) return rc;
    if (rows->n_edges == 0) return GNNTRK_OK;
    if (!W) return fail(GNNTRK_EINVAL, "efmlp_forward: NULL output");
    const EfLayout L = ef_layout(m, false);
    rc = check_workspace("efmlp_forward", workspace, workspace_bytes, L.total * sizeof(float));
    if (rc) return rc;
    if ((uintptr_t)workspace & 15) return fail(GNNTRK_EINVAL, "efmlp_forward: workspace misaligned");
    float *frag = reinterpret_cast<float *>(workspace);
    rc = ef_pack(m, frag, L, false, stream);
    if (rc) return rc;
    EfArgs a;
    ef_fill_args(a, m, rows, frag, L, 0, rows->n_edges);
    a.out = W;
    return ef_launch_fwd(a, stream);
}

int64_t gnntrk_efmlp_backward_chunk_rows(const gnntrk_efmlp *m, int64_t n_edges, size_t cap_bytes) {
    if (!m || ef_check(m) || n_edges < 0) return 0;
    return ef_chunk_rows(m, n_edges, cap_bytes);
}

size_t gnntrk_efmlp_backward_workspace_bytes(const gnntrk_efmlp *m, int64_t n_edges, size_t cap_bytes) {
    if (!m || ef_check(m) || n_edges < 0) return 0;
    return ef_bwd_ws(m, ef_chunk_rows(m, n_edges, cap_bytes), nullptr).total;
}

int gnntrk_efmlp_backward(const gnntrk_efmlp *m, const gnntrk_edge_rows *rows, const float *gW,
                          const gnntrk_efmlp_grads *grads, int32_t accumulate, size_t cap_bytes, void *workspace,
                          size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ef_check(m);
    if (rc) return rc;
    rc = ef_check_graph(m, rows, "efmlp_backward");
    if (rc) return rc;
    if (!grads) return fail(GNNTRK_EINVAL, "efmlp_backward: NULL grads");
    const int64_t E = rows->n_edges;
    if (E > 0 && !gW) return fail(GNNTRK_EINVAL, "efmlp_backward: NULL output gradient");
    const int64_t chunk = ef_chunk_rows(m, E, cap_bytes);
    const EfBwdWs w = ef_bwd_ws(m, chunk, workspace);
    rc = check_workspace("efmlp_backward", workspace, workspace_bytes, w.total);
    if (rc) return rc;
    if ((uintptr_t)workspace & 15) return fail(GNNTRK_EINVAL, "efmlp_backward: workspace misaligned");
    const EfLayout L = ef_layout(m, true);
    const int PT = ef_part_total(m), HT = rf_ht(m->hidden);

    // segments of a partial block in the kernel's order: dec W, hidden n_hidden .. 1, enc W
    RfReduceArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.part = w.part;
    ra.part_total = PT;
    int n = 0, off = 0;
    auto seg = [&](float *dst, int len) {
        ra.off[n] = off;
        ra.dst[n] = dst;
        off += len;
        ++n;
    };
    seg(grads->W_dec, m->hidden);
    for (int l = m->n_hidden; l >= 1; --l) seg(grads->W_hid[l - 1], m->hidden * m->hidden);
    seg(grads->W_enc, m->hidden * ef_in_dim(m));
    ra.off[n] = off;
    ra.n_seg = n;

    if (E == 0) {   // no edges: the gradients are zero (or stay as they are)
        ra.n_part = 0;
        ra.accumulate = accumulate;
        hipLaunchKernelGGL(resfcnn_reduce_kernel, dim3((PT + 31) / 32), dim3(256), 0, stream, ra);
        return check_launch("efmlp_reduce");
    }
    rc = ef_pack(m, w.frag, L, true, stream);
    if (rc) return rc;
    for (int64_t e0 = 0; e0 < E; e0 += chunk) {
        const int64_t nr = E - e0 < chunk ? E - e0 : chunk;
        EfArgs a;
        ef_fill_args(a, m, rows, w.frag, L, e0, nr);
        a.acts = w.acts;
        a.z = w.z;
        rc = ef_launch_fwd(a, stream);   // the chunk's residual streams and logits; W itself is not written again
        if (rc) return rc;
        a.gout = gW + e0;
        a.gstream = w.gstream;
        a.part = w.part;
        a.part_total = PT;
        const int grid = ef_bwd_grid(nr);
#define GNNTRK_EF_BWD(HT_) \
    if (HT == HT_) hipLaunchKernelGGL((efmlp_bwd_kernel<HT_>), dim3(grid), dim3(kBlock), 0, stream, a);
        GNNTRK_EF_BWD(1) GNNTRK_EF_BWD(2) GNNTRK_EF_BWD(3) GNNTRK_EF_BWD(4) GNNTRK_EF_BWD(6) GNNTRK_EF_BWD(8)
#undef GNNTRK_EF_BWD
        rc = check_launch("efmlp_backward");
        if (rc) return rc;
        // chunk order: the first chunk sets (or adds to the caller's gradients), every later one adds
        ra.n_part = grid;
        ra.accumulate = (accumulate || e0 > 0) ? 1 : 0;
        hipLaunchKernelGGL(resfcnn_reduce_kernel, dim3((PT + 31) / 32), dim3(256), 0, stream, ra);
        rc = check_launch("efmlp_reduce");
        if (rc) return rc;
    }
    return GNNTRK_OK;
}

int gnntrk_pair_invariants_forward(const float *h, int32_t dim, int32_t h_stride, int64_t n_nodes,
                                   const int64_t *edge_index, int64_t edge_stride, int64_t n_edges, float *out,
                                   void *stream) {
    int rc = pair_check(h, dim, h_stride, edge_index, edge_stride, n_nodes, n_edges);
    if (rc || n_edges == 0) return rc;
    if (!out) return fail(GNNTRK_EINVAL, "pair_invariants_forward: NULL output");
    hipLaunchKernelGGL(pair_invariants_fwd_kernel, dim3(blocks_for(n_edges * dim, 8)), dim3(256), 0, (hipStream_t)stream, h,
                       dim, h_stride, edge_index, edge_index + edge_stride, n_nodes, n_edges, out);
    return check_launch("pair_invariants_forward");
}

int gnntrk_pair_invariants_backward(const float *h, int32_t dim, int32_t h_stride, int64_t n_nodes,
                                    const int64_t *edge_index, int64_t edge_stride, int64_t n_edges, const float *gout,
                                    float *gi, float *gj, void *stream) {
    int rc = pair_check(h, dim, h_stride, edge_index, edge_stride, n_nodes, n_edges);
    if (rc || n_edges == 0) return rc;
    if (!gout || !gi || !gj) return fail(GNNTRK_EINVAL, "pair_invariants_backward: NULL pointer");
    hipLaunchKernelGGL(pair_invariants_bwd_kernel, dim3(blocks_for(n_edges * dim, 8)), dim3(256), 0, (hipStream_t)stream, h,
                       dim, h_stride, edge_index, edge_index + edge_stride, n_nodes, n_edges, gout, gi, gj);
    return check_launch("pair_invariants_backward");
}

}  // extern "C"
