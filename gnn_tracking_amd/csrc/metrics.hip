// Edge-classifier validation metrics (training/ec.py:55-84 with metrics/binary_classification.py):
//
//  * gnntrk_bcs_counts: the whole threshold scan of get_maximized_bcs (:147-195) - for every pt cut,
//    label and threshold bin the number of edges - in ONE streaming pass over the edges (LDS
//    histogram per workgroup, wave-aggregated LDS atomics, one coalesced int64 atomic per bin and
//    workgroup at the end);
//  * gnntrk_roc_auc: the exact ROC AUC and McClish-standardised partial AUCs of get_roc_auc_scores
//    (:198-231) for every pt cut - one radix sort of (order-preserving score key, cut class | label),
//    then per cut two passes over the sorted pairs with a decoupled (tile sums -> one-block scan ->
//    tile emit) int64 scan over the tie groups.  Exact in integers, deterministic.
//
// Shared edge semantics (bit for bit the reference's):
//  * positive iff int(y) == 1 (BinaryClassificationStats: y.int() == 1);
//  * cut c <= 0 takes every edge; cut c > 0 takes it iff pt[src] > c || pt[tgt] > c (NaN pt: never).
//    The cuts ascend, so "passes cut j" is monotone in j and an edge is described by its CUT CLASS,
//    the number of cuts it passes; per-cut tables are suffix sums over the classes.
#include <math.h>
#include <stdio.h>

#include "count_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kMaxCuts = GNNTRK_METRICS_MAX_CUTS;
constexpr int kMaxThr = GNNTRK_METRICS_MAX_THR;
constexpr int kMaxFpr = GNNTRK_AUC_MAX_FPR;
// LDS histograms of (cut class, label, bin): the common size (a few cuts, the reference's 200
// thresholds: 5 x 2 x 201 bins) and the largest the ABI admits (9 x 2 x 1025)
constexpr int kHistSmall = 4096;
constexpr int kHistLarge = (kMaxCuts + 1) * 2 * (kMaxThr + 1);

struct Fprs {   // (kernel arguments by value: nothing to upload)
    double v[kMaxFpr];
};

template <class ID>
__device__ __forceinline__ int cut_class(const ID *src, const ID *tgt, const float *pt, int64_t i, const Cuts &cuts) {
    if (!pt) return cuts.n;
    const float a = pt[src[i]], b = pt[tgt[i]];
    int k = 0;
    for (int j = 0; j < cuts.n; ++j) k += (cuts.v[j] <= 0.f || a > cuts.v[j] || b > cuts.v[j]) ? 1 : 0;
    return k;
}

// ----------------------------------------------------------------- threshold counts
// bin k = #{j : !(w < thr[j])}: the reference's "predicted true" is !(w < thld), so a NaN score is
// predicted true everywhere (bin n_thr).  The predicate is a prefix of the ascending table, so a
// branch-free binary search over the LDS copy finds k exactly.
template <class ID, class Y, int kCap>
__global__ __launch_bounds__(kTpb) void bcs_counts_kernel(const float *__restrict__ w, const Y *__restrict__ y,
                                                          const int32_t *__restrict__ perm, const ID *__restrict__ src,
                                                          const ID *__restrict__ tgt, const float *__restrict__ pt,
                                                          Cuts cuts, const float *__restrict__ thr, int n_thr, int64_t n,
                                                          unsigned long long *__restrict__ counts) {
    __shared__ float s_thr[kMaxThr];
    __shared__ uint32_t hist[kCap];
    const int nb = n_thr + 1, row = 2 * nb, nh = (cuts.n + 1) * row;
    for (int i = threadIdx.x; i < n_thr; i += kTpb) s_thr[i] = thr[i];
    for (int i = threadIdx.x; i < nh; i += kTpb) hist[i] = 0u;
    __syncthreads();
    int top = 0;   // largest power of two <= n_thr
    for (int s = 1; s <= n_thr; s <<= 1) top = s;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kTpb;
    // (the loop bound is wave-uniform: the ballots below need every lane of the wave)
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        int key = -1;
        if (i < n) {
            const float x = w[i];
            int k = 0;
            for (int s = top; s > 0; s >>= 1)
                if (k + s <= n_thr && !(x < s_thr[k + s - 1])) k += s;
            const uint32_t pos = is_positive(y, perm ? (int64_t)perm[i] : i);
            key = (cut_class(src, tgt, pt, i, cuts) * 2 + (int)pos) * nb + k;
        }
        // a trained classifier's scores pile up at eps and 1 - eps: most lanes of a wave share a
        // few bins.  Two leader rounds take the commonest keys with one LDS atomic each; the rest
        // (a uniform distribution's scattered keys) add directly.
        for (int r = 0; r < 2; ++r) {
            const unsigned long long live = __ballot(key >= 0);
            if (!live) break;
            const int lead = __ffsll(live) - 1;
            const int lk = __shfl(key, lead);
            const unsigned long long same = __ballot(key == lk);
            if (lane == lead) atomicAdd(&hist[lk], (unsigned)__popcll(same));
            if (key == lk) key = -1;
        }
        if (key >= 0) atomicAdd(&hist[key], 1u);
    }
    __syncthreads();
    // per cut c: the classes that pass it (c + 1 .. n_cuts); one coalesced int64 add per non-zero bin
    for (int idx = threadIdx.x; idx < cuts.n * row; idx += kTpb) {
        const int c = idx / row, r = idx - c * row;
        unsigned long long s = 0;
        for (int cls = c + 1; cls <= cuts.n; ++cls) s += hist[cls * row + r];
        if (s) atomicAdd(&counts[idx], s);
    }
}

// ------------------------------------------------------------------------- ROC AUC
// sort key: fp32 bit pattern made order-preserving as unsigned; -0.0 is +0.0 (one tie group for
// torch and sklearn), every NaN is the largest key (a tie group of its own, flagged)
constexpr uint32_t kNanKey = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t score_key(float x) {
    if (x != x) return kNanKey;
    uint32_t u = __float_as_uint(x);
    if (x == 0.f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <class ID, class Y>
__global__ __launch_bounds__(kTpb) void auc_keys_kernel(const float *__restrict__ w, const Y *__restrict__ y,
                                                        const int32_t *__restrict__ perm, const ID *__restrict__ src,
                                                        const ID *__restrict__ tgt, const float *__restrict__ pt,
                                                        Cuts cuts, int64_t n, uint32_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        keys[i] = score_key(w[i]);
        vals[i] = ((uint32_t)cut_class(src, tgt, pt, i, cuts) << 1) | is_positive(y, perm ? (int64_t)perm[i] : i);
    }
}

// Cumulative counts are packed (positives << 32 | negatives): both halves are below 2^31, sums never
// carry across, and the packed value is monotone in the position - so "the cumulative count at the
// last group head before here" is a MAX scan over the heads.  Bit 63 marks "a head was seen".
constexpr unsigned long long kHead = 1ull << 63;
constexpr int kPer = 16;                    // consecutive sorted elements per thread
constexpr int kTile = kTpb * kPer;          // per workgroup
constexpr int kScanTpb = 1024;

struct OpSum {
    __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; }
};
struct OpMax {
    __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; }
};

// exclusive scan over the workgroup (identity 0); *total = the reduction of all threads' values
template <int kThreads, class Op>
__device__ unsigned long long block_scan_excl(unsigned long long v, Op op, unsigned long long *sh,
                                              unsigned long long *total) {
    constexpr int kWaves = kThreads / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl(x, lane >= d ? lane - d : lane);
        if (lane >= d) x = op(t, x);
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0;
        for (int i = 0; i < kWaves; ++i) {
            const unsigned long long t = sh[i];
            sh[i] = a;
            a = op(a, t);
        }
        sh[kWaves] = a;
    }
    __syncthreads();
    unsigned long long ex = __shfl(x, lane > 0 ? lane - 1 : 0);
    if (lane == 0) ex = 0;
    const unsigned long long r = op(sh[wid], ex);
    *total = sh[kWaves];
    __syncthreads();   // (sh is reused by the next scan)
    return r;
}

__device__ __forceinline__ unsigned long long pair_inc(uint32_t v, int cut) {
    if ((int)(v >> 1) <= cut) return 0ull;
    return (v & 1u) ? (1ull << 32) : 1ull;
}

// one thread's run of kPer sorted elements from s (clipped at n): its own packed count and the
// count, relative to s, at its last group head (kHead-flagged; 0 = no head in the run)
__device__ __forceinline__ void run_summary(const uint32_t *keys, const uint32_t *vals, int64_t s, int64_t n, int cut,
                                            unsigned long long &sum, unsigned long long &head) {
    sum = 0;
    head = 0;
    uint32_t prev = s > 0 && s < n ? keys[s - 1] : 0u;
    for (int j = 0; j < kPer; ++j) {
        const int64_t i = s + j;
        if (i >= n) break;
        const uint32_t k = keys[i];
        if (i == 0 || k != prev) head = kHead | sum;
        sum += pair_inc(vals[i], cut);
        prev = k;
    }
}

// pass 1: per tile, the packed total and the (tile-relative) count at its last head
__global__ __launch_bounds__(kTpb) void auc_tile_kernel(const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals, int64_t n, int cut,
                                                        unsigned long long *__restrict__ tile_sum,
                                                        unsigned long long *__restrict__ tile_head) {
    __shared__ unsigned long long sh[kTpb / 64 + 1];
    const int64_t s = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    unsigned long long sum, head, tot, hmax;
    run_summary(keys, vals, s, n, cut, sum, head);
    const unsigned long long off = block_scan_excl<kTpb>(sum, OpSum(), sh, &tot);
    const unsigned long long h = head ? (kHead | (off + (head & ~kHead))) : 0ull;
    block_scan_excl<kTpb>(h, OpMax(), sh, &hmax);
    if (threadIdx.x == 0) {
        tile_sum[blockIdx.x] = tot;
        tile_head[blockIdx.x] = hmax;
    }
}

// pass 2 (one workgroup): tile_sum -> exclusive prefix, tile_head -> the absolute count at the last
// head before the tile; the cut's P / N and, per max_fpr, the sklearn cut-off: the largest fp_lim with
// fp_lim / N <= max_fpr in fp64 (roc_curve's fpr = fps / fps[-1]), handed on as L = N - fp_lim
__global__ __launch_bounds__(kScanTpb) void auc_scan_kernel(unsigned long long *__restrict__ tile_sum,
                                                            unsigned long long *__restrict__ tile_head, int64_t n_tiles,
                                                            int n_fpr, Fprs max_fpr,
                                                            long long *__restrict__ out,
                                                            unsigned long long *__restrict__ lim) {
    __shared__ unsigned long long sh[kScanTpb / 64 + 1];
    const int64_t per = (n_tiles + kScanTpb - 1) / kScanTpb;
    const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    unsigned long long s = 0, tot, hm = 0, dummy;
    for (int64_t t = t0; t < t1; ++t) s += tile_sum[t];
    const unsigned long long pre0 = block_scan_excl<kScanTpb>(s, OpSum(), sh, &tot);
    unsigned long long pre = pre0;
    for (int64_t t = t0; t < t1; ++t) {
        const unsigned long long h = tile_head[t];
        if (h) hm = OpMax()(hm, kHead | (pre + (h & ~kHead)));
        pre += tile_sum[t];
    }
    unsigned long long carry = block_scan_excl<kScanTpb>(hm, OpMax(), sh, &dummy);
    pre = pre0;
    for (int64_t t = t0; t < t1; ++t) {
        const unsigned long long h = tile_head[t], ts = tile_sum[t];
        tile_sum[t] = pre;
        tile_head[t] = carry & ~kHead;
        if (h) carry = OpMax()(carry, kHead | (pre + (h & ~kHead)));
        pre += ts;
    }
    if (threadIdx.x == 0) {
        const long long P = (long long)(tot >> 32), N = (long long)(tot & 0xFFFFFFFFull);
        out[0] = P;
        out[1] = N;
        for (int m = 0; m < n_fpr; ++m) {
            long long f = 0;
            if (N > 0) {
                const double mf = max_fpr.v[m], dn = (double)N;
                f = (long long)floor(mf * dn);
                if (f < 0) f = 0;
                if (f > N) f = N;
                while (f < N && (double)(f + 1) / dn <= mf) ++f;
                while (f > 0 && (double)f / dn > mf) --f;
            }
            out[4 + 6 * m] = f;
            lim[m] = (unsigned long long)(N - f);
        }
    }
}

// pass 3: every tie group is closed by the thread that holds its last element, which knows the
// cumulative counts at the group's start (gs) and end (ce).  In the descending ROC walk the group
// adds the trapezoid fp_g * (2 tp_before + tp_g) = fp_g * (2P - TP_start - TP_end) (units 1/(2PN));
// a partial AUC takes the groups with fp_after = N - FP_start <= fp_lim whole, and the one group that
// crosses fp_lim is handed to the host for sklearn's interpolation.
__global__ __launch_bounds__(kTpb) void auc_emit_kernel(const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals, int64_t n, int cut,
                                                        const unsigned long long *__restrict__ tile_pre,
                                                        const unsigned long long *__restrict__ tile_carry, int n_fpr,
                                                        const unsigned long long *__restrict__ lim,
                                                        long long *__restrict__ out) {
    __shared__ unsigned long long sh[kTpb / 64 + 1];
    __shared__ unsigned long long acc[1 + kMaxFpr];
    if (threadIdx.x <= kMaxFpr) acc[threadIdx.x] = 0;
    const int64_t s = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    unsigned long long sum, head, tot, hmax;
    run_summary(keys, vals, s, n, cut, sum, head);
    const unsigned long long off = block_scan_excl<kTpb>(sum, OpSum(), sh, &tot);
    const unsigned long long h = head ? (kHead | (off + (head & ~kHead))) : 0ull;
    const unsigned long long hin = block_scan_excl<kTpb>(h, OpMax(), sh, &hmax);
    const unsigned long long pre = tile_pre[blockIdx.x];
    unsigned long long cum = pre + off;
    unsigned long long gs = hin ? pre + (hin & ~kHead) : tile_carry[blockIdx.x];
    const long long P = out[0], N = out[1];
    unsigned long long L[kMaxFpr];
    for (int m = 0; m < kMaxFpr; ++m) L[m] = m < n_fpr ? lim[m] : 0ull;
    unsigned long long u2 = 0, part[kMaxFpr] = {0, 0, 0, 0};
    if (s < n) {
        uint32_t prev = s > 0 ? keys[s - 1] : 0u;
        for (int j = 0; j < kPer; ++j) {
            const int64_t i = s + j;
            if (i >= n) break;
            const uint32_t k = keys[i];
            if (i == 0 || k != prev) gs = cum;
            cum += pair_inc(vals[i], cut);
            prev = k;
            if (i + 1 < n && keys[i + 1] == k) continue;
            // group [start, i] closed
            const long long tps = (long long)(gs >> 32), fps = (long long)(gs & 0xFFFFFFFFull);
            const long long tpe = (long long)(cum >> 32), fpe = (long long)(cum & 0xFFFFFFFFull);
            const long long tp = tpe - tps, fp = fpe - fps;
            if (tp + fp == 0) continue;
            if (k == kNanKey) out[3] = tp + fp;   // (the NaN group is unique: one writer)
            const unsigned long long t = (unsigned long long)fp * (unsigned long long)(2 * P - tps - tpe);
            u2 += t;
            for (int m = 0; m < n_fpr; ++m) {
                if ((unsigned long long)fps >= L[m]) {
                    part[m] += t;
                } else if ((unsigned long long)fpe >= L[m]) {   // the crossing group (one writer)
                    long long *o = out + 4 + 6 * m;
                    o[2] = P - tpe;
                    o[3] = N - fpe;
                    o[4] = tp;
                    o[5] = fp;
                }
            }
        }
    }
    // workgroup sums, one int64 add per workgroup and value (integers: the order does not matter)
    for (int d = 32; d > 0; d >>= 1) {
        u2 += __shfl_xor(u2, d);
        for (int m = 0; m < kMaxFpr; ++m) part[m] += __shfl_xor(part[m], d);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc[0], u2);
        for (int m = 0; m < n_fpr; ++m) atomicAdd(&acc[1 + m], part[m]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&out[2]), acc[0]);
        for (int m = 0; m < n_fpr; ++m) atomicAdd(reinterpret_cast<unsigned long long *>(&out[4 + 6 * m + 1]), acc[1 + m]);
    }
}

// --------------------------------------------------------------------- host side
int check_common(const char *what, const float *w, const void *y, int32_t y_kind, const void *src, const void *tgt,
                 const float *pt, const float *cuts, int32_t n_cuts, int64_t n, Cuts &c) {
    char msg[160];
    if (n < 0) return fail(GNNTRK_EINVAL, "metrics: negative edge count");
    if (n >= (int64_t(1) << 31)) {
        snprintf(msg, sizeof(msg), "%s: %lld edges; the metrics hold counts in 31 bits (at most 2^31-1 edges)", what,
                 (long long)n);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    if (n_cuts < 1 || n_cuts > kMaxCuts) {
        snprintf(msg, sizeof(msg), "%s: n_cuts = %d, expected 1..%d", what, (int)n_cuts, kMaxCuts);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (y_kind != 0 && y_kind != 1) return fail(GNNTRK_EINVAL, "metrics: y_kind must be 0 (uint8/bool) or 1 (fp32)");
    if (n > 0 && (!w || !y)) return fail(GNNTRK_EINVAL, "metrics: NULL scores or labels");
    if (pt && n > 0 && (!src || !tgt)) return fail(GNNTRK_EINVAL, "metrics: pt cuts need the NULL-free src / tgt ids");
    if (pt && !cuts) return fail(GNNTRK_EINVAL, "metrics: pt given but the cut values are NULL");
    return fill_cuts(c, pt ? cuts : nullptr, n_cuts, "metrics");   // (without pt every edge passes every cut)
}

template <class ID, class Y>
void launch_counts(const float *w, const void *y, const int32_t *perm, const void *src, const void *tgt, const float *pt,
                   const Cuts &c, const float *thr, int n_thr, int64_t n, unsigned long long *out, hipStream_t stream) {
    const int nh = (c.n + 1) * 2 * (n_thr + 1);
    if (nh <= kHistSmall)
        hipLaunchKernelGGL((bcs_counts_kernel<ID, Y, kHistSmall>), dim3(blocks_for(n, 4)), dim3(kTpb), 0, stream, w,
                           (const Y *)y, perm, (const ID *)src, (const ID *)tgt, pt, c, thr, n_thr, n, out);
    else
        hipLaunchKernelGGL((bcs_counts_kernel<ID, Y, kHistLarge>), dim3(blocks_for(n, 2)), dim3(kTpb), 0, stream, w,
                           (const Y *)y, perm, (const ID *)src, (const ID *)tgt, pt, c, thr, n_thr, n, out);
}

template <class ID, class Y>
void launch_keys(const float *w, const void *y, const int32_t *perm, const void *src, const void *tgt, const float *pt,
                 const Cuts &c, int64_t n, uint32_t *keys, uint32_t *vals, hipStream_t stream) {
    hipLaunchKernelGGL((auc_keys_kernel<ID, Y>), dim3(blocks_for(n, 8)), dim3(kTpb), 0, stream, w, (const Y *)y, perm,
                       (const ID *)src, (const ID *)tgt, pt, c, n, keys, vals);
}

struct AucWs {
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b;
    void *temp;
    size_t temp_bytes;
    unsigned long long *tile_sum, *tile_head, *lim;
    size_t total;
};

AucWs auc_ws(void *base, int64_t n) {
    AucWs w{};
    const int64_t n_tiles = ceil_div(n, kTile) > 0 ? ceil_div(n, kTile) : 1;
    const size_t N = (size_t)n;
    Carver ws{(char *)base};
    w.keys_a = ws.take<uint32_t>(N);
    w.keys_b = ws.take<uint32_t>(N);
    w.vals_a = ws.take<uint32_t>(N);
    w.vals_b = ws.take<uint32_t>(N);
    w.temp_bytes = sort_pairs_temp_bytes(n);
    w.temp = ws.take<char>(w.temp_bytes);
    w.tile_sum = ws.take<unsigned long long>((size_t)n_tiles);
    w.tile_head = ws.take<unsigned long long>((size_t)n_tiles);
    w.lim = ws.take<unsigned long long>(kMaxFpr);
    w.total = ws.off;
    return w;
}

}  // namespace

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

int gnntrk_bcs_counts(const float *w, const void *y, int32_t y_kind, const int32_t *perm, const void *src,
                      const void *tgt, int32_t ids_i64, const float *pt, const float *cuts, int32_t n_cuts,
                      const float *thr, int32_t n_thr, int64_t n, int64_t *counts, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Cuts c;
    int rc = check_common("bcs_counts", w, y, y_kind, src, tgt, pt, cuts, n_cuts, n, c);
    if (rc) return rc;
    if (n_thr < 0 || n_thr > kMaxThr) {
        char msg[96];
        snprintf(msg, sizeof(msg), "bcs_counts: n_thr = %d, expected 0..%d", (int)n_thr, kMaxThr);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (!counts || (n_thr > 0 && !thr)) return fail(GNNTRK_EINVAL, "bcs_counts: NULL counts or threshold table");
    rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)n_cuts * 2 * (n_thr + 1), stream),
                   "bcs_counts: clear");
    if (rc || n == 0) return rc;
    auto *out = reinterpret_cast<unsigned long long *>(counts);
    if (ids_i64) {
        if (y_kind) launch_counts<int64_t, float>(w, y, perm, src, tgt, pt, c, thr, n_thr, n, out, stream);
        else launch_counts<int64_t, uint8_t>(w, y, perm, src, tgt, pt, c, thr, n_thr, n, out, stream);
    } else {
        if (y_kind) launch_counts<int32_t, float>(w, y, perm, src, tgt, pt, c, thr, n_thr, n, out, stream);
        else launch_counts<int32_t, uint8_t>(w, y, perm, src, tgt, pt, c, thr, n_thr, n, out, stream);
    }
    return check_launch("bcs_counts");
}

size_t gnntrk_roc_auc_workspace_bytes(int64_t n) { return auc_ws(nullptr, n < 0 ? 0 : n).total; }

int gnntrk_roc_auc(const float *w, const void *y, int32_t y_kind, const int32_t *perm, const void *src, const void *tgt,
                   int32_t ids_i64, const float *pt, const float *cuts, int32_t n_cuts, const double *max_fprs,
                   int32_t n_fpr, int64_t n, int64_t *out, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Cuts c;
    int rc = check_common("roc_auc", w, y, y_kind, src, tgt, pt, cuts, n_cuts, n, c);
    if (rc) return rc;
    if (n_fpr < 0 || n_fpr > kMaxFpr) return fail(GNNTRK_EINVAL, "roc_auc: n_fpr must be 0..4");
    if (n_fpr > 0 && !max_fprs) return fail(GNNTRK_EINVAL, "roc_auc: NULL max_fprs");
    for (int m = 0; m < n_fpr; ++m)
        if (!(max_fprs[m] > 0.0 && max_fprs[m] <= 1.0))
            return fail(GNNTRK_EINVAL, "roc_auc: every max_fpr must lie in (0, 1]");
    if (!out) return fail(GNNTRK_EINVAL, "roc_auc: NULL output");
    if ((rc = check_workspace("roc_auc", workspace, workspace_bytes, auc_ws(nullptr, n).total))) return rc;
    rc = check_hip(hipMemsetAsync(out, 0, sizeof(int64_t) * GNNTRK_AUC_STRIDE * (size_t)n_cuts, stream),
                   "roc_auc: clear");
    if (rc || n == 0) return rc;
    const AucWs ws = auc_ws(workspace, n);
    Fprs f{};
    for (int m = 0; m < n_fpr; ++m) f.v[m] = max_fprs[m];
    if (ids_i64) {
        if (y_kind) launch_keys<int64_t, float>(w, y, perm, src, tgt, pt, c, n, ws.keys_a, ws.vals_a, stream);
        else launch_keys<int64_t, uint8_t>(w, y, perm, src, tgt, pt, c, n, ws.keys_a, ws.vals_a, stream);
    } else {
        if (y_kind) launch_keys<int32_t, float>(w, y, perm, src, tgt, pt, c, n, ws.keys_a, ws.vals_a, stream);
        else launch_keys<int32_t, uint8_t>(w, y, perm, src, tgt, pt, c, n, ws.keys_a, ws.vals_a, stream);
    }
    if ((rc = check_launch("roc_auc: keys"))) return rc;
    rc = sort_pairs_u32(ws.keys_a, ws.keys_b, ws.vals_a, ws.vals_b, n, 32, ws.temp, ws.temp_bytes, stream);
    if (rc) return rc;
    const int64_t n_tiles = ceil_div(n, kTile);
    for (int cut = 0; cut < n_cuts; ++cut) {
        long long *o = reinterpret_cast<long long *>(out + (size_t)GNNTRK_AUC_STRIDE * cut);
        hipLaunchKernelGGL(auc_tile_kernel, dim3((unsigned)n_tiles), dim3(kTpb), 0, stream, ws.keys_b, ws.vals_b, n, cut,
                           ws.tile_sum, ws.tile_head);
        hipLaunchKernelGGL(auc_scan_kernel, dim3(1), dim3(kScanTpb), 0, stream, ws.tile_sum, ws.tile_head, n_tiles,
                           (int)n_fpr, f, o, ws.lim);
        hipLaunchKernelGGL(auc_emit_kernel, dim3((unsigned)n_tiles), dim3(kTpb), 0, stream, ws.keys_b, ws.vals_b, n, cut,
                           ws.tile_sum, ws.tile_head, (int)n_fpr, ws.lim, o);
        if ((rc = check_launch("roc_auc: scan"))) return rc;
    }
    return GNNTRK_OK;
}

}  // extern "C"
