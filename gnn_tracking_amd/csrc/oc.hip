// Object-condensation loss reductions (reference: metrics/losses/oc.py:16-347,
// utils/graph_masks.py:19-28).
//
// Both reference variants - CondensationLossRG (radius graph) and CondensationLossTiger
// (dense N x K) - reduce to sums over (hit j, condensation point k) pairs:
//     attractive  sum_{j in particle k} q_j q_k |x_j - x_k|^2
//     repulsive   sum_{pid_j != pid_k, |x_j - x_k| < r} q_j q_k (r - sqrt(eps + |x_j - x_k|^2))
// plus two means over beta.  No N x K matrix and no radius graph is materialised: one
// thread owns a hit and streams the K condensation points through LDS (K ~ 1e3, a few KB);
// the gradient w.r.t. the condensation points is the transposed pass (thread = CP, hits
// streamed).  All sums are fixed-order (per-thread -> per-block fp64 partials -> one block):
// deterministic, no atomics.  Bound: fp32 VALU (N*K*D fma); HBM traffic is negligible.
// A collated batch of events runs the same kernels (BATCH = true) with every event its own problem:
// a block is a tile of one event's hits (points) and streams that event's points (hits) only.
//
// The radius-graph variant's `max_num_neighbors` cap is not emulated (torch_cluster keeps an
// implementation-defined subset when a hit has more neighbours than the cap; the reference
// tests never reach it) - see DESIGN.md.
#include "host_util.h"
#include "wave_util.h"

namespace gnntrk {

typedef unsigned long long u64;
constexpr int kOcTpb = 256;
constexpr int kOcChunk = 128;  // condensation points staged per LDS pass
constexpr int kOcMaxDim = 32;

static int oc_grid(int64_t n) {
    int64_t g = ceil_div(n, kOcTpb);
    return (int)(g < 1 ? 1 : g);
}

__device__ __forceinline__ double oc_block_sum(double v, double *sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (wave_sum here would reorder the callers' instructions)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kOcTpb / 64; ++i) s += sh[i];
    __syncthreads();
    return s;  // valid on thread 0
}

// utils/graph_masks.py:19-28
__global__ __launch_bounds__(kOcTpb) void good_node_mask_kernel(
    const float *__restrict__ pt, const int64_t *__restrict__ pid, const float *__restrict__ reco,
    const float *__restrict__ eta, int64_t n, float pt_thld, float max_eta,
    uint8_t *__restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (i < n)
        mask[i] = (pt[i] > pt_thld && pid[i] > 0 && reco[i] > 0.f && fabsf(eta[i]) < max_eta) ? 1 : 0;
}

// ---- condensation point selection (oc.py:16-43 / :279-292) ---------------------------
__global__ __launch_bounds__(kOcTpb) void oc_keys_kernel(const int64_t *__restrict__ pid, int64_t n,
                                                         u64 *__restrict__ keys,
                                                         uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (i < n) {
        keys[i] = (u64)pid[i];
        vals[i] = (uint32_t)i;
    }
}

// ---- collated batches: every event its own problem ----------------------------
// `ptr` holds the row offsets of the events ([n_seg + 1], ascending; an empty event owns no row)
template <class P>
__device__ __forceinline__ int oc_event_of(const P *__restrict__ ptr, int n_seg, int64_t i) {
    int lo = 0, hi = n_seg;  // ptr[lo] <= i < ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)ptr[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The rows of every event are cut into tiles of kOcTpb rows and the tiles numbered event by event: a block never
// holds rows of two events (its staged LDS chunk belongs to one).  The row counts live on the device, so the host
// launches ceil(n / kOcTpb) + n_seg blocks - an upper bound - and the surplus ones leave.
struct OcTile {
    int e;             // event
    int64_t row, end;  // this thread's row, the end of the event's rows
};
template <class P>
__device__ __forceinline__ bool oc_block_tile(const P *__restrict__ ptr, int n_seg, int block, OcTile &t) {
    int first = 0;
    for (int e = 0; e < n_seg; ++e) {
        const int64_t lo = ptr[e], hi = ptr[e + 1];
        const int tiles = (int)((hi - lo + kOcTpb - 1) / kOcTpb);
        if (block < first + tiles) {
            t.e = e;
            t.row = lo + (int64_t)(block - first) * kOcTpb + threadIdx.x;
            t.end = hi;
            return true;
        }
        first += tiles;
    }
    return false;
}
// the tiles [first, first + count) of event e
template <class P>
__device__ __forceinline__ void oc_event_tiles(const P *__restrict__ ptr, int e, int &first, int &count) {
    first = 0;
    for (int i = 0; i < e; ++i) first += (int)(((int64_t)ptr[i + 1] - ptr[i] + kOcTpb - 1) / kOcTpb);
    count = (int)(((int64_t)ptr[e + 1] - ptr[e] + kOcTpb - 1) / kOcTpb);
}

// selection of a batch: after the stable sort by particle id a second stable sort by event (the ids use all 64 bits
// of their key: the event has no room in it).  `batch` is sorted, so event e owns the sorted positions
// [seg_ptr[e], seg_ptr[e + 1]) as it owns those hits.
__global__ __launch_bounds__(kOcTpb) void oc_event_keys_kernel(const uint32_t *__restrict__ order,
                                                               const int64_t *__restrict__ seg_ptr, int n_seg, int64_t n,
                                                               uint32_t *__restrict__ ekeys, uint32_t *__restrict__ epos) {
    const int64_t t = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (t < n) {
        ekeys[t] = (uint32_t)oc_event_of(seg_ptr, n_seg, order[t]);
        epos[t] = (uint32_t)t;
    }
}
__global__ __launch_bounds__(kOcTpb) void oc_event_gather_kernel(const u64 *__restrict__ keys, const uint32_t *__restrict__ order,
                                                                 const uint32_t *__restrict__ pos, int64_t n,
                                                                 u64 *__restrict__ keys_out, uint32_t *__restrict__ order_out) {
    const int64_t t = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (t < n) {
        keys_out[t] = keys[pos[t]];
        order_out[t] = order[pos[t]];
    }
}

// one thread per sorted position that starts a particle: best hit of the particle.
// mode 0 (RG):    candidates = masked hits, score = beta; qualifies iff a masked hit exists
// mode 1 (Tiger): candidates = all hits of the particle, score = q; qualifies iff any masked
// ties -> lowest hit index (the sort is stable, so hits of a particle are in index order)
// seg_ptr (a batch): a particle ends where its event's sorted positions end
__global__ __launch_bounds__(kOcTpb) void oc_segment_best_kernel(
    const u64 *__restrict__ keys, const uint32_t *__restrict__ order, const float *__restrict__ score,
    const uint8_t *__restrict__ mask, int64_t n, int mode, const int64_t *__restrict__ seg_ptr, int n_seg,
    int32_t *__restrict__ seg_flag, int32_t *__restrict__ seg_best) {
    const int64_t s = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (s >= n) return;
    int32_t flag = 0, best = -1;
    int64_t lo = 0;
    if (seg_ptr) {
        const int e = oc_event_of(seg_ptr, n_seg, s);
        lo = seg_ptr[e];
        n = seg_ptr[e + 1];
    }
    if (s == lo || keys[s] != keys[s - 1]) {
        const u64 key = keys[s];
        if (key != 0ull) {  // noise (pid 0) never is an object of interest (mask needs pid > 0)
            float bs = -1.f;
            bool any = false;
            for (int64_t t = s; t < n && keys[t] == key; ++t) {
                const uint32_t h = order[t];
                const bool m = mask[h] != 0;
                any = any || m;
                if ((mode == 1 || m) && score[h] > bs) {
                    bs = score[h];
                    best = (int32_t)h;
                }
            }
            flag = (any && best >= 0) ? 1 : 0;
        }
    }
    seg_flag[s] = flag;
    seg_best[s] = best;
}

// after the exclusive scan of seg_flag: alphas[k] = CP hit of the k-th particle of interest
// (ascending pid); gid[h] = k for every hit of that particle, else -1
// seg_ptr (a batch): k counts through the events in turn, cp_ptr[e] = first k of event e
__global__ __launch_bounds__(kOcTpb) void oc_assign_kernel(
    const u64 *__restrict__ keys, const uint32_t *__restrict__ order,
    const int32_t *__restrict__ seg_flag, const int32_t *__restrict__ seg_best,
    const int64_t *__restrict__ seg_off, int64_t n, const int64_t *__restrict__ seg_ptr, int n_seg,
    int32_t *__restrict__ alphas, int32_t *__restrict__ gid, int32_t *__restrict__ cp_ptr,
    int32_t *__restrict__ n_cp) {
    const int64_t s = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (seg_ptr)
        for (int64_t e = s; e <= n_seg; e += (int64_t)gridDim.x * kOcTpb) cp_ptr[e] = (int32_t)seg_off[seg_ptr[e]];
    if (s >= n) return;
    if (s == 0) n_cp[0] = (int32_t)seg_off[n];
    int64_t lo = 0;
    if (seg_ptr) {
        const int e = oc_event_of(seg_ptr, n_seg, s);
        lo = seg_ptr[e];
        n = seg_ptr[e + 1];
    }
    if (s == lo || keys[s] != keys[s - 1]) {
        const u64 key = keys[s];
        // gid is preset to -1: only particles of interest walk their (short) segment - the noise
        // "particle" (id 0) has a tenth of all hits and would keep one thread busy for milliseconds
        const int32_t k = seg_flag[s] ? (int32_t)seg_off[s] : -1;
        if (k >= 0) {
            alphas[k] = seg_best[s];
            for (int64_t t = s; t < n && keys[t] == key; ++t) gid[order[t]] = k;
        }
    }
}

// ---- potentials -----------------------------------------------------------------------
struct OcParams {
    const float *x;
    const float *beta;
    const int64_t *pid;
    const uint8_t *mask;
    const int32_t *gid;
    const int32_t *alphas;
    const int32_t *n_cp;
    int64_t n;
    int32_t dim, stride;
    float q_min, radius, eps_sqrt;
    int32_t mode;  // 0 RG, 1 Tiger
    float keep;    // probability of keeping a repulsive pair (>= 1: all)
    u64 seed;
    const int32_t *cap_nbr;  // RG neighbour cap: per hit its max_num_neighbors-th nearest hit inside the radius, -1: fewer
    // a batch (the BATCH instantiations): row offsets of the events' hits and of their condensation points
    const int64_t *seg_ptr;
    const int32_t *cp_ptr;
    int32_t n_seg;
};

// The radius graph's neighbour cap (oc.py:115-117 radius_graph(max_num_neighbors)), nearest first: the
// condensation point a only repels hit j if a is among j's max_num_neighbors nearest hits, i.e.
// (d2(j, a), a) <= (d2(j, cap_j), cap_j) in the kNN search's own order and arithmetic (fmaf chain over
// the dimensions in order, ties to the lower index: csrc/knn.hip).
template <int DP>
__device__ __forceinline__ float oc_d2_chain(const float (&a)[DP], const float *b) {
    float d2 = 0.f;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const float t = __fsub_rn(a[d], b[d]);
        d2 = __fmaf_rn(t, t, d2);
    }
    return d2;
}
__device__ __forceinline__ bool oc_cap_ok(float d2, int a, float cap_d2, int cap_idx) {
    return cap_idx < 0 || d2 < cap_d2 || (d2 == cap_d2 && a <= cap_idx);
}

// repulsive pair (hit j, condensation point k) kept?  splitmix64 of (seed, j, k) -> 24-bit uniform
__device__ __forceinline__ bool oc_keep_pair(const OcParams &p, int64_t j, int k) {
    if (p.keep >= 1.f) return true;
    u64 z = p.seed + 0x9E3779B97F4A7C15ull * ((u64)j * 0x100000001B3ull + (u64)(uint32_t)k + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.f / 16777216.f) < p.keep;
}

__device__ __forceinline__ float oc_q(float beta, float q_min) {
    const float a = atanhf(beta);
    return a * a + q_min;
}

// what a block of the hit passes works on: its hit and the condensation points [k_lo, K) it streams.
// BATCH: a tile of one event and that event's points (false: a surplus block)
struct OcHitBlock {
    int64_t j;
    bool live;
    int k_lo, K, e;
};
template <bool BATCH>
__device__ __forceinline__ bool oc_hit_block(const OcParams &p, OcHitBlock &b) {
    if constexpr (BATCH) {
        OcTile t;
        if (!oc_block_tile(p.seg_ptr, p.n_seg, blockIdx.x, t)) return false;  // (block-uniform: before any barrier)
        b.j = t.row;
        b.live = t.row < t.end;
        b.e = t.e;
        b.k_lo = p.cp_ptr[t.e];
        b.K = p.cp_ptr[t.e + 1];
    } else {
        b.j = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
        b.live = b.j < p.n;
        b.e = 0;
        b.k_lo = 0;
        b.K = p.n_cp[0];
    }
    return true;
}

// forward: per-block partial sums part[block][4] = {attractive, repulsive, n_rep_pairs, unused}
template <int DP, bool BATCH>
__global__ __launch_bounds__(kOcTpb) void oc_forward_kernel(const OcParams p,
                                                            double *__restrict__ part) {
    __shared__ float s_x[kOcChunk][DP];
    __shared__ float s_q[kOcChunk];
    __shared__ long long s_pid[kOcChunk];
    __shared__ int s_hit[kOcChunk];  // hit index of the staged condensation point
    __shared__ double s_red[kOcTpb / 64];
    OcHitBlock hb;
    if (!oc_hit_block<BATCH>(p, hb)) return;
    const int64_t j = hb.j;
    const bool live = hb.live;
    const int K = hb.K;
    float xj[DP];
    float qj = 0.f;
    long long pj = -1;
    int gj = -1;
    bool mj = false, is_cp = false;
#pragma unroll
    for (int d = 0; d < DP; ++d) xj[d] = (live && d < p.dim) ? p.x[j * p.stride + d] : 0.f;
    if (live) {
        qj = oc_q(p.beta[j], p.q_min);
        pj = p.pid[j];
        gj = p.gid[j];
        mj = p.mask[j] != 0;
        is_cp = gj >= 0 && p.alphas[gj] == (int32_t)j;
    }
    int cap_idx = -1;
    float cap_d2 = 0.f;
    if (live && p.cap_nbr) {
        cap_idx = p.cap_nbr[j];
        if (cap_idx >= 0) {
            float xc[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) xc[d] = d < p.dim ? p.x[(int64_t)cap_idx * p.stride + d] : 0.f;
            cap_d2 = oc_d2_chain<DP>(xj, xc);
        }
    }
    const float r2 = p.radius * p.radius;
    double va = 0.0, vr = 0.0, nrep = 0.0;
    for (int k0 = hb.k_lo; k0 < K; k0 += kOcChunk) {
        __syncthreads();
        for (int i = threadIdx.x; i < kOcChunk; i += kOcTpb) {
            const int k = k0 + i;
            if (k < K) {
                const int32_t a = p.alphas[k];
#pragma unroll
                for (int d = 0; d < DP; ++d) s_x[i][d] = d < p.dim ? p.x[(int64_t)a * p.stride + d] : 0.f;
                s_q[i] = oc_q(p.beta[a], p.q_min);
                s_pid[i] = p.pid[a];
                s_hit[i] = a;
            }
        }
        __syncthreads();
        if (!live) continue;
        const int kn = (K - k0 < kOcChunk) ? (K - k0) : kOcChunk;
        for (int i = 0; i < kn; ++i) {
            float d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const float t = xj[d] - s_x[i][d];
                d2 += t * t;
            }
            const float qq = qj * s_q[i];
            if (s_pid[i] == pj) {
                const bool att = (p.mode == 1) ? (gj == k0 + i) : (gj == k0 + i && mj && !is_cp);
                if (att) va += (double)(qq * d2);
            } else if (d2 < r2 && (cap_idx < 0 || oc_cap_ok(oc_d2_chain<DP>(xj, s_x[i]), s_hit[i], cap_d2, cap_idx))) {
                nrep += 1.0;  // (counted before the sub-sampling, as the reference's n_rep)
                if (oc_keep_pair(p, j, k0 + i)) vr += (double)(qq * (p.radius - sqrtf(p.eps_sqrt + d2)));
            }
        }
    }
    const double a = oc_block_sum(va, s_red), r = oc_block_sum(vr, s_red),
                 c = oc_block_sum(nrep, s_red);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 4 + 0] = a;
        part[blockIdx.x * 4 + 1] = r;
        part[blockIdx.x * 4 + 2] = c;
        part[blockIdx.x * 4 + 3] = 0.0;
    }
}

// out[0..3] = attractive, repulsive, coward, noise; out[4..7] = norm_att, norm_rep, K, n_rep
// BATCH: block = event, over that event's tiles, points and hits; out[event][9]
template <bool BATCH>
__global__ __launch_bounds__(kOcTpb) void oc_finalize_kernel(const OcParams p,
                                                             const double *__restrict__ part,
                                                             int n_part, float *__restrict__ out) {
    __shared__ double s_red[kOcTpb / 64];
    int k_lo = 0, k_hi = p.n_cp[0];
    int64_t j_lo = 0, j_hi = p.n;
    if constexpr (BATCH) {
        const int e = blockIdx.x;
        int first;
        oc_event_tiles(p.seg_ptr, e, first, n_part);
        part += (int64_t)first * 4;
        out += e * 9;
        k_lo = p.cp_ptr[e];
        k_hi = p.cp_ptr[e + 1];
        j_lo = p.seg_ptr[e];
        j_hi = p.seg_ptr[e + 1];
    }
    const int K = k_hi - k_lo;
    const int64_t n_hits = j_hi - j_lo;
    double va = 0, vr = 0, nrep = 0, cow = 0, noise = 0, n_noise = 0, n_oi = 0;
    for (int i = threadIdx.x; i < n_part; i += kOcTpb) {
        va += part[i * 4 + 0];
        vr += part[i * 4 + 1];
        nrep += part[i * 4 + 2];
    }
    for (int k = k_lo + threadIdx.x; k < k_hi; k += kOcTpb) cow += (double)(1.f - p.beta[p.alphas[k]]);
    for (int64_t j = j_lo + threadIdx.x; j < j_hi; j += kOcTpb) {
        const bool is_noise = (p.mode == 1) ? !(p.pid[j] > 0) : (p.pid[j] == 0);
        if (is_noise) {
            noise += (double)p.beta[j];
            n_noise += 1.0;
        }
        if (p.mask[j]) n_oi += 1.0;
    }
    va = oc_block_sum(va, s_red);
    vr = oc_block_sum(vr, s_red);
    nrep = oc_block_sum(nrep, s_red);
    cow = oc_block_sum(cow, s_red);
    noise = oc_block_sum(noise, s_red);
    n_noise = oc_block_sum(n_noise, s_red);
    n_oi = oc_block_sum(n_oi, s_red);
    if (threadIdx.x == 0) {
        const double eps = 1e-9;
        const double norm_att = eps + n_oi - (double)K;
        double norm_rep = eps + ((double)K - 1.0) * (double)n_hits;
        if (p.keep < 1.f) norm_rep *= (double)p.keep;  // oc.py:328
        out[0] = (float)(va / norm_att);
        out[1] = (float)(vr / norm_rep);
        out[2] = (float)(cow / (double)K);
        out[3] = (float)(noise / n_noise);
        out[4] = (float)norm_att;
        out[5] = (float)norm_rep;
        out[6] = (float)K;
        out[7] = (float)nrep;
        out[8] = (float)n_noise;
    }
}

// backward, hit side: gx[j] and gq[j] from the pairs of hit j; g = upstream grads of the 4
// (normalised) loss terms; norms from the forward's out[4..8]
// (BATCH: fwd is [event][9], the norms are the event's)
template <int DP, bool BATCH>
__global__ __launch_bounds__(kOcTpb) void oc_backward_hits_kernel(const OcParams p,
                                                                  const float *__restrict__ g,
                                                                  const float *__restrict__ fwd,
                                                                  float *__restrict__ gx,
                                                                  float *__restrict__ gbeta) {
    __shared__ float s_x[kOcChunk][DP];
    __shared__ float s_q[kOcChunk];
    __shared__ long long s_pid[kOcChunk];
    __shared__ int s_hit[kOcChunk];
    OcHitBlock hb;
    if (!oc_hit_block<BATCH>(p, hb)) return;
    const int64_t j = hb.j;
    const bool live = hb.live;
    const int K = hb.K;
    fwd += hb.e * 9;
    const float ca = g[0] / fwd[4], cr = g[1] / fwd[5];
    float xj[DP], gxj[DP];
    float qj = 0.f, gqj = 0.f;
    long long pj = -1;
    int gj = -1;
    bool mj = false, is_cp = false;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        xj[d] = (live && d < p.dim) ? p.x[j * p.stride + d] : 0.f;
        gxj[d] = 0.f;
    }
    float bj = 0.5f;
    if (live) {
        bj = p.beta[j];
        qj = oc_q(bj, p.q_min);
        pj = p.pid[j];
        gj = p.gid[j];
        mj = p.mask[j] != 0;
        is_cp = gj >= 0 && p.alphas[gj] == (int32_t)j;
    }
    int cap_idx = -1;
    float cap_d2 = 0.f;
    if (live && p.cap_nbr) {
        cap_idx = p.cap_nbr[j];
        if (cap_idx >= 0) {
            float xc[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) xc[d] = d < p.dim ? p.x[(int64_t)cap_idx * p.stride + d] : 0.f;
            cap_d2 = oc_d2_chain<DP>(xj, xc);
        }
    }
    const float r2 = p.radius * p.radius;
    for (int k0 = hb.k_lo; k0 < K; k0 += kOcChunk) {
        __syncthreads();
        for (int i = threadIdx.x; i < kOcChunk; i += kOcTpb) {
            const int k = k0 + i;
            if (k < K) {
                const int32_t a = p.alphas[k];
#pragma unroll
                for (int d = 0; d < DP; ++d) s_x[i][d] = d < p.dim ? p.x[(int64_t)a * p.stride + d] : 0.f;
                s_q[i] = oc_q(p.beta[a], p.q_min);
                s_pid[i] = p.pid[a];
                s_hit[i] = a;
            }
        }
        __syncthreads();
        if (!live) continue;
        const int kn = (K - k0 < kOcChunk) ? (K - k0) : kOcChunk;
        for (int i = 0; i < kn; ++i) {
            float t[DP];
            float d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                t[d] = xj[d] - s_x[i][d];
                d2 += t[d] * t[d];
            }
            float cx = 0.f, cq = 0.f;  // d/dx_j = cx * t ; d/dq_j = cq
            if (s_pid[i] == pj) {
                const bool att = (p.mode == 1) ? (gj == k0 + i) : (gj == k0 + i && mj && !is_cp);
                if (att) {
                    cx = ca * 2.f * qj * s_q[i];
                    cq = ca * s_q[i] * d2;
                }
            } else if (d2 < r2 && oc_keep_pair(p, j, k0 + i) &&
                       (cap_idx < 0 || oc_cap_ok(oc_d2_chain<DP>(xj, s_x[i]), s_hit[i], cap_d2, cap_idx))) {
                const float sd = sqrtf(p.eps_sqrt + d2);
                cx = sd > 0.f ? -cr * qj * s_q[i] / sd : 0.f;
                cq = cr * s_q[i] * (p.radius - sd);
            }
#pragma unroll
            for (int d = 0; d < DP; ++d) gxj[d] += cx * t[d];
            gqj += cq;
        }
    }
    if (live) {
        for (int d = 0; d < p.dim; ++d) gx[j * p.stride + d] = gxj[d];
        // q = atanh(beta)^2 + q_min ; plus the noise mean (the coward term is added by the CP pass)
        const float a = atanhf(bj);
        float gb = gqj * 2.f * a / (1.f - bj * bj);
        const bool is_noise = (p.mode == 1) ? !(pj > 0) : (pj == 0);
        if (is_noise) gb += g[3] / fwd[8];
        gbeta[j] = gb;
    }
}

// backward, condensation-point side: thread = CP k (of the batch [k_base, k_base + kOcCpBatch)),
// the hits are cut into gridDim.y slices streamed through LDS; every (slice, CP) writes its
// partial (d/dx_k [DP], d/dq_k) and oc_backward_cps_reduce_kernel adds the slices in slice order
// into gx[alpha_k], gbeta[alpha_k] (alpha_k are distinct hits: no conflicts).  Thread = CP alone
// would leave the chip idle: K is a few thousand (19 workgroups at K = 4625) while each of them
// walks all N hits.  Runs after the hit pass.
constexpr int kOcCpBatch = 16384;  // condensation points per launch (bounds the partial buffer)
constexpr int kOcSlices = 32;      // hit slices

// BATCH: a block is a tile of one event's points and streams that event's hits, cut into gridDim.y slices; all
// points go in one launch and the partial buffer is [slices][n] (a point's row is its index k)
constexpr int kOcBatchSlices = 8;  // (the events already spread the point pass over the chip)

template <int DP, bool BATCH>
__global__ __launch_bounds__(kOcTpb) void oc_backward_cps_kernel(const OcParams p,
                                                                 const float *__restrict__ g,
                                                                 const float *__restrict__ fwd,
                                                                 int k_base, float *__restrict__ part) {
    __shared__ float s_x[kOcChunk][DP];
    __shared__ float s_q[kOcChunk];
    __shared__ long long s_pid[kOcChunk];
    __shared__ int s_att[kOcChunk];  // gid if the hit takes part in the attractive sum, else -2
    __shared__ int s_cap[kOcChunk];  // neighbour cap of the staged hit: index (-1: none) and distance
    __shared__ float s_capd2[kOcChunk];
    int kl, k;             // CP inside the batch / the partial buffer, CP
    bool live;
    int64_t h_lo = 0, h_hi = p.n;  // the hits it meets
    if constexpr (BATCH) {
        OcTile t;
        if (!oc_block_tile(p.cp_ptr, p.n_seg, blockIdx.x, t)) return;  // (uniform: before any barrier)
        kl = k = (int)t.row;
        live = t.row < t.end;
        h_lo = p.seg_ptr[t.e];
        h_hi = p.seg_ptr[t.e + 1];
        fwd += t.e * 9;
    } else {
        const int K = p.n_cp[0];
        if (k_base + (int)blockIdx.x * kOcTpb >= K) return;  // (uniform: before any barrier)
        kl = blockIdx.x * kOcTpb + threadIdx.x;
        k = k_base + kl;
        live = k < K;
    }
    const int64_t part_rows = BATCH ? p.n : kOcCpBatch;
    const float ca = g[0] / fwd[4], cr = g[1] / fwd[5];
    float xk[DP], gxk[DP];
    float qk = 0.f, gqk = 0.f;
    long long pk = -1;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        xk[d] = 0.f;
        gxk[d] = 0.f;
    }
    int32_t ak = 0;
    if (live) {
        ak = p.alphas[k];
#pragma unroll
        for (int d = 0; d < DP; ++d) xk[d] = d < p.dim ? p.x[(int64_t)ak * p.stride + d] : 0.f;
        qk = oc_q(p.beta[ak], p.q_min);
        pk = p.pid[ak];
    }
    const float r2 = p.radius * p.radius;
    // slice of the hits (whole LDS chunks)
    const int64_t n_chunks = (h_hi - h_lo + kOcChunk - 1) / kOcChunk;
    const int64_t per = (n_chunks + gridDim.y - 1) / gridDim.y;
    const int64_t j_begin = h_lo + (int64_t)blockIdx.y * per * kOcChunk;
    const int64_t j_stop = (h_lo + (int64_t)(blockIdx.y + 1) * per * kOcChunk < h_hi) ? h_lo + (int64_t)(blockIdx.y + 1) * per * kOcChunk : h_hi;
    for (int64_t j0 = j_begin; j0 < j_stop; j0 += kOcChunk) {
        __syncthreads();
        for (int i = threadIdx.x; i < kOcChunk; i += kOcTpb) {
            const int64_t j = j0 + i;
            if (j < h_hi) {
#pragma unroll
                for (int d = 0; d < DP; ++d) s_x[i][d] = d < p.dim ? p.x[j * p.stride + d] : 0.f;
                s_q[i] = oc_q(p.beta[j], p.q_min);
                s_pid[i] = p.pid[j];
                const int gj = p.gid[j];
                bool att = gj >= 0;
                if (p.mode == 0) att = att && p.mask[j] != 0 && p.alphas[gj] != (int32_t)j;
                s_att[i] = att ? gj : -2;
                int ci = -1;
                float cd = 0.f;
                if (p.cap_nbr) {
                    ci = p.cap_nbr[j];
                    if (ci >= 0) {
                        float xa[DP];
#pragma unroll
                        for (int d = 0; d < DP; ++d) xa[d] = s_x[i][d];
                        float xc[DP];
#pragma unroll
                        for (int d = 0; d < DP; ++d) xc[d] = d < p.dim ? p.x[(int64_t)ci * p.stride + d] : 0.f;
                        cd = oc_d2_chain<DP>(xa, xc);
                    }
                }
                s_cap[i] = ci;
                s_capd2[i] = cd;
            }
        }
        __syncthreads();
        if (!live) continue;
        const int jn = (int)((h_hi - j0 < kOcChunk) ? (h_hi - j0) : kOcChunk);
        for (int i = 0; i < jn; ++i) {
            float t[DP];
            float d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                t[d] = s_x[i][d] - xk[d];  // x_j - x_k
                d2 += t[d] * t[d];
            }
            float cx = 0.f, cq = 0.f;  // d/dx_k = -cx * t ; d/dq_k = cq
            if (s_pid[i] == pk) {
                if (s_att[i] == k) {
                    cx = ca * 2.f * s_q[i] * qk;
                    cq = ca * s_q[i] * d2;
                }
            } else if (d2 < r2 && oc_keep_pair(p, j0 + i, k) &&
                       (s_cap[i] < 0 || oc_cap_ok(oc_d2_chain<DP>(s_x[i], xk), ak, s_capd2[i], s_cap[i]))) {
                const float sd = sqrtf(p.eps_sqrt + d2);
                cx = sd > 0.f ? -cr * s_q[i] * qk / sd : 0.f;
                cq = cr * s_q[i] * (p.radius - sd);
            }
#pragma unroll
            for (int d = 0; d < DP; ++d) gxk[d] -= cx * t[d];
            gqk += cq;
        }
    }
    if (live) {
        float *o = part + ((int64_t)blockIdx.y * part_rows + kl) * (DP + 1);
#pragma unroll
        for (int d = 0; d < DP; ++d) o[d] = gxk[d];
        o[DP] = gqk;
    }
}

template <int DP, bool BATCH>
__global__ __launch_bounds__(kOcTpb) void oc_backward_cps_reduce_kernel(const OcParams p,
                                                                        const float *__restrict__ g,
                                                                        const float *__restrict__ fwd,
                                                                        int k_base, int n_slices,
                                                                        const float *__restrict__ part,
                                                                        float *__restrict__ gx,
                                                                        float *__restrict__ gbeta) {
    const int K = p.n_cp[0];
    const int kl = blockIdx.x * kOcTpb + threadIdx.x, k = k_base + kl;
    if (k >= K) return;
    const int64_t part_rows = BATCH ? p.n : kOcCpBatch;
    if constexpr (BATCH) fwd += oc_event_of(p.cp_ptr, p.n_seg, k) * 9;
    float acc[DP + 1];
#pragma unroll
    for (int d = 0; d <= DP; ++d) acc[d] = 0.f;
    for (int sl = 0; sl < n_slices; ++sl) {  // fixed order: bit-reproducible
        const float *o = part + ((int64_t)sl * part_rows + kl) * (DP + 1);
#pragma unroll
        for (int d = 0; d <= DP; ++d) acc[d] += o[d];
    }
    const int32_t ak = p.alphas[k];
#pragma unroll
    for (int d = 0; d < DP; ++d)   // (unrolled: acc stays in registers)
        if (d < p.dim) gx[(int64_t)ak * p.stride + d] += acc[d];
    const float bk = p.beta[ak];
    const float a = atanhf(bk);
    gbeta[ak] += acc[DP] * 2.f * a / (1.f - bk * bk) - g[2] / fwd[6];  // coward: mean(1 - beta)
}

// ---- the same sums without the N x K walk ("spatial" passes) ----------------------------------
// A repulsive pair needs |x_j - x_k| < radius, so almost all of the N x K pairs of a large event
// contribute exactly nothing.  The hits are sorted by Morton code into chunks of 64 with bounding
// boxes (knn.hip: spatial_chunks_build); a (chunk, condensation point) pair is only looked at if
// the box is closer to the point than the radius (lower bound sum_d max(lo_d - c_d, c_d - hi_d, 0)^2
// against radius^2 with a 1e-5 relative margin - far above the rounding of either side; the
// exact test d2 < radius^2 then runs unchanged).  The attractive term has no radius, but it is a
// sum over (hit, its own condensation point) only: it is taken outside the pair loops.
//   hit pass  (forward and backward): wave = chunk of 64 sorted hits (lane = hit), the K points
//             are tested 64 at a time (lane = point) and the survivors walked through LDS;
//   point pass (backward): wave = condensation point, the chunk boxes are tested 64 at a time
//             (lane = chunk), the surviving chunks streamed (lane = hit), its own particle's hits
//             come from a by-gid ordering; one fixed-order wave reduction, no partial buffers.
// Same pairs, same per-pair arithmetic as the dense kernels above; only the order of the
// (exactly representable) zero contributions that are skipped differs.
struct OcSpatial {
    const float *xs;       // [rows][DP] sorted hits
    const int32_t *sidx;   // [rows] original hit index, -1 in the tail
    const float *box;      // [n_chunks][2 DP]
    const float *hq;       // [rows] q of the sorted hit
    const long long *hpid; // [rows]
    const int32_t *hcap;   // [rows] neighbour cap of the sorted hit (-1: none) ...
    const float *hcapd2;   // ... and its distance
    const float *cx;       // [K][DP] condensation points
    const float *cq;       // [K]
    const long long *cpid; // [K]
    const uint32_t *gorder;   // hits ordered by gid (point pass)
    const uint32_t *gkeys;    // the sorted gid keys
    const int32_t *gstart;    // [K] first position of gid k in gorder
    int n_chunks;
};

template <int DP>
__global__ __launch_bounds__(kOcTpb) void oc_hit_records_kernel(const OcParams p, OcSpatial sp, float *__restrict__ hq,
                                                                long long *__restrict__ hpid,
                                                                int32_t *__restrict__ hcap,
                                                                float *__restrict__ hcapd2) {
    const int64_t r = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (r >= (int64_t)sp.n_chunks * 64) return;
    const int32_t j = sp.sidx[r];
    float q = 0.f, cd = 0.f;
    long long pid = -1;
    int32_t ci = -1;
    if (j >= 0) {
        q = oc_q(p.beta[j], p.q_min);
        pid = p.pid[j];
        if (p.cap_nbr) {
            ci = p.cap_nbr[j];
            if (ci >= 0) {
                float xa[DP], xc[DP];
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    xa[d] = sp.xs[r * DP + d];
                    xc[d] = d < p.dim ? p.x[(int64_t)ci * p.stride + d] : 0.f;
                }
                cd = oc_d2_chain<DP>(xa, xc);
            }
        }
    }
    hq[r] = q;
    hpid[r] = pid;
    hcap[r] = ci;
    hcapd2[r] = cd;
}

template <int DP>
__global__ __launch_bounds__(kOcTpb) void oc_cp_records_kernel(const OcParams p, float *__restrict__ cx,
                                                               float *__restrict__ cq, long long *__restrict__ cpid) {
    const int K = p.n_cp[0];
    const int k = blockIdx.x * kOcTpb + threadIdx.x;
    if (k >= K) return;
    const int32_t a = p.alphas[k];
#pragma unroll
    for (int d = 0; d < DP; ++d) cx[(int64_t)k * DP + d] = d < p.dim ? p.x[(int64_t)a * p.stride + d] : 0.f;
    cq[k] = oc_q(p.beta[a], p.q_min);
    cpid[k] = p.pid[a];
}

// hit pass: workgroup = chunk of 64 sorted hits, its four waves take every fourth round of 64
// condensation points (the rounds are latency bound: more of them in flight) and their per-hit
// sums are added in wave order through LDS.  BWD = false: part[chunk][8] = {attractive, repulsive,
// n_rep_pairs, sum of beta over noise hits, noise hits, hits of interest, 0, 0}
// (oc_finalize_spatial_kernel adds the chunks); BWD = true: gx[j], gbeta[j] of every hit (the point
// pass adds the condensation points' share)
constexpr int kOcHitWaves = kOcTpb / 64;
template <int DP, bool BWD>
__global__ __launch_bounds__(kOcTpb) void oc_hits_spatial_kernel(const OcParams p, const OcSpatial sp,
                                                                 const float *__restrict__ g,
                                                                 const float *__restrict__ fwd,
                                                                 double *__restrict__ part, float *__restrict__ gx,
                                                                 float *__restrict__ gbeta) {
    __shared__ float s_x[kOcHitWaves][64][DP];
    __shared__ float s_q[kOcHitWaves][64];
    __shared__ long long s_pid[kOcHitWaves][64];
    __shared__ int s_hit[kOcHitWaves][64];
    __shared__ double s_accd[kOcHitWaves][2][64];     // forward: repulsive, pair count
    __shared__ float s_accf[kOcHitWaves][DP + 1][64];  // backward: d/dx, d/dq
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x;
    const int K = p.n_cp[0];
    const int64_t r = (int64_t)c * 64 + lane;
    const int32_t jj = sp.sidx[r];
    const bool live = jj >= 0;
    const int64_t j = live ? jj : 0;
    float xj[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) xj[d] = sp.xs[r * DP + d];
    const float qj = sp.hq[r];
    const long long pj = sp.hpid[r];
    const int cap_idx = sp.hcap[r];
    const float cap_d2 = sp.hcapd2[r];
    float blo[DP], bhi[DP];  // the chunk's box (wave-uniform)
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        blo[d] = sp.box[(int64_t)c * 2 * DP + d];
        bhi[d] = sp.box[(int64_t)c * 2 * DP + DP + d];
    }
    const float r2 = p.radius * p.radius;
    const float r2m = r2 * 1.00001f + 1e-30f;
    float ca = 0.f, cr = 0.f;
    if (BWD) {
        ca = g[0] / fwd[4];
        cr = g[1] / fwd[5];
    }
    double vr = 0.0, nrep = 0.0;
    float gxj[DP];
    float gqj = 0.f;
#pragma unroll
    for (int d = 0; d < DP; ++d) gxj[d] = 0.f;

    // lane = condensation point: distance bound to the chunk's box; the next round's coordinates
    // are in flight while the survivors of this one are walked
    auto load_cp = [&](int k0, float (&ck)[DP]) {
        const int k = k0 + lane;
        const int kc = k < K ? k : K - 1;
#pragma unroll
        for (int d = 0; d < DP; ++d) ck[d] = sp.cx[(int64_t)kc * DP + d];
    };
    float ck[DP], cn[DP];
    load_cp(wv * 64, ck);
    for (int k0 = wv * 64; k0 < K; k0 += kOcHitWaves * 64) {
        load_cp(k0 + kOcHitWaves * 64 < K ? k0 + kOcHitWaves * 64 : k0, cn);
        const int k = k0 + lane;
        const int kc = k < K ? k : K - 1;
        float lb = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const float gd = fmaxf(fmaxf(blo[d] - ck[d], ck[d] - bhi[d]), 0.f);
            lb += gd * gd;
        }
        unsigned long long near = __ballot(k < K && lb <= r2m);
        if (near != 0ull) {
            wave_sync();  // (the previous round's readers are done)
#pragma unroll
            for (int d = 0; d < DP; ++d) s_x[wv][lane][d] = ck[d];
            s_q[wv][lane] = sp.cq[kc];
            s_pid[wv][lane] = sp.cpid[kc];
            s_hit[wv][lane] = p.alphas[kc];
            wave_sync();
            while (near != 0ull) {
                const int i = __ffsll(near) - 1;
                near &= near - 1ull;
                float t[DP];
                float d2 = 0.f;
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    t[d] = xj[d] - s_x[wv][i][d];
                    d2 += t[d] * t[d];
                }
                if (live && s_pid[wv][i] != pj && d2 < r2 &&
                    (cap_idx < 0 || oc_cap_ok(oc_d2_chain<DP>(xj, s_x[wv][i]), s_hit[wv][i], cap_d2, cap_idx))) {
                    const float qk = s_q[wv][i];
                    if (!BWD) {
                        nrep += 1.0;  // (counted before the sub-sampling, as the reference's n_rep)
                        if (oc_keep_pair(p, j, k0 + i)) vr += (double)(qj * qk * (p.radius - sqrtf(p.eps_sqrt + d2)));
                    } else if (oc_keep_pair(p, j, k0 + i)) {
                        const float sd = sqrtf(p.eps_sqrt + d2);
                        const float cxr = sd > 0.f ? -cr * qj * qk / sd : 0.f;
#pragma unroll
                        for (int d = 0; d < DP; ++d) gxj[d] += cxr * t[d];
                        gqj += cr * qk * (p.radius - sd);
                    }
                }
            }
        }
#pragma unroll
        for (int d = 0; d < DP; ++d) ck[d] = cn[d];
    }
    if (!BWD) {
        s_accd[wv][0][lane] = vr;
        s_accd[wv][1][lane] = nrep;
    } else {
#pragma unroll
        for (int d = 0; d < DP; ++d) s_accf[wv][d][lane] = gxj[d];
        s_accf[wv][DP][lane] = gqj;
    }
    __syncthreads();
    if (wv != 0) return;
    if (!BWD) {
        vr = ((s_accd[0][0][lane] + s_accd[1][0][lane]) + s_accd[2][0][lane]) + s_accd[3][0][lane];
        nrep = ((s_accd[0][1][lane] + s_accd[1][1][lane]) + s_accd[2][1][lane]) + s_accd[3][1][lane];
    } else {
#pragma unroll
        for (int d = 0; d < DP; ++d)
            gxj[d] = ((s_accf[0][d][lane] + s_accf[1][d][lane]) + s_accf[2][d][lane]) + s_accf[3][d][lane];
        gqj = ((s_accf[0][DP][lane] + s_accf[1][DP][lane]) + s_accf[2][DP][lane]) + s_accf[3][DP][lane];
    }
    int gj = -1;
    bool mj = false, is_cp = false;
    float bj = 0.5f;
    if (live) {
        gj = p.gid[j];
        mj = p.mask[j] != 0;
        is_cp = gj >= 0 && p.alphas[gj] == jj;
        bj = p.beta[j];
    }
    // attractive: the hit and the condensation point of its own particle, at any distance
    double va = 0.0;
    const bool att = live && gj >= 0 && ((p.mode == 1) ? true : (mj && !is_cp));
    if (att) {
        float t[DP];
        float d2 = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            t[d] = xj[d] - sp.cx[(int64_t)gj * DP + d];
            d2 += t[d] * t[d];
        }
        const float qk = sp.cq[gj];
        if (!BWD) {
            va += (double)(qj * qk * d2);
        } else {
            const float cxa = ca * 2.f * qj * qk;
#pragma unroll
            for (int d = 0; d < DP; ++d) gxj[d] += cxa * t[d];
            gqj += ca * qk * d2;
        }
    }
    const bool is_noise = live && ((p.mode == 1) ? !(pj > 0) : (pj == 0));
    if (!BWD) {
        const double a = wave_sum(va), rr = wave_sum(vr), cc = wave_sum(nrep);
        const double ns = wave_sum(is_noise ? (double)bj : 0.0), nn = wave_sum(is_noise ? 1.0 : 0.0),
                     no = wave_sum(mj ? 1.0 : 0.0);
        if (lane == 0) {
            double *o = part + (int64_t)c * 8;
            o[0] = a; o[1] = rr; o[2] = cc; o[3] = ns; o[4] = nn; o[5] = no; o[6] = 0.0; o[7] = 0.0;
        }
    } else if (live) {
        for (int d = 0; d < p.dim; ++d) gx[j * p.stride + d] = gxj[d];
        const float a = atanhf(bj);
        float gb = gqj * 2.f * a / (1.f - bj * bj);
        if (is_noise) gb += g[3] / fwd[8];
        gbeta[j] = gb;
    }
}

// the chunks' partial sums -> out[0..8] (as oc_finalize_kernel, without its walk over all hits)
__global__ __launch_bounds__(kOcTpb) void oc_finalize_spatial_kernel(const OcParams p, const double *__restrict__ part,
                                                                     int n_part, float *__restrict__ out) {
    __shared__ double s_red[kOcTpb / 64];
    const int K = p.n_cp[0];
    double v[6] = {0, 0, 0, 0, 0, 0}, cow = 0;
    for (int i = threadIdx.x; i < n_part; i += kOcTpb)
#pragma unroll
        for (int u = 0; u < 6; ++u) v[u] += part[(int64_t)i * 8 + u];
    for (int k = threadIdx.x; k < K; k += kOcTpb) cow += (double)(1.f - p.beta[p.alphas[k]]);
#pragma unroll
    for (int u = 0; u < 6; ++u) v[u] = oc_block_sum(v[u], s_red);
    cow = oc_block_sum(cow, s_red);
    if (threadIdx.x == 0) {
        const double eps = 1e-9;
        const double norm_att = eps + v[5] - (double)K;
        double norm_rep = eps + ((double)K - 1.0) * (double)p.n;
        if (p.keep < 1.f) norm_rep *= (double)p.keep;  // oc.py:328
        out[0] = (float)(v[0] / norm_att);
        out[1] = (float)(v[1] / norm_rep);
        out[2] = (float)(cow / (double)K);
        out[3] = (float)(v[3] / v[4]);
        out[4] = (float)norm_att;
        out[5] = (float)norm_rep;
        out[6] = (float)K;
        out[7] = (float)v[2];
        out[8] = (float)v[4];
    }
}

// gstart[k] = first position of gid k in the by-gid ordering (every k < K owns at least its
// condensation point)
__global__ __launch_bounds__(kOcTpb) void oc_gid_keys_kernel(const int32_t *__restrict__ gid, int64_t n,
                                                             uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (i < n) {
        keys[i] = (uint32_t)gid[i];  // -1 -> 0xffffffff: hits of no particle of interest sort last
        vals[i] = (uint32_t)i;
    }
}
__global__ __launch_bounds__(kOcTpb) void oc_gid_starts_kernel(const uint32_t *__restrict__ keys, int64_t n,
                                                               int32_t *__restrict__ gstart) {
    const int64_t s = (int64_t)blockIdx.x * kOcTpb + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = keys[s];
    if (key != 0xffffffffu && (s == 0 || keys[s - 1] != key)) gstart[key] = (int32_t)s;
}

// point pass (backward): workgroup = condensation point k; its four waves take every fourth batch of
// 64 chunk boxes, wave 0 also the particle's own hits; fixed-order reductions (lanes, then waves)
template <int DP>
__global__ __launch_bounds__(kOcTpb) void oc_cps_spatial_kernel(const OcParams p, const OcSpatial sp,
                                                                const float *__restrict__ g,
                                                                const float *__restrict__ fwd,
                                                                float *__restrict__ gx, float *__restrict__ gbeta) {
    __shared__ float s_acc[kOcHitWaves][DP + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int K = p.n_cp[0];
    const int k = blockIdx.x;
    if (k >= K) return;  // (workgroup-uniform)
    const float ca = g[0] / fwd[4], cr = g[1] / fwd[5];
    const int32_t ak = p.alphas[k];
    float xk[DP], gxk[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        xk[d] = sp.cx[(int64_t)k * DP + d];
        gxk[d] = 0.f;
    }
    const float qk = sp.cq[k];
    const long long pk = sp.cpid[k];
    float gqk = 0.f;
    const float r2 = p.radius * p.radius;
    const float r2m = r2 * 1.00001f + 1e-30f;
    // repulsive: the chunks whose box reaches into the point's radius
    for (int c0 = wv * 64; c0 < sp.n_chunks; c0 += kOcHitWaves * 64) {
        const int c = c0 + lane;
        const int cc = c < sp.n_chunks ? c : sp.n_chunks - 1;
        float lb = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const float lo = sp.box[(int64_t)cc * 2 * DP + d], hi = sp.box[(int64_t)cc * 2 * DP + DP + d];
            const float gd = fmaxf(fmaxf(lo - xk[d], xk[d] - hi), 0.f);
            lb += gd * gd;
        }
        unsigned long long near = __ballot(c < sp.n_chunks && lb <= r2m);
        if (near == 0ull) continue;
        // the next surviving chunk's rows are in flight while this one is evaluated
        float xa[DP], xn[DP];
        int32_t jj, jn;
        long long pj, pn;
        float qj, qn;
        auto load_rows = [&](int i, float (&x)[DP], int32_t &id, long long &pid, float &q) {
            const int64_t r = (int64_t)(c0 + i) * 64 + lane;
#pragma unroll
            for (int d = 0; d < DP; ++d) x[d] = sp.xs[r * DP + d];
            id = sp.sidx[r];
            pid = sp.hpid[r];
            q = sp.hq[r];
        };
        int i = __ffsll(near) - 1;
        load_rows(i, xa, jj, pj, qj);
        while (near != 0ull) {
            near &= near - 1ull;
            const int in = near != 0ull ? __ffsll(near) - 1 : i;
            load_rows(in, xn, jn, pn, qn);
            const int64_t r = (int64_t)(c0 + i) * 64 + lane;
            float t[DP];
            float d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                t[d] = xa[d] - xk[d];  // x_j - x_k
                d2 += t[d] * t[d];
            }
            if (jj >= 0 && pj != pk && d2 < r2 && oc_keep_pair(p, jj, k)) {
                const int ci = sp.hcap[r];
                if (ci < 0 || oc_cap_ok(oc_d2_chain<DP>(xa, xk), ak, sp.hcapd2[r], ci)) {
                    const float sd = sqrtf(p.eps_sqrt + d2);
                    const float cxr = sd > 0.f ? -cr * qj * qk / sd : 0.f;
#pragma unroll
                    for (int d = 0; d < DP; ++d) gxk[d] -= cxr * t[d];
                    gqk += cr * qj * (p.radius - sd);
                }
            }
#pragma unroll
            for (int d = 0; d < DP; ++d) xa[d] = xn[d];
            jj = jn;
            pj = pn;
            qj = qn;
            i = in;
        }
    }
    // attractive: the hits of particle k (by-gid ordering), at any distance
    if (wv == 0) {
        for (int64_t s = sp.gstart[k];; s += 64) {
            const int64_t t0 = s + lane;
            const bool mine = t0 < p.n && sp.gkeys[t0 < p.n ? t0 : p.n - 1] == (uint32_t)k;
            if (mine) {
                const int64_t j = sp.gorder[t0];
                const bool att = (p.mode == 1) ? true : (p.mask[j] != 0 && ak != (int32_t)j);
                if (att) {
                    float t[DP];
                    float d2 = 0.f;
#pragma unroll
                    for (int d = 0; d < DP; ++d) {
                        t[d] = (d < p.dim ? p.x[j * p.stride + d] : 0.f) - xk[d];
                        d2 += t[d] * t[d];
                    }
                    const float qj = oc_q(p.beta[j], p.q_min);
                    const float cxa = ca * 2.f * qj * qk;
#pragma unroll
                    for (int d = 0; d < DP; ++d) gxk[d] -= cxa * t[d];
                    gqk += ca * qj * d2;
                }
            }
            if (__ballot(mine) != ~0ull) break;  // the run of gid k ended inside this step
        }
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) gxk[d] = wave_sum(gxk[d]);
    gqk = wave_sum(gqk);
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < DP; ++d) s_acc[wv][d] = gxk[d];
        s_acc[wv][DP] = gqk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int d = 0; d < p.dim; ++d)
            gx[(int64_t)ak * p.stride + d] += ((s_acc[0][d] + s_acc[1][d]) + s_acc[2][d]) + s_acc[3][d];
        const float gq = ((s_acc[0][DP] + s_acc[1][DP]) + s_acc[2][DP]) + s_acc[3][DP];
        const float bk = p.beta[ak];
        const float a = atanhf(bk);
        gbeta[ak] += gq * 2.f * a / (1.f - bk * bk) - g[2] / fwd[6];  // coward: mean(1 - beta)
    }
}

// ---- host side: workspaces, checks; the C entries launch -----------------------------------
struct SelectWs {
    u64 *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    int32_t *flag, *best;
    int64_t *off;   // [n + 1]
    char *temp;
    size_t temp_bytes, total;
    uint32_t *ekeys_a, *ekeys_b, *epos_a, *epos_b;  // a batch: the second sort, by event
    char *etemp;
    size_t etemp_bytes;
};
static SelectWs select_ws(void *base, int64_t n, bool batched = false) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    SelectWs w{};
    Carver ws{(char *)base};
    w.keys_a = ws.take<u64>(nn);
    w.keys_b = ws.take<u64>(nn);
    w.vals_a = ws.take<uint32_t>(nn);
    w.vals_b = ws.take<uint32_t>(nn);
    w.flag = ws.take<int32_t>(nn);
    w.best = ws.take<int32_t>(nn);
    w.off = ws.take<int64_t>((size_t)(n + 1));
    w.temp_bytes = sort_pairs_u64_temp_bytes(n);
    w.temp = ws.take<char>(w.temp_bytes);
    if (batched) {
        w.ekeys_a = ws.take<uint32_t>(nn);
        w.ekeys_b = ws.take<uint32_t>(nn);
        w.epos_a = ws.take<uint32_t>(nn);
        w.epos_b = ws.take<uint32_t>(nn);
        w.etemp_bytes = sort_pairs_temp_bytes(n);
        w.etemp = ws.take<char>(w.etemp_bytes);
    }
    w.total = ws.off;
    return w;
}
static int oc_check(const gnntrk_oc_args *a) {
    if (!a || !a->x || !a->beta || !a->particle_id || !a->mask || !a->gid || !a->alphas || !a->n_cp)
        return fail(GNNTRK_EINVAL, "oc_potential: NULL pointer");
    if (a->n < 1 || a->dim < 1 || a->dim > kOcMaxDim || a->stride < a->dim)
        return fail(GNNTRK_EINVAL, "oc_potential: bad sizes (1 <= dim <= 32)");
    if (a->mode != 0 && a->mode != 1) return fail(GNNTRK_EINVAL, "oc_potential: mode must be 0 or 1");
    return GNNTRK_OK;
}

static OcParams oc_params(const gnntrk_oc_args *a) {
    OcParams p;
    p.x = a->x; p.beta = a->beta; p.pid = a->particle_id; p.mask = a->mask; p.gid = a->gid;
    p.alphas = a->alphas; p.n_cp = a->n_cp; p.n = a->n; p.dim = a->dim; p.stride = a->stride;
    p.q_min = a->q_min; p.radius = a->radius; p.eps_sqrt = a->eps_sqrt; p.mode = a->mode;
    p.keep = a->rep_keep_prob > 0.f ? a->rep_keep_prob : 1.f;   // (0 = field left unset: all pairs)
    p.seed = a->rep_seed;
    p.cap_nbr = a->cap_nbr;
    p.seg_ptr = nullptr; p.cp_ptr = nullptr; p.n_seg = 0;
    return p;
}

// ---- spatial passes: workspace layout and launchers ------------------------------------------
// the chunks, the view `sp` the kernels read, and the arrays of it that the launchers fill
struct OcSpatialWs {
    SpatialChunks c;
    OcSpatial sp;
    float *hq, *hcapd2, *cx, *cq;
    long long *hpid, *cpid;
    int32_t *hcap, *gstart;
    double *part;   // [n_chunks][8] of the forward
    uint32_t *gkeys_a, *gkeys_b, *gvals_a, *gvals_b;
    char *gtemp;
    size_t gtemp_bytes, total;
};
static OcSpatialWs oc_spatial_ws(void *base, int64_t n, int dim) {
    OcSpatialWs w{};
    Carver ws{(char *)base};
    w.c = take_chunks(ws, n, dim);
    const size_t rows = (size_t)w.c.n_chunks * 64, N = (size_t)n;
    w.hq = ws.take<float>(rows);
    w.hpid = ws.take<long long>(rows);
    w.hcap = ws.take<int32_t>(rows);
    w.hcapd2 = ws.take<float>(rows);
    w.cx = ws.take<float>(N * w.c.dp);
    w.cq = ws.take<float>(N);
    w.cpid = ws.take<long long>(N);
    w.part = ws.take<double>((size_t)w.c.n_chunks * 8);
    w.gkeys_a = ws.take<uint32_t>(N);
    w.gkeys_b = ws.take<uint32_t>(N);
    w.gvals_a = ws.take<uint32_t>(N);
    w.gvals_b = ws.take<uint32_t>(N);
    w.gstart = ws.take<int32_t>(N);
    w.gtemp_bytes = sort_pairs_temp_bytes(n);
    w.gtemp = ws.take<char>(w.gtemp_bytes);
    take_chunks_scratch(ws, w.c, n);
    w.total = ws.off;
    w.sp = OcSpatial{w.c.xs, w.c.sidx, w.c.box, w.hq, w.hpid, w.hcap, w.hcapd2, w.cx, w.cq, w.cpid,
                     w.gvals_b /* gorder */, w.gkeys_b /* gkeys */, w.gstart, w.c.n_chunks};
    return w;
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

int gnntrk_good_node_mask(const float *pt, const int64_t *particle_id, const float *reconstructable, const float *eta,
                          int64_t n, float pt_thld, float max_eta, uint8_t *mask, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0) return fail(GNNTRK_EINVAL, "good_node_mask: bad argument");
    if (n == 0) return GNNTRK_OK;
    if (!pt || !particle_id || !reconstructable || !eta || !mask)
        return fail(GNNTRK_EINVAL, "good_node_mask: NULL pointer");
    hipLaunchKernelGGL(good_node_mask_kernel, dim3(oc_grid(n)), dim3(kOcTpb), 0, stream, pt, particle_id,
                       reconstructable, eta, n, pt_thld, max_eta, mask);
    return check_launch("good_node_mask");
}

size_t gnntrk_oc_select_workspace_bytes(int64_t n) { return select_ws(nullptr, n).total; }

// seg_ptr != NULL: the selection of a batch
static int oc_select(const float *score, const int64_t *particle_id, const uint8_t *mask, int64_t n, int32_t mode,
                     const int64_t *seg_ptr, int32_t n_seg, int32_t *alphas, int32_t *gid, int32_t *cp_ptr, int32_t *n_cp,
                     void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!score || !particle_id || !mask || !alphas || !gid || !n_cp || n < 1 || (mode != 0 && mode != 1))
        return fail(GNNTRK_EINVAL, "oc_select_cps: bad argument");
    if (n > 0x7fffffff) return fail(GNNTRK_EUNSUPPORTED, "oc_select_cps: n must fit int32");
    const SelectWs w = select_ws(workspace, n, seg_ptr != nullptr);
    if (!workspace || workspace_bytes < w.total) return fail(GNNTRK_EINVAL, "oc_select_cps: workspace too small");
    const int grid = oc_grid(n);
    hipLaunchKernelGGL(oc_keys_kernel, dim3(grid), dim3(kOcTpb), 0, stream, particle_id, n, w.keys_a, w.vals_a);
    int rc = sort_pairs_u64(w.keys_a, w.keys_b, w.vals_a, w.vals_b, n, w.temp, w.temp_bytes, stream);
    if (rc) return rc;
    const u64 *keys = w.keys_b;
    const uint32_t *order = w.vals_b;
    if (seg_ptr) {
        int bits = 1;
        while (bits < 31 && (1 << bits) < n_seg) ++bits;
        hipLaunchKernelGGL(oc_event_keys_kernel, dim3(grid), dim3(kOcTpb), 0, stream, order, seg_ptr, n_seg, n, w.ekeys_a,
                           w.epos_a);
        rc = sort_pairs_u32(w.ekeys_a, w.ekeys_b, w.epos_a, w.epos_b, n, bits, w.etemp, w.etemp_bytes, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(oc_event_gather_kernel, dim3(grid), dim3(kOcTpb), 0, stream, keys, order,
                           (const uint32_t *)w.epos_b, n, w.keys_a, w.vals_a);
        keys = w.keys_a;
        order = w.vals_a;
    }
    hipLaunchKernelGGL(oc_segment_best_kernel, dim3(grid), dim3(kOcTpb), 0, stream, keys, order, score, mask, n, mode,
                       seg_ptr, n_seg, w.flag, w.best);
    scan_counts_launch(w.flag, 0x7fffffff, n, w.off, stream);
    rc = check_hip(hipMemsetAsync(gid, 0xff, (size_t)n * sizeof(int32_t), stream), "oc_select_cps(memset)");
    if (rc) return rc;
    hipLaunchKernelGGL(oc_assign_kernel, dim3(grid), dim3(kOcTpb), 0, stream, keys, order, (const int32_t *)w.flag,
                       (const int32_t *)w.best, (const int64_t *)w.off, n, seg_ptr, n_seg, alphas, gid, cp_ptr, n_cp);
    return check_launch("oc_select_cps");
}

int gnntrk_oc_select_cps(const float *score, const int64_t *particle_id, const uint8_t *mask, int64_t n, int32_t mode,
                         int32_t *alphas, int32_t *gid, int32_t *n_cp, void *workspace, size_t workspace_bytes,
                         void *stream_) {
    return oc_select(score, particle_id, mask, n, mode, nullptr, 0, alphas, gid, nullptr, n_cp, workspace, workspace_bytes,
                     (hipStream_t)stream_);
}

size_t gnntrk_oc_select_batched_workspace_bytes(int64_t n) { return select_ws(nullptr, n, true).total; }

int gnntrk_oc_select_cps_batched(const float *score, const int64_t *particle_id, const uint8_t *mask, int64_t n,
                                 int32_t mode, const int64_t *seg_ptr, int32_t n_seg, int32_t *alphas, int32_t *gid,
                                 int32_t *cp_ptr, int32_t *n_cp, void *workspace, size_t workspace_bytes, void *stream_) {
    if (!seg_ptr || !cp_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "oc_select_cps_batched: bad argument");
    return oc_select(score, particle_id, mask, n, mode, seg_ptr, n_seg, alphas, gid, cp_ptr, n_cp, workspace,
                     workspace_bytes, (hipStream_t)stream_);
}

size_t gnntrk_oc_forward_workspace_bytes(int64_t n) { return (size_t)oc_grid(n) * 4 * sizeof(double); }

int gnntrk_oc_forward(const gnntrk_oc_args *args, float *out, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = oc_check(args);
    if (rc) return rc;
    if (!out || !workspace || workspace_bytes < gnntrk_oc_forward_workspace_bytes(args->n))
        return fail(GNNTRK_EINVAL, "oc_forward: workspace too small");
    const OcParams p = oc_params(args);
    const int grid = oc_grid(args->n);
    double *part = reinterpret_cast<double *>(workspace);
    dispatch_dp<2, 4, 8, 16, 32>(args->dim, [&](auto DP) {
        hipLaunchKernelGGL((oc_forward_kernel<decltype(DP)::value, false>), dim3(grid), dim3(kOcTpb), 0, stream, p, part);
    });
    hipLaunchKernelGGL(oc_finalize_kernel<false>, dim3(1), dim3(kOcTpb), 0, stream, p, (const double *)part, grid, out);
    return check_launch("oc_forward");
}

// ---- a batch of events: the same launches, a block = a tile of ONE event (oc_block_tile) ------
static int oc_batch_params(const gnntrk_oc_args *args, const int64_t *seg_ptr, const int32_t *cp_ptr, int32_t n_seg,
                           OcParams &p) {
    int rc = oc_check(args);
    if (rc) return rc;
    if (!seg_ptr || !cp_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "oc_potential (batched): seg_ptr, cp_ptr, n_seg >= 1");
    if (args->rep_keep_prob > 0.f && args->rep_keep_prob < 1.f)
        return fail(GNNTRK_EUNSUPPORTED, "oc_potential (batched): rep_keep_prob is per event; not supported in a batch");
    p = oc_params(args);
    p.seg_ptr = seg_ptr; p.cp_ptr = cp_ptr; p.n_seg = n_seg;
    return GNNTRK_OK;
}
static int oc_batch_grid(int64_t n, int32_t n_seg) { return (int)(ceil_div(n, kOcTpb) + n_seg); }

size_t gnntrk_oc_forward_batched_workspace_bytes(int64_t n, int32_t n_seg) {
    return (size_t)oc_batch_grid(n, n_seg) * 4 * sizeof(double);
}

int gnntrk_oc_forward_batched(const gnntrk_oc_args *args, const int64_t *seg_ptr, const int32_t *cp_ptr, int32_t n_seg,
                              float *out, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    OcParams p;
    int rc = oc_batch_params(args, seg_ptr, cp_ptr, n_seg, p);
    if (rc) return rc;
    if (!out || !workspace || workspace_bytes < gnntrk_oc_forward_batched_workspace_bytes(args->n, n_seg))
        return fail(GNNTRK_EINVAL, "oc_forward_batched: workspace too small");
    const int grid = oc_batch_grid(args->n, n_seg);
    double *part = reinterpret_cast<double *>(workspace);
    dispatch_dp<2, 4, 8, 16, 32>(args->dim, [&](auto DP) {
        hipLaunchKernelGGL((oc_forward_kernel<decltype(DP)::value, true>), dim3(grid), dim3(kOcTpb), 0, stream, p, part);
    });
    hipLaunchKernelGGL(oc_finalize_kernel<true>, dim3(n_seg), dim3(kOcTpb), 0, stream, p, (const double *)part, 0, out);
    return check_launch("oc_forward_batched");
}

// partial buffer of the point pass: [kOcBatchSlices][n][dim padded + 1] floats
size_t gnntrk_oc_backward_batched_workspace_bytes(int64_t n, int32_t dim) {
    const int dp = dim <= 2 ? 2 : dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : 32;
    return (size_t)kOcBatchSlices * (size_t)(n > 0 ? n : 1) * (dp + 1) * sizeof(float);
}

int gnntrk_oc_backward_batched(const gnntrk_oc_args *args, const int64_t *seg_ptr, const int32_t *cp_ptr, int32_t n_seg,
                               const float *g, const float *fwd, float *gx, float *gbeta, void *workspace,
                               size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    OcParams p;
    int rc = oc_batch_params(args, seg_ptr, cp_ptr, n_seg, p);
    if (rc) return rc;
    if (!g || !fwd || !gx || !gbeta) return fail(GNNTRK_EINVAL, "oc_backward_batched: bad argument");
    if (!workspace || workspace_bytes < gnntrk_oc_backward_batched_workspace_bytes(args->n, args->dim))
        return fail(GNNTRK_EINVAL, "oc_backward_batched: workspace too small");
    // (at most n points in all: the tile bound of the hits holds for the points, cp_ptr in place of seg_ptr)
    const int grid = oc_batch_grid(args->n, n_seg);
    float *part = reinterpret_cast<float *>(workspace);
    dispatch_dp<2, 4, 8, 16, 32>(args->dim, [&](auto DP) {
        constexpr int dp = decltype(DP)::value;
        hipLaunchKernelGGL((oc_backward_hits_kernel<dp, true>), dim3(grid), dim3(kOcTpb), 0, stream, p, g, fwd, gx, gbeta);
        hipLaunchKernelGGL((oc_backward_cps_kernel<dp, true>), dim3(grid, kOcBatchSlices), dim3(kOcTpb), 0, stream, p, g,
                           fwd, 0, part);
        hipLaunchKernelGGL((oc_backward_cps_reduce_kernel<dp, true>), dim3(oc_grid(args->n)), dim3(kOcTpb), 0, stream, p, g,
                           fwd, 0, (int)kOcBatchSlices, (const float *)part, gx, gbeta);
    });
    return check_launch("oc_backward_batched");
}

// partial buffer of the condensation-point pass: [slices][kOcCpBatch][dim padded + 1] floats
size_t gnntrk_oc_backward_workspace_bytes(int64_t n, int32_t dim) {
    (void)n;
    const int dp = dim <= 2 ? 2 : dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : 32;
    return (size_t)kOcSlices * kOcCpBatch * (dp + 1) * sizeof(float);
}

int gnntrk_oc_backward(const gnntrk_oc_args *args, const float *g, const float *fwd, float *gx, float *gbeta,
                       int64_t max_cps, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = oc_check(args);
    if (rc) return rc;
    if (!g || !fwd || !gx || !gbeta || max_cps < 1) return fail(GNNTRK_EINVAL, "oc_backward: bad argument");
    if (!workspace || workspace_bytes < gnntrk_oc_backward_workspace_bytes(args->n, args->dim))
        return fail(GNNTRK_EINVAL, "oc_backward: workspace too small");
    const OcParams p = oc_params(args);
    const int grid = oc_grid(args->n);
    dispatch_dp<2, 4, 8, 16, 32>(args->dim, [&](auto DP) {
        hipLaunchKernelGGL((oc_backward_hits_kernel<decltype(DP)::value, false>), dim3(grid), dim3(kOcTpb), 0, stream, p, g,
                           fwd, gx, gbeta);
    });
    // condensation-point side in batches of kOcCpBatch (the count K lives on the device: batches
    // past it exit at once), each batch cut into hit slices
    int64_t n_chunks = (args->n + kOcChunk - 1) / kOcChunk;
    const int slices = (int)(n_chunks < kOcSlices ? n_chunks : kOcSlices);
    float *part = reinterpret_cast<float *>(workspace);
    for (int64_t kb = 0; kb < max_cps; kb += kOcCpBatch) {
        const int64_t in_batch = (max_cps - kb < kOcCpBatch) ? (max_cps - kb) : kOcCpBatch;
        const int kgrid = oc_grid(in_batch);
        dispatch_dp<2, 4, 8, 16, 32>(args->dim, [&](auto DP) {
            constexpr int dp = decltype(DP)::value;
            hipLaunchKernelGGL((oc_backward_cps_kernel<dp, false>), dim3(kgrid, slices), dim3(kOcTpb), 0, stream, p, g, fwd,
                               (int)kb, part);
            hipLaunchKernelGGL((oc_backward_cps_reduce_kernel<dp, false>), dim3(kgrid), dim3(kOcTpb), 0, stream, p, g, fwd,
                               (int)kb, slices, (const float *)part, gx, gbeta);
        });
    }
    return check_launch("oc_backward");
}

size_t gnntrk_oc_spatial_workspace_bytes(int64_t n, int32_t dim) {
    if (n < 1 || n > 0x7fffffff || dim < 1 || dim > 16) return 0;
    return oc_spatial_ws(nullptr, n, dim).total;
}

int gnntrk_oc_forward_spatial(const gnntrk_oc_args *args, float *out, void *spatial, size_t spatial_bytes,
                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = oc_check(args);
    if (rc) return rc;
    if (args->dim > 16) return fail(GNNTRK_EUNSUPPORTED, "oc_forward_spatial: dim > 16 (use gnntrk_oc_forward)");
    const OcSpatialWs w = oc_spatial_ws(spatial, args->n, args->dim);
    if (!out || !spatial || spatial_bytes < w.total)
        return fail(GNNTRK_EINVAL, "oc_forward_spatial: workspace too small");
    const OcParams p = oc_params(args);
    rc = spatial_chunks_build(args->x, args->n, args->dim, args->stride, nullptr, 0, w.c, stream);
    if (rc) return rc;
    const int rgrid = oc_grid((int64_t)w.c.n_chunks * 64), kgrid = oc_grid(args->n), hgrid = w.c.n_chunks;
    dispatch_dp<4, 8, 16>(args->dim, [&](auto DP) {
        constexpr int dp = decltype(DP)::value;
        hipLaunchKernelGGL(oc_hit_records_kernel<dp>, dim3(rgrid), dim3(kOcTpb), 0, stream, p, w.sp, w.hq, w.hpid, w.hcap,
                           w.hcapd2);
        hipLaunchKernelGGL(oc_cp_records_kernel<dp>, dim3(kgrid), dim3(kOcTpb), 0, stream, p, w.cx, w.cq, w.cpid);
        hipLaunchKernelGGL((oc_hits_spatial_kernel<dp, false>), dim3(hgrid), dim3(kOcTpb), 0, stream, p, w.sp,
                           (const float *)nullptr, (const float *)nullptr, w.part, (float *)nullptr, (float *)nullptr);
    });
    hipLaunchKernelGGL(oc_finalize_spatial_kernel, dim3(1), dim3(kOcTpb), 0, stream, p, (const double *)w.part,
                       w.c.n_chunks, out);
    return check_launch("oc_forward_spatial");
}

int gnntrk_oc_backward_spatial(const gnntrk_oc_args *args, const float *g, const float *fwd, float *gx, float *gbeta,
                               int64_t max_cps, void *spatial, size_t spatial_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = oc_check(args);
    if (rc) return rc;
    if (args->dim > 16) return fail(GNNTRK_EUNSUPPORTED, "oc_backward_spatial: dim > 16 (use gnntrk_oc_backward)");
    if (!g || !fwd || !gx || !gbeta || max_cps < 1) return fail(GNNTRK_EINVAL, "oc_backward_spatial: bad argument");
    const OcSpatialWs w = oc_spatial_ws(spatial, args->n, args->dim);
    if (!spatial || spatial_bytes < w.total) return fail(GNNTRK_EINVAL, "oc_backward_spatial: workspace too small");
    const OcParams p = oc_params(args);
    const int hgrid = w.c.n_chunks, ngrid = oc_grid(args->n);
    // the by-gid ordering of the hits (for the points' attractive share)
    hipLaunchKernelGGL(oc_gid_keys_kernel, dim3(ngrid), dim3(kOcTpb), 0, stream, args->gid, args->n, w.gkeys_a,
                       w.gvals_a);
    rc = sort_pairs_u32(w.gkeys_a, w.gkeys_b, w.gvals_a, w.gvals_b, args->n, 32, w.gtemp, w.gtemp_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(oc_gid_starts_kernel, dim3(ngrid), dim3(kOcTpb), 0, stream, (const uint32_t *)w.gkeys_b, args->n,
                       w.gstart);
    const int cgrid = (int)(max_cps < args->n ? max_cps : args->n);
    dispatch_dp<4, 8, 16>(args->dim, [&](auto DP) {
        constexpr int dp = decltype(DP)::value;
        hipLaunchKernelGGL((oc_hits_spatial_kernel<dp, true>), dim3(hgrid), dim3(kOcTpb), 0, stream, p, w.sp, g, fwd,
                           (double *)nullptr, gx, gbeta);
        hipLaunchKernelGGL(oc_cps_spatial_kernel<dp>, dim3(cgrid), dim3(kOcTpb), 0, stream, p, w.sp, g, fwd, gx, gbeta);
    });
    return check_launch("oc_backward_spatial");
}

}  // extern "C"
