// The EC threshold scan of the track-graph statistics (analysis/edge_classification.py:24-112): for every threshold t of
// an ascending list, the binary-classification counts of the edge scores and, per selected particle, the number of
// segments, the largest segment and the largest number of its hits in one connected component of the graph of the
// edges with w > t.  The graphs are nested (an edge with w > t is in the graph of every smaller threshold), so the
// scan walks the thresholds from the largest to the smallest on two union-find forests (union_find.h) that are never
// reset: every edge is united once per scan, whatever the number of thresholds.
//
//   gnntrk_ec_scan_prepare  (edges)  es_bin_kernel        per edge the graph bin g = #{j : w > t_j} and the BCS bin
//                                                         k = #{j : !(w < t_j)} by a branch-free binary search over an LDS
//                                                         copy of the thresholds; histogram of (event, mask class, label,
//                                                         k) and of g; "is the end of an edge" per hit; bad edges counted
//                           (bins)   es_offsets_kernel    exclusive scan of the g histogram: one workgroup
//                           (edges)  es_scatter_kernel    counting sort: edge ids into order[], bucket by bucket, slots
//                                                         claimed with one atomic per wave and bucket
//                           (hits)   es_particles_kernel  particle table keyed by (event, id) as tg_particles_kernel: hits,
//                                                         "has a good hit"; orphan counts; parent[i] = i for both forests
//                           (slots)  es_rows_kernel       a row number and the row (event, id, hits) per selected particle
//   gnntrk_ec_scan_steps, per threshold j = n_thr - 1 .. 0:
//                           (bucket) es_union_kernel      the edges of bucket g == j + 1: into the component forest and, with
//                                                         equal ids, into the segment forest
//                           (hits)   es_count_kernel      both forests compressed; segments per particle and the largest
//                                                         one; the table of the pairs (particle, component) and the
//                                                         largest pair count
//                           (slots)  es_emit_kernel       steps[j][row] = (segments, largest segment, largest component);
//                                                         clears what es_count_kernel filled, for the next threshold
//
// A running maximum replaces the second pass of track_graph.hip: a counter that only grows takes its final value
// with its last increment, so max over the increments of (old + 1) is the final count - for the size of a segment
// (counted at its root) and for the hits of a pair.  Every output is an integer that depends on the input alone;
// only the row number of a particle depends on the order in which atomics land: the caller sorts rows by (event, id).
// Bucket 0 (w <= t_0, NaN, bad edges) is never united.  Bounds: order[] holds each edge id once, at a slot below the
// end of its bucket (the histogram counted it); es_union_kernel checks the ids and the ends again, the workspace
// being the caller's between the two entries.  The work is integer, atomic- and latency-bound; no roofline applies.
#include <stdio.h>

#include "count_util.h"
#include "track_graph_util.h"
#include "union_find.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kMaxThr = GNNTRK_EC_SCAN_MAX_THR;
constexpr int kHistCap = 4096;   // words of the LDS histogram of (event, mask class, label, k); larger ones go to L2

struct Ws {
    int32_t *parent_c;   // [n]  forest of the components
    int32_t *parent_s;   // [n]  forest of the segments (edges between equal ids)
    uint32_t *hslot;     // [n]  particle slot of every hit with id > 0
    int32_t *order;      // [M]  edge ids sorted by graph bin
    uint16_t *gbin;      // [M]  graph bin of every edge
    uint32_t *bstart;    // [n_thr + 2]  first slot of every bucket of order[], then M
    uint32_t *prow;      // [S]  row of a selected particle
    // cleared by prepare
    uint32_t *ghist;     // [n_thr + 1]  edges per graph bin
    uint32_t *cursor;    // [n_thr + 1]  slots handed out per bucket
    uint8_t *touched;    // [n]  the hit is an end of an edge
    int32_t *ptab;       // [S]  particle table: first hit + 1, 0 = empty
    uint32_t *pcnt;      // [S]  hits per particle
    uint32_t *psel;      // [S]  the particle has a hit in the node mask
    // per threshold: cleared by prepare, then by es_emit_kernel
    uint32_t *segsize;   // [n]  size of the segment rooted at the hit
    uint32_t *pseg;      // [S]  segments per particle
    uint32_t *pmaxs;     // [S]  largest segment per particle
    uint32_t *pmaxc;     // [S]  largest pair count per particle
    int32_t *ctab;       // [S]  table of the pairs (particle, component): first hit + 1
    uint32_t *ccnt;      // [S]  hits per pair
    size_t zero_from, total;
    uint64_t S;
};

Ws make_ws(void *base, int64_t n, int64_t m, int32_t n_thr) {
    Ws w{};
    w.S = table_size(n);
    const size_t S = w.S, N = (size_t)n, M = (size_t)m, B = (size_t)n_thr + 1;
    Carver ws{(char *)base};
    w.parent_c = ws.take<int32_t>(N);
    w.parent_s = ws.take<int32_t>(N);
    w.hslot = ws.take<uint32_t>(N);
    w.order = ws.take<int32_t>(M);
    w.gbin = ws.take<uint16_t>(M);
    w.bstart = ws.take<uint32_t>(B + 1);
    w.prow = ws.take<uint32_t>(S);
    w.zero_from = ws.off;   // everything from here on is cleared
    w.ghist = ws.take<uint32_t>(B);
    w.cursor = ws.take<uint32_t>(B);
    w.touched = ws.take<uint8_t>(N);
    w.ptab = ws.take<int32_t>(S);
    w.pcnt = ws.take<uint32_t>(S);
    w.psel = ws.take<uint32_t>(S);
    w.segsize = ws.take<uint32_t>(N);
    w.pseg = ws.take<uint32_t>(S);
    w.pmaxs = ws.take<uint32_t>(S);
    w.pmaxc = ws.take<uint32_t>(S);
    w.ctab = ws.take<int32_t>(S);
    w.ccnt = ws.take<uint32_t>(S);
    w.total = ws.off;
    return w;
}

// ------------------------------------------------------------------------------- prepare
// #{j : pred(t_j)} for a predicate that holds on a prefix of the ascending table; top: the largest power of two <= n
template <class Pred> __device__ __forceinline__ int prefix_count(const float *t, int n, int top, Pred pred) {
    int k = 0;
    for (int s = top; s > 0; s >>= 1)
        if (k + s <= n && pred(t[k + s - 1])) k += s;
    return k;
}

// bcs: [events][2 mask classes][2 labels][n_thr + 1] (events = 1 without per_event); bad: out of range, across events
template <class Y, bool LDS>
__global__ __launch_bounds__(kTpb) void es_bin_kernel(const int64_t *__restrict__ ei, int64_t m,
                                                      const float *__restrict__ w, const Y *__restrict__ y,
                                                      const uint8_t *__restrict__ mask, int64_t n, Events ev,
                                                      int per_event, const float *__restrict__ thr, int n_thr, Ws ws,
                                                      unsigned long long *__restrict__ bcs, unsigned long long *bad) {
    __shared__ float s_thr[kMaxThr];
    __shared__ uint32_t s_g[kMaxThr + 1];
    __shared__ uint32_t hist[LDS ? kHistCap : 1];
    const int nb = n_thr + 1;
    const int nh = LDS ? (per_event ? ev.n : 1) * 4 * nb : 0;
    for (int i = threadIdx.x; i < n_thr; i += kTpb) s_thr[i] = thr[i];
    for (int i = threadIdx.x; i < nb; i += kTpb) s_g[i] = 0u;
    for (int i = threadIdx.x; i < nh; i += kTpb) hist[i] = 0u;
    __syncthreads();
    int top = 0;   // largest power of two <= n_thr
    for (int s = 1; s <= n_thr; s <<= 1) top = s;
    const int lane = threadIdx.x & 63;
    uint32_t nbad[2] = {0u, 0u};
    // (the loop bound is wave-uniform: the ballots below need every lane of the wave)
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {
        const int64_t i = base + threadIdx.x;
        int key = -1;
        if (i < m) {
            const int64_t a = ei[i], b = ei[m + i];
            const float x = w[i];
            int g = 0;
            if (a < 0 || a >= n || b < 0 || b >= n) {
                nbad[0] += 1u;
            } else {
                int64_t lo, hi;
                const int e = tg_event_rows(ev, n, a, lo, hi);
                if (b < lo || b >= hi)
                    nbad[1] += 1u;
                else
                    g = prefix_count(s_thr, n_thr, top, [&](float t) { return x > t; });
                ws.touched[a] = 1;   // (every writer stores the same value)
                ws.touched[b] = 1;
                const int k = prefix_count(s_thr, n_thr, top, [&](float t) { return !(x < t); });
                const int cls = (mask[a] && mask[b]) ? 1 : 0;
                key = (((per_event ? e : 0) * 2 + cls) * 2 + (int)is_positive(y, i)) * nb + k;
            }
            ws.gbin[i] = (uint16_t)g;
            atomicAdd(&s_g[g], 1u);
        }
        // two leader rounds take the commonest keys of the wave with one atomic each (bcs_counts_kernel), the rest
        // add directly
        for (int r = 0; r < 3; ++r) {
            const unsigned long long live = __ballot(key >= 0);
            if (!live) break;
            int lk = key;
            uint32_t cnt = 1u;
            bool add = key >= 0;
            if (r < 2) {
                const int lead = __builtin_ctzll(live);
                lk = __shfl(key, lead);
                const unsigned long long same = __ballot(key == lk);
                cnt = (uint32_t)__popcll(same);
                add = lane == lead;
                if (key == lk) key = -1;
            } else {
                key = -1;
            }
            if (add) {
                if (LDS) atomicAdd(&hist[lk], cnt);
                else atomicAdd(&bcs[lk], (unsigned long long)cnt);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += kTpb)
        if (s_g[i]) atomicAdd(&ws.ghist[i], s_g[i]);
    for (int i = threadIdx.x; i < nh; i += kTpb)
        if (hist[i]) atomicAdd(&bcs[i], (unsigned long long)hist[i]);
    block_add(nbad, bad);
}

// one workgroup: bstart[g] = edges in the bins below g, for g = 0 .. n_thr + 1
__global__ __launch_bounds__(kTpb) void es_offsets_kernel(Ws ws, int n_thr) {
    __shared__ uint32_t s[kMaxThr + 1];
    const int nb = n_thr + 1;
    for (int i = threadIdx.x; i < nb; i += kTpb) s[i] = ws.ghist[i];
    __syncthreads();
    for (int i = threadIdx.x; i <= nb; i += kTpb) {
        uint32_t a = 0u;
        for (int j = 0; j < i; ++j) a += s[j];
        ws.bstart[i] = a;
    }
}

// the lanes of a wave that share a bucket claim their slots with one atomic; the order inside a bucket is free
__global__ __launch_bounds__(kTpb) void es_scatter_kernel(int64_t m, Ws ws) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {
        const int64_t i = base + threadIdx.x;
        int g = i < m ? (int)ws.gbin[i] : 0;   // (bucket 0 is never read: its slots stay as they are)
        for (;;) {
            const unsigned long long live = __ballot(g > 0);
            if (!live) break;   // (uniform in the wave)
            const int lead = __builtin_ctzll(live);
            const int lg = __shfl(g, lead);
            const unsigned long long same = __ballot(g == lg);
            uint32_t first = 0u;
            if (lane == lead) first = atomicAdd(&ws.cursor[lg], (uint32_t)__popcll(same));
            first = __shfl(first, lead);
            if (g == lg) {
                const int64_t slot = (int64_t)ws.bstart[lg] + first + __popcll(same & ((1ull << lane) - 1ull));
                if (slot < m) ws.order[slot] = (int32_t)i;
                g = 0;
            }
        }
    }
}

// orphans: [events][3] hits without an edge that are bad, good, all (events = 1 without per_event)
__global__ __launch_bounds__(kTpb) void es_particles_kernel(const int64_t *__restrict__ pid,
                                                            const uint8_t *__restrict__ mask, int64_t n, Events ev,
                                                            int per_event, Ws w, unsigned long long *orphans) {
    const uint64_t smask = w.S - 1;
    uint32_t oc[3] = {0u, 0u, 0u};
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < n; base += (int64_t)gridDim.x * kTpb) {
        const int64_t i = base + threadIdx.x;
        int e = 0;
        if (i < n) {
            w.parent_c[i] = (int32_t)i;
            w.parent_s[i] = (int32_t)i;
            int64_t lo, hi;
            e = tg_event_rows(ev, n, i, lo, hi);
            const bool good = mask[i] != 0;
            if (!w.touched[i]) {
                oc[good ? 1 : 0] += 1u;
                oc[2] += 1u;
            }
            const int64_t key = pid[i];
            if (key > 0) {   // (a selected id is the id of a good hit: > 0)
                const uint64_t s = table_claim(w.ptab, smask, particle_hash<true>(key, e), i,
                                               [&](int32_t h) { return pid[h] == key; },
                                               [&](int32_t h) { return h >= lo && h < hi; });
                w.hslot[i] = (uint32_t)s;
                atomicAdd(&w.pcnt[s], 1u);
                if (good) w.psel[s] = 1u;   // (every writer stores the same value)
            }
        }
        if (per_event) event_add(oc, e, orphans, 3);
    }
    if (!per_event) block_add(oc, orphans);
}

// head[0] rows; particles: [n][3] event, id, hits
__global__ __launch_bounds__(kTpb) void es_rows_kernel(const int64_t *__restrict__ pid, Events ev, Ws w,
                                                       int64_t *__restrict__ particles, unsigned long long *head) {
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        const int32_t first = w.ptab[s];
        if (first == 0 || !w.psel[s]) continue;
        const int64_t r = (int64_t)atomicAdd(&head[0], 1ull);
        w.prow[s] = (uint32_t)r;
        particles[3 * r + 0] = segment_of(ev.ptr, ev.n, first - 1);
        particles[3 * r + 1] = pid[first - 1];
        particles[3 * r + 2] = w.pcnt[s];
    }
}

// --------------------------------------------------------------------------------- steps
__global__ __launch_bounds__(kTpb) void es_union_kernel(const int64_t *__restrict__ ei, int64_t m,
                                                        const int64_t *__restrict__ pid, int64_t n, Ws w, int bucket) {
    const int64_t lo = w.bstart[bucket];
    int64_t hi = w.bstart[bucket + 1];
    hi = hi > m ? m : hi;
    for (int64_t at = lo + (int64_t)blockIdx.x * kTpb + threadIdx.x; at < hi; at += (int64_t)gridDim.x * kTpb) {
        const int64_t e = w.order[at];
        if (e < 0 || e >= m) continue;
        const int64_t a = ei[e], b = ei[m + e];
        if (a < 0 || a >= n || b < 0 || b >= n || a == b) continue;
        ks_unite(w.parent_c, (int32_t)a, (int32_t)b);
        if (pid[a] == pid[b]) ks_unite(w.parent_s, (int32_t)a, (int32_t)b);   // (no `> 0` test, as cc_labels' same_pid)
    }
}

// No union runs beside it: a root is final, storing it into parent[i] moves i up its own path (union_find.h), and the
// component of another hit is read off the forest (its root) where the pair table compares keys.
__global__ __launch_bounds__(kTpb) void es_count_kernel(const int64_t *__restrict__ pid, int64_t n, Ws w) {
    const uint64_t smask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int32_t r = ks_find(w.parent_s, (int32_t)i), c = ks_find(w.parent_c, (int32_t)i);
        store_i32(&w.parent_s[i], r);
        store_i32(&w.parent_c[i], c);
        if (pid[i] <= 0) continue;
        const uint32_t s = w.hslot[i];   // (a segment lies in one event and has one id: this is its particle)
        if (r == (int32_t)i) atomicAdd(&w.pseg[s], 1u);
        atomicMax(&w.pmaxs[s], atomicAdd(&w.segsize[r], 1u) + 1u);
        const uint64_t cs = table_claim(w.ctab, smask, mix64(((uint64_t)s << 32) ^ (uint64_t)c), i, [&](int32_t h) {
            return w.hslot[h] == s && ks_find(w.parent_c, h) == c;
        });
        atomicMax(&w.pmaxc[s], atomicAdd(&w.ccnt[cs], 1u) + 1u);
    }
}

// out: the rows of this threshold, [n_rows][3]
__global__ __launch_bounds__(kTpb) void es_emit_kernel(int64_t n, Ws w, int64_t n_rows, int32_t *__restrict__ out) {
    const int64_t S = (int64_t)w.S;   // (S >= 2 n: the loop passes every hit as well)
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        if (s < n) w.segsize[s] = 0u;
        if (w.ctab[s] != 0) {
            w.ctab[s] = 0;
            w.ccnt[s] = 0u;
        }
        if (w.ptab[s] == 0) continue;
        const uint32_t n_seg = w.pseg[s], seg = w.pmaxs[s], comp = w.pmaxc[s];
        w.pseg[s] = 0u;
        w.pmaxs[s] = 0u;
        w.pmaxc[s] = 0u;
        const int64_t r = w.prow[s];
        if (!w.psel[s] || r >= n_rows) continue;
        out[3 * r + 0] = (int32_t)n_seg;
        out[3 * r + 1] = (int32_t)seg;
        out[3 * r + 2] = (int32_t)comp;
    }
}

// the checks that both entries share; *w: the workspace carved for these sizes
int check_sizes(const char *entry, int64_t n, int64_t n_edges, int32_t n_thr, void *workspace, size_t workspace_bytes,
                Ws *w) {
    char msg[160];
    int rc = check_count_i30(entry, "hit", n);
    if (rc) return rc;
    if (n_edges < 0) {
        snprintf(msg, sizeof(msg), "%s: negative edge count", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n_edges > 0x3fffffff) {
        snprintf(msg, sizeof(msg), "%s: at most 2^30-1 edges", entry);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    if (n_thr < 1 || n_thr > kMaxThr) {
        snprintf(msg, sizeof(msg), "%s: n_thr = %d, expected 1..%d", entry, (int)n_thr, kMaxThr);
        return fail(n_thr > kMaxThr ? GNNTRK_EUNSUPPORTED : GNNTRK_EINVAL, msg);
    }
    *w = make_ws(workspace, n, n_edges, n_thr);
    if (n > 0) return check_workspace(entry, workspace, workspace_bytes, w->total);
    return GNNTRK_OK;
}

}  // namespace

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_ec_scan_prepare_workspace_bytes(int64_t n, int64_t n_edges, int32_t n_thr) {
    return make_ws(nullptr, n < 0 ? 0 : n, n_edges < 0 ? 0 : n_edges, n_thr < 1 ? 1 : (n_thr > kMaxThr ? kMaxThr : n_thr))
        .total;
}

int gnntrk_ec_scan_prepare(const int64_t *edge_index, int64_t n_edges, const float *w, const void *y, int32_t y_kind,
                           const int64_t *particle_id, const uint8_t *node_mask, int64_t n, const int64_t *seg_ptr,
                           int32_t n_seg, const float *thresholds, int32_t n_thr, int32_t per_event, int64_t *head,
                           int64_t *particles, int64_t *bcs, int64_t *orphans, void *workspace, size_t workspace_bytes,
                           void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Ws ws{};
    int rc = check_sizes("ec_scan_prepare", n, n_edges, n_thr, workspace, workspace_bytes, &ws);
    if (rc || (rc = check_events("ec_scan_prepare", seg_ptr, n_seg))) return rc;
    if (y_kind != 0 && y_kind != 1) return fail(GNNTRK_EINVAL, "ec_scan_prepare: y_kind must be 0 (bytes) or 1 (float32)");
    if (!thresholds || !head || !bcs || !orphans)
        return fail(GNNTRK_EINVAL, "ec_scan_prepare: NULL thresholds, head, bcs or orphans");
    if (n > 0 && (!particle_id || !node_mask || !particles))
        return fail(GNNTRK_EINVAL, "ec_scan_prepare: NULL particle ids, node mask or particles");
    if (n_edges > 0 && (!edge_index || !w || !y)) return fail(GNNTRK_EINVAL, "ec_scan_prepare: NULL edge_index, w or y");
    const size_t n_ev = per_event ? (size_t)n_seg : 1, n_bins = n_ev * 4 * ((size_t)n_thr + 1);
    if ((rc = check_hip(hipMemsetAsync(head, 0, 4 * sizeof(int64_t), stream), "ec_scan_prepare: clear")) ||
        (rc = check_hip(hipMemsetAsync(bcs, 0, n_bins * sizeof(int64_t), stream), "ec_scan_prepare: clear")) ||
        (rc = check_hip(hipMemsetAsync(orphans, 0, n_ev * 3 * sizeof(int64_t), stream), "ec_scan_prepare: clear")))
        return rc;
    if (n == 0) return GNNTRK_OK;   // (nothing is read: with n_edges > 0 every edge is out of range, the caller's to refuse)
    if ((rc = check_hip(hipMemsetAsync((char *)workspace + ws.zero_from, 0, ws.total - ws.zero_from, stream),
                        "ec_scan_prepare: clear workspace")))
        return rc;
    const Events ev{seg_ptr, n_seg};
    auto *h = reinterpret_cast<unsigned long long *>(head);
    auto *b = reinterpret_cast<unsigned long long *>(bcs);
    if (n_edges > 0) {
        const int gm = blocks_for(n_edges, 8);
        lift_bools(
            [&](auto is_float, auto lds) {
                using Y = std::conditional_t<decltype(is_float)::value, float, uint8_t>;
                launch(es_bin_kernel<Y, decltype(lds)::value>, gm, kTpb, stream, edge_index, n_edges, w, (const Y *)y,
                       node_mask, n, ev, (int)(per_event != 0), thresholds, (int)n_thr, ws, b, h + 2);
            },
            y_kind == 1, n_bins <= (size_t)kHistCap);
        launch(es_offsets_kernel, 1, kTpb, stream, ws, (int)n_thr);
        launch(es_scatter_kernel, gm, kTpb, stream, n_edges, ws);
    }
    launch(es_particles_kernel, blocks_for(n, 8), kTpb, stream, particle_id, node_mask, n, ev, (int)(per_event != 0), ws,
           reinterpret_cast<unsigned long long *>(orphans));
    launch(es_rows_kernel, blocks_for((int64_t)ws.S, 8), kTpb, stream, particle_id, ev, ws, particles, h);
    return check_launch("ec_scan_prepare");
}

int gnntrk_ec_scan_steps(const int64_t *edge_index, int64_t n_edges, const int64_t *particle_id, int64_t n,
                         int32_t n_thr, int64_t n_particles, int32_t *steps, void *workspace, size_t workspace_bytes,
                         void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Ws ws{};
    int rc = check_sizes("ec_scan_steps", n, n_edges, n_thr, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    if (n_particles < 0 || n_particles > n)
        return fail(GNNTRK_EINVAL, "ec_scan_steps: n_particles must be the head[0] of ec_scan_prepare, 0..n");
    if (n_particles == 0) return GNNTRK_OK;
    if (!particle_id || !steps) return fail(GNNTRK_EINVAL, "ec_scan_steps: NULL particle ids or steps");
    if (n_edges > 0 && !edge_index) return fail(GNNTRK_EINVAL, "ec_scan_steps: NULL edge_index");
    const int gm = blocks_for(n_edges, 8), gn = blocks_for(n, 8), gs = blocks_for((int64_t)ws.S, 8);
    for (int j = n_thr - 1; j >= 0; --j) {
        if (n_edges > 0) launch(es_union_kernel, gm, kTpb, stream, edge_index, n_edges, particle_id, n, ws, j + 1);
        launch(es_count_kernel, gn, kTpb, stream, particle_id, n, ws);
        launch(es_emit_kernel, gs, kTpb, stream, n, ws, n_particles, steps + (size_t)j * (size_t)n_particles * 3);
        if ((rc = check_launch("ec_scan_steps"))) return rc;
    }
    return GNNTRK_OK;
}

}  // extern "C"
