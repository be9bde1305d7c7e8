// Track-graph statistics of a built graph (analysis/graphs.py:49-192): per selected particle the number of
// hits, the number of segments, the largest segment, the largest number of its hits in one connected
// component, and the graph distance between its two largest segments.  The reference walks networkx once per
// particle and runs a shortest-path search for every pair of hits of the two segments; here the table is
// integer counting on two label arrays of gnntrk_cc_labels (kscan.hip) and the distance is ONE multi-source
// breadth-first search per split particle.
//
//   gnntrk_track_graph_table      (hits)   tg_particles_kernel   particle table of the hits with id > 0 keyed by
//                                                                 (event, id) (open addressing, count_util.h): n_hits,
//                                                                 "has a good hit"; size of every segment at its root
//                                 (hits)   tg_segments_kernel    per particle: number of segments and the largest one;
//                                                                 the table of the pairs (particle, component) with
//                                                                 the particle's hits per component
//                                 (slots)  tg_second_kernel      per particle: the second-largest segment and the
//                                                                 largest pair count
//                                 (slots)  tg_rows_kernel        one row per selected particle; the rows whose two
//                                                                 top segments share a component go to the search list
//   gnntrk_track_graph_adjacency  (edges)  tg_degree_kernel      degrees; bad and cross-event edges counted and left out
//                                 (hits)   scan_counts_kernel    (knn.hip) exclusive scan -> row pointer
//                                 (edges)  tg_fill_kernel        neighbours of both directions
//   gnntrk_track_graph_distance   (search list) tg_distance_kernel   the search, one workgroup per particle
//
// A segment's label is its smallest hit index (cc_labels with same_pid), so "size of a segment" is a counter at that
// hit and a segment is ranked by the 64-bit key (size << 32) | (2^32 - 1 - label): the largest key is the largest
// segment, ties going to the SMALLEST label - the tie rule of graph_analysis.py.  Every value of a row is an integer
// that depends on the input alone (counts, maxima of keys), so nothing depends on the order in which atomics land;
// the ORDER of the rows does (a row is claimed with an atomic counter): the caller sorts them by (event, id).
//
// The search (tg_distance_kernel) is level-synchronous over three bitmaps of the particle's EVENT (local index = hit
// - first hit of the event): visited, frontier, next.  The frontier starts as the hits of segment A; a level walks the
// adjacency rows of the frontier's hits, marks unvisited neighbours (atomicOr) in visited and next and raises `found`
// when one of them carries segment B's label: the level number is then the fewest edges between the segments.  Bounds:
// the level loop runs at most (hits of the event) times and ends on an empty frontier - a level without a newly
// visited hit - so it cannot spin; every hit enters the frontier once, so a search walks every adjacency row of its
// component at most once: O(hits / 32 * levels + edges of the component).  The bitmaps live in LDS when the event has
// at most `lds_hits` hits (3 x 20 KB for the default 163 840 hits: two workgroups per CU of 160 KB) and otherwise in
// the workgroup's slice of the workspace, behind the same pointer.  Nothing here is floating point; the work is
// latency- and atomic-bound, there is no roofline to quote for it.
#include <limits.h>
#include <stdio.h>

#include "count_util.h"
#include "track_graph_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kCols = GNNTRK_TRACK_GRAPH_COLUMNS;
constexpr int kLdsWords = 5120;               // words of ONE bitmap in LDS: 163 840 hits, 3 x 20 KB per workgroup
constexpr int kLdsHits = kLdsWords * 32;
constexpr int kSearchBlocksPerCu = 2;         // (what the LDS of a CU holds)

// columns of a row
enum { T_EVENT = 0, T_PID, T_HITS, T_SEGMENTS, T_LARGEST_SEGMENT, T_LARGEST_COMPONENT, T_DISTANCE, T_SEG_A, T_SEG_B };
constexpr int64_t kNoPath = -1, kPending = -2;   // T_DISTANCE: no path / waits for the search

// --------------------------------------------------------------------------- the table
struct Ws {
    uint32_t *hslot;             // [n]  particle slot of every hit with id > 0
    int32_t *ptab;               // [S]  particle table: first hit + 1, 0 = empty
    uint32_t *pcnt;              // [S]  hits per particle
    uint32_t *pseg;              // [S]  segments per particle
    uint32_t *psel;              // [S]  the particle has a hit in the node mask
    uint32_t *pmaxc;             // [S]  the particle's largest number of hits in one component
    unsigned long long *top1;    // [S]  key of the largest segment
    unsigned long long *top2;    // [S]  key of the second-largest segment
    uint32_t *segsize;           // [n]  size of the segment rooted at the hit
    int32_t *ctab;               // [S]  table of the pairs (particle, component): first hit + 1
    uint32_t *ccnt;              // [S]  hits per pair
    size_t zero_from, total;
    uint64_t S;
};

Ws make_ws(void *base, int64_t n) {
    Ws w{};
    w.S = table_size(n);
    const size_t S = w.S, N = (size_t)n;
    Carver ws{(char *)base};
    w.hslot = ws.take<uint32_t>(N);
    w.zero_from = ws.off;   // everything from here on is cleared
    w.ptab = ws.take<int32_t>(S);
    w.pcnt = ws.take<uint32_t>(S);
    w.pseg = ws.take<uint32_t>(S);
    w.psel = ws.take<uint32_t>(S);
    w.pmaxc = ws.take<uint32_t>(S);
    w.top1 = ws.take<unsigned long long>(S);
    w.top2 = ws.take<unsigned long long>(S);
    w.segsize = ws.take<uint32_t>(N);
    w.ctab = ws.take<int32_t>(S);
    w.ccnt = ws.take<uint32_t>(S);
    w.total = ws.off;
    return w;
}

__global__ __launch_bounds__(kTpb) void tg_particles_kernel(const int64_t *__restrict__ seg,
                                                            const int64_t *__restrict__ pid,
                                                            const uint8_t *__restrict__ mask, int64_t n, Events ev, Ws w) {
    const uint64_t smask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int64_t key = pid[i];
        if (key <= 0) continue;   // (a selected id is the id of a good hit: > 0)
        int64_t lo, hi;
        const int e = tg_event_rows(ev, n, i, lo, hi);
        const uint64_t s = table_claim(w.ptab, smask, particle_hash<true>(key, e), i,
                                       [&](int32_t h) { return pid[h] == key; },
                                       [&](int32_t h) { return h >= lo && h < hi; });
        w.hslot[i] = (uint32_t)s;
        atomicAdd(&w.pcnt[s], 1u);
        if (mask[i]) w.psel[s] = 1u;   // (every writer stores the same value)
        const int64_t r = seg[i];
        if (r >= 0 && r < n) atomicAdd(&w.segsize[r], 1u);
    }
}

__global__ __launch_bounds__(kTpb) void tg_segments_kernel(const int64_t *__restrict__ seg,
                                                           const int64_t *__restrict__ comp,
                                                           const int64_t *__restrict__ pid, int64_t n, Ws w) {
    const uint64_t smask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        if (pid[i] <= 0) continue;
        const uint32_t s = w.hslot[i];
        if (seg[i] == i) {   // the root of a segment
            atomicAdd(&w.pseg[s], 1u);
            max_u64(&w.top1[s], seg_key(w.segsize[i], i));
        }
        const int64_t c = comp[i];
        const uint64_t cs = table_claim(w.ctab, smask, mix64(((uint64_t)s << 32) ^ (uint64_t)c), i,
                                        [&](int32_t h) { return w.hslot[h] == s && comp[h] == c; });
        atomicAdd(&w.ccnt[cs], 1u);
    }
}

// over max(n, S) indices: the hits for the second-largest segment, the pair slots for the largest pair count
__global__ __launch_bounds__(kTpb) void tg_second_kernel(const int64_t *__restrict__ seg,
                                                         const int64_t *__restrict__ pid, int64_t n, Ws w) {
    const int64_t S = (int64_t)w.S;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < S; i += (int64_t)gridDim.x * kTpb) {
        if (i < n && pid[i] > 0 && seg[i] == i) {
            const uint32_t s = w.hslot[i];
            const unsigned long long key = seg_key(w.segsize[i], i);
            if (key != w.top1[s]) max_u64(&w.top2[s], key);
        }
        const int32_t first = w.ctab[i];
        if (first != 0) atomicMax(&w.pmaxc[w.hslot[first - 1]], w.ccnt[i]);
    }
}

// counts[0] rows, counts[1] entries of the search list
__global__ __launch_bounds__(kTpb) void tg_rows_kernel(const int64_t *__restrict__ comp,
                                                       const int64_t *__restrict__ pid, Events ev, Ws w,
                                                       int64_t *__restrict__ table, int32_t *__restrict__ search,
                                                       unsigned long long *counts) {
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        const int32_t first = w.ptab[s];
        if (first == 0 || !w.psel[s]) continue;
        const int64_t r = (int64_t)atomicAdd(&counts[0], 1ull);
        int64_t *row = table + r * kCols;
        const unsigned long long k1 = w.top1[s], k2 = w.top2[s];
        const uint32_t n_seg = w.pseg[s];
        row[T_EVENT] = segment_of(ev.ptr, ev.n, first - 1);
        row[T_PID] = pid[first - 1];
        row[T_HITS] = w.pcnt[s];
        row[T_SEGMENTS] = n_seg;
        row[T_LARGEST_SEGMENT] = (int64_t)(k1 >> 32);
        row[T_LARGEST_COMPONENT] = w.pmaxc[s];
        const int64_t a = key_label(k1), b = n_seg > 1 ? key_label(k2) : -1;
        row[T_SEG_A] = a;
        row[T_SEG_B] = b;
        int64_t dist = 0;
        if (n_seg > 1) {
            dist = kNoPath;
            if (comp[a] == comp[b]) {
                dist = kPending;
                search[atomicAdd(&counts[1], 1ull)] = (int32_t)r;
            }
        }
        row[T_DISTANCE] = dist;
    }
}

// ----------------------------------------------------------------------------- the adjacency
// an edge counts as bad[0] with an end outside [0, n), as bad[1] with its ends in two events; neither enters a row
__device__ __forceinline__ bool tg_edge(const int64_t *__restrict__ ei, int64_t m, int64_t e, int64_t n, const Events &ev,
                                        int64_t &a, int64_t &b, uint32_t (&nbad)[2]) {
    a = ei[e];
    b = ei[m + e];
    if (a < 0 || a >= n || b < 0 || b >= n) {
        nbad[0] += 1u;
        return false;
    }
    int64_t lo, hi;
    tg_event_rows(ev, n, a, lo, hi);
    if (b < lo || b >= hi) {
        nbad[1] += 1u;
        return false;
    }
    return a != b;   // (a self loop adds nothing to a search)
}

__global__ __launch_bounds__(kTpb) void tg_degree_kernel(const int64_t *__restrict__ ei, int64_t m, int64_t n, Events ev,
                                                         int32_t *deg, unsigned long long *bad) {
    uint32_t nbad[2] = {0u, 0u};
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {
        const int64_t e = base + threadIdx.x;
        int64_t a, b;
        if (e < m && tg_edge(ei, m, e, n, ev, a, b, nbad)) {
            atomicAdd(&deg[a], 1);
            atomicAdd(&deg[b], 1);
        }
    }
    block_add(nbad, bad);
}

// (deg counts down to zero: the place of an entry in its row is whatever the atomics give it)
__global__ __launch_bounds__(kTpb) void tg_fill_kernel(const int64_t *__restrict__ ei, int64_t m, int64_t n, Events ev,
                                                       int32_t *deg, const int64_t *__restrict__ rowptr,
                                                       int32_t *__restrict__ nbr) {
    uint32_t nbad[2] = {0u, 0u};
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < m; e += (int64_t)gridDim.x * kTpb) {
        int64_t a, b;
        if (!tg_edge(ei, m, e, n, ev, a, b, nbad)) continue;
        nbr[rowptr[a] + atomicAdd(&deg[a], -1) - 1] = (int32_t)b;
        nbr[rowptr[b] + atomicAdd(&deg[b], -1) - 1] = (int32_t)a;
    }
}

// -------------------------------------------------------------------------------- the search
// A bitmap word is set by atomicOr, which works in L2 when the bitmaps live in the workspace: it is read and cleared
// with agent-scope atomics as well, so that no read is served from a line that the CU's vector cache loaded before.
__device__ __forceinline__ uint32_t bits_load(const uint32_t *p) { return (uint32_t)load_i32((const int32_t *)p); }
__device__ __forceinline__ void bits_store(uint32_t *p, uint32_t v) { store_i32((int32_t *)p, (int32_t)v); }

__global__ __launch_bounds__(kTpb) void tg_distance_kernel(int64_t *table, const int32_t *__restrict__ search,
                                                           const unsigned long long *__restrict__ counts,
                                                           const int64_t *__restrict__ seg,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ nbr, Events ev, int64_t n,
                                                           int32_t lds_hits, uint32_t *ws_bits, size_t ws_words) {
    __shared__ uint32_t s_bits[3 * kLdsWords];
    __shared__ int s_found, s_any;
    const int tid = threadIdx.x;
    const int64_t n_search = (int64_t)counts[1];
    for (int64_t p = blockIdx.x; p < n_search; p += gridDim.x) {
        int64_t *row = table + (int64_t)search[p] * kCols;
        const int64_t a = row[T_SEG_A], b = row[T_SEG_B];
        int64_t lo, hi;
        tg_event_rows(ev, n, a, lo, hi);
        const int64_t ne = hi - lo;   // (a lies in [lo, hi): ne >= 1)
        const int64_t words = (ne + 31) >> 5;
        uint32_t *base = ne <= lds_hits ? s_bits : ws_bits + (size_t)blockIdx.x * 3 * ws_words;
        uint32_t *visited = base, *frontier = base + words, *next = base + 2 * words;
        for (int64_t i = tid; i < 3 * words; i += kTpb) bits_store(&base[i], 0u);
        if (tid == 0) {
            s_found = 0;
            s_any = 0;
        }
        __syncthreads();
        for (int64_t i = tid; i < ne; i += kTpb)
            if (seg[lo + i] == a) {
                atomicOr(&visited[i >> 5], 1u << (i & 31));
                atomicOr(&frontier[i >> 5], 1u << (i & 31));
            }
        __syncthreads();
        int64_t dist = kNoPath;
        for (int64_t level = 1; level <= ne; ++level) {
            for (int64_t wd = tid; wd < words; wd += kTpb) {
                uint32_t f = bits_load(&frontier[wd]);
                while (f) {
                    const int64_t v = lo + (wd << 5) + __builtin_ctz(f);
                    f &= f - 1u;
                    for (int64_t j = rowptr[v], end = rowptr[v + 1]; j < end; ++j) {
                        const int64_t u = nbr[j];
                        if (u < lo || u >= hi) continue;   // (never for a row of tg_fill_kernel with this seg_ptr)
                        const int64_t lu = u - lo;
                        const uint32_t bit = 1u << (lu & 31);
                        if (atomicOr(&visited[lu >> 5], bit) & bit) continue;
                        atomicOr(&next[lu >> 5], bit);
                        s_any = 1;
                        if (seg[u] == b) s_found = 1;
                    }
                }
            }
            __syncthreads();
            const int found = s_found, any = s_any;
            __syncthreads();
            if (found) dist = level;
            if (found || !any) break;   // (uniform in the workgroup)
            for (int64_t wd = tid; wd < words; wd += kTpb) bits_store(&frontier[wd], 0u);
            if (tid == 0) s_any = 0;
            uint32_t *t = frontier;
            frontier = next;
            next = t;
            __syncthreads();
        }
        if (tid == 0) row[T_DISTANCE] = dist;
        __syncthreads();
    }
}

int search_blocks(int64_t n) {
    const int64_t most = n / 2 < 1 ? 1 : n / 2, cap = (int64_t)cu_count() * kSearchBlocksPerCu;   // (a split particle: >= 2 hits)
    return (int)(most < cap ? most : cap);
}
size_t bitmap_words(int64_t n) { return (size_t)ceil_div(n < 1 ? 1 : n, 32); }
size_t distance_ws_bytes(int64_t n, int32_t lds_hits) {
    if (n <= lds_hits) return 0;   // every event fits the LDS bitmaps
    return align_up((size_t)search_blocks(n) * 3 * bitmap_words(n) * sizeof(uint32_t), 256);
}

int distance(int64_t *table, const int32_t *search, const int64_t *counts, const int64_t *segment_labels,
             const int64_t *rowptr, const int32_t *neighbors, int64_t n, const int64_t *seg_ptr, int32_t n_seg,
             int32_t lds_hits, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    int rc = check_count_i30("track_graph_distance", "hit", n);
    if (rc || (rc = check_events("track_graph_distance", seg_ptr, n_seg))) return rc;
    if (lds_hits < 1 || lds_hits > kLdsHits) {
        char msg[160];
        snprintf(msg, sizeof(msg), "track_graph_distance: lds_hits = %d, expected 1..%d", (int)lds_hits, kLdsHits);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n == 0) return GNNTRK_OK;
    if (!table || !search || !counts || !segment_labels || !rowptr)
        return fail(GNNTRK_EINVAL, "track_graph_distance: NULL table, search list, counts, labels or row pointer");
    const size_t need = distance_ws_bytes(n, lds_hits);
    if (need && (rc = check_workspace("track_graph_distance", workspace, workspace_bytes, need))) return rc;
    hipLaunchKernelGGL(tg_distance_kernel, dim3(search_blocks(n)), dim3(kTpb), 0, stream, table, search,
                       reinterpret_cast<const unsigned long long *>(counts), segment_labels, rowptr, neighbors,
                       Events{seg_ptr, n_seg}, n, lds_hits, (uint32_t *)workspace, bitmap_words(n));
    return check_launch("track_graph_distance");
}

}  // namespace

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_track_graph_table_workspace_bytes(int64_t n) { return make_ws(nullptr, n < 0 ? 0 : n).total; }

int gnntrk_track_graph_table(const int64_t *segment_labels, const int64_t *component_labels, const int64_t *particle_id,
                             const uint8_t *node_mask, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t *table,
                             int32_t *search, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_count_i30("track_graph_table", "hit", n);
    if (rc || (rc = check_events("track_graph_table", seg_ptr, n_seg))) return rc;
    if (!counts) return fail(GNNTRK_EINVAL, "track_graph_table: NULL counts");
    if (n > 0 && (!segment_labels || !component_labels || !particle_id || !node_mask || !table || !search))
        return fail(GNNTRK_EINVAL, "track_graph_table: NULL labels, particle ids, node mask, table or search list");
    const Ws w = make_ws(workspace, n);
    if (n > 0 && (rc = check_workspace("track_graph_table", workspace, workspace_bytes, w.total))) return rc;
    rc = check_hip(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), stream), "track_graph_table: clear");
    if (rc || n == 0) return rc;
    if ((rc = check_hip(hipMemsetAsync((char *)workspace + w.zero_from, 0, w.total - w.zero_from, stream),
                        "track_graph_table: clear workspace")))
        return rc;
    const Events ev{seg_ptr, n_seg};
    const int gn = blocks_for(n, 8), gs = blocks_for((int64_t)w.S, 8);
    launch(tg_particles_kernel, gn, kTpb, stream, segment_labels, particle_id, node_mask, n, ev, w);
    launch(tg_segments_kernel, gn, kTpb, stream, segment_labels, component_labels, particle_id, n, w);
    launch(tg_second_kernel, gs, kTpb, stream, segment_labels, particle_id, n, w);
    launch(tg_rows_kernel, gs, kTpb, stream, component_labels, particle_id, ev, w, table, search,
           reinterpret_cast<unsigned long long *>(counts));
    return check_launch("track_graph_table");
}

size_t gnntrk_track_graph_adjacency_workspace_bytes(int64_t n) {
    return align_up(sizeof(int32_t) * (size_t)(n < 0 ? 0 : n), 256);
}

int gnntrk_track_graph_adjacency(const int64_t *edge_index, int64_t n_edges, int64_t n, const int64_t *seg_ptr,
                                 int32_t n_seg, int64_t *rowptr, int32_t *neighbors, int64_t *n_bad, void *workspace,
                                 size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_count_i30("track_graph_adjacency", "hit", n);
    if (rc || (rc = check_events("track_graph_adjacency", seg_ptr, n_seg))) return rc;
    if (n_edges < 0) return fail(GNNTRK_EINVAL, "track_graph_adjacency: negative edge count");
    if (n_edges > 0x3fffffff) return fail(GNNTRK_EUNSUPPORTED, "track_graph_adjacency: at most 2^30-1 edges");
    if (!rowptr || !n_bad) return fail(GNNTRK_EINVAL, "track_graph_adjacency: NULL row pointer or bad-edge counts");
    if (n_edges > 0 && (!edge_index || !neighbors))
        return fail(GNNTRK_EINVAL, "track_graph_adjacency: NULL edge_index or neighbours");
    if (n > 0 && (rc = check_workspace("track_graph_adjacency", workspace, workspace_bytes,
                                       gnntrk_track_graph_adjacency_workspace_bytes(n))))
        return rc;
    if ((rc = check_hip(hipMemsetAsync(n_bad, 0, 2 * sizeof(int64_t), stream), "track_graph_adjacency: clear")))
        return rc;
    if (n == 0) return check_hip(hipMemsetAsync(rowptr, 0, sizeof(int64_t), stream), "track_graph_adjacency: clear");
    auto *deg = (int32_t *)workspace;
    if ((rc = check_hip(hipMemsetAsync(deg, 0, sizeof(int32_t) * (size_t)n, stream), "track_graph_adjacency: clear")))
        return rc;
    const Events ev{seg_ptr, n_seg};
    const int gm = blocks_for(n_edges, 8);
    if (n_edges > 0)
        launch(tg_degree_kernel, gm, kTpb, stream, edge_index, n_edges, n, ev, deg,
               reinterpret_cast<unsigned long long *>(n_bad));
    scan_counts_launch(deg, INT_MAX, n, rowptr, stream);
    if (n_edges > 0) launch(tg_fill_kernel, gm, kTpb, stream, edge_index, n_edges, n, ev, deg, rowptr, neighbors);
    return check_launch("track_graph_adjacency");
}

size_t gnntrk_track_graph_distance_workspace_bytes(int64_t n, int32_t lds_hits) {
    return distance_ws_bytes(n, lds_hits < 1 || lds_hits > kLdsHits ? kLdsHits : lds_hits);
}

int gnntrk_track_graph_distance(int64_t *table, const int32_t *search, const int64_t *counts,
                                const int64_t *segment_labels, const int64_t *rowptr, const int32_t *neighbors, int64_t n,
                                const int64_t *seg_ptr, int32_t n_seg, void *workspace, size_t workspace_bytes,
                                void *stream) {
    return distance(table, search, counts, segment_labels, rowptr, neighbors, n, seg_ptr, n_seg, kLdsHits, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int gnntrk_track_graph_distance_ex(int64_t *table, const int32_t *search, const int64_t *counts,
                                   const int64_t *segment_labels, const int64_t *rowptr, const int32_t *neighbors,
                                   int64_t n, const int64_t *seg_ptr, int32_t n_seg, int32_t lds_hits, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return distance(table, search, counts, segment_labels, rowptr, neighbors, n, seg_ptr, n_seg, lds_hits, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
