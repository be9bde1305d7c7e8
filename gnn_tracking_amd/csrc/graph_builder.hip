// Geometric graph builder (graph_construction/graph_builder.py:162-394, 457-469): the edges between the hits of two
// layers that pass the cuts on phi slope, z0, dR and the intersecting-line cut, for a list of layer pairs, with the
// truth labels, their barrel-to-endcap correction and the counts of the measurement record.  The reference cross-joins
// the two layers in pandas, pair by pair; here a candidate pair costs one lane a few float64 operations and nothing is
// materialised but the edges that survive.
//
//   gnntrk_graph_builder_count  (hits)   gb_keys_kernel      key (event, layer) per hit; hits on a layer outside
//                                                            [0, GNNTRK_GB_MAX_LAYERS) are counted and are in no group
//                                        sort_pairs_u32      STABLE sort by key: hit index ascends inside a group
//                               (hits)   gb_groups_kernel    group offsets; r / phi / z (float32) and eta (float64, once
//                                                            per hit) in group order: a group's hits are contiguous
//                               (blocks) gb_blocks_kernel    a block is (event, layer pair): as many rows as layer 1
//                                                            has hits there, none when layer 2 has none
//                                        scan_counts_kernel  (knn.hip) row offset of every block
//                               (rows)   gb_rows_kernel<0>   a row is (event, layer pair, hit 1), ONE WAVE per row: the
//                                                            lanes test 64 hits of layer 2 at a time, in index order;
//                                                            the row's count is the sum of the ballots' popcounts
//                                        scan_counts_kernel  edge offset of every row; the total is head[0]
//   gnntrk_graph_builder_fill   (rows)   gb_rows_kernel<1>   the same traversal: a survivor's slot is the row's offset
//                                                            + the survivors of the earlier ballots + those of the
//                                                            lower lanes.  Ordered compaction, no atomics.
//   gnntrk_graph_builder_truth  (hits)   gb_particles_kernel particle table keyed by (event, int64 id), first hit
//                               (hits)   gb_layers_kernel    occupied layers per particle; hits per (particle, layer)
//                               (edges)  gb_transitions_kernel  per particle the set of barrel-to-endcap layer pairs among
//                                                            its true edges
//                               (edges)  gb_labels_kernel    relabelling, and the per-event edge counts
//                               (slots)  gb_truth_edges_kernel  products of hit counts on consecutive occupied layers
//
// Order of the edges: event, layer pair (the caller's list), hit 1, hit 2, the last two ascending in hit index - rows are
// numbered in that order and a row's edges are written in candidate order.  gb_rows_kernel<0> and <1> decide with the
// SAME function gb_pair on the same operands, so a row fills exactly the slots it counted; a slot is checked against
// n_edges all the same.  Every cut is evaluated in float64 from the float32 columns with IEEE division and square root
// (-ffp-contract=off: no fused multiply-add): dr == 0 gives inf or nan, which pass no cut.  The traversal reads the four
// group-ordered columns of layer 2 coalesced (64 consecutive hits per load) and every wave of a block of rows reads the
// same group: they are served from L2 after the first.  There is no LDS tile: at 3 000 hits per layer a group is 60 KB
// and stays in the 4 MB L2 of an XCD for the whole block.  The work is 15 float64 operations and two divisions per
// candidate, far below the device's rate at a few 10^8 candidates per event: the kernels are latency bound on the
// ballots, not on arithmetic.
//
// Counts (gb_labels_kernel, gb_truth_edges_kernel) are integers added with atomics: nothing depends on their order.
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "count_util.h"
#include "track_graph_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kWaves = kTpb / 64;
constexpr int kLayers = GNNTRK_GB_MAX_LAYERS;
constexpr int kMaxPairs = GNNTRK_GB_MAX_PAIRS;
constexpr int kCounts = GNNTRK_GB_COUNTS;
constexpr int kPt = 5;
constexpr double kPi = 3.141592653589793, kZEdge = 490.975;
// columns of a row of counts
enum { C_EDGES = 0, C_TRUE, C_TRUE_PT, C_CORRECTED = C_TRUE_PT + kPt, C_TRUTH, C_BAD_LAYER = C_TRUTH + kPt };
static_assert(C_BAD_LAYER + 1 == kCounts, "GNNTRK_GB_COUNTS");

struct Pairs {   // (a kernel argument by value)
    double radius[kMaxPairs];   // of the intersecting-line cut; 0: none
    uint8_t l1[kMaxPairs], l2[kMaxPairs];
    int32_t n;
};
struct GbCuts {
    double phi_slope_max, z0_max, dr_max;
    int32_t remove_intersecting;
};
struct PtCuts {
    float v[kPt];
};
constexpr PtCuts kPtCuts{{0.f, 0.1f, 0.5f, 0.9f, 1.0f}};

struct HitD {
    double r, phi, z, eta;
};

// THE predicate of a candidate pair (hit a on layer 1, hit b on layer 2) and its four attributes before scaling
__device__ __forceinline__ bool gb_pair(const HitD &a, const HitD &b, double radius, const GbCuts &c, double (&q)[4]) {
    double dphi = b.phi - a.phi;
    if (dphi > kPi) dphi -= 2.0 * kPi;
    if (dphi < -kPi) dphi += 2.0 * kPi;
    const double dz = b.z - a.z, dr = b.r - a.r, deta = b.eta - a.eta;
    const double dR = sqrt(deta * deta + dphi * dphi);
    const double phi_slope = dphi / dr;
    const double z0 = a.z - a.r * dz / dr;
    bool good = fabs(phi_slope) < c.phi_slope_max && fabs(z0) < c.z0_max && dR < c.dr_max;   // (nan: false)
    if (c.remove_intersecting && radius > 0.0) {
        const double z_coord = radius * dz / dr + z0;
        if (z_coord > -kZEdge && z_coord < kZEdge) good = false;
    }
    q[0] = dr;
    q[1] = dphi;
    q[2] = dz;
    q[3] = dR;
    return good;
}

// ------------------------------------------------------------------------------- workspace of count / fill
struct Ws {
    uint32_t *keys_a, *keys_b, *vals_a, *order;   // [n]; order: hit index of every place of the group order
    char *temp;                                   // of the sort
    size_t temp_bytes;
    int32_t *group_ptr;                           // [n_groups + 2]
    float *gr, *gphi, *gz;                        // [n] in group order
    double *geta;                                 // [n]
    int32_t *block_cnt;                           // [n_blocks]
    int64_t *block_ptr;                           // [n_blocks + 1]
    int32_t *row_cnt;                             // [max_rows]
    int64_t *row_off;                             // [max_rows + 1]
    int64_t n_groups, n_blocks, max_rows;
    size_t total;
};

// most rows a hit can start: the most pairs that share one layer 1
int rows_per_hit(const int32_t *pairs, int32_t n_pairs) {
    int most = 0, per[kLayers] = {};
    for (int p = 0; p < n_pairs; ++p) {
        const int32_t l = pairs[2 * p];
        if (l >= 0 && l < kLayers && ++per[l] > most) most = per[l];
    }
    return most;
}

Ws make_ws(void *base, int64_t n, int32_t n_seg, const int32_t *pairs, int32_t n_pairs) {
    Ws w{};
    const size_t N = (size_t)n;
    w.n_groups = (int64_t)n_seg * kLayers;
    w.n_blocks = (int64_t)n_seg * n_pairs;
    w.max_rows = n * rows_per_hit(pairs, n_pairs);
    Carver ws{(char *)base};
    w.keys_a = ws.take<uint32_t>(N);
    w.keys_b = ws.take<uint32_t>(N);
    w.vals_a = ws.take<uint32_t>(N);
    w.order = ws.take<uint32_t>(N);
    w.temp_bytes = sort_pairs_temp_bytes(n);
    w.temp = ws.take<char>(w.temp_bytes);
    w.group_ptr = ws.take<int32_t>((size_t)w.n_groups + 2);
    w.gr = ws.take<float>(N);
    w.gphi = ws.take<float>(N);
    w.gz = ws.take<float>(N);
    w.geta = ws.take<double>(N);
    w.block_cnt = ws.take<int32_t>((size_t)w.n_blocks + 4);
    w.block_ptr = ws.take<int64_t>((size_t)w.n_blocks + 1);
    w.row_cnt = ws.take<int32_t>((size_t)w.max_rows + 4);
    w.row_off = ws.take<int64_t>((size_t)w.max_rows + 1);
    w.total = ws.off;
    return w;
}

__global__ __launch_bounds__(kTpb) void gb_keys_kernel(const int64_t *__restrict__ layer, int64_t n, Events ev,
                                                       uint32_t n_groups, uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, unsigned long long *bad) {
    uint32_t nbad[1] = {0u};
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int64_t l = layer[i];
        uint32_t key = n_groups;   // (behind every group)
        if (l >= 0 && l < kLayers) key = (uint32_t)(ev.n > 1 ? segment_of(ev.ptr, ev.n, i) : 0) * kLayers + (uint32_t)l;
        else nbad[0] += 1u;
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    block_add(nbad, bad);
}

// over max(n, n_groups + 2) indices: group_ptr[g] = the first place whose key is >= g (g = n_groups: the hits that are
// in a group; g = n_groups + 1: n), and the columns of place j
__global__ __launch_bounds__(kTpb) void gb_groups_kernel(const float *__restrict__ x, int64_t x_stride, int64_t n,
                                                         const uint32_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ order, int64_t n_groups, Ws w) {
    const int64_t span = n > n_groups + 2 ? n : n_groups + 2;
    for (int64_t j = (int64_t)blockIdx.x * kTpb + threadIdx.x; j < span; j += (int64_t)gridDim.x * kTpb) {
        if (j < n_groups + 2) {
            int64_t lo = 0, hi = n;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)keys[mid] < j) lo = mid + 1; else hi = mid;
            }
            w.group_ptr[j] = (int32_t)lo;
        }
        if (j < n) {
            const float *row = x + (int64_t)order[j] * x_stride;
            const float r = row[0], z = row[2];
            w.gr[j] = r;
            w.gphi[j] = row[1];
            w.gz[j] = z;
            w.geta[j] = -log(tan(atan2((double)r, (double)z) / 2.0));
        }
    }
}

__global__ __launch_bounds__(kTpb) void gb_blocks_kernel(const int32_t *__restrict__ group_ptr, int64_t n_blocks, Pairs P,
                                                         int32_t *__restrict__ block_cnt) {
    for (int64_t b = (int64_t)blockIdx.x * kTpb + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * kTpb) {
        const int64_t e = b / P.n;
        const int p = (int)(b % P.n);
        const int64_t g1 = e * kLayers + P.l1[p], g2 = e * kLayers + P.l2[p];
        const int32_t n1 = group_ptr[g1 + 1] - group_ptr[g1], n2 = group_ptr[g2 + 1] - group_ptr[g2];
        block_cnt[b] = n2 > 0 ? n1 : 0;
    }
}

struct Out {   // of the fill
    const int64_t *pid;
    const float *pt;
    int64_t *edge_index;
    float *edge_attr, *y, *edge_pt;
    int64_t n_edges;
};

template <bool FILL>
__global__ __launch_bounds__(kTpb) void gb_rows_kernel(Ws w, Pairs P, GbCuts c, Out o) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * kWaves;
    const int64_t n_rows = w.block_ptr[w.n_blocks];   // (<= max_rows: every hit starts at most rows_per_hit rows)
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < n_rows; r += n_waves) {   // (uniform in the wave)
        const int64_t b = segment_of(w.block_ptr, (int)w.n_blocks, r);
        const int64_t e = b / P.n;
        const int p = (int)(b % P.n);
        const int64_t g1 = e * kLayers + P.l1[p], g2 = e * kLayers + P.l2[p];
        const int32_t j1 = w.group_ptr[g1] + (int32_t)(r - w.block_ptr[b]);
        const int32_t lo = w.group_ptr[g2], hi = w.group_ptr[g2 + 1];
        const HitD a{(double)w.gr[j1], (double)w.gphi[j1], (double)w.gz[j1], w.geta[j1]};
        const double radius = P.radius[p];
        const int64_t first = FILL ? w.row_off[r] : 0;
        const int64_t i1 = FILL ? (int64_t)w.order[j1] : 0;
        uint32_t total = 0;
        for (int32_t base = lo; base < hi; base += 64) {
            const int32_t j2 = base + lane;
            double q[4];
            bool ok = false;
            if (j2 < hi) {
                const HitD h{(double)w.gr[j2], (double)w.gphi[j2], (double)w.gz[j2], w.geta[j2]};
                ok = gb_pair(a, h, radius, c, q);
            }
            const unsigned long long m = __ballot(ok);
            if (FILL && ok) {
                const int64_t s = first + total + __popcll(m & below);
                if (s < o.n_edges) {   // (always: the row counted these survivors)
                    const int64_t i2 = (int64_t)w.order[j2];
                    o.edge_index[s] = i1;
                    o.edge_index[o.n_edges + s] = i2;
                    o.edge_attr[s] = (float)(q[0] / 1000.0);
                    o.edge_attr[o.n_edges + s] = (float)(q[1] / kPi);
                    o.edge_attr[2 * o.n_edges + s] = (float)(q[2] / 1000.0);
                    o.edge_attr[3 * o.n_edges + s] = (float)q[3];
                    const int64_t k = o.pid[i1];
                    o.y[s] = (k == o.pid[i2] && k > 0) ? 1.f : 0.f;
                    o.edge_pt[s] = o.pt[i1];
                }
            }
            total += (uint32_t)__popcll(m);
        }
        if (!FILL && lane == 0) w.row_cnt[r] = (int32_t)total;
    }
}

// edge_ptr[e] = the first edge of event e (e = n_seg: the number of edges)
__global__ __launch_bounds__(kTpb) void gb_edge_ptr_kernel(Ws w, int32_t n_seg, int32_t n_pairs,
                                                           int64_t *__restrict__ edge_ptr) {
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e <= n_seg; e += (int64_t)gridDim.x * kTpb)
        edge_ptr[e] = w.row_off[w.block_ptr[e * n_pairs]];
}

int rows_grid(int64_t max_rows) {
    const int64_t g = ceil_div(max_rows, kWaves), cap = (int64_t)cu_count() * 8;
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

// the checks that count and fill share; P and c filled from the caller's arrays
int check_build(const char *entry, const float *x, int64_t x_stride, const int64_t *layer, int64_t n,
                const int64_t *seg_ptr, int32_t n_seg, const int32_t *pairs, const double *radius, int32_t n_pairs,
                const double *cuts, Pairs &P, GbCuts &c) {
    char msg[200];
    int rc = check_count_i30(entry, "hit", n);
    if (rc || (rc = check_events(entry, seg_ptr, n_seg))) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !radius)) || !cuts) {
        snprintf(msg, sizeof(msg), "%s: NULL layer pairs, radii or cuts, or a negative number of pairs", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n_pairs > kMaxPairs) {
        snprintf(msg, sizeof(msg), "%s: %d layer pairs, at most %d", entry, (int)n_pairs, kMaxPairs);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    P = Pairs{};
    P.n = n_pairs;
    for (int p = 0; p < n_pairs; ++p) {
        const int32_t l1 = pairs[2 * p], l2 = pairs[2 * p + 1];
        if (l1 < 0 || l1 >= kLayers || l2 < 0 || l2 >= kLayers || !(radius[p] >= 0.0)) {
            snprintf(msg, sizeof(msg), "%s: pair %d = (%d, %d): layers must lie in [0, %d), radii be >= 0", entry, p, (int)l1,
                     (int)l2, kLayers);
            return fail(GNNTRK_EINVAL, msg);
        }
        P.l1[p] = (uint8_t)l1;
        P.l2[p] = (uint8_t)l2;
        P.radius[p] = radius[p];
    }
    c = GbCuts{cuts[0], cuts[1], cuts[2], cuts[3] != 0.0};
    if (n > 0 && (!x || !layer || x_stride < 3)) {
        snprintf(msg, sizeof(msg), "%s: NULL x or layer, or rows of fewer than 3 columns", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n > 0 && n * (int64_t)rows_per_hit(pairs, n_pairs) > 0x3fffffff) {
        snprintf(msg, sizeof(msg), "%s: %lld hits in up to %d pairs each; at most 2^30-1 rows", entry, (long long)n,
                 rows_per_hit(pairs, n_pairs));
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    return GNNTRK_OK;
}

// ----------------------------------------------------------------------------------------------- the truth
struct Tw {
    uint32_t *hslot;     // [n]   particle slot of every hit with id > 0
    int32_t *ptab;       // [S]   particle table: a hit + 1, 0 = empty
    uint32_t *pmask;     // [S]   barrel-to-endcap pairs among the particle's true edges: bit (l1 - 7) + 4 * (l2 == 11)
    uint32_t *lmask;     // [2S]  occupied layers
    int32_t *ctab;       // [S]   table of the pairs (particle, layer): a hit + 1
    uint32_t *ccnt;      // [S]   hits per pair
    int32_t *pfirst;     // [S]   first hit of the particle (cleared to 0x7f7f7f7f)
    size_t zero_from, first_from, total;
    uint64_t S;
};

Tw make_tw(void *base, int64_t n) {
    Tw w{};
    w.S = table_size(n);
    const size_t S = w.S;
    Carver ws{(char *)base};
    w.hslot = ws.take<uint32_t>((size_t)n);
    w.zero_from = ws.off;
    w.ptab = ws.take<int32_t>(S);
    w.pmask = ws.take<uint32_t>(S);
    w.lmask = ws.take<uint32_t>(2 * S);
    w.ctab = ws.take<int32_t>(S);
    w.ccnt = ws.take<uint32_t>(S);
    w.first_from = ws.off;
    w.pfirst = ws.take<int32_t>(S);
    w.total = ws.off;
    return w;
}

__device__ __forceinline__ int gb_event(const Events &ev, int64_t i) { return ev.n > 1 ? segment_of(ev.ptr, ev.n, i) : 0; }
__device__ __forceinline__ uint64_t gb_layer_hash(uint32_t s, int64_t l) { return mix64(((uint64_t)s << 32) ^ (uint64_t)l); }

__global__ __launch_bounds__(kTpb) void gb_particles_kernel(const int64_t *__restrict__ pid,
                                                            const int64_t *__restrict__ layer, int64_t n, Events ev, Tw w,
                                                            unsigned long long *counts) {
    const uint64_t smask = w.S - 1;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < n; base += (int64_t)gridDim.x * kTpb) {   // (uniform in the wave)
        const int64_t i = base + threadIdx.x;
        uint32_t bad[1] = {0u};
        int e = 0;
        if (i < n) {
            const int64_t key = pid[i], l = layer[i];
            int64_t lo, hi;
            e = tg_event_rows(ev, n, i, lo, hi);
            bad[0] = (l < 0 || l >= kLayers) ? 1u : 0u;
            if (key > 0) {
                const uint64_t s = table_claim(w.ptab, smask, particle_hash<true>(key, e), i,
                                               [&](int32_t h) { return pid[h] == key; },
                                               [&](int32_t h) { return h >= lo && h < hi; });
                w.hslot[i] = (uint32_t)s;
                atomicMin(&w.pfirst[s], (int32_t)i);
                if (!bad[0]) atomicOr(&w.lmask[2 * s + (l >> 5)], 1u << (l & 31));
            }
        }
        event_add(bad, e, counts + C_BAD_LAYER, kCounts);
    }
}

__global__ __launch_bounds__(kTpb) void gb_layers_kernel(const int64_t *__restrict__ pid, const int64_t *__restrict__ layer,
                                                         int64_t n, Tw w) {
    const uint64_t smask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int64_t l = layer[i];
        if (pid[i] <= 0 || l < 0 || l >= kLayers) continue;
        const uint32_t s = w.hslot[i];
        const uint64_t cs = table_claim(w.ctab, smask, gb_layer_hash(s, l), i,
                                        [&](int32_t h) { return w.hslot[h] == s && layer[h] == l; });
        atomicAdd(&w.ccnt[cs], 1u);
    }
}

// the transition bit of a true edge a -> b, or -1: y == 1, both ends hits, the id of a > 0, a barrel layer 7..10 to 6 / 11
__device__ __forceinline__ int gb_transition(const int64_t *__restrict__ ei, int64_t m, int64_t e,
                                             const float *__restrict__ y, const int64_t *__restrict__ pid,
                                             const int64_t *__restrict__ layer, int64_t n, int64_t &a) {
    a = ei[e];
    const int64_t b = ei[m + e];
    if (!(y[e] == 1.f) || a < 0 || a >= n || b < 0 || b >= n || pid[a] <= 0) return -1;
    const int64_t la = layer[a], lb = layer[b];
    if (la < 7 || la > 10 || (lb != 6 && lb != 11)) return -1;
    return (int)(la - 7) + (lb == 11 ? 4 : 0);
}

__global__ __launch_bounds__(kTpb) void gb_transitions_kernel(const int64_t *__restrict__ ei, int64_t m,
                                                              const float *__restrict__ y,
                                                              const int64_t *__restrict__ pid,
                                                              const int64_t *__restrict__ layer, int64_t n, Tw w) {
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < m; e += (int64_t)gridDim.x * kTpb) {
        int64_t a;
        const int bit = gb_transition(ei, m, e, y, pid, layer, n, a);
        if (bit >= 0) atomicOr(&w.pmask[w.hslot[a]], 1u << bit);
    }
}

__global__ __launch_bounds__(kTpb) void gb_labels_kernel(const int64_t *__restrict__ ei, int64_t m, float *__restrict__ y,
                                                         const float *__restrict__ edge_pt,
                                                         const int64_t *__restrict__ pid,
                                                         const int64_t *__restrict__ layer, int64_t n, Events ev, Tw w,
                                                         int relabel, PtCuts cuts, unsigned long long *counts) {
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {   // (uniform in the wave)
        const int64_t e = base + threadIdx.x;
        uint32_t v[C_CORRECTED + 1] = {};
        int event = 0;
        if (e < m) {
            int64_t a;
            const int bit = gb_transition(ei, m, e, y, pid, layer, n, a);
            if (relabel && bit >= 0) {
                const uint32_t pm = w.pmask[w.hslot[a]];
                const uint32_t prec = (pm | (pm >> 4)) & 15u;   // the precedences present: both endcaps share one scale
                if (__popc(pm) > 1 && (prec >> ((bit & 3) + 1)) != 0u) {
                    y[e] = 0.f;
                    v[C_CORRECTED] = 1u;
                }
            }
            event = gb_event(ev, a < 0 ? 0 : (a >= n ? n - 1 : a));
            v[C_EDGES] = 1u;
            if (y[e] == 1.f) {
                v[C_TRUE] = 1u;
                const float pt = edge_pt[e];
                for (int k = 0; k < kPt; ++k) v[C_TRUE_PT + k] = pt > cuts.v[k] ? 1u : 0u;
            }
        }
        event_add(v, event, counts, kCounts);
    }
}

__global__ __launch_bounds__(kTpb) void gb_truth_edges_kernel(const int64_t *__restrict__ layer,
                                                              const float *__restrict__ pt, Events ev, Tw w, PtCuts cuts,
                                                              unsigned long long *counts) {
    const int64_t S = (int64_t)w.S;
    const uint64_t smask = w.S - 1;
    for (int64_t cs = (int64_t)blockIdx.x * kTpb + threadIdx.x; cs < S; cs += (int64_t)gridDim.x * kTpb) {
        const int32_t h = w.ctab[cs];
        if (h == 0) continue;
        const uint32_t s = w.hslot[h - 1];
        const int l = (int)layer[h - 1];
        // the next occupied layer above l
        uint64_t occ = ((uint64_t)w.lmask[2 * s + 1] << 32) | w.lmask[2 * s];
        occ = l >= 63 ? 0ull : occ >> (l + 1);
        if (occ == 0ull) continue;
        const int64_t l2 = l + 1 + __builtin_ctzll(occ);
        const uint64_t cs2 = table_find(w.ctab, smask, gb_layer_hash(s, l2),
                                        [&](int32_t g) { return w.hslot[g] == s && layer[g] == l2; });
        const unsigned long long prod = (unsigned long long)w.ccnt[cs] * (unsigned long long)w.ccnt[cs2];
        const int32_t first = w.pfirst[s];
        const float p = pt[first];
        unsigned long long *row = counts + (size_t)gb_event(ev, first) * kCounts + C_TRUTH;
        for (int k = 0; k < kPt; ++k)
            if (p > cuts.v[k]) atomicAdd(&row[k], prod);
    }
}

}  // namespace
}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_graph_builder_count_workspace_bytes(int64_t n, int32_t n_seg, const int32_t *pairs, int32_t n_pairs) {
    if (n <= 0 || n_seg < 1 || n_pairs < 1 || n_pairs > kMaxPairs || !pairs) return 0;
    return make_ws(nullptr, n, n_seg, pairs, n_pairs).total;
}

int gnntrk_graph_builder_count(const float *x, int64_t x_stride, const int64_t *layer, int64_t n, const int64_t *seg_ptr,
                               int32_t n_seg, const int32_t *pairs, const double *radius, int32_t n_pairs,
                               const double *cuts, int64_t *head, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Pairs P;
    GbCuts c;
    int rc = check_build("graph_builder_count", x, x_stride, layer, n, seg_ptr, n_seg, pairs, radius, n_pairs, cuts, P, c);
    if (rc) return rc;
    if (!head) return fail(GNNTRK_EINVAL, "graph_builder_count: NULL head");
    rc = check_hip(hipMemsetAsync(head, 0, 2 * sizeof(int64_t), stream), "graph_builder_count: clear");
    if (rc || n == 0 || n_pairs == 0) return rc;   // (no pair, no edge: the layers are not looked at)
    auto *bad = reinterpret_cast<unsigned long long *>(head + 1);
    const Events ev{seg_ptr, n_seg};
    const Ws w = make_ws(workspace, n, n_seg, pairs, n_pairs);
    if ((rc = check_workspace("graph_builder_count", workspace, workspace_bytes, w.total))) return rc;
    int bits = 1;
    while ((1ull << bits) <= (unsigned long long)w.n_groups) ++bits;
    launch(gb_keys_kernel, blocks_for(n, 8), kTpb, stream, layer, n, ev, (uint32_t)w.n_groups, w.keys_a, w.vals_a, bad);
    if ((rc = sort_pairs_u32(w.keys_a, w.keys_b, w.vals_a, w.order, n, bits, w.temp, w.temp_bytes, stream))) return rc;
    const int64_t span = n > w.n_groups + 2 ? n : w.n_groups + 2;
    launch(gb_groups_kernel, blocks_for(span, 8), kTpb, stream, x, x_stride, n, (const uint32_t *)w.keys_b,
           (const uint32_t *)w.order, w.n_groups, w);
    launch(gb_blocks_kernel, blocks_for(w.n_blocks, 8), kTpb, stream, (const int32_t *)w.group_ptr, w.n_blocks, P,
           w.block_cnt);
    scan_counts_launch(w.block_cnt, INT_MAX, w.n_blocks, w.block_ptr, stream);
    if ((rc = check_hip(hipMemsetAsync(w.row_cnt, 0, sizeof(int32_t) * (size_t)w.max_rows, stream),
                        "graph_builder_count: clear rows")))
        return rc;
    launch(gb_rows_kernel<false>, rows_grid(w.max_rows), kTpb, stream, w, P, c, Out{});
    scan_counts_launch(w.row_cnt, INT_MAX, w.max_rows, w.row_off, stream);
    if ((rc = check_hip(hipMemcpyAsync(head, w.row_off + w.max_rows, sizeof(int64_t), hipMemcpyDeviceToDevice, stream),
                        "graph_builder_count: total")))
        return rc;
    return check_launch("graph_builder_count");
}

int gnntrk_graph_builder_fill(const float *x, int64_t x_stride, const int64_t *layer, const int64_t *particle_id,
                              const float *pt, int64_t n, const int64_t *seg_ptr, int32_t n_seg, const int32_t *pairs,
                              const double *radius, int32_t n_pairs, const double *cuts, int64_t n_edges,
                              int64_t *edge_index, float *edge_attr, float *y, float *edge_pt, int64_t *edge_ptr,
                              void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Pairs P;
    GbCuts c;
    int rc = check_build("graph_builder_fill", x, x_stride, layer, n, seg_ptr, n_seg, pairs, radius, n_pairs, cuts, P, c);
    if (rc) return rc;
    if (n_edges < 0) return fail(GNNTRK_EINVAL, "graph_builder_fill: negative edge count");
    if (n_edges > 0x3fffffff) return fail(GNNTRK_EUNSUPPORTED, "graph_builder_fill: at most 2^30-1 edges");
    if (!edge_ptr) return fail(GNNTRK_EINVAL, "graph_builder_fill: NULL edge_ptr");
    if (n == 0 || n_pairs == 0) {
        if (n_edges > 0) return fail(GNNTRK_EINVAL, "graph_builder_fill: edges without hits or layer pairs");
        return check_hip(hipMemsetAsync(edge_ptr, 0, sizeof(int64_t) * ((size_t)n_seg + 1), stream),
                         "graph_builder_fill: clear");
    }
    if (!particle_id || !pt || (n_edges > 0 && (!edge_index || !edge_attr || !y || !edge_pt)))
        return fail(GNNTRK_EINVAL, "graph_builder_fill: NULL particle ids, pt, edge_index, edge_attr, y or edge_pt");
    const Ws w = make_ws(workspace, n, n_seg, pairs, n_pairs);
    if ((rc = check_workspace("graph_builder_fill", workspace, workspace_bytes, w.total))) return rc;
    if (n_edges > 0)
        launch(gb_rows_kernel<true>, rows_grid(w.max_rows), kTpb, stream, w, P, c,
               Out{particle_id, pt, edge_index, edge_attr, y, edge_pt, n_edges});
    launch(gb_edge_ptr_kernel, blocks_for((int64_t)n_seg + 1, 8), kTpb, stream, w, n_seg, n_pairs, edge_ptr);
    return check_launch("graph_builder_fill");
}

size_t gnntrk_graph_builder_truth_workspace_bytes(int64_t n) { return make_tw(nullptr, n < 0 ? 0 : n).total; }

int gnntrk_graph_builder_truth(const int64_t *edge_index, int64_t n_edges, float *y, const float *edge_pt,
                               const int64_t *layer, const int64_t *particle_id, const float *pt, int64_t n,
                               const int64_t *seg_ptr, int32_t n_seg, int32_t relabel, int64_t *counts, void *workspace,
                               size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_count_i30("graph_builder_truth", "hit", n);
    if (rc || (rc = check_events("graph_builder_truth", seg_ptr, n_seg))) return rc;
    if (n_edges < 0) return fail(GNNTRK_EINVAL, "graph_builder_truth: negative edge count");
    if (n_edges > 0x3fffffff) return fail(GNNTRK_EUNSUPPORTED, "graph_builder_truth: at most 2^30-1 edges");
    if (!counts) return fail(GNNTRK_EINVAL, "graph_builder_truth: NULL counts");
    if ((n > 0 && (!layer || !particle_id || !pt)) || (n_edges > 0 && (!edge_index || !y || !edge_pt)))
        return fail(GNNTRK_EINVAL, "graph_builder_truth: NULL layers, particle ids, pt, edge_index, y or edge_pt");
    if (n == 0 && n_edges > 0) return fail(GNNTRK_EINVAL, "graph_builder_truth: edges without hits");
    rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * kCounts * (size_t)n_seg, stream), "graph_builder_truth: clear");
    if (rc || n == 0) return rc;
    const Tw w = make_tw(workspace, n);
    if ((rc = check_workspace("graph_builder_truth", workspace, workspace_bytes, w.total))) return rc;
    char *base = (char *)workspace;
    if ((rc = check_hip(hipMemsetAsync(base + w.zero_from, 0, w.first_from - w.zero_from, stream),
                        "graph_builder_truth: clear workspace")) ||
        (rc = check_hip(hipMemsetAsync(base + w.first_from, 0x7f, w.total - w.first_from, stream),
                        "graph_builder_truth: clear workspace")))
        return rc;
    const Events ev{seg_ptr, n_seg};
    auto *cnt = reinterpret_cast<unsigned long long *>(counts);
    const int gn = blocks_for(n, 8), gm = blocks_for(n_edges, 8), gs = blocks_for((int64_t)w.S, 8);
    launch(gb_particles_kernel, gn, kTpb, stream, particle_id, layer, n, ev, w, cnt);
    launch(gb_layers_kernel, gn, kTpb, stream, particle_id, layer, n, w);
    if (n_edges > 0) {
        if (relabel)
            launch(gb_transitions_kernel, gm, kTpb, stream, edge_index, n_edges, (const float *)y, particle_id, layer, n, w);
        launch(gb_labels_kernel, gm, kTpb, stream, edge_index, n_edges, y, edge_pt, particle_id, layer, n, ev, w,
               (int)(relabel != 0), kPtCuts, cnt);
    }
    launch(gb_truth_edges_kernel, gs, kTpb, stream, layer, pt, ev, w, kPtCuts, cnt);
    return check_launch("graph_builder_truth");
}

}  // extern "C"
