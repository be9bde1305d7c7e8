// Point cloud builder (preprocessing/point_cloud_builder.py:156-353, 397-450; exatrkx_cell_features.py:174-250): the
// four tables of a TrackML event (hits, cells, particles, truth) and the detector's module table to the sector point
// clouds that the graph builder and the learned graph construction read.  The reference is a chain of pandas merges and
// group-bys and a Python loop over the particle ids of every sector; here every step is a flat pass over one table.
//
//   gnntrk_point_cloud_select   (hits)      pc_hit_table_kernel    hit_id -> hit (open-addressing table), the hit's layer,
//                                                                  duplicate ids counted
//                               (particles) pc_particle_table_kernel  particle_id -> row of the particle table
//                               (truth)     pc_truth_kernel        truth row of every hit (join by hit_id)
//                               (cells)     pc_cell_keys_kernel    hit of every cell (join by hit_id)
//                                           sort_pairs_u32         STABLE: a hit's cells contiguous, in cell order
//                               (hits)      pc_hit_reduce_kernel   ONE THREAD per hit walks its cells in order: count,
//                                                                  float64 sum, min / max of ch0, ch1; the particle join
//                                                                  and the keep flag
//                                           compact_bytes_launch   kept hits in hit order (compact.hip)
//                               (kept)      pc_particle_counts_kernel  n_hits and the layer_id bit mask per particle
//                               (kept)      pc_rows_kernel         the feature row (float64, one rounding) and the
//                                                                  truth columns of every kept hit; the event's counts
//   gnntrk_point_cloud_sectors  (kept x sectors) pc_sector_flags_kernel  THE predicate pc_wedges of a (hit, sector);
//                                                                  integer counts per (particle, sector)
//                                           compact_bytes_launch   rows of all clouds, sector-major, in hit order
//                               (particles x sectors) pc_sector_finish_kernel  the per-sector integers of the records
//   gnntrk_point_cloud_gather   (rows)      pc_gather_kernel       the clouds' columns and the `sector` column
//   gnntrk_truth_edges_count    (hits)      te_slots_kernel<1>     pairs per segment: a hit adds the number of earlier
//                                                                  claims of its particle
//   gnntrk_truth_edges_fill     (hits)      te_slots_kernel<0>     key = the particle's slot
//                                           sort_pairs_u32         STABLE: a particle's hits contiguous, ascending
//                               (hits)      te_ranks_kernel        pairs a hit starts = its later partners
//                                           scan_counts_kernel     (knn.hip) offset of every hit's pairs
//                               (hits)      te_fill_kernel         (i, j), i < j, lexicographic: rows in hit order, a row's
//                                                                  partners ascending
//
// Nothing here is arithmetic bound: a full event is 1.2e5 hits and 6e5 cells, every pass reads or writes a few MB.
// All joins are by key (hit_id, particle_id: int64, compared exactly), never by position.  The sums over a hit's cells
// are sequential in one thread, in cell order: no floating-point atomics, bit-identical from run to run.  Every other
// atomic adds or ors integers, whose result does not depend on the order.  The sector predicate uses float64 + - * only
// (-ffp-contract=off: no fused multiply-add) on constants that the host computed with numpy, so membership is the
// reference's bit for bit.
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "count_util.h"
#include "track_graph_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kMaxF = GNNTRK_PC_MAX_FEATURES;
constexpr int kIds = GNNTRK_PC_MAX_IDS;   // volume_id and layer_id lie in [0, kIds)
constexpr int kHead = GNNTRK_PC_HEAD;
constexpr int kSecCounts = GNNTRK_PC_SECTOR_COUNTS;
enum { H_KEPT = 0, H_DUP_HIT, H_NO_CELL, H_NO_MODULE, H_BAD_ID, H_DUP_TRUTH, H_DUP_PARTICLE, H_PARTICLES, H_NOISE };
enum { S_WEDGE = 0, S_EXT, S_UNIQUE, S_MAJ_NUM, S_MAJ_DEN, S_PAIRS };
static_assert(H_NOISE < kHead && S_PAIRS < kSecCounts, "GNNTRK_PC_HEAD / GNNTRK_PC_SECTOR_COUNTS");
enum {
    F_X = 0, F_Y, F_Z, F_R, F_PHI, F_ETA_RZ, F_U, F_V, F_CHARGE_FRAC, F_CELL_COUNT, F_CELL_VAL, F_LETA, F_LPHI, F_LX,
    F_LY, F_LZ, F_GETA, F_GPHI, F_VOLUME, F_END = F_VOLUME + 9
};
static_assert(F_END == GNNTRK_PC_FEATURE_CODES, "GNNTRK_PC_FEATURE_CODES");

struct Features {   // (a kernel argument by value)
    double scale[kMaxF];
    int32_t code[kMaxF];
    int32_t n;
};
struct VolumeIds {
    int32_t v[9];
};
constexpr VolumeIds kVolumes{{7, 8, 9, 12, 13, 14, 16, 17, 18}};

__device__ __forceinline__ uint64_t id_hash(int64_t id) { return mix64((uint64_t)id); }
__device__ __forceinline__ double calc_eta(double r, double z) { return -log(tan(atan2(r, z) / 2.0)); }

// ------------------------------------------------------------------------------------ workspace of the selection
struct Ws {
    int32_t *htab, *ptab;              // [SH], [SP]   hit_id -> hit + 1, particle_id -> row + 1
    int32_t *htruth;                   // [H]   truth row of the hit, -1: none
    int32_t *hlayer;                   // [H]   layer, -1: none
    uint32_t *keys_a, *keys_b, *vals_a, *corder;   // [C]  cell sort: key = hit (H: none)
    char *temp;
    size_t temp_bytes;
    double *csum;                      // [H]
    int32_t *ccount, *cnu, *cnv;       // [H]   cells, extent of ch0 / ch1
    int32_t *pslot;                    // [H]   row of the hit's particle (P: noise)
    uint8_t *keep;                     // [H]
    int32_t *kidx;                     // [H]   kept hits, ascending
    uint32_t *pcnt, *lmask;            // [P + 1], [2 (P + 1)]
    char *cws;                         // of the compaction
    size_t cws_bytes, zero_from, zero_to, total;
    uint64_t SH, SP;
};

Ws make_ws(void *base, int64_t H, int64_t Cn, int64_t P) {
    Ws w{};
    w.SH = table_size(H);
    w.SP = table_size(P);
    Carver ws{(char *)base};
    w.zero_from = ws.off;
    w.htab = ws.take<int32_t>(w.SH);
    w.ptab = ws.take<int32_t>(w.SP);
    w.pcnt = ws.take<uint32_t>((size_t)P + 1);
    w.lmask = ws.take<uint32_t>(2 * ((size_t)P + 1));
    w.zero_to = ws.off;
    w.htruth = ws.take<int32_t>((size_t)H);
    w.hlayer = ws.take<int32_t>((size_t)H);
    w.keys_a = ws.take<uint32_t>((size_t)Cn + 1);
    w.keys_b = ws.take<uint32_t>((size_t)Cn + 1);
    w.vals_a = ws.take<uint32_t>((size_t)Cn + 1);
    w.corder = ws.take<uint32_t>((size_t)Cn + 1);
    w.temp_bytes = sort_pairs_temp_bytes(Cn > 0 ? Cn : 1);
    w.temp = ws.take<char>(w.temp_bytes);
    w.csum = ws.take<double>((size_t)H);
    w.ccount = ws.take<int32_t>((size_t)H);
    w.cnu = ws.take<int32_t>((size_t)H);
    w.cnv = ws.take<int32_t>((size_t)H);
    w.pslot = ws.take<int32_t>((size_t)H);
    w.keep = ws.take<uint8_t>((size_t)H + 8);
    w.kidx = ws.take<int32_t>((size_t)H);
    w.cws_bytes = compact_ws_bytes(H);
    w.cws = ws.take<char>(w.cws_bytes);
    w.total = ws.off;
    return w;
}

__global__ __launch_bounds__(kTpb) void pc_hit_table_kernel(const int64_t *__restrict__ hit_id,
                                                            const int32_t *__restrict__ vlm, int64_t H,
                                                            const int32_t *__restrict__ layer_map, Ws w,
                                                            unsigned long long *head) {
    const uint64_t mask = w.SH - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < H; i += (int64_t)gridDim.x * kTpb) {
        const int64_t key = hit_id[i];
        const uint64_t s = table_claim(w.htab, mask, id_hash(key), i, [&](int32_t h) { return hit_id[h] == key; });
        if (load_i32(&w.htab[s]) != (int32_t)(i + 1)) atomicAdd(&head[H_DUP_HIT], 1ull);
        const int32_t v = vlm[3 * i], l = vlm[3 * i + 1];
        int32_t layer = -1;
        if (v < 0 || v >= kIds || l < 0 || l >= kIds) atomicAdd(&head[H_BAD_ID], 1ull);
        else layer = layer_map[v * kIds + l];
        w.hlayer[i] = layer;
    }
}

__global__ __launch_bounds__(kTpb) void pc_particle_table_kernel(const int64_t *__restrict__ part_id, int64_t P, Ws w,
                                                                 unsigned long long *head) {
    const uint64_t mask = w.SP - 1;
    for (int64_t p = (int64_t)blockIdx.x * kTpb + threadIdx.x; p < P; p += (int64_t)gridDim.x * kTpb) {
        const int64_t key = part_id[p];
        const uint64_t s = table_claim(w.ptab, mask, id_hash(key), p, [&](int32_t h) { return part_id[h] == key; });
        if (load_i32(&w.ptab[s]) != (int32_t)(p + 1)) atomicAdd(&head[H_DUP_PARTICLE], 1ull);
    }
}

// the hit with this id, or -1
__device__ __forceinline__ int32_t pc_find_hit(const Ws &w, const int64_t *__restrict__ hit_id, int64_t key) {
    const uint64_t s = table_find(w.htab, w.SH - 1, id_hash(key), [&](int32_t h) { return hit_id[h] == key; });
    return w.htab[s] - 1;
}

__global__ __launch_bounds__(kTpb) void pc_truth_kernel(const int64_t *__restrict__ truth_hit,
                                                        const int64_t *__restrict__ hit_id, int64_t T, Ws w,
                                                        unsigned long long *head) {
    for (int64_t t = (int64_t)blockIdx.x * kTpb + threadIdx.x; t < T; t += (int64_t)gridDim.x * kTpb) {
        const int32_t h = pc_find_hit(w, hit_id, truth_hit[t]);
        if (h < 0) continue;
        if (cas_i32(&w.htruth[h], -1, (int32_t)t) != -1) atomicAdd(&head[H_DUP_TRUTH], 1ull);
    }
}

__global__ __launch_bounds__(kTpb) void pc_cell_keys_kernel(const int64_t *__restrict__ cell_hit,
                                                            const int64_t *__restrict__ hit_id, int64_t Cn, int64_t H, Ws w) {
    for (int64_t c = (int64_t)blockIdx.x * kTpb + threadIdx.x; c < Cn; c += (int64_t)gridDim.x * kTpb) {
        const int32_t h = pc_find_hit(w, hit_id, cell_hit[c]);
        w.keys_a[c] = h < 0 ? (uint32_t)H : (uint32_t)h;
        w.vals_a[c] = (uint32_t)c;
    }
}

// first place of the sorted keys that is >= key
__device__ __forceinline__ int64_t lower_bound_u32(const uint32_t *__restrict__ keys, int64_t n, uint32_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kTpb) void pc_hit_reduce_kernel(const int32_t *__restrict__ cell_ch,
                                                             const double *__restrict__ cell_value, int64_t Cn,
                                                             const int64_t *__restrict__ truth_pid,
                                                             const int64_t *__restrict__ part_id, int64_t H, int64_t P,
                                                             int remove_noise, Ws w, unsigned long long *head) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < H; i += (int64_t)gridDim.x * kTpb) {
        uint8_t keep = 0;
        if (w.hlayer[i] >= 0) {   // (the reference aggregates the cells of every hit on a layer)
            int64_t c = lower_bound_u32(w.keys_b, Cn, (uint32_t)i);
            double sum = 0.0;
            int32_t n = 0, u0 = INT_MAX, u1 = INT_MIN, v0 = INT_MAX, v1 = INT_MIN;
            for (; c < Cn && w.keys_b[c] == (uint32_t)i; ++c, ++n) {   // in cell order: the sort is stable
                const uint32_t cell = w.corder[c];
                const int32_t a = cell_ch[2 * (size_t)cell], b = cell_ch[2 * (size_t)cell + 1];
                sum += cell_value[cell];
                u0 = a < u0 ? a : u0;
                u1 = a > u1 ? a : u1;
                v0 = b < v0 ? b : v0;
                v1 = b > v1 ? b : v1;
            }
            if (n == 0) atomicAdd(&head[H_NO_CELL], 1ull);
            w.csum[i] = sum;
            w.ccount[i] = n;
            w.cnu[i] = n ? u1 - u0 + 1 : 0;
            w.cnv[i] = n ? v1 - v0 + 1 : 0;
            const int32_t t = w.htruth[i];
            if (t >= 0) {
                const int64_t key = truth_pid[t];
                if (key == 0) {
                    keep = remove_noise ? 0 : 1;
                    w.pslot[i] = (int32_t)P;
                } else if (P > 0) {
                    const uint64_t s = table_find(w.ptab, w.SP - 1, id_hash(key), [&](int32_t h) { return part_id[h] == key; });
                    const int32_t p = w.ptab[s] - 1;
                    keep = p >= 0;
                    w.pslot[i] = p;
                }
            }
        }
        w.keep[i] = keep;
    }
}

__global__ __launch_bounds__(kTpb) void pc_particle_counts_kernel(const int32_t *__restrict__ vlm, int64_t H, Ws w,
                                                                  const int64_t *__restrict__ n_kept) {
    const int64_t n = n_kept[0] < H ? n_kept[0] : H;
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k < n; k += (int64_t)gridDim.x * kTpb) {
        const int32_t i = w.kidx[k], s = w.pslot[i], l = vlm[3 * (size_t)i + 1];   // (0 <= l < kIds: the hit has a layer)
        atomicAdd(&w.pcnt[s], 1u);
        atomicOr(&w.lmask[2 * (size_t)s + (l >> 5)], 1u << (l & 31));
    }
}

struct Rows {   // the columns of the kept hits, every one with room for all hits
    float *x;          // [H][n_feat]
    int64_t *cols;     // [GNNTRK_PC_COLUMNS][H]: layer, particle_id, reconstructable, n_hits, n_layers_hit, hit
    float *pt_eta;     // [2][H]
    double *uv;        // [H][2]
    int32_t *slot;     // [H]
};

__device__ __forceinline__ void spherical(double x, double y, double z, double &eta, double &phi) {
    const double r3 = sqrt(x * x + y * y + z * z);
    phi = atan2(y, x);
    eta = -log(tan(0.5 * acos(z / r3)));
}

__global__ __launch_bounds__(kTpb) void pc_rows_kernel(const double *__restrict__ xyz, const int32_t *__restrict__ vlm,
                                                       int64_t H, const int64_t *__restrict__ truth_pid,
                                                       const double *__restrict__ part_p, int64_t P,
                                                       const int32_t *__restrict__ det_index, int32_t nv, int32_t nl,
                                                       int32_t nm, const double *__restrict__ det_rows, Features F,
                                                       VolumeIds vol, Ws w, Rows o, unsigned long long *head) {
    const int64_t n = (int64_t)head[H_KEPT] < H ? (int64_t)head[H_KEPT] : H;
    const int64_t span = n > P + 1 ? n : P + 1;
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k < span; k += (int64_t)gridDim.x * kTpb) {
        if (k <= P && w.pcnt[k] > 0u) {   // the particles of the event (noise is one), and its noise hits
            atomicAdd(&head[H_PARTICLES], 1ull);
            if (k == P) atomicAdd(&head[H_NOISE], (unsigned long long)w.pcnt[k]);
        }
        if (k >= n) continue;
        const int32_t i = w.kidx[k], s = w.pslot[i];
        const double x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        const int32_t v = vlm[3 * (size_t)i], l = vlm[3 * (size_t)i + 1], m = vlm[3 * (size_t)i + 2];
        int32_t row = -1;
        if (v < nv && l < nl && m >= 0 && m < nm) row = det_index[((size_t)v * nl + l) * nm + m];
        double d[12] = {};
        if (row >= 0)
            for (int q = 0; q < 12; ++q) d[q] = det_rows[12 * (size_t)row + q];
        else atomicAdd(&head[H_NO_MODULE], 1ull);
        const double r2 = x * x + y * y, r = sqrt(r2), u = x / r2, vv = y / r2;
        const double sum = w.csum[i], cnt = (double)w.ccount[i];
        const double lu = (double)w.cnu[i] * d[10], lv = (double)w.cnv[i] * d[11], lw = 2.0 * d[9];
        const double gx = d[0] * lu + d[1] * lv + d[2] * lw, gy = d[3] * lu + d[4] * lv + d[5] * lw,
                     gz = d[6] * lu + d[7] * lv + d[8] * lw;
        double leta, lphi, geta, gphi;
        spherical(lu, lv, lw, leta, lphi);
        spherical(gx, gy, gz, geta, gphi);
        for (int f = 0; f < F.n; ++f) {
            double q;
            switch (F.code[f]) {
                case F_X: q = x; break;
                case F_Y: q = y; break;
                case F_Z: q = z; break;
                case F_R: q = r; break;
                case F_PHI: q = atan2(y, x); break;
                case F_ETA_RZ: q = calc_eta(r, z); break;
                case F_U: q = u; break;
                case F_V: q = vv; break;
                case F_CHARGE_FRAC: q = sum / cnt; break;
                case F_CELL_COUNT: q = cnt; break;
                case F_CELL_VAL: q = (double)(float)sum; break;   // (the reference keeps it as float32)
                case F_LETA: q = leta; break;
                case F_LPHI: q = lphi; break;
                case F_LX: q = lu; break;
                case F_LY: q = lv; break;
                case F_LZ: q = lw; break;
                case F_GETA: q = geta; break;
                case F_GPHI: q = gphi; break;
                default: q = v == vol.v[F.code[f] - F_VOLUME] ? 1.0 : 0.0;
            }
            o.x[(size_t)k * F.n + f] = (float)(q / F.scale[f]);
        }
        double pt = 0.0, eta = NAN;   // noise: pt 0, eta missing (the reference's concat leaves it NaN)
        if (s < P) {
            const double px = part_p[3 * (size_t)s], py = part_p[3 * (size_t)s + 1];
            pt = sqrt(px * px + py * py);
            eta = calc_eta(pt, part_p[3 * (size_t)s + 2]);
        }
        const int64_t n_layers = __popc(w.lmask[2 * (size_t)s]) + __popc(w.lmask[2 * (size_t)s + 1]);
        const int64_t key = truth_pid[w.htruth[i]];
        o.cols[k] = w.hlayer[i];
        o.cols[H + k] = key;
        o.cols[2 * H + k] = (n_layers >= 3 && key > 0) ? 1 : 0;
        o.cols[3 * H + k] = w.pcnt[s];
        o.cols[4 * H + k] = n_layers;
        o.cols[5 * H + k] = i;
        o.pt_eta[k] = (float)pt;
        o.pt_eta[H + k] = (float)eta;
        o.uv[2 * (size_t)k] = u;
        o.uv[2 * (size_t)k + 1] = vv;
        o.slot[k] = s;
    }
}

// ---------------------------------------------------------------------------------------------------- sectors
struct Wedge {   // slope = arctan(pi / n_sectors), ext = sector_ds * slope, di = sector_di, thld; single: one sector
    double slope, ext, di, thld;
    int32_t single;
};

struct Sw {
    uint32_t *cnt4;      // [(P + 1) S][4]  hits of (particle, sector): wedge, extended, both without the ur > 0 term
    uint8_t *flags;      // [S cap]
    int32_t *rows;       // [S cap]         s * cap + kept hit, ascending
    char *cws;
    size_t cws_bytes, zero_to, total;
};

Sw make_sw(void *base, int64_t cap, int64_t P, int32_t S) {
    Sw w{};
    Carver ws{(char *)base};
    w.cnt4 = ws.take<uint32_t>(4 * ((size_t)P + 1) * S);
    w.flags = ws.take<uint8_t>((size_t)cap * S + 8);
    w.zero_to = ws.off;
    w.rows = ws.take<int32_t>((size_t)cap * S);
    w.cws_bytes = compact_ws_bytes(cap * S);
    w.cws = ws.take<char>(w.cws_bytes);
    w.total = ws.off;
    return w;
}

// THE predicate of a (hit, sector): bit 0 in the wedge, bit 1 in the extended wedge, bits 2 and 3 the same without the
// ur > 0 term (the measurement record's form).  The expressions are the reference's, operation by operation.
__device__ __forceinline__ uint32_t pc_wedges(double u, double v, double c, double s, const Wedge &g) {
    const double ur = u * c - v * s;
    const double vr = u * s + v * c;
    const bool in = (vr > -g.slope * ur) && (vr < g.slope * ur);
    const double lower = -g.ext * ur - g.di, upper = g.ext * ur + g.di;
    const bool ext = (vr > lower) && (vr < upper);
    const bool pos = ur > 0.0;
    return (in && pos ? 1u : 0u) | (ext && pos ? 2u : 0u) | (in ? 4u : 0u) | (ext ? 8u : 0u);
}

__global__ __launch_bounds__(kTpb) void pc_sector_flags_kernel(const double *__restrict__ uv, const int32_t *__restrict__ slot,
                                                               const int64_t *__restrict__ n_kept, int64_t cap, int32_t S,
                                                               const double *__restrict__ cs, Wedge g, Sw w) {
    const int64_t n = n_kept[0] < cap ? n_kept[0] : cap;
    for (int64_t j = (int64_t)blockIdx.x * kTpb + threadIdx.x; j < n * S; j += (int64_t)gridDim.x * kTpb) {
        const int64_t s = j / n, k = j - s * n;
        const int32_t p = slot[k];
        uint32_t *c = w.cnt4 + 4 * ((size_t)p * S + s);
        if (g.single) {
            w.flags[k] = 1;
            atomicAdd(&c[1], 1u);
            continue;
        }
        const uint32_t b = pc_wedges(uv[2 * k], uv[2 * k + 1], cs[2 * s], cs[2 * s + 1], g);
        for (int q = 0; q < 4; ++q)
            if (b >> q & 1u) atomicAdd(&c[q], 1u);
        if (b & 2u) w.flags[s * cap + k] = 1;
    }
}

__global__ __launch_bounds__(kTpb) void pc_sector_finish_kernel(const double *__restrict__ part_p, int64_t P, int32_t S, Wedge g,
                                                                Sw w, unsigned long long *counts, unsigned long long *head) {
    for (int64_t j = (int64_t)blockIdx.x * kTpb + threadIdx.x; j < (P + 1) * S; j += (int64_t)gridDim.x * kTpb) {
        const int64_t p = j / S, s = j - p * S;
        const uint32_t *c = w.cnt4 + 4 * (size_t)j;
        const uint32_t wedge = c[0], ext = c[1];
        unsigned long long *row = counts + (size_t)s * kSecCounts;
        if (wedge) atomicAdd(&row[S_WEDGE], (unsigned long long)wedge);
        if (ext == 0u) continue;
        atomicAdd(&row[S_EXT], (unsigned long long)ext);
        atomicAdd(&row[S_UNIQUE], 1ull);
        if (p == P) continue;   // noise: in no pair, in no majority
        const unsigned long long pairs = (unsigned long long)ext * (ext - 1u) / 2ull;
        if (pairs) {
            atomicAdd(&row[S_PAIRS], pairs);
            atomicAdd(&head[1], pairs);
        }
        const double px = part_p[3 * (size_t)p], py = part_p[3 * (size_t)p + 1], pt = sqrt(px * px + py * py);
        // the reference divides both counts by the length of the particle's ROW of the per-particle table, which is 1
        if ((pt >= g.thld ? c[2] : 0u) == 0u) continue;
        atomicAdd(&row[S_MAJ_DEN], 1ull);
        if ((pt > g.thld ? c[3] : 0u) == 1u) atomicAdd(&row[S_MAJ_NUM], 1ull);
    }
}

struct Cloud {
    float *x;          // [n_rows][n_feat]
    int64_t *cols;     // [GNNTRK_PC_COLUMNS][n_rows]: layer, particle_id, reconstructable, n_hits, n_layers_hit, sector
    float *pt_eta;     // [2][n_rows]
};

__global__ __launch_bounds__(kTpb) void pc_gather_kernel(Rows in, int64_t cap, int32_t n_feat, int64_t P, int32_t S,
                                                         int32_t single, int64_t n_rows, Sw w, Cloud o) {
    const int64_t stride = (int64_t)gridDim.x * kTpb, first = (int64_t)blockIdx.x * kTpb + threadIdx.x;
    for (int64_t q = first; q < n_rows * n_feat; q += stride) {
        const int64_t r = q / n_feat, f = q - r * n_feat;
        o.x[q] = in.x[(size_t)(w.rows[r] % cap) * n_feat + f];
    }
    for (int64_t r = first; r < n_rows; r += stride) {
        const int64_t j = w.rows[r], s = j / cap, k = j - s * cap;
        for (int c = 0; c < 5; ++c) o.cols[c * n_rows + r] = in.cols[c * cap + k];
        const int32_t p = in.slot[k];
        int64_t sector = 0;
        if (!single) sector = (p < P && w.cnt4[4 * ((size_t)p * S + s)] >= 1u) ? s : -1;   // (as above: count / 1 >= 0.5)
        o.cols[5 * n_rows + r] = sector;
        o.pt_eta[r] = in.pt_eta[k];
        o.pt_eta[n_rows + r] = in.pt_eta[cap + k];
    }
}

// ------------------------------------------------------------------------------------------------ truth edges
struct Tw {
    int32_t *tab;                                  // [S]  (segment, particle id) -> a hit + 1
    uint32_t *tcnt;                                // [S]  claims of the slot so far
    uint32_t *keys_a, *keys_b, *vals_a, *order;    // [n]
    char *temp;
    size_t temp_bytes;
    int32_t *rcnt, *pos;                           // [n]  pairs that the hit starts; its place in the order
    int64_t *row_off;                              // [n + 1]
    size_t zero_to, total;
    uint64_t S;
};

Tw make_tw(void *base, int64_t n) {
    Tw w{};
    w.S = table_size(n);
    Carver ws{(char *)base};
    w.tab = ws.take<int32_t>(w.S);
    w.tcnt = ws.take<uint32_t>(w.S);
    w.zero_to = ws.off;
    w.keys_a = ws.take<uint32_t>((size_t)n);
    w.keys_b = ws.take<uint32_t>((size_t)n);
    w.vals_a = ws.take<uint32_t>((size_t)n);
    w.order = ws.take<uint32_t>((size_t)n);
    w.temp_bytes = sort_pairs_temp_bytes(n > 0 ? n : 1);
    w.temp = ws.take<char>(w.temp_bytes);
    w.rcnt = ws.take<int32_t>((size_t)n + 4);
    w.pos = ws.take<int32_t>((size_t)n);
    w.row_off = ws.take<int64_t>((size_t)n + 1);
    w.total = ws.off;
    return w;
}

// COUNT: a hit adds the earlier claims of its particle's slot to its segment's count - over a particle with m hits
// 0 + 1 + ... + (m - 1) pairs, whatever the order.  Otherwise: the sort key of the hit.
template <bool COUNT>
__global__ __launch_bounds__(kTpb) void te_slots_kernel(const int64_t *__restrict__ pid, int64_t n, Events ev, Tw w,
                                                        unsigned long long *counts) {
    const uint64_t smask = w.S - 1;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < n; base += (int64_t)gridDim.x * kTpb) {   // (uniform in the wave)
        const int64_t i = base + threadIdx.x;
        uint32_t v[1] = {0u};
        int e = 0;
        if (i < n) {
            const int64_t key = pid[i];
            uint32_t sortkey = (uint32_t)w.S;   // noise: behind every particle
            if (key != 0) {
                int64_t lo, hi;
                e = event_rows<true>(ev, n, i, lo, hi);
                const uint64_t s = table_claim(w.tab, smask, particle_hash<true>(key, e), i,
                                               [&](int32_t h) { return pid[h] == key; },
                                               [&](int32_t h) { return h >= lo && h < hi; });
                if (COUNT) v[0] = atomicAdd(&w.tcnt[s], 1u);
                sortkey = (uint32_t)s;
            }
            if (!COUNT) {
                w.keys_a[i] = sortkey;
                w.vals_a[i] = (uint32_t)i;
            }
        }
        if (COUNT) event_add(v, e, counts, 1);
    }
}

__global__ __launch_bounds__(kTpb) void te_ranks_kernel(int64_t n, Tw w) {
    for (int64_t q = (int64_t)blockIdx.x * kTpb + threadIdx.x; q < n; q += (int64_t)gridDim.x * kTpb) {
        const uint32_t key = w.keys_b[q], i = w.order[q];
        int32_t c = 0;
        if (key != (uint32_t)w.S) c = (int32_t)(lower_bound_u32(w.keys_b, n, key + 1u) - 1 - q);
        w.rcnt[i] = c;
        w.pos[i] = (int32_t)q;
    }
}

__global__ __launch_bounds__(kTpb) void te_fill_kernel(int64_t n, Events ev, Tw w, int64_t n_edges, int global_ids,
                                                       int64_t *__restrict__ edge_index, int64_t *__restrict__ edge_ptr) {
    const int64_t span = n > ev.n + 1 ? n : ev.n + 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < span; i += (int64_t)gridDim.x * kTpb) {
        if (i <= ev.n) edge_ptr[i] = w.row_off[ev.ptr[i] < 0 ? 0 : (ev.ptr[i] > n ? n : ev.ptr[i])];
        const int32_t c = i < n ? w.rcnt[i] : 0;
        if (c == 0) continue;
        int64_t lo, hi;
        event_rows<true>(ev, n, i, lo, hi);
        const int64_t first = w.row_off[i], base = w.row_off[lo], m = w.row_off[hi] - base, q = w.pos[i];
        if (base + m > n_edges) continue;   // (never: the caller's count is the scan's total)
        for (int32_t t = 0; t < c; ++t) {
            const int64_t at = first + t, j = w.order[q + 1 + t];
            if (global_ids) {
                edge_index[at] = i;
                edge_index[n_edges + at] = j;
            } else {   // the segment's own [2, m] block, ids local to the segment
                edge_index[2 * base + (at - base)] = i - lo;
                edge_index[2 * base + m + (at - base)] = j - lo;
            }
        }
    }
}

int check_truth_edges(const char *entry, const int64_t *pid, int64_t n, const int64_t *seg_ptr, int32_t n_seg) {
    int rc = check_count_i30(entry, "hit", n);
    if (rc || (rc = check_events(entry, seg_ptr, n_seg))) return rc;
    if (n > 0 && !pid) {
        char msg[96];
        snprintf(msg, sizeof(msg), "%s: NULL particle ids", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    return GNNTRK_OK;
}

int bits_for(uint64_t max_key) {
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= max_key) ++bits;
    return bits;
}

}  // namespace
}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_point_cloud_select_workspace_bytes(int64_t n_hits, int64_t n_cells, int64_t n_particles) {
    if (n_hits <= 0 || n_cells < 0 || n_particles < 0) return 0;
    return make_ws(nullptr, n_hits, n_cells, n_particles).total;
}

int gnntrk_point_cloud_select(const int64_t *hit_id, const double *hit_xyz, const int32_t *hit_vlm, int64_t n_hits,
                              const int64_t *cell_hit_id, const int32_t *cell_ch, const double *cell_value, int64_t n_cells,
                              const int64_t *part_id, const double *part_p, int64_t n_particles,
                              const int64_t *truth_hit_id, const int64_t *truth_pid, int64_t n_truth,
                              const int32_t *layer_map, const int32_t *det_index, const int32_t *det_dims,
                              const double *det_rows, int64_t n_modules, const int32_t *feat_code, const double *feat_scale,
                              int32_t n_feat, int32_t remove_noise, float *x, int64_t *cols, float *pt_eta, double *uv,
                              int32_t *slot, int64_t *head, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "point_cloud_select";
    const int64_t H = n_hits, Cn = n_cells, P = n_particles, T = n_truth;
    int rc = check_count_i30(who, "hit", H);
    if (rc || (rc = check_count_i30(who, "cell", Cn)) || (rc = check_count_i30(who, "particle", P)) ||
        (rc = check_count_i30(who, "truth row", T)))
        return rc;
    if (!head) return fail(GNNTRK_EINVAL, "point_cloud_select: NULL head");
    if (!feat_code || !feat_scale || n_feat < 1) return fail(GNNTRK_EINVAL, "point_cloud_select: NULL or empty feature list");
    if (n_feat > kMaxF) return fail(GNNTRK_EUNSUPPORTED, "point_cloud_select: more features than GNNTRK_PC_MAX_FEATURES");
    Features F{};
    F.n = n_feat;
    for (int f = 0; f < n_feat; ++f) {
        if (feat_code[f] < 0 || feat_code[f] >= F_END || !(feat_scale[f] == feat_scale[f]))
            return fail(GNNTRK_EINVAL, "point_cloud_select: a feature code outside [0, GNNTRK_PC_FEATURE_CODES) or a NaN scale");
        F.code[f] = feat_code[f];
        F.scale[f] = feat_scale[f];
    }
    if (!det_dims || n_modules < 0 || det_dims[0] < 0 || det_dims[1] < 0 || det_dims[2] < 0 ||
        (n_modules > 0 && (!det_index || !det_rows)))
        return fail(GNNTRK_EINVAL, "point_cloud_select: NULL detector index, dims or rows, or negative sizes");
    rc = check_hip(hipMemsetAsync(head, 0, sizeof(int64_t) * kHead, stream), "point_cloud_select: clear");
    if (rc || H == 0) return rc;
    if (!hit_id || !hit_xyz || !hit_vlm || !layer_map || (Cn > 0 && (!cell_hit_id || !cell_ch || !cell_value)) ||
        (P > 0 && (!part_id || !part_p)) || (T > 0 && (!truth_hit_id || !truth_pid)))
        return fail(GNNTRK_EINVAL, "point_cloud_select: NULL column of the hits, cells, particles or truth, or NULL layer map");
    if (!x || !cols || !pt_eta || !uv || !slot) return fail(GNNTRK_EINVAL, "point_cloud_select: NULL output");
    const Ws w = make_ws(workspace, H, Cn, P);
    if ((rc = check_workspace(who, workspace, workspace_bytes, w.total))) return rc;
    char *base = (char *)workspace;
    if ((rc = check_hip(hipMemsetAsync(base + w.zero_from, 0, w.zero_to - w.zero_from, stream), "point_cloud_select: clear")) ||
        (rc = check_hip(hipMemsetAsync(w.htruth, 0xff, sizeof(int32_t) * (size_t)H, stream), "point_cloud_select: clear")))
        return rc;
    auto *hd = reinterpret_cast<unsigned long long *>(head);
    const int gh = blocks_for(H, 8);
    launch(pc_hit_table_kernel, gh, kTpb, stream, hit_id, hit_vlm, H, layer_map, w, hd);
    if (P > 0) launch(pc_particle_table_kernel, blocks_for(P, 8), kTpb, stream, part_id, P, w, hd);
    if (T > 0) launch(pc_truth_kernel, blocks_for(T, 8), kTpb, stream, truth_hit_id, hit_id, T, w, hd);
    if (Cn > 0) {
        launch(pc_cell_keys_kernel, blocks_for(Cn, 8), kTpb, stream, cell_hit_id, hit_id, Cn, H, w);
        if ((rc = sort_pairs_u32(w.keys_a, w.keys_b, w.vals_a, w.corder, Cn, bits_for((uint64_t)H), w.temp, w.temp_bytes,
                                 stream)))
            return rc;
    }
    launch(pc_hit_reduce_kernel, gh, kTpb, stream, cell_ch, cell_value, Cn, truth_pid, part_id, H, P, (int)(remove_noise != 0),
           w, hd);
    if ((rc = compact_bytes_launch(w.keep, H, w.kidx, nullptr, head + H_KEPT, w.cws, w.cws_bytes, stream))) return rc;
    launch(pc_particle_counts_kernel, gh, kTpb, stream, hit_vlm, H, w, (const int64_t *)head);
    const Rows o{x, cols, pt_eta, uv, slot};
    launch(pc_rows_kernel, blocks_for(H > P + 1 ? H : P + 1, 8), kTpb, stream, hit_xyz, hit_vlm, H, truth_pid, part_p, P,
           det_index, det_dims[0], det_dims[1], det_dims[2], det_rows, F, kVolumes, w, o, hd);
    return check_launch(who);
}

size_t gnntrk_point_cloud_sectors_workspace_bytes(int64_t capacity, int64_t n_particles, int32_t n_sectors) {
    if (capacity <= 0 || n_particles < 0 || n_sectors < 1 || capacity * n_sectors > INT_MAX) return 0;
    return make_sw(nullptr, capacity, n_particles, n_sectors).total;
}

static int check_sectors(const char *who, int64_t cap, int64_t P, int32_t S) {
    char msg[160];
    int rc = check_count_i30(who, "hit", cap);
    if (rc || (rc = check_count_i30(who, "particle", P))) return rc;
    if (S < 1) {
        snprintf(msg, sizeof(msg), "%s: n_sectors must be >= 1", who);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (cap * S > 0x3fffffff || (P + 1) * S > 0x3fffffff) {
        snprintf(msg, sizeof(msg), "%s: hits x sectors and particles x sectors must stay below 2^30", who);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    return GNNTRK_OK;
}

int gnntrk_point_cloud_sectors(const double *uv, const int32_t *slot, const int64_t *n_kept,
                               int64_t capacity, const double *part_p, int64_t n_particles, int32_t n_sectors,
                               const double *sector_cs, double slope, double sector_ds, double sector_di, double thld,
                               int64_t *counts, int64_t *head, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "point_cloud_sectors";
    const int64_t cap = capacity, P = n_particles;
    const int32_t S = n_sectors;
    int rc = check_sectors(who, cap, P, S);
    if (rc) return rc;
    if (!counts || !head) return fail(GNNTRK_EINVAL, "point_cloud_sectors: NULL counts or head");
    if ((rc = check_hip(hipMemsetAsync(head, 0, 2 * sizeof(int64_t), stream), "point_cloud_sectors: clear")) ||
        (rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * kSecCounts * (size_t)S, stream), "point_cloud_sectors: clear")))
        return rc;
    if (cap == 0) return GNNTRK_OK;
    if (!uv || !slot || !n_kept || (P > 0 && !part_p) || (S > 1 && !sector_cs))
        return fail(GNNTRK_EINVAL, "point_cloud_sectors: NULL uv, slot, n_kept, particle momenta or sector constants");
    const Sw w = make_sw(workspace, cap, P, S);
    if ((rc = check_workspace(who, workspace, workspace_bytes, w.total))) return rc;
    if ((rc = check_hip(hipMemsetAsync(workspace, 0, w.zero_to, stream), "point_cloud_sectors: clear"))) return rc;
    const Wedge g{slope, sector_ds * slope, sector_di, thld, S == 1};
    launch(pc_sector_flags_kernel, blocks_for(cap * S, 8), kTpb, stream, uv, slot, n_kept, cap, S, sector_cs, g, w);
    if ((rc = compact_bytes_launch(w.flags, cap * S, w.rows, nullptr, head, w.cws, w.cws_bytes, stream))) return rc;
    launch(pc_sector_finish_kernel, blocks_for((P + 1) * S, 8), kTpb, stream, part_p, P, S, g, w,
           reinterpret_cast<unsigned long long *>(counts), reinterpret_cast<unsigned long long *>(head));
    return check_launch(who);
}

int gnntrk_point_cloud_gather(const float *x, const int64_t *cols, const float *pt_eta, const int32_t *slot,
                              int64_t capacity, int32_t n_feat, int64_t n_particles, int32_t n_sectors, int64_t n_rows,
                              float *x_out, int64_t *cols_out, float *pt_eta_out, void *workspace, size_t workspace_bytes,
                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "point_cloud_gather";
    int rc = check_sectors(who, capacity, n_particles, n_sectors);
    if (rc) return rc;
    if (n_rows < 0 || n_feat < 1) return fail(GNNTRK_EINVAL, "point_cloud_gather: negative row count or no feature");
    if (n_rows > capacity * n_sectors) return fail(GNNTRK_EINVAL, "point_cloud_gather: more rows than hits x sectors");
    if (n_feat > kMaxF) return fail(GNNTRK_EUNSUPPORTED, "point_cloud_gather: more features than GNNTRK_PC_MAX_FEATURES");
    if (n_rows == 0) return GNNTRK_OK;
    if (!x || !cols || !pt_eta || !slot || !x_out || !cols_out || !pt_eta_out)
        return fail(GNNTRK_EINVAL, "point_cloud_gather: NULL column");
    const Sw w = make_sw(workspace, capacity, n_particles, n_sectors);
    if ((rc = check_workspace(who, workspace, workspace_bytes, w.total))) return rc;
    const Rows in{const_cast<float *>(x), const_cast<int64_t *>(cols), const_cast<float *>(pt_eta), nullptr,
                  const_cast<int32_t *>(slot)};
    launch(pc_gather_kernel, blocks_for(n_rows * n_feat, 8), kTpb, stream, in, capacity, n_feat, n_particles, n_sectors,
           (int32_t)(n_sectors == 1), n_rows, w, Cloud{x_out, cols_out, pt_eta_out});
    return check_launch(who);
}

size_t gnntrk_truth_edges_workspace_bytes(int64_t n) { return n <= 0 ? 0 : make_tw(nullptr, n).total; }

int gnntrk_truth_edges_count(const int64_t *particle_id, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t *counts,
                             void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "truth_edges_count";
    int rc = check_truth_edges(who, particle_id, n, seg_ptr, n_seg);
    if (rc) return rc;
    if (!counts) return fail(GNNTRK_EINVAL, "truth_edges_count: NULL counts");
    rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)n_seg, stream), "truth_edges_count: clear");
    if (rc || n == 0) return rc;
    const Tw w = make_tw(workspace, n);
    if ((rc = check_workspace(who, workspace, workspace_bytes, w.total))) return rc;
    if ((rc = check_hip(hipMemsetAsync(workspace, 0, w.zero_to, stream), "truth_edges_count: clear"))) return rc;
    launch(te_slots_kernel<true>, blocks_for(n, 8), kTpb, stream, particle_id, n, Events{seg_ptr, n_seg}, w,
           reinterpret_cast<unsigned long long *>(counts));
    return check_launch(who);
}

int gnntrk_truth_edges_fill(const int64_t *particle_id, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t n_edges,
                            int32_t global_ids, int64_t *edge_index, int64_t *edge_ptr, void *workspace,
                            size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "truth_edges_fill";
    int rc = check_truth_edges(who, particle_id, n, seg_ptr, n_seg);
    if (rc) return rc;
    if (n_edges < 0) return fail(GNNTRK_EINVAL, "truth_edges_fill: negative edge count");
    if (n_edges > 0x3fffffff) return fail(GNNTRK_EUNSUPPORTED, "truth_edges_fill: at most 2^30-1 edges");
    if (!edge_ptr || (n_edges > 0 && !edge_index)) return fail(GNNTRK_EINVAL, "truth_edges_fill: NULL edge_index or edge_ptr");
    if (n == 0 && n_edges > 0) return fail(GNNTRK_EINVAL, "truth_edges_fill: edges without hits");
    rc = check_hip(hipMemsetAsync(edge_ptr, 0, sizeof(int64_t) * ((size_t)n_seg + 1), stream), "truth_edges_fill: clear");
    if (rc || n == 0) return rc;
    const Tw w = make_tw(workspace, n);
    if ((rc = check_workspace(who, workspace, workspace_bytes, w.total))) return rc;
    if ((rc = check_hip(hipMemsetAsync(workspace, 0, w.zero_to, stream), "truth_edges_fill: clear"))) return rc;
    const Events ev{seg_ptr, n_seg};
    const int g = blocks_for(n, 8);
    launch(te_slots_kernel<false>, g, kTpb, stream, particle_id, n, ev, w, (unsigned long long *)nullptr);
    if ((rc = sort_pairs_u32(w.keys_a, w.keys_b, w.vals_a, w.order, n, bits_for(w.S), w.temp, w.temp_bytes, stream))) return rc;
    launch(te_ranks_kernel, g, kTpb, stream, n, w);
    scan_counts_launch(w.rcnt, INT_MAX, n, w.row_off, stream);
    launch(te_fill_kernel, blocks_for(n > n_seg + 1 ? n : n_seg + 1, 8), kTpb, stream, n, ev, w, n_edges, (int)(global_ids != 0), edge_index, edge_ptr);
    return check_launch(who);
}

}  // extern "C"
