// Graph index: stable target-sorted (CSR) and source-sorted views of a COO edge list.
// See gnntrk_graph_index in include/gnntrk.h (replaces the gather / scatter bookkeeping of PyG's
// MessagePassing.propagate, models/interaction_network.py:36,67).  HBM-bound integer work.
//
// Two forms with the same results.  The own two-level counting sort below is the one that runs; the library radix
// sort (further down) takes what the own form does not: very dense graphs (own_plan's `dense`), tables beyond
// kMaxTable, and flags bit 0, which the tests use as their reference (bit 1 forces the own form).  There is one
// path through the own form and one build hook, GNNTRK_GI_HUB_BITMAP_MIN; the variants it was measured against are
// written up in DESIGN.md section 4.5.
//
//   a node id is split into (bucket = id >> 8, low = id & 255).  The edge list is cut into chunks of
//   consecutive edges (one workgroup each).
//     1. count   per (bucket, chunk) edge counts: LDS histogram per chunk, written into a dense
//                bucket-major table
//     2. scan    one exclusive scan over the flattened table = the output offset of every
//                (bucket, chunk) run
//     3. split   every edge goes to its bucket's region (position from an LDS cursor per bucket) as
//                one 8-byte record {low | payload, value}
//     4. sort    one workgroup per bucket (256 nodes, a few thousand edges, held in LDS): histogram
//                over `low` -> row pointers of the bucket's nodes; the rank of a record inside its
//                node's list is the number of records of that node with a smaller value (edge id /
//                CSR position), so the result is the STABLE order whatever order step 3's cursors
//                handed out - deterministic, bit-identical to a stable sort.
//   Run twice: by target over the COO list (value = edge id, payload = source) and by source over
//   the CSR list (value = CSR position).  Row pointers, `src[perm]`, `tgt` and the inverse
//   permutation fall out of step 4 - no key extraction, gather or boundary passes.
//
//   What makes steps 1 / 3 stream: a collated batch is a list of events with disjoint id ranges and
//   contiguous edge ranges, so a chunk only touches the few hundred buckets of its own event: the
//   counters of a chunk live in an LDS window of 4096 buckets (kWin) placed a third below the chunk's first id and the
//   runs it writes are hundreds of bytes long.  Ids outside the window (one giant unsorted graph)
//   take global atomics on the table itself - slower, same result.  A bucket beyond the LDS
//   capacity is sorted in groups of nodes that fit, a hub node run by run from global memory (gi_sort_group,
//   gi_hub_walk, gi_hub_bitmaps) - slower, same result.
//
//   Algorithmic bytes per edge: count 8 + split 16 + 8 + sort 8 + 12, then 4 + 4 + 8 + 8 + 8 = 84
//   (+ 0.3 table entries per edge x 12 B); the library path moved about 260.  Renumbered, with a carried label
//   and carried rows (the training step): remap with the count inside 16 + 8, split 8 + 1 + 16 in and 16 out (the
//   row rides in the record), sort 16 in and 12 + 1 + 8 out, then the same 32 by source = 134.
#include "host_util.h"
#include "tile_bf16.h"

namespace gnntrk {

constexpr int kTpb = 256;

// ------------------------------------------------------------------ own counting sort
constexpr int kSH = 8;                  // nodes per bucket = 256
constexpr int kBins = 1 << kSH;
constexpr int kSortTpb = 512;
constexpr int kSortR = 10;              // records a thread of the bucket sort holds in registers
constexpr int kCap = kSortTpb * kSortR; // records of a bucket the bucket sort holds in LDS (5120)
constexpr int kWin = 4096;              // bucket counters a chunk holds in LDS
// One split workgroup of 1024 lanes per CU.  Two resident workgroups (768 lanes at <= 85 registers) measured
// SLOWER (split by target 1.18 against 1.12 ms, by source 0.38 against 0.33): the open (bucket, chunk) runs of
// the resident chunks - about 600 partially written lines per chunk and output array - then no longer fit an
// XCD's 4 MB L2, and the runs leave it in pieces.
constexpr int kSplitTpb = 1024;
constexpr int kSplitWg = 1;             // split workgroups resident on a CU
constexpr int kCountTpb = 1024;
constexpr int kSplitR = 4;              // edges per thread and tile of the split
constexpr int kSplitTile = kSplitTpb * kSplitR;
constexpr int kMaxChunks = 512;
#ifndef GNNTRK_GI_HUB_BITMAP_MIN
// hub nodes above this degree are ranked through per-run bitmaps.  The one build hook of this unit: the emulator
// build of the tests sets 8192, so that the bitmap path is reachable at emulator sizes
#define GNNTRK_GI_HUB_BITMAP_MIN 65536
#endif
constexpr int64_t kMaxTable = (int64_t)96 << 20;   // table entries (4 B each)
constexpr int kScanTpb = 256, kScanItems = 16, kScanTile = kScanTpb * kScanItems;

// A node id as the caller gave it: outside [0, N) it is counted in *bad and clamped.  kNullable: `bad` may be
// nullptr, for an id that another pass counts (the passes that always count are spared the test)
template <bool kNullable>
__device__ __forceinline__ int64_t gi_clamped(int64_t v, int64_t N, int *bad) {
    if (v < 0 || v >= N) {
        if (!kNullable || bad) atomicAdd(bad, 1);
        v = v < 0 ? 0 : N - 1;
    }
    return v;
}
// Four consecutive int32 a[e .. e + 3] of an own 16-byte aligned array (e a multiple of four, e1 = end of the
// lane's range): one 16-byte load, item by item with 0 past e1 at the tail
__device__ __forceinline__ int4 gi_load4(const int32_t *a, int64_t e, int64_t e1) {
    if (e + 4 <= e1) return *reinterpret_cast<const int4 *>(a + e);
    return int4{e < e1 ? a[e] : 0, e + 1 < e1 ? a[e + 1] : 0, e + 2 < e1 ? a[e + 2] : 0, 0};
}

// first sort: key = target (COO row 1), payload = source (row 0), value = edge id.  Two per-edge
// inputs of the caller can ride along into CSR order (gnntrk_graph_index_carry): a 1-byte label in
// bit 31 of the value (edge ids are below 2^31), a row of four floats as four bf16 in the second
// half of a 16-byte record
struct KeysCoo {
    const int64_t *src, *tgt;
    int64_t N;
    const uint8_t *label;
    const float *rows;
    int rows_stride;
    __device__ __forceinline__ uint32_t key(int64_t e, int *bad) const { return checked(tgt[e], bad); }
    // four consecutive edges e .. e + 3 of one lane (e a multiple of four): with `vec` (16-byte aligned id rows,
    // 4-byte aligned labels) the ids come as 16-byte loads - 8-byte-per-lane streams top out near 3 TB/s here
    int vec;
    // optional renumbering of the nodes (gnntrk_graph_index_carry.node_rank: old id -> new id, a permutation of
    // [0, N) that keeps every event's id range): applied where an id is read, so the whole index comes out in
    // the new numbering.  The table of one event (600 KB at 150 k hits) stays in the XCD's L2.
    const int32_t *rank;
    __device__ __forceinline__ uint32_t checked(int64_t v, int *bad) const {
        v = gi_clamped<true>(v, N, bad);
        return rank ? (uint32_t)rank[v] : (uint32_t)v;
    }
    __device__ __forceinline__ void keys4(int64_t e, int64_t e1, uint32_t k[4], int *bad) const {
        if (vec && e + 4 <= e1) {
            const longlong2 a = *reinterpret_cast<const longlong2 *>(tgt + e);
            const longlong2 b = *reinterpret_cast<const longlong2 *>(tgt + e + 2);
            k[0] = checked(a.x, bad);
            k[1] = checked(a.y, bad);
            k[2] = checked(b.x, bad);
            k[3] = checked(b.y, bad);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) k[q] = e + q < e1 ? key(e + q, bad) : 0u;
        }
    }
    // the split holds the NEXT tile's ids as loaded (converted only when their tile starts: a conversion at the
    // load would wait for it on the spot)
    struct Raw {
        longlong2 ta, tb, sa, sb;
        uint32_t l4;
    };
    __device__ __forceinline__ void load_raw(int64_t e, int64_t e1, Raw &r) const {
        if (vec && e + 4 <= e1) {
            r.ta = *reinterpret_cast<const longlong2 *>(tgt + e);
            r.tb = *reinterpret_cast<const longlong2 *>(tgt + e + 2);
            r.sa = *reinterpret_cast<const longlong2 *>(src + e);
            r.sb = *reinterpret_cast<const longlong2 *>(src + e + 2);
            r.l4 = label ? *reinterpret_cast<const uint32_t *>(label + e) : 0u;
        } else {
            long long t[4], u[4];
            r.l4 = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = e + q < e1;
                t[q] = in ? tgt[e + q] : 0;
                u[q] = in ? src[e + q] : 0;
                if (in && label && label[e + q]) r.l4 |= 1u << (8 * q);
            }
            r.ta = longlong2{t[0], t[1]};
            r.tb = longlong2{t[2], t[3]};
            r.sa = longlong2{u[0], u[1]};
            r.sb = longlong2{u[2], u[3]};
        }
    }
    // (ids out of range: the targets were counted by step 1, the sources are counted here)
    __device__ __forceinline__ void decode(const Raw &r, int64_t e, uint32_t k[4], uint32_t p[4], uint32_t v[4],
                                           int *bad) const {
        k[0] = checked(r.ta.x, nullptr);
        k[1] = checked(r.ta.y, nullptr);
        k[2] = checked(r.tb.x, nullptr);
        k[3] = checked(r.tb.y, nullptr);
        p[0] = checked(r.sa.x, bad);
        p[1] = checked(r.sa.y, bad);
        p[2] = checked(r.sb.x, bad);
        p[3] = checked(r.sb.y, bad);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (uint32_t)(e + q) | (((r.l4 >> (8 * q)) & 0xffu) ? 0x80000000u : 0u);
    }
    __device__ __forceinline__ f32x4 row_raw(int64_t e) const {
        return *reinterpret_cast<const f32x4 *>(rows + e * rows_stride);
    }
};
// first sort over a RENUMBERED edge list (gnntrk_graph_index_carry.node_rank): gi_remap_count_kernel has written
// both endpoint rows as validated int32 new ids (one streaming pass with every lane's eight table lookups in flight:
// inside the count / split kernels, whose occupancy is one workgroup per CU, the same lookups cost 1.7 ms per
// 64 M edges, here under half of that) and has counted the targets on the way; the split then reads 8 bytes per
// edge instead of 16
struct KeysCoo32 {
    const int32_t *src, *tgt;
    const uint8_t *label;
    const float *rows;
    int rows_stride;
    int vec;   // 4-byte aligned labels
    __device__ __forceinline__ uint32_t key(int64_t e, int *) const { return (uint32_t)tgt[e]; }
    struct Raw {
        int4 t, s;
        uint32_t l4;
    };
    __device__ __forceinline__ void load_raw(int64_t e, int64_t e1, Raw &r) const {
        if (e + 4 <= e1) {   // (own 16-byte aligned arrays; e is a multiple of four)
            r.t = *reinterpret_cast<const int4 *>(tgt + e);
            r.s = *reinterpret_cast<const int4 *>(src + e);
            if (!label) {
                r.l4 = 0u;
            } else if (vec) {
                r.l4 = *reinterpret_cast<const uint32_t *>(label + e);
            } else {
                r.l4 = (label[e] ? 1u : 0u) | (label[e + 1] ? 0x100u : 0u) | (label[e + 2] ? 0x10000u : 0u) |
                       (label[e + 3] ? 0x1000000u : 0u);
            }
        } else {
            int t[4], u[4];
            r.l4 = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = e + q < e1;
                t[q] = in ? tgt[e + q] : 0;
                u[q] = in ? src[e + q] : 0;
                if (in && label && label[e + q]) r.l4 |= 1u << (8 * q);
            }
            r.t = int4{t[0], t[1], t[2], t[3]};
            r.s = int4{u[0], u[1], u[2], u[3]};
        }
    }
    __device__ __forceinline__ void decode(const Raw &r, int64_t e, uint32_t k[4], uint32_t p[4], uint32_t v[4],
                                           int *) const {
        k[0] = (uint32_t)r.t.x;
        k[1] = (uint32_t)r.t.y;
        k[2] = (uint32_t)r.t.z;
        k[3] = (uint32_t)r.t.w;
        p[0] = (uint32_t)r.s.x;
        p[1] = (uint32_t)r.s.y;
        p[2] = (uint32_t)r.s.z;
        p[3] = (uint32_t)r.s.w;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (uint32_t)(e + q) | (((r.l4 >> (8 * q)) & 0xffu) ? 0x80000000u : 0u);
    }
    __device__ __forceinline__ f32x4 row_raw(int64_t e) const {
        return *reinterpret_cast<const f32x4 *>(rows + e * rows_stride);
    }
};
// both endpoint rows of the COO list through the renumbering: ids checked (counted, clamped), translated, written
// as int32.  A lane takes four consecutive edges e .. e + 3 (e a multiple of four, e1 = end of the lane's range):
// 16-byte id loads, eight lookups in flight, 16-byte stores.  kt[] = the translated targets (0 past e1).
__device__ __forceinline__ void gi_remap4(const int64_t *__restrict__ src, const int64_t *__restrict__ tgt, int64_t e,
                                          int64_t e1, int64_t N, const int32_t *__restrict__ rank, int vec,
                                          int32_t *__restrict__ src32, int32_t *__restrict__ tgt32,
                                          int *__restrict__ bad, uint32_t kt[4]) {
    if (vec && e + 4 <= e1) {
        // (the id streams and the outputs pass through once: non-temporal, the lookup table keeps the L2)
        typedef int i4_hw __attribute__((ext_vector_type(4)));
        auto ld2 = [](const int64_t *p, long long &a, long long &b) {   // two ids as one 16-byte non-temporal load
            const i4_hw v = __builtin_nontemporal_load(reinterpret_cast<const i4_hw *>(p));
            a = (long long)(((unsigned long long)(uint32_t)v[1] << 32) | (uint32_t)v[0]);
            b = (long long)(((unsigned long long)(uint32_t)v[3] << 32) | (uint32_t)v[2]);
        };
        long long it[4], is[4];
        ld2(tgt + e, it[0], it[1]);
        ld2(tgt + e + 2, it[2], it[3]);
        ld2(src + e, is[0], is[1]);
        ld2(src + e + 2, is[2], is[3]);
        // (all eight ids checked before the first lookup: the lookups then leave together)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            it[q] = gi_clamped<false>(it[q], N, bad);
            is[q] = gi_clamped<false>(is[q], N, bad);
        }
        const i4_hw ot = {rank[it[0]], rank[it[1]], rank[it[2]], rank[it[3]]};
        const i4_hw os = {rank[is[0]], rank[is[1]], rank[is[2]], rank[is[3]]};
        __builtin_nontemporal_store(ot, reinterpret_cast<i4_hw *>(tgt32 + e));
        __builtin_nontemporal_store(os, reinterpret_cast<i4_hw *>(src32 + e));
#pragma unroll
        for (int q = 0; q < 4; ++q) kt[q] = (uint32_t)ot[q];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            kt[q] = 0u;
            if (e + q < e1) {
                const int t = rank[gi_clamped<false>(tgt[e + q], N, bad)], u = rank[gi_clamped<false>(src[e + q], N, bad)];
                tgt32[e + q] = t;
                src32[e + q] = u;
                kt[q] = (uint32_t)t;
            }
        }
    }
}
// second sort: key = source of the CSR-ordered list (already validated), value = CSR position
struct KeysCsr {
    const int32_t *src;
    __device__ __forceinline__ uint32_t key(int64_t e, int *) const { return (uint32_t)src[e]; }
    __device__ __forceinline__ void keys4(int64_t e, int64_t e1, uint32_t k[4], int *) const {
        const int4 a = gi_load4(src, e, e1);
        k[0] = (uint32_t)a.x;
        k[1] = (uint32_t)a.y;
        k[2] = (uint32_t)a.z;
        k[3] = (uint32_t)a.w;
    }
    struct Raw {
        int4 a;
    };
    __device__ __forceinline__ void load_raw(int64_t e, int64_t e1, Raw &r) const { r.a = gi_load4(src, e, e1); }
    __device__ __forceinline__ void decode(const Raw &r, int64_t e, uint32_t k[4], uint32_t p[4], uint32_t v[4],
                                           int *) const {
        k[0] = (uint32_t)r.a.x;
        k[1] = (uint32_t)r.a.y;
        k[2] = (uint32_t)r.a.z;
        k[3] = (uint32_t)r.a.w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[q] = 0u;
            v[q] = (uint32_t)(e + q);
        }
    }
    __device__ __forceinline__ f32x4 row_raw(int64_t) const { return f32x4{0.f, 0.f, 0.f, 0.f}; }
};

// The LDS window of a chunk starts a third of its width below the bucket of the chunk's first id: a
// chunk that begins inside event A and runs into event B sees ids from A's first to B's last
__device__ __forceinline__ int gi_window_start(uint32_t first_key) {
    const int b = (int)(first_key >> kSH) - kWin / 3;
    return b < 0 ? 0 : b;
}

// Which chunk a workgroup of gi_remap_count_kernel takes.  Workgroups b and b + 8 are observed to share an XCD
// (nothing promises it: it buys speed only), so a run of consecutive chunks goes to ONE XCD, whose L2 then holds the
// renumbering tables of those chunks' events instead of a little of every event's.  The grid is
// gi_chunk_grid(n_chunks) workgroups; a chunk >= n_chunks is none.  (The split gains nothing from this order:
// 788 against 790 us per 64 M edges.)
constexpr int kXcd = 8;
__device__ __forceinline__ int gi_chunk_of_block() {
    return (int)(blockIdx.x % kXcd) * (int)(gridDim.x / kXcd) + (int)(blockIdx.x / kXcd);
}
static int gi_chunk_grid(int n_chunks) { return (n_chunks + kXcd - 1) / kXcd * kXcd; }

// step 1.  tbl[bucket * n_chunks + chunk] = edges of the chunk in the bucket (tbl zeroed before);
// range[chunk] = (first, last) touched window slot.
// The keys k4[] of a lane's four consecutive edges e .. e + 3 into the chunk's counters
// (consecutive edges of an ordered list share their bucket: one counter update per run of a lane's four)
__device__ __forceinline__ void gi_count4(const uint32_t k4[4], int64_t e, int64_t e1, int w0, uint32_t *s_cnt,
                                          uint32_t *__restrict__ tbl, int n_chunks, int c) {
    auto bump = [&](uint32_t b, uint32_t by) {
        const uint32_t d = b - (uint32_t)w0;
        if (d < (uint32_t)kWin)
            atomicAdd(&s_cnt[d], by);
        else
            atomicAdd(&tbl[(size_t)b * n_chunks + c], by);
    };
    uint32_t run_b = k4[0] >> kSH, run_n = 1;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        if (e + q >= e1) break;
        const uint32_t b = k4[q] >> kSH;
        if (b == run_b) {
            run_n += 1;
        } else {
            bump(run_b, run_n);
            run_b = b;
            run_n = 1;
        }
    }
    bump(run_b, run_n);
}
// the chunk's window into the table, its touched range into range[c] (all threads of the workgroup; s_lo / s_hi
// start at kWin / -1)
template <int TPB>
__device__ __forceinline__ void gi_count_flush(const uint32_t *s_cnt, int *s_lo, int *s_hi, int w0, int n_chunks, int c,
                                               uint32_t *__restrict__ tbl, int2 *__restrict__ range) {
    const int tid = threadIdx.x;
    __syncthreads();
    int lo = kWin, hi = -1;
    for (int d = tid; d < kWin; d += TPB) {
        const uint32_t v = s_cnt[d];
        if (v) {
            tbl[(size_t)(w0 + d) * n_chunks + c] = v;
            lo = d < lo ? d : lo;
            hi = d > hi ? d : hi;
        }
    }
    if (hi >= 0) {
        atomicMin(s_lo, lo);
        atomicMax(s_hi, hi);
    }
    __syncthreads();
    if (tid == 0) range[c] = int2{*s_lo, *s_hi};
}
template <class K>
__global__ __launch_bounds__(kCountTpb) void gi_count_kernel(K keys, int64_t E, int chunk, int n_chunks, int NB,
                                                             uint32_t *__restrict__ tbl, int2 *__restrict__ range,
                                                             int *__restrict__ bad) {
    __shared__ uint32_t s_cnt[kWin];
    __shared__ int s_lo, s_hi;
    const int tid = threadIdx.x, c = blockIdx.x;
    const int64_t e0 = (int64_t)c * chunk, e1 = e0 + chunk < E ? e0 + chunk : E;
    for (int d = tid; d < kWin; d += kCountTpb) s_cnt[d] = 0;
    if (tid == 0) {
        s_lo = kWin;
        s_hi = -1;
    }
    __syncthreads();
    const int w0 = gi_window_start(keys.key(e0, nullptr));   // (e0 is counted below)
    for (int64_t e = e0 + 4 * tid; e < e1; e += 4 * kCountTpb) {
        uint32_t k4[4];
        keys.keys4(e, e1, k4, bad);
        gi_count4(k4, e, e1, w0, s_cnt, tbl, n_chunks, c);
    }
    gi_count_flush<kCountTpb>(s_cnt, &s_lo, &s_hi, w0, n_chunks, c, tbl, range);
    (void)NB;
}
// The remap pass in the sort's chunk geometry (one workgroup per chunk), counting the translated targets as it
// writes them: step 1 of the by-target sort without a pass of its own over tgt32.  The lookups want every lane
// slot of a CU filled (inside the count / split kernels, one 1024-lane workgroup per CU, they cost 1.7 ms per
// 64 M edges): two workgroups of 1024 lanes per CU - at most 64 registers, a 16 KB window each.
constexpr int kRemapTpb = 1024;
__global__ __launch_bounds__(kRemapTpb, 8) void gi_remap_count_kernel(
    const int64_t *__restrict__ src, const int64_t *__restrict__ tgt, int64_t E, int64_t N,
    const int32_t *__restrict__ rank, int vec, int32_t *__restrict__ src32, int32_t *__restrict__ tgt32, int chunk,
    int n_chunks, uint32_t *__restrict__ tbl, int2 *__restrict__ range, int *__restrict__ bad) {
    __shared__ uint32_t s_cnt[kWin];
    __shared__ int s_lo, s_hi, s_w0;
    // (all chunks are in flight at once, and a chunk's lookups go to its own event's table - 600 KB at 150 k hits: in
    // launch order every XCD's L2 sees the tables of all 32 events and the whole build takes 4.33 ms, this way 3.57)
    const int tid = threadIdx.x, c = gi_chunk_of_block();
    if (c >= n_chunks) return;
    const int64_t e0 = (int64_t)c * chunk, e1 = e0 + chunk < E ? e0 + chunk : E;
    for (int d = tid; d < kWin; d += kRemapTpb) s_cnt[d] = 0;
    if (tid == 0) {
        s_lo = kWin;
        s_hi = -1;
        // the window starts from the chunk's first TRANSLATED target (clamped as the pass below clamps it, counted there)
        s_w0 = gi_window_start((uint32_t)rank[gi_clamped<true>(tgt[e0], N, nullptr)]);
    }
    __syncthreads();
    const int w0 = s_w0;
    for (int64_t e = e0 + 4 * tid; e < e1; e += 4 * kRemapTpb) {
        uint32_t k4[4];
        gi_remap4(src, tgt, e, e1, N, rank, vec, src32, tgt32, bad, k4);
        gi_count4(k4, e, e1, w0, s_cnt, tbl, n_chunks, c);
    }
    gi_count_flush<kRemapTpb>(s_cnt, &s_lo, &s_hi, w0, n_chunks, c, tbl, range);
}

// step 2: exclusive scan of tbl[0 .. T] in place (tbl[T] = total), two kernels: the tiles' sums, then every tile
// scans itself behind the sum of the tiles before it (a tile adds those up itself: a few thousand values out of the
// L2) and leaves base[b] = the scanned tbl[b * n_chunks], the first record of bucket b (b <= NB), on the way
__global__ __launch_bounds__(kScanTpb) void gi_scan_sums_kernel(const uint32_t *__restrict__ v, int64_t n,
                                                                uint32_t *__restrict__ sums) {
    __shared__ uint32_t s[kScanTpb];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)tid * kScanItems;
    uint32_t t = 0;
    if (i0 + kScanItems <= n) {
#pragma unroll
        for (int q = 0; q < kScanItems / 4; ++q) {
            const uint4 a = *reinterpret_cast<const uint4 *>(v + i0 + 4 * q);
            t += a.x + a.y + a.z + a.w;
        }
    } else {
        for (int q = 0; q < kScanItems; ++q) t += i0 + q < n ? v[i0 + q] : 0u;
    }
    s[tid] = t;
    __syncthreads();
    for (int d = kScanTpb / 2; d > 0; d >>= 1) {
        if (tid < d) s[tid] += s[tid + d];
        __syncthreads();
    }
    if (tid == 0) sums[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kScanTpb) void gi_scan_apply_kernel(uint32_t *__restrict__ v, int64_t n,
                                                                 const uint32_t *__restrict__ sums, int n_chunks,
                                                                 uint32_t *__restrict__ base) {
    __shared__ uint32_t s[kScanTpb];
    __shared__ uint32_t s_before[kScanTpb / 64];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)tid * kScanItems;
    uint32_t before = 0;   // sum of the tiles before this one
    for (int i = tid; i < (int)blockIdx.x; i += kScanTpb) before += sums[i];
    for (int o = 32; o > 0; o >>= 1) before += (uint32_t)__shfl_xor((int)before, o);
    if ((tid & 63) == 0) s_before[tid >> 6] = before;
    uint32_t x[kScanItems];
    const bool full = i0 + kScanItems <= n;
    if (full) {
#pragma unroll
        for (int q = 0; q < kScanItems / 4; ++q) {
            const uint4 a = *reinterpret_cast<const uint4 *>(v + i0 + 4 * q);
            x[4 * q] = a.x;
            x[4 * q + 1] = a.y;
            x[4 * q + 2] = a.z;
            x[4 * q + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kScanItems; ++q) x[q] = i0 + q < n ? v[i0 + q] : 0u;
    }
    uint32_t t = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) t += x[q];
    s[tid] = t;
    __syncthreads();
    before = 0;
#pragma unroll
    for (int w = 0; w < kScanTpb / 64; ++w) before += s_before[w];
    for (int d = 1; d < kScanTpb; d <<= 1) {
        const uint32_t u = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += u;
        __syncthreads();
    }
    uint32_t run = before + s[tid] - t;
    // (entries b * n_chunks among the thread's sixteen: the first at `nb`, relative to i0)
    int64_t bk = (i0 + n_chunks - 1) / n_chunks;
    int64_t nb = bk * n_chunks - i0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
        const uint32_t c = x[q];
        x[q] = run;
        run += c;
        if (q == nb && i0 + q < n) {
            base[bk] = x[q];
            bk += 1;
            nb += n_chunks;
        }
    }
    if (full) {
#pragma unroll
        for (int q = 0; q < kScanItems / 4; ++q)
            *reinterpret_cast<uint4 *>(v + i0 + 4 * q) = uint4{x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
    } else {
#pragma unroll
        for (int q = 0; q < kScanItems; ++q)
            if (i0 + q < n) v[i0 + q] = x[q];
    }
}

// exclusive scan of one value per thread over a workgroup of kSplitTpb threads (wave shuffles + one
// LDS round for the 16 wave totals); also returns the total
__device__ __forceinline__ uint32_t gi_block_exscan(uint32_t v, uint32_t *s_wsum, uint32_t *total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl(inc, lane - d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kSplitTpb / 64; ++w) {
        const uint32_t t = s_wsum[w];
        pre += w < wv ? t : 0u;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

// step 3.  part[pos] = {x: value (edge id [| label << 31] / CSR position), y: low << pbits | payload}.
// A tile of 4096 edges is first grouped by bucket in LDS (rank inside the tile's bucket from an LDS
// counter, tile-local starts from a scan over the chunk's touched window range), then written out
// with consecutive lanes on consecutive records of a run: the stores coalesce.  ROWS: the
// caller's per-edge row (four floats -> four bf16) is the record's second half {z, w}: one 16-byte
// record per edge through one staging image.
template <bool ROWS>
struct GiRec {
    typedef uint2 type;
    static __device__ __forceinline__ uint2 make(uint32_t x, uint32_t y, const f32x4 &) { return uint2{x, y}; }
};
template <>
struct GiRec<true> {
    typedef uint4 type;
    static __device__ __forceinline__ uint4 make(uint32_t x, uint32_t y, const f32x4 &rv) {
        return uint4{x, y, bf16x2_pack(rv[0], rv[1]), bf16x2_pack(rv[2], rv[3])};
    }
};
template <class K, bool ROWS>
__global__ __launch_bounds__(kSplitTpb, kSplitWg * kSplitTpb / 256) void gi_split_kernel(K keys, int64_t E, int chunk, int n_chunks, int pbits,
                                                             uint32_t *__restrict__ tbl,
                                                             const int2 *__restrict__ range,
                                                             typename GiRec<ROWS>::type *__restrict__ part,
                                                             int *__restrict__ bad) {
    typedef typename GiRec<ROWS>::type Rec;
    __shared__ uint32_t s_off[kWin];     // next free record of the (bucket, chunk) run
    __shared__ uint32_t s_cnt[kWin];     // tile: records per bucket, then the tile-local start
    __shared__ Rec s_stage[kSplitTile];
    __shared__ uint16_t s_slot[kSplitTile];
    __shared__ uint32_t s_wsum[kSplitTpb / 64];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int64_t e0 = (int64_t)c * chunk, e1 = e0 + chunk < E ? e0 + chunk : E;
    const int w0 = gi_window_start(keys.key(e0, nullptr));
    const int2 r = range[c];
    const int n_r = r.y >= r.x ? r.y - r.x + 1 : 0;         // touched window slots
    const int per = (n_r + kSplitTpb - 1) / kSplitTpb;      // ... per thread in the scans (1 for a collated batch)
    for (int d = r.x + tid; d <= r.y; d += kSplitTpb) {
        s_off[d] = tbl[(size_t)(w0 + d) * n_chunks + c];
        s_cnt[d] = 0;
    }
    __syncthreads();
    // the next tile's ids are loaded while the current tile goes through its LDS phases; the carried rows of
    // the current tile are loaded at its start and used in its last phase
    static_assert(kSplitR == 4, "a lane takes four consecutive edges of a tile");
    typename K::Raw nraw;
    keys.load_raw(e0 + 4 * tid, e1, nraw);
    for (int64_t t0 = e0; t0 < e1; t0 += kSplitTile) {
        uint2 rec[kSplitR];
        f32x4 rraw[ROWS ? kSplitR : 1];
        uint32_t slot[kSplitR], rk[kSplitR];
        const int64_t et = t0 + 4 * tid;
        {
            uint32_t nk[kSplitR], np[kSplitR], nv[kSplitR];
            keys.decode(nraw, et, nk, np, nv, bad);
            keys.load_raw(et + kSplitTile, e1, nraw);
#pragma unroll
            for (int q = 0; q < kSplitR; ++q) {
                const int64_t e = et + q;
                slot[q] = 0xffffffffu;
                if (ROWS) rraw[q] = e < e1 ? keys.row_raw(e) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (e < e1) {
                    const uint32_t v = nk[q], pl = np[q];
                    const uint32_t b = v >> kSH, low = v & (kBins - 1);
                    const uint32_t d = b - (uint32_t)w0;
                    rec[q] = uint2{nv[q], (low << pbits) | pl};
                    if (d < (uint32_t)kWin) {
                        slot[q] = d;
                        rk[q] = atomicAdd(&s_cnt[d], 1u);
                    } else {   // outside the chunk's LDS window: cursor in the table itself, direct stores
                        const uint32_t pos = atomicAdd(&tbl[(size_t)b * n_chunks + c], 1u);
                        part[pos] = GiRec<ROWS>::make(rec[q].x, rec[q].y, rraw[ROWS ? q : 0]);
                    }
                }
            }
        }
        __syncthreads();
        // tile-local starts: exclusive scan of the counts over the touched range
        const int d0 = r.x + tid * per;
        uint32_t mine = 0;
#pragma unroll 1
        for (int i = 0; i < per; ++i)
            if (d0 + i <= r.y) mine += s_cnt[d0 + i];
        uint32_t tile_n;
        uint32_t run = gi_block_exscan(mine, s_wsum, &tile_n);
#pragma unroll 1
        for (int i = 0; i < per; ++i)
            if (d0 + i <= r.y) {
                const uint32_t cn = s_cnt[d0 + i];
                s_cnt[d0 + i] = run;
                run += cn;
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kSplitR; ++q)
            if (slot[q] != 0xffffffffu) {
                const uint32_t spq = s_cnt[slot[q]] + rk[q];
                s_stage[spq] = GiRec<ROWS>::make(rec[q].x, rec[q].y, rraw[ROWS ? q : 0]);
                s_slot[spq] = (uint16_t)slot[q];
            }
        __syncthreads();
        for (uint32_t j = tid; j < tile_n; j += kSplitTpb) {
            const uint32_t d = s_slot[j];
            part[s_off[d] - s_cnt[d] + j] = s_stage[j];
        }
        __syncthreads();
        // advance the run cursors by the tile's counts (count = next start - own start; the last
        // touched entry ends at tile_n), then clear the counters for the next tile
#pragma unroll 1
        for (int i = 0; i < per; ++i)
            if (d0 + i <= r.y) {
                const int d = d0 + i;
                s_off[d] += (d == r.y ? tile_n : s_cnt[d + 1]) - s_cnt[d];
            }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < per; ++i)
            if (d0 + i <= r.y) s_cnt[d0 + i] = 0;
        __syncthreads();
    }
}

// step 4 outputs.  kValMask: bits of a record's value that order it; kRows: 16-byte records whose second half is
// the carried row (row(): the row of final position k); node_start(): the row pointer of a node, entry N = E
template <bool ROWS>
struct OutCsr {   // first sort
    static constexpr uint32_t kValMask = 0x7fffffffu;
    static constexpr bool kRows = ROWS;
    int32_t *perm, *tgt, *src, *rowptr;
    uint32_t pmask;
    uint8_t *label_csr;
    uint16_t *rows_csr;
    int rows_out_stride;
    __device__ __forceinline__ void ranked(uint32_t k, uint32_t val, uint32_t hi) const {
        perm[k] = (int32_t)(val & kValMask);
        src[k] = (int32_t)(hi & pmask);
        if (label_csr) label_csr[k] = (uint8_t)(val >> 31);
    }
    __device__ __forceinline__ void row(uint32_t k, uint2 r) const {
        if (ROWS) *reinterpret_cast<uint2 *>(rows_csr + (size_t)k * rows_out_stride) = r;
    }
    __device__ __forceinline__ void slot(uint32_t k, uint32_t node) const { tgt[k] = (int32_t)node; }
    __device__ __forceinline__ void node_start(int64_t node, uint32_t pos) const { rowptr[node] = (int32_t)pos; }
};
struct OutSrc {   // second sort
    static constexpr uint32_t kValMask = 0xffffffffu;
    static constexpr bool kRows = false;
    int32_t *spos, *spos_inv, *rowptr;
    __device__ __forceinline__ void ranked(uint32_t k, uint32_t val, uint32_t) const {
        spos[k] = (int32_t)val;
        if (spos_inv) spos_inv[val] = (int32_t)k;
    }
    __device__ __forceinline__ void row(uint32_t, uint2) const {}
    __device__ __forceinline__ void slot(uint32_t, uint32_t) const {}
    __device__ __forceinline__ void node_start(int64_t node, uint32_t pos) const { rowptr[node] = (int32_t)pos; }
};

// step 4: the four regimes of gi_bucket_sort_kernel.  Common arguments: `part` = the bucket's region as 8-byte
// halves (half kRS * i is record i's {value, low | payload}, the half behind it its row), base = its first output
// position, M = its records, node0 = its first node, s_hist / s_start = records per node / first record of a node
// inside the bucket, s_rec = the record image.
template <class O>
constexpr uint32_t kGiRS = O::kRows ? 2 : 1;
// records a group of nodes may hold: with carried rows the last third of the record image holds 32-bit positions in
// the bucket's region (the row is fetched from its record at write-out)
template <class O>
constexpr uint32_t kGiCapG = O::kRows ? (uint32_t)kCap * 2 / 3 : (uint32_t)kCap;

// The bucket fits the image (M <= kCap).  rec / rrow: the thread's records as loaded (record tid + q * kSortTpb),
// ord: their order of arrival inside their node's list.
template <class O>
__device__ __forceinline__ void gi_sort_fits(uint2 (&rec)[kSortR], const uint2 (&rrow)[O::kRows ? kSortR : 1],
                                             uint32_t (&ord)[kSortR], uint32_t base, uint32_t M, uint32_t node0,
                                             int pbits, const uint32_t *s_hist, const uint32_t *s_start, uint2 *s_rec,
                                             uint16_t *s_fin, const O &out) {
    constexpr uint32_t VM = O::kValMask;
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kSortR; ++q)
        if (tid + q * kSortTpb < M) {
            const uint32_t sl = s_start[rec[q].y >> pbits] + ord[q];
            s_rec[sl] = rec[q];
            ord[q] = sl;
        }
    __syncthreads();
    // rank every record inside its node's list, then bring the image into the final order in place, so
    // that the arrays leave with consecutive lanes on consecutive positions (a wave's store touches a few
    // lines instead of up to 64)
    uint32_t dst[kSortR];
#pragma unroll
    for (int q = 0; q < kSortR; ++q) {
        const uint32_t j = tid + q * kSortTpb;
        if (j < M) {
            const uint2 r = s_rec[j];
            const uint32_t low = r.y >> pbits, st = s_start[low], n = s_hist[low];
            uint32_t cnt = 0;
            for (uint32_t t = 0; t < n; ++t) cnt += (s_rec[st + t].x & VM) < (r.x & VM) ? 1u : 0u;
            rec[q] = r;
            dst[q] = st + cnt;
            if (O::kRows) s_fin[j] = (uint16_t)dst[q];
            out.slot(base + j, node0 + low);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSortR; ++q)
        if (tid + q * kSortTpb < M) s_rec[dst[q]] = rec[q];
    __syncthreads();
    for (uint32_t j = tid; j < M; j += kSortTpb) {
        const uint2 r = s_rec[j];
        out.ranked(base + j, r.x, r.y);
    }
    if (O::kRows) {   // the rows through the same image, from the threads that hold them
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kSortR; ++q)
            if (tid + q * kSortTpb < M) s_rec[s_fin[ord[q]]] = rrow[O::kRows ? q : 0];
        __syncthreads();
        for (uint32_t j = tid; j < M; j += kSortTpb) out.row(base + j, s_rec[j]);
    }
}

// A group of consecutive nodes g0 .. g1 - 1 whose lists fit the image together: one pass over the bucket's records
// (served by the L2) collects them.  s_cur: a cursor per node.
template <class O>
__device__ __forceinline__ void gi_sort_group(const uint2 *__restrict__ part, uint32_t base, uint32_t M, uint32_t node0,
                                              int pbits, int g0, int g1, const uint32_t *s_hist,
                                              const uint32_t *s_start, uint32_t *s_cur, uint2 *s_rec, const O &out) {
    constexpr uint32_t VM = O::kValMask, kRS = kGiRS<O>;
    const int tid = threadIdx.x;
    uint32_t *s_pos32 = reinterpret_cast<uint32_t *>(s_rec + kGiCapG<O>);
    const uint32_t st0 = s_start[g0], n_g = (g1 < kBins ? s_start[g1] : M) - st0;
    __syncthreads();
    if (tid < kBins) s_cur[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < M; i += kSortTpb) {
        const uint2 r = part[(size_t)i * kRS];
        const int low = (int)(r.y >> pbits);
        if (low >= g0 && low < g1) {
            const uint32_t sl = s_start[low] - st0 + atomicAdd(&s_cur[low], 1u);
            s_rec[sl] = r;
            if (O::kRows) s_pos32[sl] = i;
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < n_g; j += kSortTpb) {
        const uint2 r = s_rec[j];
        const uint32_t low = r.y >> pbits, st = s_start[low] - st0, n = s_hist[low];
        uint32_t cnt = 0;
        for (uint32_t t = 0; t < n; ++t) cnt += (s_rec[st + t].x & VM) < (r.x & VM) ? 1u : 0u;
        out.ranked(base + st0 + st + cnt, r.x, r.y);
        if (O::kRows) out.row(base + st0 + st + cnt, part[(size_t)s_pos32[j] * kRS + (kRS - 1)]);
        out.slot(base + st0 + j, node0 + low);
    }
}

// A hub: node g0's list alone exceeds the image.
// The bucket's region is a sequence of runs, one per CHUNK of the edge list, in chunk order (step 2's scan lays
// (bucket, chunk) out chunk after chunk), and a record's value - an edge id / a CSR position - says which chunk it
// came from: value / chunk.  So a hub record's rank is the number of hub records in earlier runs (a histogram over
// the chunks) + the number of hub records of its OWN run with a smaller value.  (Comparing every hub record with
// every record of the bucket is O(M^2 / 512) per workgroup - seconds for a million-edge hub.)
// gi_hub_runs leaves h_all[ck] = first record of chunk ck's run, h_hub[ck] = hub records in the runs before it.
template <class O>
__device__ __forceinline__ void gi_hub_runs(const uint2 *__restrict__ part, uint32_t M, int pbits, int chunk, int g0,
                                            uint32_t *h_all, uint32_t *h_hub) {
    constexpr uint32_t VM = O::kValMask, kRS = kGiRS<O>;
    const int tid = threadIdx.x;
    __syncthreads();
    for (int t = tid; t < 2 * kMaxChunks; t += kSortTpb) h_all[t] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < M; i += kSortTpb) {
        const uint2 r = part[(size_t)i * kRS];
        const uint32_t ck = (r.x & VM) / (uint32_t)chunk;
        atomicAdd(&h_all[ck], 1u);
        if ((int)(r.y >> pbits) == g0) atomicAdd(&h_hub[ck], 1u);
    }
    __syncthreads();
    if (tid == 0) {   // exclusive scans over at most 512 chunks
        uint32_t a_ = 0, h_ = 0;
        for (int ck = 0; ck < kMaxChunks; ++ck) {
            const uint32_t va = h_all[ck], vh = h_hub[ck];
            h_all[ck] = a_;
            h_hub[ck] = h_;
            a_ += va;
            h_ += vh;
        }
    }
    __syncthreads();
}
// ... the rank inside the own run by a walk over that run only (pos0 = the hub's first output position)
template <class O>
__device__ __forceinline__ void gi_hub_walk(const uint2 *__restrict__ part, uint32_t pos0, uint32_t M, int pbits,
                                            int chunk, int g0, const uint32_t *h_all, const uint32_t *h_hub,
                                            const O &out) {
    constexpr uint32_t VM = O::kValMask, kRS = kGiRS<O>;
    for (uint32_t i = threadIdx.x; i < M; i += kSortTpb) {
        const uint2 r = part[(size_t)i * kRS];
        if ((int)(r.y >> pbits) != g0) continue;
        const uint32_t ck = (r.x & VM) / (uint32_t)chunk;
        const uint32_t r0 = h_all[ck], r1 = ck + 1 < (uint32_t)kMaxChunks ? h_all[ck + 1] : M;
        uint32_t cnt = h_hub[ck];
        for (uint32_t t = r0; t < r1; ++t) {
            const uint2 q = part[(size_t)t * kRS];
            cnt += ((int)(q.y >> pbits) == g0 && (q.x & VM) < (r.x & VM)) ? 1u : 0u;
        }
        out.ranked(pos0 + cnt, r.x, r.y);
        if (O::kRows) out.row(pos0 + cnt, part[(size_t)i * kRS + (kRS - 1)]);
    }
}
// ... a large hub (n records): the values of a run are distinct ids of ONE chunk, so the hub records of a run are
// the set bits of a bitmap over the chunk's id range (spans of 128 K ids: 16 KB of LDS) and a record's rank inside
// its run is the number of set bits below its own - linear in the bucket's size (a 2 M-edge hub: 5 s with the walk
// above, milliseconds this way).  bm: the span's bitmap, pw: the exclusive prefix of its words' bit counts.
constexpr uint32_t kHubSpanW = 4096, kHubSpan = kHubSpanW * 32;
template <class O>
__device__ __forceinline__ void gi_hub_bitmaps(const uint2 *__restrict__ part, uint32_t pos0, uint32_t M, uint32_t n,
                                               int pbits, int chunk, int g0, const uint32_t *h_all,
                                               const uint32_t *h_hub, uint32_t *bm, uint32_t *pw, const O &out) {
    constexpr uint32_t VM = O::kValMask, kRS = kGiRS<O>, kSpanW = kHubSpanW, kSpan = kHubSpan;
    const int tid = threadIdx.x;
    for (int ck = 0; ck < kMaxChunks; ++ck) {
        const uint32_t r0 = h_all[ck], r1 = ck + 1 < kMaxChunks ? h_all[ck + 1] : M;
        const uint32_t hub_here = (ck + 1 < kMaxChunks ? h_hub[ck + 1] : n) - h_hub[ck];
        if (hub_here == 0u) continue;   // (uniform)
        uint32_t before = h_hub[ck];
        for (uint32_t lo = (uint32_t)ck * (uint32_t)chunk, sub = 0; sub < (uint32_t)chunk; sub += kSpan, lo += kSpan) {
            __syncthreads();
            for (uint32_t w = tid; w < kSpanW; w += kSortTpb) bm[w] = 0u;
            __syncthreads();
            for (uint32_t t = r0 + tid; t < r1; t += kSortTpb) {
                const uint2 q = part[(size_t)t * kRS];
                const uint32_t d = (q.x & VM) - lo;
                if ((int)(q.y >> pbits) == g0 && d < kSpan) atomicOr(&bm[d >> 5], 1u << (d & 31u));
            }
            __syncthreads();
            // exclusive prefix of the words' bit counts: eight words per thread + a scan of the
            // 512 thread sums through pw's upper half
            uint32_t mine = 0;
            constexpr uint32_t kPer = kSpanW / kSortTpb;
            for (uint32_t j = 0; j < kPer; ++j) mine += (uint32_t)__popc(bm[tid * kPer + j]);
            uint32_t *ts = pw;   // thread sums, scanned in place
            ts[tid] = mine;
            __syncthreads();
            for (uint32_t off = 1; off < (uint32_t)kSortTpb; off <<= 1) {
                const uint32_t v = tid >= (int)off ? ts[tid - off] : 0u;
                __syncthreads();
                ts[tid] += v;
                __syncthreads();
            }
            const uint32_t excl = ts[tid] - mine, span_total = ts[kSortTpb - 1];
            __syncthreads();
            uint32_t run_ = excl;
            for (uint32_t j = 0; j < kPer; ++j) {
                const uint32_t w = tid * kPer + j, c_ = (uint32_t)__popc(bm[w]);
                pw[w] = run_;
                run_ += c_;
            }
            __syncthreads();
            for (uint32_t t = r0 + tid; t < r1; t += kSortTpb) {
                const uint2 q = part[(size_t)t * kRS];
                const uint32_t d = (q.x & VM) - lo;
                if ((int)(q.y >> pbits) == g0 && d < kSpan) {
                    const uint32_t w = d >> 5;
                    const uint32_t below = (uint32_t)__popc(bm[w] & ((1u << (d & 31u)) - 1u));
                    out.ranked(pos0 + before + pw[w] + below, q.x, q.y);
                    if (O::kRows) out.row(pos0 + before + pw[w] + below, part[(size_t)t * kRS + (kRS - 1)]);
                }
            }
            before += span_total;
        }
    }
}

template <class O>
__global__ __launch_bounds__(kSortTpb) void gi_bucket_sort_kernel(const typename GiRec<O::kRows>::type *__restrict__ part_,
                                                                  const uint32_t *__restrict__ base_arr, int NB,
                                                                  int64_t N, int64_t E, int pbits, int chunk, O out) {
    constexpr uint32_t kRS = kGiRS<O>;
    const uint2 *__restrict__ part = reinterpret_cast<const uint2 *>(part_);
    __shared__ uint32_t s_hist[kBins], s_start[kBins], s_wsum[kBins / 64], s_cur[kBins];
    __shared__ uint2 s_rec[kCap];
    __shared__ uint16_t s_fin[O::kRows ? kCap : 1];   // slot after the first placement -> final slot
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t base = base_arr[b], M = base_arr[b + 1] - base;
    part += (size_t)base * kRS;   // (the bucket's region)
    const uint32_t node0 = (uint32_t)b << kSH;
    const bool fits = M <= (uint32_t)kCap;
    if (tid < kBins) s_hist[tid] = 0;
    __syncthreads();
    // the bucket's records: all loads of a thread in flight at once, kept in registers until placed
    // (with rows: the row half stays with the thread that loaded it until the record's final slot is known)
    uint2 rec[kSortR], rrow[O::kRows ? kSortR : 1];
    uint32_t ord[kSortR];
    if (fits) {
#pragma unroll
        for (int q = 0; q < kSortR; ++q) {
            const uint32_t i = tid + q * kSortTpb;
            if constexpr (O::kRows) {
                const uint4 v = i < M ? part_[base + i] : uint4{0u, 0u, 0u, 0u};
                rec[q] = uint2{v.x, v.y};
                rrow[q] = uint2{v.z, v.w};
            } else {
                rec[q] = i < M ? part[i] : uint2{0u, 0u};
            }
        }
#pragma unroll
        for (int q = 0; q < kSortR; ++q)
            if (tid + q * kSortTpb < M) ord[q] = atomicAdd(&s_hist[rec[q].y >> pbits], 1u);
    } else {
        for (uint32_t i = tid; i < M; i += kSortTpb) atomicAdd(&s_hist[part[(size_t)i * kRS].y >> pbits], 1u);
    }
    __syncthreads();
    // exclusive scan of the 256 node counts (waves 0..3: shuffle scan + wave totals)
    uint32_t inc = 0, cnt_mine = 0;
    if (tid < kBins) {
        cnt_mine = s_hist[tid];
        inc = cnt_mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl(inc, lane - d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_wsum[wv] = inc;
    }
    __syncthreads();
    if (tid < kBins) {
        uint32_t pre = 0;
#pragma unroll
        for (int w = 0; w < kBins / 64; ++w) pre += w < wv ? s_wsum[w] : 0u;
        const uint32_t st = pre + inc - cnt_mine;
        s_start[tid] = st;
        if ((int64_t)node0 + tid < N) out.node_start(node0 + tid, base + st);
    }
    if (b == NB - 1 && tid == 0) out.node_start(N, (uint32_t)E);
    __syncthreads();
    if (fits) {
        gi_sort_fits(rec, rrow, ord, base, M, node0, pbits, s_hist, s_start, s_rec, s_fin, out);
    } else {
        // a bucket beyond the LDS capacity: groups of consecutive nodes whose lists fit are taken one
        // after the other; a single node beyond the capacity is a hub
        int g0 = 0;
        while (g0 < kBins) {
            const uint32_t st0 = s_start[g0];
            int g1 = g0;
            while (g1 < kBins && (g1 + 1 < kBins ? s_start[g1 + 1] : M) - st0 <= kGiCapG<O>) ++g1;
            if (g1 == g0) {
                const uint32_t n = s_hist[g0];
                // (s_rec is free here: the chunk histograms, the bitmap of a span and its prefix)
                uint32_t *h_all = reinterpret_cast<uint32_t *>(s_rec), *h_hub = h_all + kMaxChunks;
                uint32_t *bm = h_hub + kMaxChunks, *pw = bm + kHubSpanW;
                static_assert((2 * kMaxChunks + 2 * kHubSpanW) * sizeof(uint32_t) <= kCap * sizeof(uint2),
                              "hub scratch exceeds s_rec");
                gi_hub_runs<O>(part, M, pbits, chunk, g0, h_all, h_hub);
                if (n <= (uint32_t)GNNTRK_GI_HUB_BITMAP_MIN)
                    gi_hub_walk(part, base + st0, M, pbits, chunk, g0, h_all, h_hub, out);
                else
                    gi_hub_bitmaps(part, base + st0, M, n, pbits, chunk, g0, h_all, h_hub, bm, pw, out);
                for (uint32_t j = tid; j < n; j += kSortTpb) out.slot(base + st0 + j, node0 + (uint32_t)g0);
                __syncthreads();   // (the histograms lived in s_rec: the next group refills it)
                g0 += 1;
                continue;
            }
            gi_sort_group(part, base, M, node0, pbits, g0, g1, s_hist, s_start, s_cur, s_rec, out);
            g0 = g1;
        }
    }
}

constexpr size_t kHeader = 256;   // flag words in front of a sort's workspace (first word: ids out of range)
struct OwnPlan {
    bool ok;      // the own sort can run this shape
    bool dense;   // ... but most buckets would overflow the LDS capacity: the library form is faster
    int NB, n_chunks, chunk, bitsN;
    int64_t T;   // table entries (+ 1 total)
    int n_tiles;
    size_t off_range, off_base, off_tbl, off_sums, off_part, bytes;
};

static int bits_for(int64_t n) {
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return b;
}

static OwnPlan own_plan(int64_t N, int64_t E, bool rows) {
    OwnPlan p{};
    p.ok = false;
    if (N < 1 || E < 1) return p;
    p.bitsN = bits_for(N > 1 ? N : 2);
    if (p.bitsN + kSH > 32) return p;
    p.NB = (int)ceil_div(N, kBins);
    int nc = (int)ceil_div(E, 16384);
    if (nc > kMaxChunks) nc = kMaxChunks;
    int64_t chunk = ceil_div(E, nc);
    chunk = ceil_div(chunk, 4) * 4;   // (a lane of the count / split kernels takes four consecutive edges)
    p.chunk = (int)chunk;
    p.n_chunks = (int)ceil_div(E, chunk);
    p.T = (int64_t)p.NB * p.n_chunks;
    if (p.T > kMaxTable) return p;
    // very dense (multi)graphs: most buckets would overflow the LDS capacity of the bucket sort and take its tiled
    // path.  (The bar was 3/4 of the capacity until round 5: a kNN graph with k = 16 - 200 k hits, 3.07 M edges, at
    // most 4 096 records per bucket of 256 nodes - sat at 0.77 and took the library form: two radix sorts for a
    // graph whose every bucket fits.)
    p.dense = E / p.NB > kCap * 9 / 10;
    p.n_tiles = (int)ceil_div(p.T + 1, kScanTile);
    // (the table follows the 256-byte header - the caller's flag words - so that one fill zeroes both)
    size_t o = kHeader;
    p.off_tbl = o;
    o += align_up((size_t)(p.T + 1) * 4, 256);
    p.off_range = o;
    o += align_up((size_t)p.n_chunks * sizeof(int2), 256);
    p.off_base = o;
    o += align_up((size_t)(p.NB + 1) * 4, 256);
    p.off_sums = o;
    o += align_up((size_t)p.n_tiles * 4, 256);
    p.off_part = o;   // (with carried rows: 16-byte records)
    o += align_up((size_t)E * (rows ? 16 : 8), 256);
    p.bytes = o;
    p.ok = true;
    return p;
}

static uint32_t *own_tbl(const OwnPlan &p, char *ws) { return reinterpret_cast<uint32_t *>(ws + p.off_tbl); }
static int2 *own_range(const OwnPlan &p, char *ws) { return reinterpret_cast<int2 *>(ws + p.off_range); }

// One fill per sort (measured): the table and the `head` bytes in front of it - 0, or the flag words the table follows
static int own_zero(const OwnPlan &p, char *ws, size_t head, hipStream_t stream) {
    return check_hip(hipMemsetAsync(ws + p.off_tbl - head, 0, head + (size_t)(p.T + 1) * 4, stream),
                     "counting sort(memset)");
}

// step 1 over a zeroed table (the renumbered build has gi_remap_count_kernel in its place)
template <class K>
static void own_count(const OwnPlan &p, K keys, int64_t E, char *ws, int *bad, hipStream_t stream) {
    hipLaunchKernelGGL((gi_count_kernel<K>), dim3(p.n_chunks), dim3(kCountTpb), 0, stream, keys, E, p.chunk,
                       p.n_chunks, p.NB, own_tbl(p, ws), own_range(p, ws), bad);
}

// steps 2 - 4 over a counted table
template <class K, class O>
static void own_sort(const OwnPlan &p, K keys, O out, int pbits, int64_t N, int64_t E, char *ws, int *bad,
                     hipStream_t stream) {
    typedef typename GiRec<O::kRows>::type Rec;
    int2 *range = own_range(p, ws);
    uint32_t *tbl = own_tbl(p, ws);
    uint32_t *base = reinterpret_cast<uint32_t *>(ws + p.off_base);
    uint32_t *sums = reinterpret_cast<uint32_t *>(ws + p.off_sums);
    Rec *part = reinterpret_cast<Rec *>(ws + p.off_part);
    hipLaunchKernelGGL(gi_scan_sums_kernel, dim3(p.n_tiles), dim3(kScanTpb), 0, stream, tbl, p.T + 1, sums);
    hipLaunchKernelGGL(gi_scan_apply_kernel, dim3(p.n_tiles), dim3(kScanTpb), 0, stream, tbl, p.T + 1, sums,
                       p.n_chunks, base);
    hipLaunchKernelGGL((gi_split_kernel<K, O::kRows>), dim3(p.n_chunks), dim3(kSplitTpb), 0, stream, keys, E, p.chunk,
                       p.n_chunks, pbits, tbl, range, part, bad);
    hipLaunchKernelGGL((gi_bucket_sort_kernel<O>), dim3(p.NB), dim3(kSortTpb), 0, stream, part, base, p.NB, N, E,
                       pbits, p.chunk, out);
}

// -------------------------------------------- library path (flags bit 0, dense graphs, shapes outside the own sort)
// (ids out of range are counted and clamped, as in the own form; `rank`: see KeysCoo)
__device__ __forceinline__ uint32_t gi_checked(int64_t v, int64_t N, const int32_t *rank, int *bad) {
    v = gi_clamped<false>(v, N, bad);
    return rank ? (uint32_t)rank[v] : (uint32_t)v;
}
__global__ __launch_bounds__(kTpb) void gi_keys_kernel(const int64_t *__restrict__ ids, int64_t E,
                                                       int64_t N, const int32_t *__restrict__ rank,
                                                       uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals,
                                                       int *__restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < E;
         e += (int64_t)gridDim.x * kTpb) {
        keys[e] = gi_checked(ids[e], N, rank, bad);
        vals[e] = (uint32_t)e;
    }
}

// src_sorted[k] = src[perm[k]]; also emits the keys/vals of the second (by-source) sort
__global__ __launch_bounds__(kTpb) void gi_gather_src_kernel(const int64_t *__restrict__ src,
                                                             const uint32_t *__restrict__ perm,
                                                             int64_t E, int64_t N, const int32_t *__restrict__ rank,
                                                             int32_t *__restrict__ src_s,
                                                             uint32_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals,
                                                             int *__restrict__ bad) {
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k < E;
         k += (int64_t)gridDim.x * kTpb) {
        const uint32_t s = gi_checked(src[perm[k]], N, rank, bad);
        src_s[k] = (int32_t)s;
        keys[k] = s;
        vals[k] = (uint32_t)k;
    }
}

// rowptr[n] = first position k with sorted[k] >= n  (sorted ascending, E entries)
__global__ __launch_bounds__(kTpb) void gi_rowptr_kernel(const uint32_t *__restrict__ sorted,
                                                         int64_t E, int64_t N,
                                                         int32_t *__restrict__ rowptr) {
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k <= E;
         k += (int64_t)gridDim.x * kTpb) {
        const int64_t prev = (k == 0) ? -1 : (int64_t)sorted[k - 1];
        const int64_t cur = (k == E) ? N : (int64_t)sorted[k];
        for (int64_t n = prev + 1; n <= cur && n <= N; ++n) rowptr[n] = (int32_t)k;
    }
}

// inv[spos[k]] = k
__global__ __launch_bounds__(kTpb) void gi_invert_kernel(const int32_t *__restrict__ spos, int64_t E,
                                                         int32_t *__restrict__ inv) {
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k < E; k += (int64_t)gridDim.x * kTpb)
        inv[spos[k]] = (int32_t)k;
}

static int stream_grid(int64_t n) {
    int64_t g = ceil_div(n, kTpb);
    const int64_t cap = (int64_t)cu_count() * 8;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

static size_t library_ws_bytes(int64_t E) {
    const size_t arr = align_up((size_t)(E > 0 ? E : 1) * sizeof(uint32_t), 256);
    return 256 /* flags */ + 3 * arr + align_up(sort_pairs_temp_bytes(E), 256);
}

// (carry: bit 0 = carried rows, bit 1 = node_rank given: room for the renumbered int32 edge list behind the plan)
static size_t remap_arr_bytes(int64_t E) { return align_up((size_t)(E > 0 ? E : 1) * sizeof(int32_t), 256); }
static size_t graph_index_ws_bytes(int64_t N, int64_t E, int carry) {
    const size_t lib = library_ws_bytes(E);
    const OwnPlan p = own_plan(N, E, (carry & 1) != 0);
    const size_t own = p.ok ? align_up(p.bytes, 256) + ((carry & 2) ? 2 * remap_arr_bytes(E) : 0) : 0;
    return own > lib ? own : lib;
}

// the carried per-edge inputs behind the library form: plain gathers through perm
__global__ __launch_bounds__(kTpb) void gi_gather_label_kernel(const uint8_t *__restrict__ label,
                                                               const int32_t *__restrict__ perm, int64_t E,
                                                               uint8_t *__restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * kTpb + threadIdx.x; k < E; k += (int64_t)gridDim.x * kTpb)
        out[k] = label[perm[k]] ? 1 : 0;
}

static int library_build(const int64_t *edge_index, const gnntrk_graph_index *o, char *p, int *bad, int64_t N,
                         int64_t E, const int32_t *rank, hipStream_t stream) {
    p += 256;
    const size_t arr = align_up((size_t)(E > 0 ? E : 1) * sizeof(uint32_t), 256);
    uint32_t *keys_a = reinterpret_cast<uint32_t *>(p);
    p += arr;
    uint32_t *vals_a = reinterpret_cast<uint32_t *>(p);
    p += arr;
    uint32_t *keys_b = reinterpret_cast<uint32_t *>(p);
    p += arr;
    void *temp = p;
    const size_t temp_bytes = sort_pairs_temp_bytes(E);
    const int bits = bits_for(N > 1 ? N : 2);
    const int grid = stream_grid(E + 1);
    const int64_t *src = edge_index, *tgt = edge_index + E;
    hipLaunchKernelGGL(gi_keys_kernel, dim3(grid), dim3(kTpb), 0, stream, tgt, E, N, rank, keys_a, vals_a, bad);
    // the sorted keys ARE the CSR targets: sort straight into the output array
    uint32_t *tgt_sorted = reinterpret_cast<uint32_t *>(o->tgt);
    int rc = sort_pairs_u32(keys_a, tgt_sorted, vals_a, reinterpret_cast<uint32_t *>(o->perm), E, bits, temp,
                            temp_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(gi_rowptr_kernel, dim3(grid), dim3(kTpb), 0, stream, tgt_sorted, E, N, o->rowptr_t);
    hipLaunchKernelGGL(gi_gather_src_kernel, dim3(grid), dim3(kTpb), 0, stream, src,
                       reinterpret_cast<const uint32_t *>(o->perm), E, N, rank, o->src, keys_a, vals_a, bad);
    rc = sort_pairs_u32(keys_a, keys_b, vals_a, reinterpret_cast<uint32_t *>(o->spos), E, bits, temp, temp_bytes,
                        stream);
    if (rc) return rc;
    hipLaunchKernelGGL(gi_rowptr_kernel, dim3(grid), dim3(kTpb), 0, stream, keys_b, E, N, o->rowptr_s);
    if (o->spos_inv)
        hipLaunchKernelGGL(gi_invert_kernel, dim3(grid), dim3(kTpb), 0, stream, o->spos, E, o->spos_inv);
    return GNNTRK_OK;
}

static int graph_index_build(const int64_t *edge_index, const gnntrk_graph_index *o,
                             const gnntrk_graph_index_carry *cy, void *ws, size_t ws_bytes, int flags,
                             hipStream_t stream) {
    if (!o) return fail(GNNTRK_EINVAL, "graph_index_build: NULL output descriptor");
    const int64_t E = o->n_edges, N = o->n_nodes;
    if (E < 0 || N < 0 || E > 0x7fffffff || N > 0x7fffffff)
        return fail(GNNTRK_EUNSUPPORTED, "graph_index_build: sizes must fit int32");
    if (!o->rowptr_t || !o->rowptr_s || (E > 0 && (!o->perm || !o->tgt || !o->src || !o->spos)))
        return fail(GNNTRK_EINVAL, "graph_index_build: NULL output array");
    if (E > 0 && !edge_index) return fail(GNNTRK_EINVAL, "graph_index_build: NULL edge_index");
    const uint8_t *label = cy ? cy->edge_label : nullptr;
    const float *rows = cy ? cy->edge_rows : nullptr;
    const int32_t *rank = cy ? cy->node_rank : nullptr;
    if (E > 0 && label && !cy->label_csr) return fail(GNNTRK_EINVAL, "graph_index_build: carried label without output");
    if (E > 0 && rows &&
        (!cy->rows_csr_bf16 || cy->rows_stride < 4 || cy->rows_stride % 4 != 0 || ((uintptr_t)rows & 15) != 0 ||
         cy->out_stride < 4 || cy->out_stride % 4 != 0 || ((uintptr_t)cy->rows_csr_bf16 & 7) != 0))
        return fail(GNNTRK_EINVAL,
                    "graph_index_build: carried rows must be 16-byte aligned fp32 [E, 4] with a row stride that is a "
                    "multiple of 4 floats; the bf16 output 8-byte aligned with a stride that is a multiple of 4");
    if (!ws || ws_bytes < graph_index_ws_bytes(N, E, (rows ? 1 : 0) | (rank ? 2 : 0)))
        return fail(GNNTRK_EINVAL, "graph_index_build: workspace too small");

    char *p = reinterpret_cast<char *>(ws);
    int *bad = reinterpret_cast<int *>(p);   // (the header's first word)
    int rc = GNNTRK_OK;
    const OwnPlan plan = own_plan(N, E, rows != nullptr);
    const bool own = E > 0 && plan.ok && !(flags & 1) && (!plan.dense || (flags & 2));
    if (!own) {   // (the own form zeroes the flag words together with its table)
        rc = check_hip(hipMemsetAsync(bad, 0, kHeader, stream), "graph_index_build(memset)");
        if (rc) return rc;
    }
    if (E > 0) {
        if (own) {
            const int vec = (((uintptr_t)edge_index | (uintptr_t)(edge_index + E)) & 15) == 0 &&
                            (!label || ((uintptr_t)label & 3) == 0);
            const KeysCoo k1{edge_index, edge_index + E, N, label, rows, rows ? cy->rows_stride : 0, vec, nullptr};
            const uint32_t pmask = (uint32_t)(((uint64_t)1 << plan.bitsN) - 1);
            const OutCsr<true> o1r{o->perm, o->tgt, o->src, o->rowptr_t, pmask, label ? cy->label_csr : nullptr,
                                   rows ? cy->rows_csr_bf16 : nullptr, rows ? cy->out_stride : 0};
            const OutCsr<false> o1{o->perm, o->tgt, o->src, o->rowptr_t, pmask, label ? cy->label_csr : nullptr,
                                   nullptr, 0};
            // the record width once: 16-byte records where rows are carried
            auto first_sort = [&](auto keys) {
                if (rows)
                    own_sort(plan, keys, o1r, plan.bitsN, N, E, p, bad, stream);
                else
                    own_sort(plan, keys, o1, plan.bitsN, N, E, p, bad, stream);
            };
            rc = own_zero(plan, p, kHeader, stream);
            if (rc) return rc;
            if (rank) {   // renumbered: one pass writes the translated int32 list and counts it, the sort reads that
                int32_t *src32 = reinterpret_cast<int32_t *>(p + align_up(plan.bytes, 256));
                int32_t *tgt32 = reinterpret_cast<int32_t *>(p + align_up(plan.bytes, 256) + remap_arr_bytes(E));
                const int vec_ids = (((uintptr_t)edge_index | (uintptr_t)(edge_index + E)) & 15) == 0;
                hipLaunchKernelGGL(gi_remap_count_kernel, dim3(gi_chunk_grid(plan.n_chunks)), dim3(kRemapTpb), 0, stream, edge_index,
                                   edge_index + E, E, N, rank, vec_ids, src32, tgt32, plan.chunk, plan.n_chunks,
                                   own_tbl(plan, p), own_range(plan, p), bad);
                first_sort(KeysCoo32{src32, tgt32, label, rows, rows ? cy->rows_stride : 0,
                                     (!label || ((uintptr_t)label & 3) == 0) ? 1 : 0});
            } else {
                own_count(plan, k1, E, p, bad, stream);
                first_sort(k1);
            }
            const KeysCsr k2{o->src};
            const OutSrc o2{o->spos, o->spos_inv, o->rowptr_s};
            rc = own_zero(plan, p, 0, stream);
            if (rc) return rc;
            own_count(plan, k2, E, p, bad, stream);
            own_sort(plan, k2, o2, 0, N, E, p, bad, stream);
        } else {
            rc = library_build(edge_index, o, p, bad, N, E, rank, stream);
            if (rc) return rc;
            if (label)
                hipLaunchKernelGGL(gi_gather_label_kernel, dim3(stream_grid(E)), dim3(kTpb), 0, stream, label, o->perm, E,
                                   cy->label_csr);
            if (rows)
                rc = rows_to_bf16_launch(rows, 4, cy->rows_stride, o->perm, E, cy->rows_csr_bf16, cy->out_stride, stream);
        }
        if (rc) return rc;
    } else {
        rc = check_hip(hipMemsetAsync(o->rowptr_t, 0, (size_t)(N + 1) * 4, stream), "memset");
        if (rc) return rc;
        rc = check_hip(hipMemsetAsync(o->rowptr_s, 0, (size_t)(N + 1) * 4, stream), "memset");
        if (rc) return rc;
    }
    return check_launch("graph_index_build");
}

// ------------------------------------------------------------------ collation of per-event indices
// A collated batch is a list of disjoint graphs with contiguous id / edge ranges, so its stable target sort, its
// source sort and their inverse are the events' own, shifted: one streaming pass per event places a cached
// per-event index into the batch arrays (20 B/edge + 8 B/node read and written, + the carried label / row bytes)
// instead of sorting the batch again (gnntrk_graph_index_place).
__global__ __launch_bounds__(kTpb) void gi_place_kernel(gnntrk_graph_index part, gnntrk_graph_index batch, int32_t noff,
                                                        int32_t eoff, const uint8_t *__restrict__ lab_in,
                                                        uint8_t *__restrict__ lab_out, const uint2 *__restrict__ rows_in,
                                                        uint2 *__restrict__ rows_out, const int32_t *__restrict__ nperm_in,
                                                        int32_t *__restrict__ nperm_out, const int32_t *__restrict__ nrank_in,
                                                        int32_t *__restrict__ nrank_out) {
    const int64_t E = part.n_edges, N = part.n_nodes;
    const int64_t n4 = (E + 3) / 4;
    const bool vec = ((eoff & 3) == 0);   // (16-byte aligned destinations)
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kTpb) {
        const int64_t k = 4 * i;
        if (vec && k + 4 <= E) {
            auto mv = [&](const int32_t *src, int32_t *dst, int32_t add) {
                int4 v = *reinterpret_cast<const int4 *>(src + k);
                v.x += add;
                v.y += add;
                v.z += add;
                v.w += add;
                *reinterpret_cast<int4 *>(dst + eoff + k) = v;
            };
            mv(part.perm, batch.perm, eoff);
            mv(part.tgt, batch.tgt, noff);
            mv(part.src, batch.src, noff);
            mv(part.spos, batch.spos, eoff);
            if (part.spos_inv && batch.spos_inv) mv(part.spos_inv, batch.spos_inv, eoff);
            if (lab_in) *reinterpret_cast<uint32_t *>(lab_out + eoff + k) = *reinterpret_cast<const uint32_t *>(lab_in + k);
            if (rows_in) {
#pragma unroll
                for (int q = 0; q < 4; ++q) rows_out[eoff + k + q] = rows_in[k + q];
            }
        } else {
            for (int q = 0; q < 4 && k + q < E; ++q) {
                const int64_t j = k + q;
                batch.perm[eoff + j] = part.perm[j] + eoff;
                batch.tgt[eoff + j] = part.tgt[j] + noff;
                batch.src[eoff + j] = part.src[j] + noff;
                batch.spos[eoff + j] = part.spos[j] + eoff;
                if (part.spos_inv && batch.spos_inv) batch.spos_inv[eoff + j] = part.spos_inv[j] + eoff;
                if (lab_in) lab_out[eoff + j] = lab_in[j];
                if (rows_in) rows_out[eoff + j] = rows_in[j];
            }
        }
    }
    for (int64_t n = (int64_t)blockIdx.x * kTpb + threadIdx.x; n <= N; n += (int64_t)gridDim.x * kTpb) {
        batch.rowptr_t[noff + n] = part.rowptr_t[n] + eoff;   // (entry N of an event = entry 0 of the next: same value)
        batch.rowptr_s[noff + n] = part.rowptr_s[n] + eoff;
        if (n < N && nperm_in) {
            nperm_out[noff + n] = nperm_in[n] + noff;
            nrank_out[noff + n] = nrank_in[n] + noff;
        }
    }
}
// ------------------------------------------------------------------ node order (gnntrk_node_order)
// Per-event renumbering of the nodes by a caller-supplied key (one float per node: the hits' azimuth for
// tracking graphs, whose edges join hits of neighbouring azimuth): new ids = rank of (event, key, old id).
// One 64-bit radix sort of N pairs; the graph-index build then reads every node id through `rank`
// (gnntrk_graph_index_carry.node_rank), so neighbouring nodes of the graph get neighbouring rows - the
// gathers of x[src] and the source-sorted gradient stores become local.
// The order-preserving integer image of a float (NaNs at the ends), and its inverse
__device__ __forceinline__ uint32_t no_image(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float no_unimage(uint32_t u) {
    return __uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u);
}
__global__ __launch_bounds__(kTpb) void no_keys_kernel(const float *__restrict__ key, int64_t stride,
                                                       const int64_t *__restrict__ batch, int64_t n,
                                                       unsigned long long *__restrict__ keys,
                                                       uint32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const uint32_t u = no_image(key[i * stride]);
        const unsigned long long b = batch ? (unsigned long long)(uint32_t)batch[i] : 0ull;
        keys[i] = (b << 32) | u;
        vals[i] = (uint32_t)i;
    }
}
// the same as ONE 32-bit key where the event ids need at most eight bits: event in the top `ebits` bits, below it
// the top 32 - ebits bits of the key's order-preserving image (>= 24: sign, exponent and 15 mantissa bits - keys
// that agree that far keep their old order) - four radix passes over 4-byte keys instead of five over 8-byte ones
__global__ __launch_bounds__(kTpb) void no_keys32_kernel(const float *__restrict__ key, int64_t stride,
                                                         const int64_t *__restrict__ batch, int64_t n, int ebits,
                                                         uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const uint32_t u = no_image(key[i * stride]);
        const uint32_t b = (batch && ebits > 0) ? (uint32_t)batch[i] << (32 - ebits) : 0u;
        keys[i] = b | (ebits > 0 ? u >> ebits : u);
        vals[i] = (uint32_t)i;
    }
}
__global__ __launch_bounds__(kTpb) void no_finish_kernel(const uint32_t *__restrict__ sorted, int64_t n,
                                                         int32_t *__restrict__ perm, int32_t *__restrict__ rank) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const uint32_t v = sorted[i];
        perm[i] = (int32_t)v;
        rank[v] = (int32_t)i;
    }
}
// ---- own form (round 6): a counting sort on a QUANTISED key - locality is all the key has to buy (locality.py), so
// the per-event order need not resolve more than the 65 536 levels of
//     q = trunc((key - lo) * (65535 / (hi - lo))),   lo / hi = min / max of the key over the nodes of the call (fp32),
// and the pair (event, q) is one small integer: the two-level counting sort of the edge lists above takes it as a
// "node id" (records = nodes, value = old id, stable: nodes that share a level keep their old order).  One min / max
// pass, one key pass and the sort's own passes over N records instead of four radix passes of the library.
constexpr int kNoLevels = 1 << 16;
constexpr int kNoMaxEvents = 64;
constexpr size_t kNoHead = 1024;   // bytes of the own form's minima / maxima and flag words
// per EVENT: mm[2 b] = max of the INVERTED order-preserving image of the key (= the minimum), mm[2 b + 1] = max of the
// image; both start from a zero fill.  (Per event, not per call: an event then gets the same levels - hence the same
// order - whether it is ordered alone or inside a collated batch, which is what lets cached per-event indices be
// placed into a batch, gnntrk_graph_index_place.)
// keyc (optional): the key column as a dense array - the key pass then reads 4 bytes per node instead of a line of
// the caller's rows
__global__ __launch_bounds__(kTpb) void no_minmax_kernel(const float *__restrict__ key, int64_t stride,
                                                         const int64_t *__restrict__ batch, int64_t n, int64_t n_events,
                                                         uint32_t *__restrict__ mm, float *__restrict__ keyc) {
    __shared__ uint32_t s_mm[2 * kNoMaxEvents];
    for (int t = threadIdx.x; t < 2 * kNoMaxEvents; t += kTpb) s_mm[t] = 0u;
    __syncthreads();
    for (int64_t i0 = (int64_t)blockIdx.x * kTpb; i0 < n; i0 += (int64_t)gridDim.x * kTpb) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < n;
        const float v = in ? key[i * stride] : 0.f;
        if (in && keyc) keyc[i] = v;
        long long b = (in && batch) ? batch[i] : 0;
        b = b < 0 ? 0 : b >= n_events ? n_events - 1 : b;   // (counted as bad in the key pass)
        const uint32_t u = no_image(v);
        const bool on = in && v == v;   // (NaN keys take the last level, they do not set the range)
        uint32_t nlo = on ? ~u : 0u, hi = on ? u : 0u;
        const int b0 = __shfl((int)b, 0);
        if (__ballot(in && (int)b != b0) == 0ull) {   // one event per wave (the rule): one LDS atomic pair per wave
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t l2 = (uint32_t)__shfl_xor((int)nlo, o), h2 = (uint32_t)__shfl_xor((int)hi, o);
                nlo = l2 > nlo ? l2 : nlo;
                hi = h2 > hi ? h2 : hi;
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMax(&s_mm[2 * b0], nlo);
                atomicMax(&s_mm[2 * b0 + 1], hi);
            }
        } else if (on) {
            atomicMax(&s_mm[2 * (int)b], nlo);
            atomicMax(&s_mm[2 * (int)b + 1], hi);
        }
    }
    __syncthreads();
    // (maxima: the result does not depend on the order of the atomics)
    for (int t = threadIdx.x; t < 2 * kNoMaxEvents; t += kTpb)
        if (s_mm[t]) atomicMax(&mm[t], s_mm[t]);
}
__global__ __launch_bounds__(kTpb) void no_qkeys_kernel(const float *__restrict__ key, int64_t stride,
                                                        const int64_t *__restrict__ batch, int64_t n, int64_t n_events,
                                                        const uint32_t *__restrict__ mm, int32_t *__restrict__ q,
                                                        int *__restrict__ bad) {
    __shared__ float s_lo[kNoMaxEvents], s_scale[kNoMaxEvents];
    for (int t = threadIdx.x; t < kNoMaxEvents; t += kTpb) {
        const uint32_t ulo = ~mm[2 * t], uhi = mm[2 * t + 1];
        const bool any = t < n_events && ulo <= uhi;   // (no finite key in the event: one level)
        const float lo = any ? no_unimage(ulo) : 0.f, hi = any ? no_unimage(uhi) : 0.f;
        s_lo[t] = lo;
        s_scale[t] = hi > lo ? (float)(kNoLevels - 1) / (hi - lo) : 0.f;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const float v = key[i * stride];
        long long b = batch ? batch[i] : 0;
        // (an event id outside the stated count: counted, clamped.  The count stays in the workspace, word 2 *
        // kNoMaxEvents of its head block, and nothing reads it: reading it back would make the host wait)
        if (b < 0 || b >= n_events) {
            atomicAdd(bad, 1);
            b = b < 0 ? 0 : n_events - 1;
        }
        float t = (v - s_lo[b]) * s_scale[b];
        t = t < 0.f ? 0.f : t;
        const uint32_t lvl = (v != v || t >= (float)(kNoLevels - 1)) ? (uint32_t)(kNoLevels - 1) : (uint32_t)t;
        q[i] = (int32_t)((uint32_t)b * (uint32_t)kNoLevels + lvl);
    }
}
struct OutNode {   // the sort's outputs for the node order: perm[new] = old, rank[old] = new
    static constexpr uint32_t kValMask = 0xffffffffu;
    static constexpr bool kRows = false;
    int32_t *perm, *rank;
    __device__ __forceinline__ void ranked(uint32_t k, uint32_t val, uint32_t) const {
        perm[k] = (int32_t)val;
        rank[val] = (int32_t)k;
    }
    __device__ __forceinline__ void row(uint32_t, uint2) const {}
    __device__ __forceinline__ void slot(uint32_t, uint32_t) const {}
    // (nobody asks where an (event, level) pair starts: up to 4 M row pointers per call stay unwritten)
    __device__ __forceinline__ void node_start(int64_t, uint32_t) const {}
};
// (event, level) pairs the own form takes: the table of the counting sort is bounded by it
constexpr int64_t kNoMaxKeys = (int64_t)kNoMaxEvents * kNoLevels;
static bool node_order_own(int64_t n, int64_t n_events, const int64_t *batch, OwnPlan &plan, int64_t &keys) {
    const int64_t ev = batch ? n_events : 1;
    if (ev < 1) return false;   // (event count not stated: the exact radix form)
    if (ev > kNoMaxEvents) return false;
    keys = ev * kNoLevels;
    if (keys > kNoMaxKeys) return false;
    plan = own_plan(keys, n, false);
    return plan.ok && !plan.dense;
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_graph_index_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    return graph_index_ws_bytes(n_nodes, n_edges, 0);
}

size_t gnntrk_graph_index_workspace_bytes_carry(int64_t n_nodes, int64_t n_edges, int32_t carry_rows) {
    return graph_index_ws_bytes(n_nodes, n_edges, carry_rows);
}

int gnntrk_graph_index_build(const int64_t *edge_index, const gnntrk_graph_index *out, void *workspace,
                             size_t workspace_bytes, void *stream) {
    return graph_index_build(edge_index, out, nullptr, workspace, workspace_bytes, 0, (hipStream_t)stream);
}

int gnntrk_graph_index_build_ex(const int64_t *edge_index, const gnntrk_graph_index *out, void *workspace,
                                size_t workspace_bytes, int32_t flags, void *stream) {
    return graph_index_build(edge_index, out, nullptr, workspace, workspace_bytes, flags, (hipStream_t)stream);
}

int gnntrk_graph_index_build_carry(const int64_t *edge_index, const gnntrk_graph_index *out,
                                   const gnntrk_graph_index_carry *carry, void *workspace, size_t workspace_bytes,
                                   int32_t flags, void *stream) {
    return graph_index_build(edge_index, out, carry, workspace, workspace_bytes, flags, (hipStream_t)stream);
}

int gnntrk_graph_index_place(const gnntrk_graph_index *part, int64_t node_offset, int64_t edge_offset,
                             const gnntrk_graph_index *batch, const uint8_t *label_part, uint8_t *label_batch,
                             const uint16_t *rows_part, uint16_t *rows_batch, const int32_t *node_perm_part,
                             int32_t *node_perm_batch, const int32_t *node_rank_part, int32_t *node_rank_batch,
                             void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!part || !batch) return fail(GNNTRK_EINVAL, "graph_index_place: NULL descriptor");
    if (node_offset < 0 || edge_offset < 0 || node_offset + part->n_nodes > batch->n_nodes ||
        edge_offset + part->n_edges > batch->n_edges || batch->n_edges > 0x7fffffff || batch->n_nodes > 0x7fffffff)
        return fail(GNNTRK_EINVAL, "graph_index_place: the event does not fit the batch at these offsets");
    if ((label_part != nullptr) != (label_batch != nullptr) || (rows_part != nullptr) != (rows_batch != nullptr) ||
        (node_perm_part != nullptr) != (node_perm_batch != nullptr) || (node_perm_part != nullptr) != (node_rank_part != nullptr) ||
        (node_rank_part != nullptr) != (node_rank_batch != nullptr))
        return fail(GNNTRK_EINVAL, "graph_index_place: carried / node-order arrays must come in pairs");
    if (rows_part && ((((uintptr_t)rows_part | (uintptr_t)rows_batch) & 7) != 0))
        return fail(GNNTRK_EINVAL, "graph_index_place: carried rows are 8-byte rows");
    const int64_t work = part->n_edges / 4 > part->n_nodes ? part->n_edges / 4 : part->n_nodes;
    hipLaunchKernelGGL(gi_place_kernel, dim3(stream_grid(work + 1)), dim3(kTpb), 0, stream, *part, *batch,
                       (int32_t)node_offset, (int32_t)edge_offset, label_part, label_batch,
                       reinterpret_cast<const uint2 *>(rows_part), reinterpret_cast<uint2 *>(rows_batch), node_perm_part,
                       node_perm_batch, node_rank_part, node_rank_batch);
    return check_launch("graph_index_place");
}

size_t gnntrk_node_order_workspace_bytes(int64_t n_nodes) {
    const size_t m = (size_t)(n_nodes > 0 ? n_nodes : 1);
    const size_t t64 = sort_pairs_u64_temp_bytes(n_nodes), t32 = sort_pairs_temp_bytes(n_nodes);
    const size_t lib = 2 * align_up(m * 8, 256) + 2 * align_up(m * 4, 256) + align_up(t64 > t32 ? t64 : t32, 256);
    // own form: min / max + flag words | the sort's plan | quantised keys | dense keys
    const OwnPlan p = own_plan(kNoMaxKeys, n_nodes > 0 ? n_nodes : 1, false);
    const size_t own = kNoHead + (p.ok ? align_up(p.bytes, 256) : 0) + 2 * align_up(m * 4, 256);
    return lib > own ? lib : own;
}

int gnntrk_node_order(const float *key, int64_t key_stride, const int64_t *batch, int64_t n_events, int64_t n_nodes,
                      int32_t *perm, int32_t *rank, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_nodes < 0 || n_nodes > 0x7fffffff) return fail(GNNTRK_EUNSUPPORTED, "node_order: sizes must fit int32");
    if (n_nodes == 0) return GNNTRK_OK;
    if (!key || key_stride < 1 || !perm || !rank) return fail(GNNTRK_EINVAL, "node_order: NULL argument");
    if (!workspace || workspace_bytes < gnntrk_node_order_workspace_bytes(n_nodes))
        return fail(GNNTRK_EINVAL, "node_order: workspace too small");
    char *p = reinterpret_cast<char *>(workspace);
    const int grid = stream_grid(n_nodes);
    OwnPlan plan;
    int64_t n_keys = 0;
    if (node_order_own(n_nodes, n_events, batch, plan, n_keys)) {
        // per event {~min image, max image}; [128]: bad event ids.  The sort's header is the end of this block, so that
        // its table follows the block and the sort's one fill zeroes the minima / maxima, the flag word and the table
        static_assert((2 * kNoMaxEvents + 1) * sizeof(uint32_t) <= kNoHead - kHeader, "the head block holds the minima / maxima and the flag word");
        uint32_t *mm = reinterpret_cast<uint32_t *>(p);
        int *bad = reinterpret_cast<int *>(mm + 2 * kNoMaxEvents);
        char *sort_ws = p + kNoHead - kHeader;
        const size_t arr = align_up((size_t)n_nodes * 4, 256);
        int32_t *q = reinterpret_cast<int32_t *>(p + kNoHead + align_up(plan.bytes, 256));
        float *keyc = reinterpret_cast<float *>(reinterpret_cast<char *>(q) + arr);
        const int rc = own_zero(plan, sort_ws, kNoHead, stream);
        if (rc) return rc;
        const int64_t ev = batch ? n_events : 1;
        // (the min / max pass leaves the key column as a dense array: the key pass then reads 4 bytes per node
        // instead of a line of the caller's rows)
        hipLaunchKernelGGL(no_minmax_kernel, dim3(grid), dim3(kTpb), 0, stream, key, key_stride, batch, n_nodes, ev,
                           mm, keyc);
        hipLaunchKernelGGL(no_qkeys_kernel, dim3(grid), dim3(kTpb), 0, stream, keyc, (int64_t)1, batch, n_nodes, ev, mm,
                           q, bad);
        const KeysCsr keys{q};
        own_count(plan, keys, n_nodes, sort_ws, bad, stream);
        own_sort(plan, keys, OutNode{perm, rank}, 0, n_keys, n_nodes, sort_ws, bad, stream);
        return check_launch("node_order");
    }
    const size_t k8 = align_up((size_t)n_nodes * 8, 256), v4 = align_up((size_t)n_nodes * 4, 256);
    unsigned long long *ka = reinterpret_cast<unsigned long long *>(p), *kb = reinterpret_cast<unsigned long long *>(p + k8);
    uint32_t *va = reinterpret_cast<uint32_t *>(p + 2 * k8), *vb = reinterpret_cast<uint32_t *>(p + 2 * k8 + v4);
    void *temp = p + 2 * k8 + 2 * v4;
    // sorted bits: the 32 of the key + what the event ids need (n_events <= 0: not stated - all 32)
    int ebits = batch ? 32 : 0;
    if (batch && n_events > 0) {
        ebits = 0;
        while (ebits < 32 && ((int64_t)1 << ebits) < n_events) ++ebits;
    }
    int rc;
    if (ebits <= 8) {   // one 32-bit key (see no_keys32_kernel)
        uint32_t *k32a = reinterpret_cast<uint32_t *>(ka), *k32b = reinterpret_cast<uint32_t *>(kb);
        hipLaunchKernelGGL(no_keys32_kernel, dim3(grid), dim3(kTpb), 0, stream, key, key_stride, batch, n_nodes, ebits,
                           k32a, va);
        rc = sort_pairs_u32(k32a, k32b, va, vb, n_nodes, 32, temp, sort_pairs_temp_bytes(n_nodes), stream);
    } else {
        hipLaunchKernelGGL(no_keys_kernel, dim3(grid), dim3(kTpb), 0, stream, key, key_stride, batch, n_nodes, ka, va);
        rc = sort_pairs_u64_bits(ka, kb, va, vb, n_nodes, 32 + ebits, temp, sort_pairs_u64_temp_bytes(n_nodes), stream);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(no_finish_kernel, dim3(grid), dim3(kTpb), 0, stream, vb, n_nodes, perm, rank);
    return check_launch("node_order");
}

}  // extern "C"
