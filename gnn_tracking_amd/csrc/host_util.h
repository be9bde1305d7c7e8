// Host-side helpers shared by the translation units of libgnntrk.so: thread-local last-error string, launch
// checking, device queries (host_util.hip), and the few workers that one unit defines and another calls.
// The C entries are not declared here: each is defined once, in its unit, against its prototype in gnntrk.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "gnntrk.h"

namespace gnntrk {

// records msg as the thread's last error and returns code
int fail(int code, const char *msg);
// hipGetLastError() -> GNNTRK_OK / GNNTRK_EHIP / GNNTRK_ENOMEM (+ message)
int check_launch(const char *what);
int check_hip(hipError_t e, const char *what);
int cu_count();

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// grid of a grid-stride kernel over n items: one workgroup of tpb threads per tpb items, at least one, at
// most per_cu per compute unit
inline int blocks_for(int64_t n, int per_cu, int tpb = 256) {
    const int64_t g = ceil_div(n, tpb), cap = (int64_t)cu_count() * per_cu;
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

// carves a workspace into arrays, each aligned to 256 bytes; `off` is the size carved so far (base may
// be NULL when only the sizes are wanted)
struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t count) {
        const size_t at = off;
        off = align_up(off + sizeof(T) * count, 256);
        return (T *)(base + at);
    }
};

// a runtime dim to a compile-time padded width: calls f(int_c<W>{}) for the first of the ascending Widths
// with dim <= W (for the last one if there is none: the callers have refused such a dim)
template <int V> using int_c = std::integral_constant<int, V>;
template <int W, int... Rest, class F> void dispatch_dp(int dim, F &&f) {
    if constexpr (sizeof...(Rest) == 0) {
        f(int_c<W>{});
    } else {
        if (dim <= W) f(int_c<W>{});
        else dispatch_dp<Rest...>(dim, f);
    }
}

// The same for the instantiation lists of the fused-MLP launchers.  tag<T>: a type as a value, what a visitor of a
// class list hands to its callback.  lift_*: a run-time value to a compile-time constant over an EXPLICIT list of
// allowed values - f(int_c<V>{}) for the V equal to v; false if v is not in the list (no instantiation).
template <class T> struct tag { using type = T; };
template <int... Vs, class F> bool lift_int(int v, F &&f) { return ((v == Vs && (f(int_c<Vs>{}), true)) || ...); }
template <int A, int B> struct int2_c { static constexpr int a = A, b = B; };
template <class... Ps, class F> bool lift_int2(int a, int b, F &&f) {
    return ((a == Ps::a && b == Ps::b && (f(Ps{}), true)) || ...);
}
// f(c1, c2, ...) with every run-time flag as std::true_type / std::false_type
template <class F> void lift_bools(F &&f) { f(); }
template <class F, class... B> void lift_bools(F &&f, bool b, B... rest) {
    if (b) lift_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else lift_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// one kernel launch without dynamic LDS (the arguments are copied into the kernel's parameter types)
template <class K, class... A> void launch(K kfn, int grid, int block, hipStream_t stream, const A &...args) {
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(block), 0, stream, args...);
}

// guards of the entries that index hits in int32 tables: "<entry>: negative <what> count" (EINVAL),
// "<entry>: <n> <what>s; at most 2^30-1" (EUNSUPPORTED)
int check_count_i30(const char *entry, const char *what, int64_t n);
// "<entry>: workspace of <have> bytes, need <need> (gnntrk_<entry>_workspace_bytes)" if it is NULL or too small
int check_workspace(const char *entry, const void *workspace, size_t have, size_t need);

// stable LSD radix sort of (key,value) pairs on the device (sort_pairs.hip: rocPRIM)
size_t sort_pairs_temp_bytes(int64_t n);
int sort_pairs_u32(const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in,
                   uint32_t *vals_out, int64_t n, int end_bit, void *temp, size_t temp_bytes,
                   hipStream_t stream);
size_t sort_pairs_u64_temp_bytes(int64_t n);
int sort_pairs_u64(const unsigned long long *keys_in, unsigned long long *keys_out, const uint32_t *vals_in,
                   uint32_t *vals_out, int64_t n, void *temp, size_t temp_bytes, hipStream_t stream);
// (keys whose bits from `end_bit` up are all zero: the passes over them are skipped)
int sort_pairs_u64_bits(const unsigned long long *keys_in, unsigned long long *keys_out, const uint32_t *vals_in,
                        uint32_t *vals_out, int64_t n, int end_bit, void *temp, size_t temp_bytes, hipStream_t stream);

// knn.hip: points sorted by (event, Morton code) in chunks of 64 with bounding boxes
void scan_counts_launch(const int32_t *cnt, int k_take, int64_t n, int64_t *off, hipStream_t stream);
int spatial_dp(int dim);
int spatial_n_chunks(int64_t n);
size_t spatial_scratch_bytes(int64_t n);
struct SpatialChunks {
    float *xs;       // [n_chunks * 64][dp] the points in sorted order, the tail of the last chunk repeats the last point
    int32_t *sidx;   // [n_chunks * 64] their original indices, -1 in the tail
    float *box;      // [n_chunks][2 * dp] lo | hi of every chunk
    void *scratch;   // of the build only
    size_t scratch_bytes;
    int n_chunks, dp;
};
// the three arrays for n points of dimension dim, then (at once, or after the regions a unit keeps in
// between) the build's scratch
inline SpatialChunks take_chunks(Carver &ws, int64_t n, int dim) {
    SpatialChunks c{};
    c.dp = spatial_dp(dim);
    c.n_chunks = spatial_n_chunks(n);
    const size_t rows = (size_t)c.n_chunks * 64;
    c.xs = ws.take<float>(rows * c.dp);
    c.sidx = ws.take<int32_t>(rows);
    c.box = ws.take<float>((size_t)c.n_chunks * 2 * c.dp);
    return c;
}
inline void take_chunks_scratch(Carver &ws, SpatialChunks &c, int64_t n) {
    c.scratch_bytes = spatial_scratch_bytes(n);
    c.scratch = ws.take<char>(c.scratch_bytes);
}
// the workspace that holds the chunks and nothing else (pruned k-NN search, radius graph): *total = its size
inline SpatialChunks chunks_ws(void *base, int64_t n, int dim, size_t *total) {
    Carver ws{(char *)base};
    SpatialChunks c = take_chunks(ws, n, dim);
    take_chunks_scratch(ws, c, n);
    *total = ws.off;
    return c;
}
int spatial_chunks_build(const float *x, int64_t n, int dim, int stride, const int64_t *seg_ptr, int n_seg,
                         const SpatialChunks &c, hipStream_t stream);

// mlp.hip: fixed-order sum of the backward kernels' partial blocks into the gradient tensors
int reduce_partials_launch(const float *part, int n_part, const gnntrk_mlp *mlp, float *const gW[3],
                           float *const gb[3], int accumulate, hipStream_t stream);

// mlp_bf16.hip: the bf16 half of gnntrk_mlp_kernel_name (mlp.hip)
int mlp16_kernel_name(const gnntrk_mlp *m, int n_seg, const gnntrk_seg *seg, int backward, char *buf,
                      size_t len);
// hidden width 128 with biases (eight hidden tiles, accumulator-initialised biases): mlp_bf16_bi8.hip
struct SlotPlan;
int launch_fwd16_bi8(const gnntrk_mlp_fwd_args *a, const SlotPlan &P, int grid, hipStream_t stream);
int launch_bwd16_bi8(const gnntrk_mlp_bwd_args *a, const SlotPlan &P, int GT, int grid, float *part, uint8_t *trash,
                     hipStream_t stream);

// compact.hip: the workspace of one compaction over n flags, and the compaction of a byte mask (dbscan.hip)
size_t compact_ws_bytes(int64_t n);
int compact_bytes_launch(const uint8_t *flags, int64_t n, int32_t *idx, int32_t *newid, int64_t *n_out, void *ws,
                         size_t ws_bytes, hipStream_t stream);

// rows_bf16.hip: fp32 rows to bf16 rows (graph_index.hip: the carried edge rows)
int rows_to_bf16_launch(const float *in, int dim, int in_stride, const int32_t *idx, int64_t n_rows,
                        uint16_t *out, int out_stride, hipStream_t stream);

}  // namespace gnntrk
