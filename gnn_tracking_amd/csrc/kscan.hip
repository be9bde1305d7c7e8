// The k-scan of the metric-learning validation (graph_construction/k_scanner.py:203-285): connected
// components on the device and the integer counts around them, for every k of a list on ONE neighbour
// table.  The reference builds, per k, a networkx graph from a host copy of the true edges and walks its
// components in Python twice (analysis/graphs.py:281-343); here the components are a lock-free
// union-find and every figure is a count:
//
//   once per call   (hits)        ks_init_kernel        parent[i] = i for both component problems
//                   (hits)        ks_particles_kernel   particle table of the masked hits (open addressing,
//                                                       slot = first hit + 1), hits per particle c_p
//                   (true edges)  ks_true_edges_kernel  |{t: m[t0] & m[t1]}|
//   per k, ascending (new edges)  ks_union_kernel       the edges of rank [k_prev, k) of the table: edge counts
//                                                       of the step, union of same-id edges in problem A (all
//                                                       hits) and, if both ends are masked, in problem B
//                   (hits)        ks_compress_kernel    labels A of this k (int64, smallest hit index of the
//                                                       component); size of every B component at its root
//                   (hits)        ks_segmax_kernel      per particle the largest B component s_p
//                   (slots)       ks_segments_kernel    n_pids, |{2 s_p > c_p}|, |{4 s_p > 3 c_p}|, |{s_p = c_p}|
//   once            (events)      ks_finish_kernel      prefix sums of the step counts into the rows of `out`
//
// The graphs are nested in k (the k nearest are a prefix of a query's sorted neighbours), so the forest
// of one k is the starting point of the next larger k: every table edge is united once per call, whatever
// the number of ks.  The label of a hit is the smallest hit index of its component: roots are only ever
// hooked under SMALLER roots, so parent[x] <= x always holds and the root of a tree is its minimum - the
// result is unique and does not depend on the order in which atomics land.  Every output is an integer.
//
// The memory-order argument of the union-find (ks_find / ks_unite) stands with them in union_find.h.
//
// kscan_counts_batched: the same scan for every event of a collated batch from the same launch sequence (the
// BATCH = true instantiations; hits [seg_ptr[s], seg_ptr[s + 1]) are event s).  What is keyed per event:
//   - an edge belongs to the event of its query, a true edge to the event of its ends; a neighbour entry outside the
//     query's event and a true edge across two events are never united: they count as bad, as an index outside
//     [0, n) does, in the event of the query / of the true edge's first end (the first end inside [0, n))
//   - a particle is the pair (event, particle id): both are parts of the table's key, a slot counts for the event
//     of its first hit
//   - the step counts, the two totals and the rows of `out` exist once per event; ks_finish_kernel does one event
//     per thread
//   - a label is the smallest hit index of the component minus the event's first row
// The union-find argument above is unchanged: parent[] holds batch-wide indices, and components never cross
// events because no cross-event edge is united; the smallest index of a component lies in its event.
// Per-event counters (event_add, count_util.h): a thread adds to the counters of ITS event.  Hits are sorted by
// event, so the 64 lanes of a wave that walks consecutive queries share one event unless an event edge falls
// among them: a wave sum and one int64 atomic per value; a wave that holds an event edge, and the slots of the
// particle table, whose events are mixed, add lane by lane with int64 atomics.  Either way every addend is an
// integer that depends on the input alone (the event of a hit, the flags of an edge, and c_p / s_p, which are
// unique by the argument above) and integer addition is associative and commutative: the sums are the same
// whatever form a wave takes and whatever order the atomics land in.
//
// The work is integer, atomic- and latency-bound (random 4-8 byte accesses into arrays of a few MB that
// stay in L2 / MALL); there is no HBM roofline to quote for it.
#include <stdio.h>

#include "count_util.h"
#include "union_find.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kCols = GNNTRK_KSCAN_COLUMNS;
constexpr int kMaxKs = GNNTRK_KSCAN_MAX_KS;

// columns of the output table
enum { C_EDGES = 0, C_MASKED, C_TRUE_MASKED, C_TRUE_EDGES_MASKED, C_PIDS, C_N50, C_N75, C_N100, C_BAD };

// --------------------------------------------------------------------------- plain components
__global__ __launch_bounds__(kTpb) void cc_init_kernel(int32_t *__restrict__ parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb)
        parent[i] = (int32_t)i;
}

__device__ __forceinline__ bool keep_edge(int64_t a, int64_t b, const int64_t *pid, const uint8_t *mask) {
    if (pid && pid[a] != pid[b]) return false;
    if (mask && !(mask[a] && mask[b])) return false;
    return true;
}

__global__ __launch_bounds__(kTpb) void cc_union_edges_kernel(const int64_t *__restrict__ ei, int64_t m, int64_t n,
                                                              const int64_t *__restrict__ pid,
                                                              const uint8_t *__restrict__ mask, int32_t *parent,
                                                              unsigned long long *bad) {
    uint32_t nbad[1] = {0u};
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {
        const int64_t e = base + threadIdx.x;
        if (e >= m) continue;
        const int64_t a = ei[e], b = ei[m + e];
        if (a < 0 || a >= n || b < 0 || b >= n) {
            nbad[0] += 1u;
            continue;
        }
        if (a != b && keep_edge(a, b, pid, mask)) ks_unite(parent, (int32_t)a, (int32_t)b);
    }
    if (bad) block_add(nbad, bad);
}

__global__ __launch_bounds__(kTpb) void cc_union_table_kernel(const int32_t *__restrict__ nbr,
                                                              const int32_t *__restrict__ cnt, int64_t n,
                                                              int32_t k_stride, int32_t k,
                                                              const int64_t *__restrict__ pid,
                                                              const uint8_t *__restrict__ mask, int32_t *parent,
                                                              unsigned long long *bad) {
    uint32_t nbad[1] = {0u};
    const int64_t total = n * k;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < total; base += (int64_t)gridDim.x * kTpb) {
        const int64_t idx = base + threadIdx.x;
        if (idx >= total) continue;
        const int64_t q = idx / k;
        const int32_t i = (int32_t)(idx - q * k);
        if (i >= cnt[q]) continue;
        const int64_t j = nbr[q * k_stride + i];
        if (j < 0 || j >= n) {
            nbad[0] += 1u;
            continue;
        }
        if (j != q && keep_edge(j, q, pid, mask)) ks_unite(parent, (int32_t)j, (int32_t)q);
    }
    if (bad) block_add(nbad, bad);
}

__global__ __launch_bounds__(kTpb) void cc_labels_kernel(int32_t *parent, int64_t n, int64_t *__restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb)
        labels[i] = ks_find(parent, (int32_t)i);
}

// --------------------------------------------------------------------------- the scan
// (one event: n_seg = 1 and n_ks = kMaxKs rows of step counts, whatever the call's number of ks)
struct Ws {
    int32_t *parent_a;          // [n]  components of the same-id edges, all hits
    int32_t *parent_b;          // [n]  components of the same-id edges with both ends masked
    uint32_t *hslot;            // [n]  particle slot of every masked hit
    uint32_t *csize;            // [n]  size of the B component rooted at the hit (cleared by its reader)
    int32_t *ptab;              // [S]  particle table of the masked hits: first hit + 1, 0 = empty
    uint32_t *pcnt;             // [S]  masked hits per particle c_p
    uint32_t *smax;             // [S]  largest B component per particle s_p (cleared by its reader)
    unsigned long long *steps;  // [n_seg][n_ks][3] edge counts of every step
    unsigned long long *tail;   // [n_seg][2] true edges masked, bad
    size_t step_stride;         // 3 * n_ks
    size_t zero_from, total;
    uint64_t S;
};

Ws make_ws(void *base, int64_t n, int32_t n_seg = 1, int32_t n_ks = kMaxKs) {
    Ws w{};
    w.S = table_size(n);
    const size_t S = w.S, N = (size_t)n;
    Carver ws{(char *)base};
    w.parent_a = ws.take<int32_t>(N);
    w.parent_b = ws.take<int32_t>(N);
    w.hslot = ws.take<uint32_t>(N);
    w.zero_from = ws.off;   // everything from here on is cleared
    w.csize = ws.take<uint32_t>(N);
    w.ptab = ws.take<int32_t>(S);
    w.pcnt = ws.take<uint32_t>(S);
    w.smax = ws.take<uint32_t>(S);
    w.step_stride = 3 * (size_t)n_ks;
    w.steps = ws.take<unsigned long long>((w.step_stride + 2) * (size_t)n_seg);
    w.tail = w.steps + w.step_stride * (size_t)n_seg;
    w.total = ws.off;
    return w;
}

struct Plan {
    int32_t k[kMaxKs];     // ascending
    int32_t row[kMaxKs];   // row of `out` / `labels` of the s-th smallest k
    int32_t n;
};

__global__ __launch_bounds__(kTpb) void ks_init_kernel(Ws w, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        w.parent_a[i] = (int32_t)i;
        w.parent_b[i] = (int32_t)i;
    }
}

// event_rows with the rows clipped to [0, n): whatever seg_ptr holds, an index inside them is a hit
template <bool BATCH>
__device__ __forceinline__ int ks_event_rows(const Events &ev, int64_t n, int64_t i, int64_t &lo, int64_t &hi) {
    const int e = event_rows<BATCH>(ev, n, i, lo, hi);
    if (BATCH) {
        lo = lo < 0 ? 0 : lo;
        hi = hi > n ? n : hi;
    }
    return e;
}

template <bool BATCH>
__global__ __launch_bounds__(kTpb) void ks_particles_kernel(const int64_t *__restrict__ pid,
                                                            const uint8_t *__restrict__ mask, int64_t n, Events ev,
                                                            Ws w) {
    const uint64_t smask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        if (!mask[i]) continue;
        const int64_t key = pid[i];
        int64_t lo, hi;
        const int e = event_rows<BATCH>(ev, n, i, lo, hi);
        const uint64_t s = table_claim(w.ptab, smask, particle_hash<BATCH>(key, e), i,
                                       [&](int32_t h) { return pid[h] == key; },
                                       [&](int32_t h) { return !BATCH || (h >= lo && h < hi); });
        w.hslot[i] = (uint32_t)s;
        atomicAdd(&w.pcnt[s], 1u);
    }
}

template <bool BATCH>
__global__ __launch_bounds__(kTpb) void ks_true_edges_kernel(const int64_t *__restrict__ te, int64_t m, int64_t n,
                                                             const uint8_t *__restrict__ mask, Events ev, Ws w) {
    uint32_t c[2] = {0u, 0u};   // both ends masked, out of range (BATCH: or across two events)
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < m; base += (int64_t)gridDim.x * kTpb) {
        const int64_t t = base + threadIdx.x;
        int e = 0;
        if (t < m) {
            const int64_t a = te[t], b = te[m + t];
            const bool in_a = a >= 0 && a < n, in_b = b >= 0 && b < n;
            int64_t lo = 0, hi = n;
            if (in_a || in_b) e = ks_event_rows<BATCH>(ev, n, in_a ? a : b, lo, hi);
            if (!in_a || b < lo || b >= hi)
                c[1] += 1u;
            else
                c[0] += (mask[a] && mask[b]) ? 1u : 0u;
        }
        if (BATCH) event_add(c, e, w.tail, 2);
    }
    if (!BATCH) block_add(c, w.tail);
}

// the table edges of rank [lo, hi): (nbr[q * k_stride + i], q) for lo <= i < min(hi, cnt[q])
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void ks_union_kernel(const int32_t *__restrict__ nbr,
                                                        const int32_t *__restrict__ cnt, int64_t n,
                                                        int32_t k_stride, int32_t lo, int32_t hi,
                                                        const int64_t *__restrict__ pid,
                                                        const uint8_t *__restrict__ mask, Events ev, Ws w,
                                                        int32_t step) {
    uint32_t c[3] = {0u, 0u, 0u};   // edges, masked, true and masked
    uint32_t nbad[1] = {0u};
    const int32_t width = hi - lo;
    const int64_t total = n * width;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < total; base += (int64_t)gridDim.x * kTpb) {
        const int64_t idx = base + threadIdx.x;
        const int64_t q = idx / width;
        const int32_t i = lo + (int32_t)(idx - q * width);
        int e = 0;
        if (idx < total && i < cnt[q]) {
            const int64_t j = nbr[q * k_stride + i];
            int64_t first, last;   // the rows of the query's event
            e = ks_event_rows<BATCH>(ev, n, q, first, last);
            if (j < first || j >= last) {
                nbad[0] += 1u;
            } else {
                const bool mj = mask[j] != 0, mq = mask[q] != 0;
                const bool y = pid[j] == pid[q];   // (no `> 0` test: k_scanner.py:267-269)
                c[0] += 1u;
                c[1] += (mj || mq) ? 1u : 0u;
                c[2] += (y && (mj || mq)) ? 1u : 0u;
                if (y && j != q) {
                    ks_unite(w.parent_a, (int32_t)j, (int32_t)q);
                    if (mj && mq) ks_unite(w.parent_b, (int32_t)j, (int32_t)q);
                }
            }
        }
        if (BATCH) {
            event_add(c, e, w.steps + 3 * step, w.step_stride);
            event_add(nbad, e, w.tail + 1, 2);
        }
    }
    if (!BATCH) {
        block_add(c, w.steps + 3 * step);
        block_add(nbad, w.tail + 1);
    }
}

// (BATCH: the label is local to the event)
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void ks_compress_kernel(const uint8_t *__restrict__ mask, int64_t n, Events ev,
                                                           Ws w, int64_t *__restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        int64_t lo, hi;
        event_rows<BATCH>(ev, n, i, lo, hi);
        labels[i] = ks_find(w.parent_a, (int32_t)i) - lo;
        if (mask[i]) atomicAdd(&w.csize[ks_find(w.parent_b, (int32_t)i)], 1u);
    }
}

// every B component is single-id: its root's particle slot is its particle
__global__ __launch_bounds__(kTpb) void ks_segmax_kernel(int64_t n, Ws w) {
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const uint32_t s = w.csize[i];
        if (s == 0) continue;
        w.csize[i] = 0u;   // (ready for the next k)
        atomicMax(&w.smax[w.hslot[i]], s);
    }
}

// out_row: the row of this k in the first event's table; BATCH: an event's table is row_stride values on
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void ks_segments_kernel(Ws w, Events ev, unsigned long long *__restrict__ out_row,
                                                           size_t row_stride) {
    uint32_t c[4] = {0u, 0u, 0u, 0u};   // n_pids, n50, n75, n100
    const int64_t S = (int64_t)w.S;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < S; base += (int64_t)gridDim.x * kTpb) {
        const int64_t s = base + threadIdx.x;
        const int32_t first = s < S ? w.ptab[s] : 0;
        int e = 0;
        if (first != 0) {
            const uint64_t cp = w.pcnt[s], sp = w.smax[s];
            w.smax[s] = 0u;   // (ready for the next k)
            c[0] += 1u;
            c[1] += 2 * sp > cp ? 1u : 0u;
            c[2] += 4 * sp > 3 * cp ? 1u : 0u;
            c[3] += sp == cp ? 1u : 0u;
            if (BATCH) e = segment_of(ev.ptr, ev.n, first - 1);
        }
        if (BATCH) event_add(c, e, out_row + C_PIDS, row_stride);
    }
    if (!BATCH) block_add(c, out_row + C_PIDS);
}

// one event per thread (one event: one thread)
__global__ void ks_finish_kernel(Ws w, Plan plan, int32_t n_seg, unsigned long long *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_seg) return;
    const unsigned long long *steps = w.steps + (size_t)e * w.step_stride, *tail = w.tail + 2 * (size_t)e;
    unsigned long long run[3] = {0ull, 0ull, 0ull};
    for (int s = 0; s < plan.n; ++s) {
        unsigned long long *row = out + ((size_t)e * plan.n + plan.row[s]) * kCols;
        for (int c = 0; c < 3; ++c) {
            run[c] += steps[3 * s + c];
            row[C_EDGES + c] = run[c];
        }
        row[C_TRUE_EDGES_MASKED] = tail[0];
        row[C_BAD] = tail[1];
    }
}

// gnntrk_kscan_counts (BATCH = false, ev.n = 1) and gnntrk_kscan_counts_batched
template <bool BATCH>
int kscan_counts(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride, const int32_t *ks, int32_t n_ks,
                 const int64_t *particle_id, const uint8_t *node_mask, const int64_t *true_edge_index,
                 int64_t n_true_edges, Events ev, int64_t *out, int64_t *labels, void *workspace,
                 size_t workspace_bytes, hipStream_t stream) {
    char msg[160];
    int rc = check_count_i30("kscan_counts", "hit", n);
    if (rc) return rc;
    if (n_ks < 1 || n_ks > kMaxKs) {
        snprintf(msg, sizeof(msg), "kscan_counts: n_ks = %d, expected 1..%d", (int)n_ks, kMaxKs);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (!ks) return fail(GNNTRK_EINVAL, "kscan_counts: NULL ks");
    if (k_stride < 1) return fail(GNNTRK_EINVAL, "kscan_counts: k_stride < 1");
    for (int s = 0; s < n_ks; ++s)
        if (ks[s] < 1 || ks[s] > k_stride) {
            snprintf(msg, sizeof(msg), "kscan_counts: k = %d, expected 1..k_stride = %d", (int)ks[s], (int)k_stride);
            return fail(GNNTRK_EINVAL, msg);
        }
    if (n_true_edges < 0) return fail(GNNTRK_EINVAL, "kscan_counts: negative number of true edges");
    if (n_true_edges > 0 && !true_edge_index) return fail(GNNTRK_EINVAL, "kscan_counts: NULL true_edge_index");
    if (!out) return fail(GNNTRK_EINVAL, "kscan_counts: NULL output");
    if (n > 0 && (!nbr || !cnt || !particle_id || !node_mask || !labels))
        return fail(GNNTRK_EINVAL, "kscan_counts: NULL neighbour table, particle ids, node mask or labels");
    const Ws w = BATCH ? make_ws(workspace, n < 0 ? 0 : n, ev.n, n_ks) : make_ws(workspace, n < 0 ? 0 : n);
    if (n > 0 && (rc = check_workspace(BATCH ? "kscan_counts_batched" : "kscan_counts", workspace, workspace_bytes,
                                       w.total)))
        return rc;
    rc = check_hip(hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)ev.n * n_ks * kCols, stream), "kscan_counts: clear");
    if (rc || n == 0) return rc;
    Plan plan{};
    plan.n = n_ks;
    for (int s = 0; s < n_ks; ++s) {   // insertion sort of the rows by k (stable)
        int at = s;
        while (at > 0 && plan.k[at - 1] > ks[s]) {
            plan.k[at] = plan.k[at - 1];
            plan.row[at] = plan.row[at - 1];
            --at;
        }
        plan.k[at] = ks[s];
        plan.row[at] = s;
    }
    if ((rc = check_hip(hipMemsetAsync((char *)workspace + w.zero_from, 0, w.total - w.zero_from, stream),
                        "kscan_counts: clear workspace")))
        return rc;
    auto *o = reinterpret_cast<unsigned long long *>(out);
    const size_t row_stride = (size_t)n_ks * kCols;   // from an event's table to the next
    const int gn = blocks_for(n, 8);
    hipLaunchKernelGGL(ks_init_kernel, dim3(gn), dim3(kTpb), 0, stream, w, n);
    hipLaunchKernelGGL(ks_particles_kernel<BATCH>, dim3(gn), dim3(kTpb), 0, stream, particle_id, node_mask, n, ev, w);
    if (n_true_edges > 0)
        hipLaunchKernelGGL(ks_true_edges_kernel<BATCH>, dim3(blocks_for(n_true_edges, 8)), dim3(kTpb), 0, stream,
                           true_edge_index, n_true_edges, n, node_mask, ev, w);
    if ((rc = check_launch("kscan_counts: setup"))) return rc;
    int32_t lo = 0;
    for (int s = 0; s < n_ks; ++s) {
        const int32_t hi = plan.k[s];
        if (hi > lo) {
            hipLaunchKernelGGL(ks_union_kernel<BATCH>, dim3(blocks_for(n * (hi - lo), 8)), dim3(kTpb), 0, stream, nbr,
                               cnt, n, k_stride, lo, hi, particle_id, node_mask, ev, w, (int32_t)s);
            lo = hi;
        }
        hipLaunchKernelGGL(ks_compress_kernel<BATCH>, dim3(gn), dim3(kTpb), 0, stream, node_mask, n, ev, w,
                           labels + (size_t)plan.row[s] * n);
        hipLaunchKernelGGL(ks_segmax_kernel, dim3(gn), dim3(kTpb), 0, stream, n, w);
        hipLaunchKernelGGL(ks_segments_kernel<BATCH>, dim3(blocks_for((int64_t)w.S, 4)), dim3(kTpb), 0, stream, w, ev,
                           o + (size_t)plan.row[s] * kCols, row_stride);
        if ((rc = check_launch("kscan_counts: scan"))) return rc;
    }
    hipLaunchKernelGGL(ks_finish_kernel, dim3((unsigned)ceil_div(ev.n, 64)), dim3(64), 0, stream, w, plan, ev.n, o);
    return check_launch("kscan_counts: finish");
}

}  // namespace

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_cc_labels_workspace_bytes(int64_t n) { return align_up(4 * (size_t)(n < 0 ? 0 : n), 256); }

int gnntrk_cc_labels(const int64_t *edge_index, int64_t n_edges, const int32_t *nbr, const int32_t *cnt,
                     int32_t k_stride, int32_t k, const int64_t *same_pid, const uint8_t *node_mask, int64_t n,
                     int64_t *labels, int64_t *n_bad, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    char msg[160];
    int rc = check_count_i30("cc_labels", "node", n);
    if (rc) return rc;
    const bool table = edge_index == nullptr;
    if (table) {
        if (k < 1 || k_stride < 1 || k > k_stride) {
            snprintf(msg, sizeof(msg), "cc_labels: k = %d, expected 1..k_stride = %d", (int)k, (int)k_stride);
            return fail(GNNTRK_EINVAL, msg);
        }
        if (n > 0 && (!nbr || !cnt)) return fail(GNNTRK_EINVAL, "cc_labels: NULL edge_index and NULL neighbour table");
    } else if (n_edges < 0) {
        return fail(GNNTRK_EINVAL, "cc_labels: negative edge count");
    }
    if (n > 0 && !labels) return fail(GNNTRK_EINVAL, "cc_labels: NULL labels");
    if (n > 0 && (rc = check_workspace("cc_labels", workspace, workspace_bytes, gnntrk_cc_labels_workspace_bytes(n))))
        return rc;
    if (n_bad && (rc = check_hip(hipMemsetAsync(n_bad, 0, sizeof(int64_t), stream), "cc_labels: clear"))) return rc;
    if (n == 0) return GNNTRK_OK;
    auto *parent = (int32_t *)workspace;
    auto *bad = reinterpret_cast<unsigned long long *>(n_bad);
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(n, 8)), dim3(kTpb), 0, stream, parent, n);
    if (table)
        hipLaunchKernelGGL(cc_union_table_kernel, dim3(blocks_for(n * k, 8)), dim3(kTpb), 0, stream, nbr, cnt, n,
                           k_stride, k, same_pid, node_mask, parent, bad);
    else if (n_edges > 0)
        hipLaunchKernelGGL(cc_union_edges_kernel, dim3(blocks_for(n_edges, 8)), dim3(kTpb), 0, stream, edge_index,
                           n_edges, n, same_pid, node_mask, parent, bad);
    hipLaunchKernelGGL(cc_labels_kernel, dim3(blocks_for(n, 8)), dim3(kTpb), 0, stream, parent, n, labels);
    return check_launch("cc_labels");
}

size_t gnntrk_kscan_counts_workspace_bytes(int64_t n) { return make_ws(nullptr, n < 0 ? 0 : n).total; }

int gnntrk_kscan_counts(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride, const int32_t *ks,
                        int32_t n_ks, const int64_t *particle_id, const uint8_t *node_mask,
                        const int64_t *true_edge_index, int64_t n_true_edges, int64_t *out, int64_t *labels,
                        void *workspace, size_t workspace_bytes, void *stream) {
    return kscan_counts<false>(nbr, cnt, n, k_stride, ks, n_ks, particle_id, node_mask, true_edge_index, n_true_edges,
                               Events{nullptr, 1}, out, labels, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t gnntrk_kscan_counts_batched_workspace_bytes(int64_t n, int32_t n_seg, int32_t n_ks) {
    return make_ws(nullptr, n < 0 ? 0 : n, n_seg < 1 ? 1 : n_seg, n_ks < 1 ? 1 : n_ks).total;
}

int gnntrk_kscan_counts_batched(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride, const int32_t *ks,
                                int32_t n_ks, const int64_t *particle_id, const uint8_t *node_mask,
                                const int64_t *true_edge_index, int64_t n_true_edges, const int64_t *seg_ptr,
                                int32_t n_seg, int64_t *out, int64_t *labels, void *workspace, size_t workspace_bytes,
                                void *stream) {
    if (!seg_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "kscan_counts_batched: seg_ptr needs n_seg >= 1 events");
    if (n_seg > GNNTRK_KSCAN_MAX_EVENTS) {
        char msg[160];
        snprintf(msg, sizeof(msg), "kscan_counts_batched: n_seg = %d, at most %d events per call", (int)n_seg,
                 GNNTRK_KSCAN_MAX_EVENTS);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    return kscan_counts<true>(nbr, cnt, n, k_stride, ks, n_ks, particle_id, node_mask, true_edge_index, n_true_edges,
                              Events{seg_ptr, n_seg}, out, labels, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
