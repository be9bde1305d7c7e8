// Size spectra behind the clustering scores of metrics/cluster_metrics.py:400-456 (count_hits_per_cluster
// and common_metrics' v_measure / homogeneity / completeness / adjusted_rand / fowlkes_mallows, which the
// reference hands to sklearn on host copies of one trial's labels at a time).
//
// Every one of these scores is a function of three multisets of integers: the sizes a_i of the truth
// classes, the sizes b_j of the predicted clusters and the non-zero cells n_ij of their contingency table.
// Each multiset is needed only as its SPECTRUM - the distinct sizes v with their multiplicities m - and the
// sizes of one spectrum sum to n, so it has at most D(n) = floor((sqrt(8n + 1) - 1) / 2) entries
// (1 + 2 + ... + D <= n): 547 for 150 k hits.  The device does the exact integer counting for all trials of
// a call, the host reads a few hundred integers per trial and does the floating point.
//
// Labels and truth ids are CATEGORIES of any int64 value (sklearn's view): a negative label is an ordinary
// cluster (DBSCAN's -1 noise is one cluster), truth id 0 an ordinary class; nothing is densified.  The
// groupings are the open-addressing tables of count_util.h (slots hold "first hit + 1"), one table per
// spectrum, table k next to table k - 1:
//
//   table 0          truth classes, keyed by truth[i]                         (once per call)
//   table 1 + 2t     clusters of trial t, keyed by labels[t][i]
//   table 2 + 2t     cells of trial t, keyed by (labels[t][i], truth slot of i)
//
//   once per call (hits)       cs_classes_kernel   class table, count per slot, the class slot of every hit
//   all trials at once (hits)  cs_hits_kernel      cluster and cell tables, counts per slot
//   (slots, y = spectrum)      cs_spectrum_kernel  every occupied slot adds 1 to the multiplicity of its count
//                                                  v: nearly all slots have a small v, so v < 2048 goes to an
//                                                  LDS histogram per workgroup that is flushed with one global
//                                                  atomic per non-zero bin; v >= 2048 (at most n / 2048 slots
//                                                  of a spectrum) to a small global table keyed by v
//   (bins, y = spectrum)       cs_compact_kernel   the non-zero bins as (v, m) pairs behind their number d
//
// cluster_spectra_batched: the spectra of every event of a collated batch from the same tables (BATCH = true: a class
// is (event, truth id), a cluster (event, label), a cell belongs to the event of its class slot), then
//   (hits, x = event, y = spectrum)  cs_event_spectrum_kernel  the block walks the hits of its event - hit i stands for
//                                                  its group iff the slot it finds holds i + 1 -, so its LDS histogram
//                                                  is the event's spectrum and goes to the pooled output as (event,
//                                                  v, m) triples; v >= 2048 through the event's region of the keyed table
//
// All arithmetic is integer (uint32 counts, int64 outputs); the pairs of a spectrum are written in the order
// in which their appends land, the SET of pairs does not depend on it (the host sorts them).
#include <stdio.h>

#include "count_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kBins = 2048;   // sizes below this are counted in the LDS histogram (8 KB)

struct Ws {
    int32_t *tab;     // [K][S] tables: first hit + 1, 0 = empty (K = 1 + 2T spectra)
    uint32_t *cnt;    // [K][S] hits per slot
    uint32_t *hist;   // [K][kBins] multiplicity of every size < kBins
    int32_t *bkey;    // [K][B] table of the sizes >= kBins: the size, 0 = empty
    uint32_t *bcnt;   // [K][B] their multiplicities
    size_t zero_bytes;   // everything before aslot is cleared
    uint32_t *aslot;  // [n] class slot of every hit
    size_t total;
    uint64_t S, B;
};

Ws make_ws(void *base, int64_t n, int32_t T) {
    Ws w{};
    w.S = table_size(n);
    w.B = table_size(n / kBins + 1);   // more slots than there can be sizes >= kBins in one spectrum
    const size_t K = 1 + 2 * (size_t)T;
    Carver ws{(char *)base};
    w.tab = ws.take<int32_t>(K * w.S);
    w.cnt = ws.take<uint32_t>(K * w.S);
    w.hist = ws.take<uint32_t>(K * kBins);
    w.bkey = ws.take<int32_t>(K * w.B);
    w.bcnt = ws.take<uint32_t>(K * w.B);
    w.zero_bytes = ws.off;
    w.aslot = ws.take<uint32_t>((size_t)n);
    w.total = ws.off;
    return w;
}

// D(n): the most distinct sizes that can sum to n
int64_t capacity(int64_t n) {
    if (n <= 0) return 0;
    const uint64_t x = 8 * (uint64_t)n + 1;
    uint64_t r = 0;   // floor(sqrt(x)) by bits: integer arithmetic only
    for (uint64_t bit = 1ull << 31; bit; bit >>= 1)
        if ((r | bit) * (r | bit) <= x) r |= bit;
    return (int64_t)((r - 1) / 2);
}

// ------------------------------------------------------------------ once per call
// BATCH (cluster_spectra_batched): a class is the pair (event, truth id) - the same id and a first hit inside the
// event's rows -, hashed as a particle of count_util.h
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void cs_classes_kernel(const int64_t *__restrict__ truth, int64_t n, Events ev, Ws w) {
    const uint64_t mask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int64_t key = truth[i];
        int64_t lo, hi;
        const int e = event_rows<BATCH>(ev, n, i, lo, hi);
        const uint64_t s = table_claim(w.tab, mask, particle_hash<BATCH>(key, e), i, [&](int32_t h) {
            return truth[h] == key && (!BATCH || (h >= lo && h < hi));
        });
        w.aslot[i] = (uint32_t)s;
        atomicAdd(&w.cnt[s], 1u);
    }
}

// ------------------------------------------------------------------- all trials
// hits of every trial (flattened [T][n]); has_truth = 0: the cluster tables only.  BATCH: a cluster is the pair
// (event, label) - labels are categories of any value, so -1 of two events is two clusters -; a cell keeps its key
// (label, class slot): the class slot is the event's own
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void cs_hits_kernel(const int64_t *__restrict__ labels, int64_t n, int64_t tn,
                                                       int has_truth, Events ev, Ws w) {
    const uint64_t mask = w.S - 1;
    for (int64_t idx = (int64_t)blockIdx.x * kTpb + threadIdx.x; idx < tn; idx += (int64_t)gridDim.x * kTpb) {
        const int64_t t = idx / n, i = idx - t * n;
        const int64_t *lt = labels + t * n;
        const int64_t lab = lt[i];
        int64_t lo, hi;
        const int e = event_rows<BATCH>(ev, n, i, lo, hi);
        const uint64_t hl = particle_hash<BATCH>(lab, e);
        const size_t kb = (size_t)(1 + 2 * t) * w.S;
        const uint64_t sb = table_claim(w.tab + kb, mask, hl, i, [&](int32_t h) {
            return lt[h] == lab && (!BATCH || (h >= lo && h < hi));
        });
        atomicAdd(&w.cnt[kb + sb], 1u);
        if (!has_truth) continue;
        const uint32_t as = w.aslot[i];
        const size_t kc = kb + w.S;
        const uint64_t sc = table_claim(w.tab + kc, mask, mix64(hl + as), i, [&](int32_t h) { return lt[h] == lab; },
                                        [&](int32_t h) { return w.aslot[h] == as; });
        atomicAdd(&w.cnt[kc + sc], 1u);
    }
}

// the spectrum of blockIdx.y: step 1 all of them, step 2 the cluster spectra 1, 3, 5, ... only
__device__ __forceinline__ size_t spectrum_of_block(int step) { return step == 1 ? blockIdx.y : 1 + 2 * (size_t)blockIdx.y; }

__global__ __launch_bounds__(kTpb) void cs_spectrum_kernel(int step, Ws w) {
    __shared__ uint32_t bins[kBins];
    for (int b = threadIdx.x; b < kBins; b += kTpb) bins[b] = 0u;
    __syncthreads();
    const size_t k = spectrum_of_block(step);
    const int32_t *tab = w.tab + k * w.S;
    const uint32_t *cnt = w.cnt + k * w.S;
    int32_t *bkey = w.bkey + k * w.B;
    const uint64_t bmask = w.B - 1;
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        if (tab[s] == 0) continue;
        const uint32_t v = cnt[s];
        if (v < (uint32_t)kBins) {
            atomicAdd(&bins[v], 1u);
            continue;
        }
        // claim the slot of size v (v < 2^30 fits the int32 key; the table has free slots: make_ws)
        uint64_t b = mix64(v) & bmask;
        for (;;) {
            const int32_t h = cas_i32(&bkey[b], 0, (int32_t)v);
            if (h == 0 || h == (int32_t)v) break;
            b = (b + 1) & bmask;
        }
        atomicAdd(&w.bcnt[k * w.B + b], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kTpb)
        if (bins[b]) atomicAdd(&w.hist[k * kBins + b], bins[b]);
}

// out: per spectrum 1 + 2 * cap values, [0] = d, then d pairs (size, multiplicity)
__global__ __launch_bounds__(kTpb) void cs_compact_kernel(int step, int64_t cap, Ws w,
                                                          unsigned long long *__restrict__ out) {
    const size_t k = spectrum_of_block(step);
    unsigned long long *o = out + k * (size_t)(1 + 2 * cap);
    const int64_t nb = kBins + (int64_t)w.B;
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < nb; e += (int64_t)gridDim.x * kTpb) {
        uint32_t v, m;
        if (e < kBins) {
            v = (uint32_t)e;
            m = w.hist[k * kBins + e];
        } else {
            v = (uint32_t)w.bkey[k * w.B + (e - kBins)];
            m = w.bcnt[k * w.B + (e - kBins)];
        }
        if (m == 0) continue;
        const unsigned long long at = atomicAdd(&o[0], 1ull);
        if ((int64_t)at >= cap) continue;   // (cannot happen: distinct sizes that sum to n)
        o[1 + 2 * at] = v;
        o[2 + 2 * at] = m;
    }
}

// ------------------------------------------------------------------ collated batches
// cluster_spectra_batched: the spectra of every event.  The slots of the events are interleaved in the hashed tables,
// the hits are not: they are sorted by event.  So the HITS are walked, one block per (event x, spectrum y): hit i
// stands for its group iff the slot it finds holds i + 1 (it claimed it), and then adds 1 to the multiplicity of
// cnt[slot].  The block sees all hits of its event, so its LDS histogram is the event's whole spectrum below kBins and
// goes straight to the output - no global histogram per event, the workspace keeps its size.  Sizes >= kBins (at
// most n_e / kBins groups of the event) go to the event's own REGION of the spectrum's keyed table: slots
// [2 (lo / kBins), 2 (hi / kBins)) for the rows [lo, hi).  The regions of two events do not overlap, a region has at
// least 2 (n_e / kBins) slots - more than twice the groups it can get, so a probe ends - and all end below
// 2 (n / kBins) < B; inside its region the key is the size alone.
// out: per spectrum 1 + 3 * cap values, [0] = d, then d triples (event, size, multiplicity).
__global__ __launch_bounds__(kTpb) void cs_event_spectrum_kernel(const int64_t *__restrict__ labels, int64_t n,
                                                                 Events ev, int step, int64_t cap, Ws w,
                                                                 unsigned long long *__restrict__ out) {
    __shared__ uint32_t bins[kBins];
    const int e = (int)blockIdx.x;
    const int64_t lo = ev.ptr[e], hi = ev.ptr[e + 1];
    if (hi <= lo) return;   // (uniform in the block)
    for (int b = threadIdx.x; b < kBins; b += kTpb) bins[b] = 0u;
    __syncthreads();
    const size_t k = spectrum_of_block(step);
    const int32_t *tab = w.tab + k * w.S;
    const uint32_t *cnt = w.cnt + k * w.S;
    int32_t *bkey = w.bkey + k * w.B;
    uint32_t *bcnt = w.bcnt + k * w.B;
    const uint64_t mask = w.S - 1;
    const uint64_t r0 = 2 * (uint64_t)(lo / kBins), rlen = 2 * (uint64_t)(hi / kBins) - r0;
    const bool cells = k != 0 && (k & 1) == 0;
    const int64_t *lt = labels + (k ? (int64_t)(k - 1) / 2 : 0) * n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kTpb) {
        uint64_t s;
        if (k == 0) {
            s = w.aslot[i];
        } else {
            const int64_t lab = lt[i];
            const uint64_t hl = particle_hash<true>(lab, e);
            if (cells) {
                const uint32_t as = w.aslot[i];
                s = table_find(tab, mask, mix64(hl + as), [&](int32_t h) { return lt[h] == lab && w.aslot[h] == as; });
            } else {
                s = table_find(tab, mask, hl, [&](int32_t h) { return lt[h] == lab && h >= lo && h < hi; });
            }
        }
        if ((int64_t)tab[s] != i + 1) continue;   // another hit stands for this group
        const uint32_t v = cnt[s];
        if (v < (uint32_t)kBins) {
            atomicAdd(&bins[v], 1u);
            continue;
        }
        // (v >= kBins: n_e >= kBins, so the region is not empty)
        uint64_t b = mix64(v) % rlen;
        for (;;) {
            const int32_t h = cas_i32(&bkey[r0 + b], 0, (int32_t)v);
            if (h == 0 || h == (int32_t)v) break;
            b = b + 1 < rlen ? b + 1 : 0;
        }
        atomicAdd(&bcnt[r0 + b], 1u);
    }
    __syncthreads();
    unsigned long long *o = out + k * (size_t)(1 + 3 * cap);
    for (int64_t j = threadIdx.x; j < kBins + (int64_t)rlen; j += kTpb) {
        uint32_t v, m;
        if (j < kBins) {
            v = (uint32_t)j;
            m = bins[j];
        } else {   // (written with atomics by this block: read the same way)
            v = (uint32_t)load_i32(&bkey[r0 + (j - kBins)]);
            m = v ? atomicAdd(&bcnt[r0 + (j - kBins)], 0u) : 0u;
        }
        if (m == 0) continue;
        const unsigned long long at = atomicAdd(&o[0], 1ull);
        if ((int64_t)at >= cap) continue;   // (cannot happen: capacity_batched bounds the distinct sizes of all events)
        o[1 + 3 * at] = (unsigned long long)e;
        o[2 + 3 * at] = v;
        o[3 + 3 * at] = m;
    }
}

// n_seg (D(ceil(n / n_seg)) + 1) >= the sum of D(n_e) over n_seg events of n hits in all: D(x) <= f(x) =
// (sqrt(8x + 1) - 1) / 2, f is concave with f(0) = 0, so sum D(n_e) <= sum f(n_e) <= n_seg f(n / n_seg) <
// n_seg (D(ceil(n / n_seg)) + 1)
int64_t capacity_batched(int64_t n, int32_t n_seg) {
    if (n <= 0 || n_seg < 1) return 0;
    return (int64_t)n_seg * (capacity(ceil_div(n, n_seg)) + 1);
}

// gnntrk_cluster_spectra (BATCH = false) and gnntrk_cluster_spectra_batched
template <bool BATCH>
int cluster_spectra(const int64_t *labels, int32_t n_trials, const int64_t *truth, int64_t n, Events ev, int64_t *out,
                    void *workspace, size_t workspace_bytes, hipStream_t stream) {
    char msg[160];
    int rc = check_count_i30("cluster_spectra", "hit", n);
    if (rc) return rc;
    if (n_trials < 1 || n_trials > GNNTRK_TRACKING_MAX_TRIALS) {
        snprintf(msg, sizeof(msg), "cluster_spectra: n_trials = %d, expected 1..%d", (int)n_trials,
                 GNNTRK_TRACKING_MAX_TRIALS);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (!out) return fail(GNNTRK_EINVAL, "cluster_spectra: NULL output");
    if (n > 0 && !labels) return fail(GNNTRK_EINVAL, "cluster_spectra: NULL labels");
    if (n > 0 && (rc = check_workspace("cluster_spectra", workspace, workspace_bytes, make_ws(nullptr, n, n_trials).total)))
        return rc;
    const int64_t cap = BATCH ? capacity_batched(n, ev.n) : capacity(n);
    const size_t K = 1 + 2 * (size_t)n_trials, per = 1 + (BATCH ? 3 : 2) * (size_t)cap;
    rc = check_hip(hipMemsetAsync(out, 0, sizeof(int64_t) * K * per, stream), "cluster_spectra: clear");
    if (rc || n == 0) return rc;
    const Ws w = make_ws(workspace, n, n_trials);
    if ((rc = check_hip(hipMemsetAsync(w.tab, 0, w.zero_bytes, stream), "cluster_spectra: clear workspace"))) return rc;
    const int64_t tn = (int64_t)n_trials * n;
    if (truth) launch(cs_classes_kernel<BATCH>, blocks_for(n, 8), kTpb, stream, truth, n, ev, w);
    launch(cs_hits_kernel<BATCH>, blocks_for(tn, 8), kTpb, stream, labels, n, tn, truth ? 1 : 0, ev, w);
    if ((rc = check_launch("cluster_spectra: tables"))) return rc;
    // without truth the class and cell tables are empty: their spectra keep d = 0
    const int step = truth ? 1 : 2;
    const unsigned ny = truth ? (unsigned)K : (unsigned)n_trials;
    auto *o = reinterpret_cast<unsigned long long *>(out);
    if (BATCH) {
        hipLaunchKernelGGL(cs_event_spectrum_kernel, dim3((unsigned)ev.n, ny), dim3(kTpb), 0, stream, labels, n, ev, step,
                           cap, w, o);
        return check_launch("cluster_spectra: spectra");
    }
    const int gs = (int)ceil_div(blocks_for((int64_t)w.S, 8), ny), gc = (int)ceil_div(blocks_for(kBins + (int64_t)w.B, 8), ny);
    hipLaunchKernelGGL(cs_spectrum_kernel, dim3(gs < 1 ? 1 : gs, ny), dim3(kTpb), 0, stream, step, w);
    hipLaunchKernelGGL(cs_compact_kernel, dim3(gc < 1 ? 1 : gc, ny), dim3(kTpb), 0, stream, step, cap, w, o);
    return check_launch("cluster_spectra: spectra");
}

}  // namespace

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

int64_t gnntrk_cluster_spectra_capacity(int64_t n) { return capacity(n); }

size_t gnntrk_cluster_spectra_workspace_bytes(int64_t n, int32_t n_trials) {
    return make_ws(nullptr, n < 0 ? 0 : n, n_trials < 1 ? 1 : n_trials).total;
}

int gnntrk_cluster_spectra(const int64_t *labels, int32_t n_trials, const int64_t *truth, int64_t n, int64_t *out,
                           void *workspace, size_t workspace_bytes, void *stream) {
    return cluster_spectra<false>(labels, n_trials, truth, n, Events{nullptr, 1}, out, workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

int64_t gnntrk_cluster_spectra_batched_capacity(int64_t n, int32_t n_seg) { return capacity_batched(n, n_seg); }

int gnntrk_cluster_spectra_batched(const int64_t *labels, int32_t n_trials, const int64_t *truth, int64_t n,
                                   const int64_t *seg_ptr, int32_t n_seg, int64_t *out, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    if (!seg_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "cluster_spectra: seg_ptr needs n_seg >= 1 events");
    return cluster_spectra<true>(labels, n_trials, truth, n, Events{seg_ptr, n_seg}, out, workspace, workspace_bytes,
                                 (hipStream_t)stream);
}

}  // extern "C"
