// Tracking metrics of the object-condensation validation (metrics/cluster_metrics.py:76-259 as
// postprocessing/dbscanscanner.py:146-187 calls it once per DBSCAN trial): for every trial and pt cut
// the integer counts behind TrackingMetrics - clusters passing the cluster mask and their perfect /
// double-majority / LHC matches - plus the number of particles passing the hit mask.
//
// The reference groups hits with pandas (value_counts of (cluster, particle), groupby means per
// particle).  Here both groupings are open-addressing hash tables in the workspace whose slots hold
// "first hit + 1" of their group (count_util.h: claimed by compare-and-swap; a probe compares the keys of
// the slot's hit), so particle ids of any size need no sort and no densification:
//
//   once per call (hits)        tm_particles_kernel   particle table; per particle its hit count, fp64
//                                                     sums and non-NaN counts of pt / eta / reconstructable
//                                                     and the highest cut class of its hits (hit mask)
//                     (slots)   tm_particle_kernel    per particle the cut class of its means (cluster
//                                                     mask) and n_particles per cut
//   all trials at once (hits)   tm_pairs_kernel       (cluster, particle) table per trial; pair counts
//                                                     and cluster sizes
//                     (slots)   tm_best_count_kernel  per cluster the largest pair count
//                     (slots)   tm_best_pid_kernel    per cluster the smallest particle id with that count
//                     (labels)  tm_clusters_kernel    per valid cluster its flags, summed per cut: wave
//                                                     sums, LDS, one int64 atomic per workgroup and value
//
// Every output is an integer count, so the result does not depend on the order in which atomics land.
//
// tracking_metrics_batched: the same counts for every event of a collated batch from the same launch sequence
// (BATCH = true instantiations).  A particle is (event, particle id), a cluster (event, local label) with the dense
// slot seg_ptr[event] + label, so the tables keep their sizes; tm_particle_batched_kernel and
// tm_clusters_batched_kernel add to their event's rows of the output.
//
// Two more entries share the tables, the pair kernels and the tie rule:
//   tracking_metrics_windows    the same counts for up to 32 two-sided (pt, eta) windows that may overlap
//                               (tracking_metrics_vs_pt / _vs_eta, cluster_metrics.py:292-384).  Windows
//                               are not nested, so the "highest cut class" becomes a bit mask per particle:
//                               tm_particles_kernel<WinSel> ORs the windows of its hits, tmw_particle_kernel
//                               stores the windows of its means, tmw_clusters_kernel walks the set bits
//   cluster_table               one labelling's per-cluster rows (tracking_metric_df, :76-149) as dense
//                               per-label columns: tm_table_kernel
// Both have their batched entry too (tracking_metrics_windows_batched, cluster_table_batched): the BATCH = true
// tables of fill_tables, tmw_particle_batched_kernel / tmw_clusters_batched_kernel after their cut-class siblings, and
// tm_table_kernel<true>, whose row is the cluster slot seg_ptr[event] + label; majority_of<true> finds the majority
// particle among those of the cluster's event.
// Tie rule: the majority particle of a cluster is the one with the most hits in it and, among equals,
// the smallest particle id (pandas' value_counts leaves ties to an unstable sort).
#include <math.h>
#include <stdio.h>

#include "count_util.h"

namespace gnntrk {
namespace {

constexpr int kTpb = 256;
constexpr int kMaxCuts = GNNTRK_METRICS_MAX_CUTS;
constexpr int kProps = 3;   // pt, eta, reconstructable
constexpr int kMaxWin = GNNTRK_TRACKING_MAX_WINDOWS;

// signed particle id -> unsigned key of the same order (the tie rule's atomic minimum)
__device__ __forceinline__ unsigned long long pid_key(int64_t pid) { return (unsigned long long)pid ^ (1ull << 63); }

// number of ascending cuts c with !(v < c) and v >= c: NaN passes none
__device__ __forceinline__ int cut_class(float v, const Cuts &cuts) {
    int k = 0;
    for (int j = 0; j < cuts.n; ++j) k += (v >= cuts.v[j]) ? 1 : 0;
    return k;
}

// up to kMaxWin windows (pt_lo, pt_hi, eta_lo, eta_hi), passed to kernels by value
struct Windows {
    float v[kMaxWin][4];
    int32_t n;
};

// bit j: lo <= value < hi of window j for pt and (signed) eta; a NaN bound is not tested, a NaN value
// fails every test that is
__device__ __forceinline__ uint32_t window_mask(float pt, float eta, const Windows &w) {
    uint32_t m = 0u;
    for (int j = 0; j < w.n; ++j) {
        const float *b = w.v[j];
        const bool in = (b[0] != b[0] || pt >= b[0]) && (b[1] != b[1] || pt < b[1]) &&
                        (b[2] != b[2] || eta >= b[2]) && (b[3] != b[3] || eta < b[3]);
        m |= in ? (1u << j) : 0u;
    }
    return m;
}

// What a hit contributes to its particle's phit word.  CutSel: the highest cut class, nested cuts
// (tracking_metrics).  WinSel: the mask of the windows it lies in (n = 0: nothing, cluster_table).
struct CutSel {
    Cuts cuts;
    float max_eta;
    // hit mask: pt >= cut, reconstructable truthy (NaN is), |eta| < max_eta (NaN is not)
    __device__ __forceinline__ uint32_t hit(float pt, float eta, float reco) const {
        return (reco != 0.f && fabsf(eta) < max_eta) ? (uint32_t)cut_class(pt, cuts) : 0u;
    }
    __device__ __forceinline__ static void merge(uint32_t *p, uint32_t c) { atomicMax(p, c); }
};
struct WinSel {
    Windows win;
    __device__ __forceinline__ uint32_t hit(float pt, float eta, float reco) const {
        return reco != 0.f ? window_mask(pt, eta, win) : 0u;
    }
    __device__ __forceinline__ static void merge(uint32_t *p, uint32_t c) { atomicOr(p, c); }
};

// The events of a collated batch (Events, event_rows, particle_hash: count_util.h).  With BATCH a particle is the
// pair (event, particle id), and a cluster the pair (event, local label) with the dense slot ptr[s] + label < n.

// the particle table's slot of pid (present: every particle id of the hits was inserted); BATCH: of the
// particle (e, pid), e the event with the rows [lo, hi) - the same id and the event of the slot's first hit
template <bool BATCH>
__device__ __forceinline__ int64_t find_particle(const int32_t *ptab, const int64_t *pid, uint64_t mask, int64_t key,
                                                 int e, int64_t lo, int64_t hi) {
    return (int64_t)table_find(ptab, mask, particle_hash<BATCH>(key, e),
                               [&](int32_t h) { return pid[h] == key && (!BATCH || (h >= lo && h < hi)); });
}

struct Ws {
    int32_t *ptab;            // [S]  particle table: first hit + 1, 0 = empty
    uint32_t *pcnt;           // [S]  hits per particle
    uint32_t *phit;           // [S]  highest hit cut class of the particle (n_particles); windows: mask of its hits
    uint32_t *pcls;           // [S]  cut class of the particle's means (cluster mask); windows: their mask
    uint32_t *pnn;            // [3][S] non-NaN values per property
    double *psum;             // [3][S] fp64 sums of the non-NaN values
    uint32_t *hslot;          // [n]  particle slot of every hit
    int32_t *ttab;            // [T][S] (cluster, particle) table per trial: first hit + 1
    uint32_t *tcnt;           // [T][S] hits per (cluster, particle)
    uint32_t *csize;          // [T][n] cluster sizes
    uint32_t *cbest;          // [T][n] largest pair count per cluster
    unsigned long long *cpid; // [T][n] smallest pid_key with that count (filled with ones)
    size_t zero_bytes;        // everything before cpid is cleared
    size_t total;
    uint64_t S;
};

Ws make_ws(void *base, int64_t n, int32_t T) {
    Ws w{};
    w.S = table_size(n);
    const size_t S = w.S, N = (size_t)n, TS = (size_t)T * S, TN = (size_t)T * N;
    Carver ws{(char *)base};
    w.psum = ws.take<double>(kProps * S);
    w.ptab = ws.take<int32_t>(S);
    w.pcnt = ws.take<uint32_t>(S);
    w.phit = ws.take<uint32_t>(S);
    w.pcls = ws.take<uint32_t>(S);
    w.pnn = ws.take<uint32_t>(kProps * S);
    w.hslot = ws.take<uint32_t>(N);
    w.ttab = ws.take<int32_t>(TS);
    w.tcnt = ws.take<uint32_t>(TS);
    w.csize = ws.take<uint32_t>(TN);
    w.cbest = ws.take<uint32_t>(TN);
    w.zero_bytes = ws.off;
    w.cpid = ws.take<unsigned long long>(TN);
    w.total = ws.off;
    return w;
}

// ------------------------------------------------------------------ once per call
template <class Sel, bool BATCH>
__global__ __launch_bounds__(kTpb) void tm_particles_kernel(const int64_t *__restrict__ pid,
                                                            const float *__restrict__ pt,
                                                            const float *__restrict__ eta,
                                                            const float *__restrict__ reco, int64_t n, Events ev,
                                                            Sel sel, Ws w) {
    const uint64_t mask = w.S - 1;
    for (int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTpb) {
        const int64_t key = pid[i];
        int64_t lo, hi;
        const int e = event_rows<BATCH>(ev, n, i, lo, hi);
        const uint64_t s = table_claim(w.ptab, mask, particle_hash<BATCH>(key, e), i, [&](int32_t h) {
            return pid[h] == key && (!BATCH || (h >= lo && h < hi));
        });
        w.hslot[i] = (uint32_t)s;
        atomicAdd(&w.pcnt[s], 1u);
        const float v[kProps] = {pt[i], eta[i], reco[i]};
        for (int k = 0; k < kProps; ++k) {
            if (v[k] != v[k]) continue;   // (pandas' mean skips NaN)
            add_f64(&w.psum[(size_t)k * w.S + s], (double)v[k]);
            atomicAdd(&w.pnn[(size_t)k * w.S + s], 1u);
        }
        const uint32_t hc = sel.hit(v[0], v[1], v[2]);
        if (hc) Sel::merge(&w.phit[s], hc);
    }
}

// fp64 mean of property k of the particle in slot s, rounded once to fp32 (groupby().mean() keeps a
// float32 column's dtype); NaN where every value was
__device__ __forceinline__ float particle_mean(const Ws &w, int k, int64_t s) {
    const uint32_t c = w.pnn[(size_t)k * w.S + s];
    return c ? (float)(w.psum[(size_t)k * w.S + s] / (double)c) : NAN;
}

// stores the cut class of the means of the particle in slot s (cluster mask of a cluster with this majority
// particle: maj_pt >= cut, maj_reconstructable truthy - non-zero and not NaN -, |maj_eta| < max_eta) and returns
// the highest cut class of its hits (hit mask)
__device__ __forceinline__ uint32_t particle_classes(const Cuts &cuts, float max_eta, const Ws &w, int64_t s) {
    float mean[kProps];
    for (int k = 0; k < kProps; ++k) mean[k] = particle_mean(w, k, s);
    const bool ok = mean[2] != 0.f && mean[2] == mean[2] && fabsf(mean[1]) < max_eta;
    w.pcls[s] = ok ? (uint32_t)cut_class(mean[0], cuts) : 0u;
    return w.phit[s];
}

__global__ __launch_bounds__(kTpb) void tm_particle_kernel(Cuts cuts, float max_eta, Ws w,
                                                           unsigned long long *__restrict__ n_particles) {
    __shared__ uint32_t acc[kMaxCuts];
    if (threadIdx.x < kMaxCuts) acc[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t cnt[kMaxCuts] = {};
    const int64_t S = (int64_t)w.S;
    for (int64_t base = (int64_t)blockIdx.x * kTpb; base < S; base += (int64_t)gridDim.x * kTpb) {
        const int64_t s = base + threadIdx.x;
        if (s >= S || w.ptab[s] == 0) continue;
        const uint32_t hc = particle_classes(cuts, max_eta, w, s);
        for (int c = 0; c < kMaxCuts; ++c) cnt[c] += (uint32_t)c < hc ? 1u : 0u;
    }
    for (int c = 0; c < cuts.n; ++c) {
        const uint32_t t = wave_sum(cnt[c]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&acc[c], t);
    }
    __syncthreads();
    if (threadIdx.x < cuts.n && acc[threadIdx.x]) atomicAdd(&n_particles[threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// the same per event: n_particles[e][cut], e the event of the slot's first hit.  The slots of a block hold
// particles of any event, so every particle adds to its event's counts with int64 atomics
__global__ __launch_bounds__(kTpb) void tm_particle_batched_kernel(Cuts cuts, float max_eta, Ws w, Events ev,
                                                                   unsigned long long *__restrict__ n_particles) {
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        const int32_t first = w.ptab[s];
        if (first == 0) continue;
        const uint32_t hc = particle_classes(cuts, max_eta, w, s);
        if (hc == 0) continue;
        const int e = segment_of(ev.ptr, ev.n, first - 1);
        for (uint32_t c = 0; c < hc; ++c) atomicAdd(&n_particles[(size_t)e * cuts.n + c], 1ull);
    }
}

// ------------------------------------------------------------------- all trials
// hits of every trial (flattened [T][n]); noise (label < 0) joins no cluster; labels >= n are
// counted in *bad and otherwise ignored.  BATCH: labels are local to the hit's event of n_e hits - a label >= n_e is
// the bad one - and the cluster's slot is the event's first row + label.  A pair's key stays (label, particle slot):
// the particle slot is the event's own
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void tm_pairs_kernel(const int64_t *__restrict__ labels, int64_t n, int64_t tn,
                                                        Events ev, Ws w, unsigned long long *__restrict__ bad) {
    const uint64_t mask = w.S - 1;
    for (int64_t idx = (int64_t)blockIdx.x * kTpb + threadIdx.x; idx < tn; idx += (int64_t)gridDim.x * kTpb) {
        const int64_t lab = labels[idx];
        if (lab < 0) continue;
        const int64_t t = idx / n, i = idx - t * n;
        int64_t lo, hi;
        event_rows<BATCH>(ev, n, i, lo, hi);
        if (lab >= hi - lo) {
            atomicAdd(bad, 1ull);
            continue;
        }
        const int64_t cl = lo + lab;
        const int64_t *lt = labels + t * n;
        int32_t *tab = w.ttab + (size_t)t * w.S;
        const uint32_t ps = w.hslot[i];
        const uint64_t s = table_claim(tab, mask, mix64(((uint64_t)cl << 32) | ps), i,
                                       [&](int32_t h) { return lt[h] == lab; }, [&](int32_t h) { return w.hslot[h] == ps; });
        atomicAdd(&w.tcnt[(size_t)t * w.S + s], 1u);
        atomicAdd(&w.csize[t * n + cl], 1u);
    }
}

// the cluster slot of an occupied pair slot e of trial t (-1: empty)
template <bool BATCH>
__device__ __forceinline__ int64_t pair_cluster(const int64_t *labels, int64_t n, const Events &ev, const Ws &w,
                                                int64_t t, int64_t e, int32_t &hit) {
    hit = w.ttab[e];
    if (hit == 0) return -1;
    int64_t lo, hi;
    event_rows<BATCH>(ev, n, hit - 1, lo, hi);
    return lo + labels[t * n + hit - 1];
}

template <bool BATCH>
__global__ __launch_bounds__(kTpb) void tm_best_count_kernel(const int64_t *__restrict__ labels, int64_t n, int64_t ts,
                                                             Events ev, Ws w) {
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < ts; e += (int64_t)gridDim.x * kTpb) {
        const int64_t t = e / (int64_t)w.S;
        int32_t hit;
        const int64_t cl = pair_cluster<BATCH>(labels, n, ev, w, t, e, hit);
        if (cl >= 0) atomicMax(&w.cbest[t * n + cl], w.tcnt[e]);
    }
}

template <bool BATCH>
__global__ __launch_bounds__(kTpb) void tm_best_pid_kernel(const int64_t *__restrict__ labels,
                                                           const int64_t *__restrict__ pid, int64_t n, int64_t ts,
                                                           Events ev, Ws w) {
    for (int64_t e = (int64_t)blockIdx.x * kTpb + threadIdx.x; e < ts; e += (int64_t)gridDim.x * kTpb) {
        const int64_t t = e / (int64_t)w.S;
        int32_t hit;
        const int64_t cl = pair_cluster<BATCH>(labels, n, ev, w, t, e, hit);
        if (cl >= 0 && w.tcnt[e] == w.cbest[t * n + cl]) min_u64(&w.cpid[t * n + cl], pid_key(pid[hit - 1]));
    }
}

// the matches of a cluster of `size` hits, `maj` of them of its majority particle, which has `pid_hits` hits in
// all (fp64 ratios as the reference evaluates them)
struct Match {
    uint32_t perfect, dm, lhc;
};
__device__ __forceinline__ Match match_flags(uint32_t maj, uint32_t size, uint32_t pid_hits) {
    const double frac = (double)maj / (double)size, pid_frac = (double)maj / (double)pid_hits;
    Match m;
    m.perfect = (pid_hits == maj && frac > 0.99) ? 1u : 0u;
    m.dm = (pid_frac > 0.5 && frac > 0.5) ? 1u : 0u;
    m.lhc = frac > 0.75 ? 1u : 0u;
    return m;
}

// one trial per blockIdx.y; a cluster is a label with at least one hit
__global__ __launch_bounds__(kTpb) void tm_clusters_kernel(const int64_t *__restrict__ pid, int64_t n, Cuts cuts,
                                                           int32_t count_thld, Ws w,
                                                           unsigned long long *__restrict__ out) {
    __shared__ uint32_t acc[kMaxCuts * 4];
    if (threadIdx.x < kMaxCuts * 4) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = blockIdx.y;
    const uint64_t mask = w.S - 1;
    // per cut: clusters, perfect, double majority, lhc
    uint32_t cnt[kMaxCuts][4] = {};
    for (int64_t lab = (int64_t)blockIdx.x * kTpb + threadIdx.x; lab < n; lab += (int64_t)gridDim.x * kTpb) {
        const uint32_t size = w.csize[t * n + lab];
        if (size == 0 || (int64_t)size < (int64_t)count_thld) continue;   // not a valid cluster
        const uint32_t maj = w.cbest[t * n + lab];
        const int64_t key = (int64_t)(w.cpid[t * n + lab] ^ (1ull << 63));
        const int64_t ps = find_particle<false>(w.ptab, pid, mask, key, 0, 0, n);
        const uint32_t cls = w.pcls[ps];
        if (cls == 0) continue;
        const Match m = match_flags(maj, size, w.pcnt[ps]);
        for (int c = 0; c < kMaxCuts; ++c) {
            if ((uint32_t)c >= cls) break;
            cnt[c][0] += 1u;
            cnt[c][1] += m.perfect;
            cnt[c][2] += m.dm;
            cnt[c][3] += m.lhc;
        }
    }
    for (int c = 0; c < cuts.n; ++c)
        for (int k = 0; k < 4; ++k) {
            const uint32_t s = wave_sum(cnt[c][k]);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[c * 4 + k], s);
        }
    __syncthreads();
    if (threadIdx.x < cuts.n * 4 && acc[threadIdx.x])
        atomicAdd(&out[(size_t)t * cuts.n * 4 + threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// The same per event: one trial per blockIdx.y, one block per 256 cluster slots (no grid stride: a block's slots
// are consecutive rows, so most blocks lie inside one event).  out[t][e][cut][4].  A block inside one event sums as
// above - wave sums, LDS, one int64 atomic per value -; a block that spans an event edge adds every cluster to its
// event's counts with int64 atomics.
__global__ __launch_bounds__(kTpb) void tm_clusters_batched_kernel(const int64_t *__restrict__ pid, int64_t n, Cuts cuts,
                                                                   int32_t count_thld, Events ev, Ws w,
                                                                   unsigned long long *__restrict__ out) {
    __shared__ uint32_t acc[kMaxCuts * 4];
    if (threadIdx.x < kMaxCuts * 4) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = blockIdx.y;
    const uint64_t mask = w.S - 1;
    const int64_t c0 = (int64_t)blockIdx.x * kTpb, c1 = c0 + kTpb < n ? c0 + kTpb - 1 : n - 1;
    const int e0 = segment_of(ev.ptr, ev.n, c0);
    const bool one_event = e0 == segment_of(ev.ptr, ev.n, c1);
    unsigned long long *out_t = out + (size_t)t * ev.n * cuts.n * 4;
    uint32_t cnt[kMaxCuts][4] = {};
    const int64_t cl = c0 + threadIdx.x;
    if (cl < n) {
        const uint32_t size = w.csize[t * n + cl];
        if (size != 0 && (int64_t)size >= (int64_t)count_thld) {   // a valid cluster
            int64_t lo, hi;
            const int e = event_rows<true>(ev, n, cl, lo, hi);
            const uint32_t maj = w.cbest[t * n + cl];
            const int64_t key = (int64_t)(w.cpid[t * n + cl] ^ (1ull << 63));
            const int64_t ps = find_particle<true>(w.ptab, pid, mask, key, e, lo, hi);
            const uint32_t cls = w.pcls[ps];
            const Match m = match_flags(maj, size, w.pcnt[ps]);
            const uint32_t add[4] = {1u, m.perfect, m.dm, m.lhc};
            for (int c = 0; c < kMaxCuts; ++c) {
                if ((uint32_t)c >= cls) break;
                for (int k = 0; k < 4; ++k) {
                    if (one_event) cnt[c][k] += add[k];
                    else if (add[k]) atomicAdd(&out_t[((size_t)e * cuts.n + c) * 4 + k], 1ull);
                }
            }
        }
    }
    if (!one_event) return;   // (uniform in the block)
    for (int c = 0; c < cuts.n; ++c)
        for (int k = 0; k < 4; ++k) {
            const uint32_t s = wave_sum(cnt[c][k]);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[c * 4 + k], s);
        }
    __syncthreads();
    if (threadIdx.x < cuts.n * 4 && acc[threadIdx.x])
        atomicAdd(&out_t[(size_t)e0 * cuts.n * 4 + threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// ---------------------------------------------------------------------- windows
// per particle the windows of its means (cluster mask: maj_reconstructable non-zero and not NaN) and
// n_particles per window: the set bits of the hit mask into LDS, one int64 atomic per workgroup and window
__global__ __launch_bounds__(kTpb) void tmw_particle_kernel(Windows win, Ws w,
                                                            unsigned long long *__restrict__ n_particles) {
    __shared__ uint32_t acc[kMaxWin];
    if (threadIdx.x < kMaxWin) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        if (w.ptab[s] == 0) continue;
        const float reco = particle_mean(w, 2, s);
        const bool ok = reco != 0.f && reco == reco;
        w.pcls[s] = ok ? window_mask(particle_mean(w, 0, s), particle_mean(w, 1, s), win) : 0u;
        for (uint32_t m = w.phit[s]; m; m &= m - 1u) atomicAdd(&acc[__ffsll((unsigned long long)m) - 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < win.n && acc[threadIdx.x])
        atomicAdd(&n_particles[threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// the same per event: n_particles[e][window], e the event of the slot's first hit.  The slots of a block hold
// particles of any event, so every set bit adds to its event's counts with an int64 atomic
__global__ __launch_bounds__(kTpb) void tmw_particle_batched_kernel(Windows win, Ws w, Events ev,
                                                                    unsigned long long *__restrict__ n_particles) {
    const int64_t S = (int64_t)w.S;
    for (int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x; s < S; s += (int64_t)gridDim.x * kTpb) {
        const int32_t first = w.ptab[s];
        if (first == 0) continue;
        const float reco = particle_mean(w, 2, s);
        const bool ok = reco != 0.f && reco == reco;
        w.pcls[s] = ok ? window_mask(particle_mean(w, 0, s), particle_mean(w, 1, s), win) : 0u;
        uint32_t m = w.phit[s];
        if (m == 0u) continue;
        const int e = segment_of(ev.ptr, ev.n, first - 1);
        for (; m; m &= m - 1u)
            atomicAdd(&n_particles[(size_t)e * win.n + (__ffsll((unsigned long long)m) - 1)], 1ull);
    }
}

// what the tables hold about the cluster of label lab in trial t
struct Majority {
    uint32_t size, hits, pid_hits;   // cluster size, hits of the majority particle in it and anywhere
    int64_t pid, slot;               // the majority particle and its slot in the particle table
};
// lab: the cluster's dense slot - its label, with BATCH the first row of its event + its local label; the majority
// particle is looked up among the particles of that event, whose number is returned in e
template <bool BATCH>
__device__ __forceinline__ Majority majority_of(const int64_t *pid, int64_t n, const Events &ev, const Ws &w, int64_t t,
                                                int64_t lab, int &e) {
    Majority m;
    m.size = w.csize[t * n + lab];
    m.hits = w.cbest[t * n + lab];
    m.pid = (int64_t)(w.cpid[t * n + lab] ^ (1ull << 63));
    int64_t lo, hi;
    e = event_rows<BATCH>(ev, n, lab, lo, hi);
    m.slot = find_particle<BATCH>(w.ptab, pid, w.S - 1, m.pid, e, lo, hi);
    m.pid_hits = w.pcnt[m.slot];
    return m;
}

// one trial per blockIdx.y; per valid cluster its flags into the LDS counters of the windows of its
// majority particle's means (windows are mostly disjoint: one or two set bits)
__global__ __launch_bounds__(kTpb) void tmw_clusters_kernel(const int64_t *__restrict__ pid, int64_t n, int32_t n_win,
                                                            int32_t count_thld, Ws w,
                                                            unsigned long long *__restrict__ out) {
    __shared__ uint32_t acc[kMaxWin * 4];
    if (threadIdx.x < kMaxWin * 4) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = blockIdx.y;
    for (int64_t lab = (int64_t)blockIdx.x * kTpb + threadIdx.x; lab < n; lab += (int64_t)gridDim.x * kTpb) {
        const uint32_t size = w.csize[t * n + lab];
        if (size == 0 || (int64_t)size < (int64_t)count_thld) continue;   // not a valid cluster
        int e;
        const Majority c = majority_of<false>(pid, n, Events{}, w, t, lab, e);
        uint32_t m = w.pcls[c.slot];
        if (m == 0) continue;
        const Match f = match_flags(c.hits, size, c.pid_hits);
        for (; m; m &= m - 1u) {
            uint32_t *a = &acc[(__ffsll((unsigned long long)m) - 1) * 4];
            atomicAdd(&a[0], 1u);
            if (f.perfect) atomicAdd(&a[1], 1u);
            if (f.dm) atomicAdd(&a[2], 1u);
            if (f.lhc) atomicAdd(&a[3], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < n_win * 4 && acc[threadIdx.x])
        atomicAdd(&out[(size_t)t * n_win * 4 + threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// The same per event: one trial per blockIdx.y, one block per 256 cluster slots, as tm_clusters_batched_kernel (a
// block's slots are consecutive rows, so most blocks lie inside one event).  out[t][e][window][4].  A block inside
// one event counts in LDS and adds one int64 atomic per non-zero value; a block that spans an event edge adds every
// cluster to its event's counts with int64 atomics.
__global__ __launch_bounds__(kTpb) void tmw_clusters_batched_kernel(const int64_t *__restrict__ pid, int64_t n,
                                                                    int32_t n_win, int32_t count_thld, Events ev, Ws w,
                                                                    unsigned long long *__restrict__ out) {
    __shared__ uint32_t acc[kMaxWin * 4];
    if (threadIdx.x < kMaxWin * 4) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * kTpb, c1 = c0 + kTpb < n ? c0 + kTpb - 1 : n - 1;
    const int e0 = segment_of(ev.ptr, ev.n, c0);
    const bool one_event = e0 == segment_of(ev.ptr, ev.n, c1);
    unsigned long long *out_t = out + (size_t)t * ev.n * n_win * 4;
    const int64_t cl = c0 + threadIdx.x;
    if (cl < n) {
        const uint32_t size = w.csize[t * n + cl];
        if (size != 0 && (int64_t)size >= (int64_t)count_thld) {   // a valid cluster
            int e;
            const Majority c = majority_of<true>(pid, n, ev, w, t, cl, e);
            uint32_t m = w.pcls[c.slot];
            const Match f = match_flags(c.hits, size, c.pid_hits);
            const uint32_t add[4] = {1u, f.perfect, f.dm, f.lhc};
            for (; m; m &= m - 1u) {
                const int j = __ffsll((unsigned long long)m) - 1;
                for (int k = 0; k < 4; ++k) {
                    if (!add[k]) continue;
                    if (one_event) atomicAdd(&acc[j * 4 + k], 1u);
                    else atomicAdd(&out_t[((size_t)e * n_win + j) * 4 + k], 1ull);
                }
            }
        }
    }
    if (!one_event) return;   // (uniform in the block)
    __syncthreads();
    if (threadIdx.x < n_win * 4 && acc[threadIdx.x])
        atomicAdd(&out_t[(size_t)e0 * n_win * 4 + threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// ----------------------------------------------------------------- cluster table
// the rows of tracking_metric_df of one labelling, one per cluster slot (cluster_size 0: no such cluster); BATCH: the
// slot is the event's first row + the local label, the majority particle one of the event
template <bool BATCH>
__global__ __launch_bounds__(kTpb) void tm_table_kernel(const int64_t *__restrict__ pid, int64_t n, Events ev, Ws w,
                                                        int64_t *__restrict__ cluster_size,
                                                        int64_t *__restrict__ maj_hits, int64_t *__restrict__ maj_pid,
                                                        int64_t *__restrict__ maj_pid_hits, float *__restrict__ maj_pt,
                                                        float *__restrict__ maj_eta, float *__restrict__ maj_reco) {
    for (int64_t lab = (int64_t)blockIdx.x * kTpb + threadIdx.x; lab < n; lab += (int64_t)gridDim.x * kTpb) {
        Majority c{};
        float mean[kProps] = {0.f, 0.f, 0.f};
        if (w.csize[lab]) {
            int e;
            c = majority_of<BATCH>(pid, n, ev, w, 0, lab, e);
            for (int k = 0; k < kProps; ++k) mean[k] = particle_mean(w, k, c.slot);
        }
        cluster_size[lab] = (int64_t)c.size;
        maj_hits[lab] = (int64_t)c.hits;
        maj_pid[lab] = c.pid;
        maj_pid_hits[lab] = (int64_t)c.pid_hits;
        maj_pt[lab] = mean[0];
        maj_eta[lab] = mean[1];
        maj_reco[lab] = mean[2];
    }
}

// clears the tables and fills them: the particle table with sel's hit words, then per trial the pair
// table, cluster sizes, best counts and best particle ids; *bad counts the labels >= n.  BATCH: per event of ev
template <class Sel, bool BATCH = false>
int fill_tables(const char *what, const int64_t *labels, int32_t n_trials, const int64_t *pid, const float *pt,
                const float *eta, const float *reco, int64_t n, const Sel &sel, const Ws &w, unsigned long long *bad,
                hipStream_t stream, Events ev = Events{}) {
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: clear workspace", what);
    int rc;
    if ((rc = check_hip(hipMemsetAsync(w.psum, 0, w.zero_bytes, stream), msg))) return rc;
    if ((rc = check_hip(hipMemsetAsync(w.cpid, 0xFF, 8 * (size_t)n_trials * n, stream), msg))) return rc;
    const int64_t S = (int64_t)w.S, tn = (int64_t)n_trials * n, ts = (int64_t)n_trials * S;
    hipLaunchKernelGGL((tm_particles_kernel<Sel, BATCH>), dim3(blocks_for(n, 8)), dim3(kTpb), 0, stream, pid, pt, eta,
                       reco, n, ev, sel, w);
    hipLaunchKernelGGL(tm_pairs_kernel<BATCH>, dim3(blocks_for(tn, 8)), dim3(kTpb), 0, stream, labels, n, tn, ev, w, bad);
    hipLaunchKernelGGL(tm_best_count_kernel<BATCH>, dim3(blocks_for(ts, 8)), dim3(kTpb), 0, stream, labels, n, ts, ev, w);
    hipLaunchKernelGGL(tm_best_pid_kernel<BATCH>, dim3(blocks_for(ts, 8)), dim3(kTpb), 0, stream, labels, pid, n, ts, ev,
                       w);
    snprintf(msg, sizeof(msg), "%s: tables", what);
    return check_launch(msg);
}

// the checks the three entries share, before any launch
int check_hits(const char *entry, int64_t n, int32_t n_trials, const void *labels, const void *pid, const void *pt,
               const void *eta, const void *reco, const void *workspace, size_t workspace_bytes) {
    char msg[160];
    if (n_trials < 1 || n_trials > GNNTRK_TRACKING_MAX_TRIALS) {
        snprintf(msg, sizeof(msg), "%s: n_trials = %d, expected 1..%d", entry, (int)n_trials,
                 GNNTRK_TRACKING_MAX_TRIALS);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n > 0 && (!labels || !pid || !pt || !eta || !reco)) {
        snprintf(msg, sizeof(msg), "%s: NULL labels, particle ids, pt, eta or reconstructable", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n > 0) return check_workspace(entry, workspace, workspace_bytes, make_ws(nullptr, n, n_trials).total);
    return GNNTRK_OK;
}

// what the three workspace-size entries share
size_t tracking_metrics_ws_bytes(int64_t n, int32_t n_trials) {
    return make_ws(nullptr, n < 0 ? 0 : n, n_trials < 1 ? 1 : n_trials).total;
}

// gnntrk_tracking_metrics (BATCH = false, ev.n = 1) and gnntrk_tracking_metrics_batched
template <bool BATCH>
int tracking_metrics(const int64_t *labels, int32_t n_trials, const int64_t *particle_id, const float *pt,
                     const float *eta, const float *reconstructable, int64_t n, Events ev, const float *cuts,
                     int32_t n_cuts, float max_eta, int32_t predicted_count_thld, int64_t *out, void *workspace,
                     size_t workspace_bytes, hipStream_t stream) {
    char msg[160];
    int rc = check_count_i30("tracking_metrics", "hit", n);
    if (rc) return rc;
    if (n_cuts < 1 || n_cuts > kMaxCuts) {
        snprintf(msg, sizeof(msg), "tracking_metrics: n_cuts = %d, expected 1..%d", (int)n_cuts, kMaxCuts);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (!cuts) return fail(GNNTRK_EINVAL, "tracking_metrics: NULL cuts");
    CutSel sel{};
    sel.max_eta = max_eta;
    if ((rc = fill_cuts(sel.cuts, cuts, n_cuts, "tracking_metrics"))) return rc;
    if (!out) return fail(GNNTRK_EINVAL, "tracking_metrics: NULL output");
    if ((rc = check_hits("tracking_metrics", n, n_trials, labels, particle_id, pt, eta, reconstructable, workspace,
                         workspace_bytes)))
        return rc;
    const size_t n_ev = (size_t)ev.n;   // (one event: 1)
    const size_t n_out = n_ev * n_cuts + (size_t)n_trials * n_ev * n_cuts * 4 + 1;
    rc = check_hip(hipMemsetAsync(out, 0, sizeof(int64_t) * n_out, stream), "tracking_metrics: clear");
    if (rc || n == 0) return rc;
    const Ws w = make_ws(workspace, n, n_trials);
    auto *o = reinterpret_cast<unsigned long long *>(out);
    if ((rc = fill_tables<CutSel, BATCH>("tracking_metrics", labels, n_trials, particle_id, pt, eta, reconstructable, n,
                                         sel, w, o + n_out - 1, stream, ev)))
        return rc;
    if (BATCH) {
        hipLaunchKernelGGL(tm_particle_batched_kernel, dim3(blocks_for((int64_t)w.S, 4)), dim3(kTpb), 0, stream,
                           sel.cuts, max_eta, w, ev, o);
        hipLaunchKernelGGL(tm_clusters_batched_kernel, dim3((unsigned)ceil_div(n, kTpb), (unsigned)n_trials), dim3(kTpb),
                           0, stream, particle_id, n, sel.cuts, predicted_count_thld, ev, w, o + n_ev * n_cuts);
        return check_launch("tracking_metrics: clusters");
    }
    hipLaunchKernelGGL(tm_particle_kernel, dim3(blocks_for((int64_t)w.S, 4)), dim3(kTpb), 0, stream, sel.cuts, max_eta,
                       w, o);
    const int gx = (int)((blocks_for(n, 8) + n_trials - 1) / n_trials);
    hipLaunchKernelGGL(tm_clusters_kernel, dim3(gx < 1 ? 1 : gx, (unsigned)n_trials), dim3(kTpb), 0, stream,
                       particle_id, n, sel.cuts, predicted_count_thld, w, o + n_cuts);
    return check_launch("tracking_metrics: clusters");
}

// gnntrk_tracking_metrics_windows (BATCH = false, ev.n = 1) and gnntrk_tracking_metrics_windows_batched
template <bool BATCH>
int tracking_metrics_windows(const int64_t *labels, int32_t n_trials, const int64_t *particle_id, const float *pt,
                             const float *eta, const float *reconstructable, int64_t n, Events ev, const float *windows,
                             int32_t n_win, int32_t predicted_count_thld, int64_t *out, void *workspace,
                             size_t workspace_bytes, hipStream_t stream) {
    char msg[160];
    int rc = check_count_i30("tracking_metrics_windows", "hit", n);
    if (rc) return rc;
    if (n_win < 1 || n_win > kMaxWin) {
        snprintf(msg, sizeof(msg), "tracking_metrics_windows: n_win = %d, expected 1..%d", (int)n_win, kMaxWin);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (!windows) return fail(GNNTRK_EINVAL, "tracking_metrics_windows: NULL windows");
    if (!out) return fail(GNNTRK_EINVAL, "tracking_metrics_windows: NULL output");
    if ((rc = check_hits("tracking_metrics_windows", n, n_trials, labels, particle_id, pt, eta, reconstructable,
                         workspace, workspace_bytes)))
        return rc;
    WinSel sel{};
    sel.win.n = n_win;
    for (int j = 0; j < n_win; ++j)
        for (int k = 0; k < 4; ++k) sel.win.v[j][k] = windows[4 * j + k];
    const size_t n_ev = (size_t)ev.n;   // (one event: 1)
    const size_t n_out = n_ev * n_win + (size_t)n_trials * n_ev * n_win * 4 + 1;
    rc = check_hip(hipMemsetAsync(out, 0, sizeof(int64_t) * n_out, stream), "tracking_metrics_windows: clear");
    if (rc || n == 0) return rc;
    const Ws w = make_ws(workspace, n, n_trials);
    auto *o = reinterpret_cast<unsigned long long *>(out);
    if ((rc = fill_tables<WinSel, BATCH>("tracking_metrics_windows", labels, n_trials, particle_id, pt, eta,
                                         reconstructable, n, sel, w, o + n_out - 1, stream, ev)))
        return rc;
    if (BATCH) {
        hipLaunchKernelGGL(tmw_particle_batched_kernel, dim3(blocks_for((int64_t)w.S, 4)), dim3(kTpb), 0, stream,
                           sel.win, w, ev, o);
        hipLaunchKernelGGL(tmw_clusters_batched_kernel, dim3((unsigned)ceil_div(n, kTpb), (unsigned)n_trials),
                           dim3(kTpb), 0, stream, particle_id, n, n_win, predicted_count_thld, ev, w, o + n_ev * n_win);
        return check_launch("tracking_metrics_windows: clusters");
    }
    hipLaunchKernelGGL(tmw_particle_kernel, dim3(blocks_for((int64_t)w.S, 4)), dim3(kTpb), 0, stream, sel.win, w, o);
    const int gx = (int)((blocks_for(n, 8) + n_trials - 1) / n_trials);
    hipLaunchKernelGGL(tmw_clusters_kernel, dim3(gx < 1 ? 1 : gx, (unsigned)n_trials), dim3(kTpb), 0, stream,
                       particle_id, n, n_win, predicted_count_thld, w, o + n_win);
    return check_launch("tracking_metrics_windows: clusters");
}

// gnntrk_cluster_table (BATCH = false) and gnntrk_cluster_table_batched
template <bool BATCH>
int cluster_table(const int64_t *labels, const int64_t *particle_id, const float *pt, const float *eta,
                  const float *reconstructable, int64_t n, Events ev, int64_t *cluster_size, int64_t *maj_hits,
                  int64_t *maj_pid, int64_t *maj_pid_hits, float *maj_pt, float *maj_eta, float *maj_reconstructable,
                  int64_t *n_bad, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    int rc = check_count_i30("cluster_table", "hit", n);
    if (rc) return rc;
    if (!n_bad) return fail(GNNTRK_EINVAL, "cluster_table: NULL n_bad");
    if (n > 0 &&
        (!cluster_size || !maj_hits || !maj_pid || !maj_pid_hits || !maj_pt || !maj_eta || !maj_reconstructable))
        return fail(GNNTRK_EINVAL, "cluster_table: NULL output column");
    if ((rc = check_hits("cluster_table", n, 1, labels, particle_id, pt, eta, reconstructable, workspace, workspace_bytes)))
        return rc;
    rc = check_hip(hipMemsetAsync(n_bad, 0, sizeof(int64_t), stream), "cluster_table: clear");
    if (rc || n == 0) return rc;
    const Ws w = make_ws(workspace, n, 1);
    // (no windows: the hits leave no mask, only the particle table and its sums are wanted)
    if ((rc = fill_tables<WinSel, BATCH>("cluster_table", labels, 1, particle_id, pt, eta, reconstructable, n, WinSel{},
                                         w, reinterpret_cast<unsigned long long *>(n_bad), stream, ev)))
        return rc;
    hipLaunchKernelGGL(tm_table_kernel<BATCH>, dim3(blocks_for(n, 8)), dim3(kTpb), 0, stream, particle_id, n, ev, w,
                       cluster_size, maj_hits, maj_pid, maj_pid_hits, maj_pt, maj_eta, maj_reconstructable);
    return check_launch("cluster_table: rows");
}

}  // namespace
}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_tracking_metrics_workspace_bytes(int64_t n, int32_t n_trials) {
    return tracking_metrics_ws_bytes(n, n_trials);
}

size_t gnntrk_tracking_metrics_windows_workspace_bytes(int64_t n, int32_t n_trials) {
    return tracking_metrics_ws_bytes(n, n_trials);
}

size_t gnntrk_cluster_table_workspace_bytes(int64_t n) { return tracking_metrics_ws_bytes(n, 1); }

int gnntrk_tracking_metrics(const int64_t *labels, int32_t n_trials, const int64_t *particle_id, const float *pt,
                            const float *eta, const float *reconstructable, int64_t n, const float *cuts,
                            int32_t n_cuts, float max_eta, int32_t predicted_count_thld, int64_t *out, void *workspace,
                            size_t workspace_bytes, void *stream) {
    return tracking_metrics<false>(labels, n_trials, particle_id, pt, eta, reconstructable, n, Events{nullptr, 1}, cuts,
                                   n_cuts, max_eta, predicted_count_thld, out, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}

int gnntrk_tracking_metrics_batched(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                    const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                    const int64_t *seg_ptr, int32_t n_seg, const float *cuts, int32_t n_cuts,
                                    float max_eta, int32_t predicted_count_thld, int64_t *out, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (!seg_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "tracking_metrics: seg_ptr needs n_seg >= 1 events");
    return tracking_metrics<true>(labels, n_trials, particle_id, pt, eta, reconstructable, n, Events{seg_ptr, n_seg},
                                  cuts, n_cuts, max_eta, predicted_count_thld, out, workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

int gnntrk_tracking_metrics_windows(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                    const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                    const float *windows, int32_t n_win, int32_t predicted_count_thld, int64_t *out,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    return tracking_metrics_windows<false>(labels, n_trials, particle_id, pt, eta, reconstructable, n,
                                           Events{nullptr, 1}, windows, n_win, predicted_count_thld, out, workspace,
                                           workspace_bytes, (hipStream_t)stream);
}

int gnntrk_tracking_metrics_windows_batched(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                            const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                            const int64_t *seg_ptr, int32_t n_seg, const float *windows, int32_t n_win,
                                            int32_t predicted_count_thld, int64_t *out, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    if (!seg_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "tracking_metrics_windows: seg_ptr needs n_seg >= 1 events");
    return tracking_metrics_windows<true>(labels, n_trials, particle_id, pt, eta, reconstructable, n,
                                          Events{seg_ptr, n_seg}, windows, n_win, predicted_count_thld, out, workspace,
                                          workspace_bytes, (hipStream_t)stream);
}

int gnntrk_cluster_table(const int64_t *labels, const int64_t *particle_id, const float *pt, const float *eta,
                         const float *reconstructable, int64_t n, int64_t *cluster_size, int64_t *maj_hits,
                         int64_t *maj_pid, int64_t *maj_pid_hits, float *maj_pt, float *maj_eta,
                         float *maj_reconstructable, int64_t *n_bad, void *workspace, size_t workspace_bytes,
                         void *stream) {
    return cluster_table<false>(labels, particle_id, pt, eta, reconstructable, n, Events{nullptr, 1}, cluster_size,
                                maj_hits, maj_pid, maj_pid_hits, maj_pt, maj_eta, maj_reconstructable, n_bad, workspace,
                                workspace_bytes, (hipStream_t)stream);
}

int gnntrk_cluster_table_batched(const int64_t *labels, const int64_t *particle_id, const float *pt, const float *eta,
                                 const float *reconstructable, int64_t n, const int64_t *seg_ptr, int32_t n_seg,
                                 int64_t *cluster_size, int64_t *maj_hits, int64_t *maj_pid, int64_t *maj_pid_hits,
                                 float *maj_pt, float *maj_eta, float *maj_reconstructable, int64_t *n_bad,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (!seg_ptr || n_seg < 1) return fail(GNNTRK_EINVAL, "cluster_table: seg_ptr needs n_seg >= 1 events");
    return cluster_table<true>(labels, particle_id, pt, eta, reconstructable, n, Events{seg_ptr, n_seg}, cluster_size,
                               maj_hits, maj_pid, maj_pid_hits, maj_pt, maj_eta, maj_reconstructable, n_bad, workspace,
                               workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
