// Device-side helpers shared by the integer-counting units (metrics.hip, tracking_metrics.hip,
// kscan.hip): atomics, the open-addressing table keyed by "first hit + 1", the block reduction (wave
// sum of wave_util.h -> LDS -> one global atomic per workgroup and value), the events of a collated batch with the
// per-event form of that sum, and the pt cuts passed to kernels by value.
#pragma once

#include <stdio.h>

#include "host_util.h"
#include "wave_util.h"

namespace gnntrk {

// ------------------------------------------------------------------------------ atomics
// Relaxed, agent scope.  The CPU emulator build of the units (g++, host pointers) takes the GCC
// builtins.
__device__ __forceinline__ int32_t load_i32(const int32_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
__device__ __forceinline__ void store_i32(int32_t *p, int32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
__device__ __forceinline__ int32_t cas_i32(int32_t *p, int32_t expect, int32_t desired) {
#ifdef __HIP_DEVICE_COMPILE__
    return atomicCAS(p, expect, desired);
#else
    __atomic_compare_exchange_n(p, &expect, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
#endif
}
__device__ __forceinline__ void add_f64(double *p, double v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, v);
#else
    double old, nw;
    __atomic_load(p, &old, __ATOMIC_RELAXED);
    do {
        nw = old + v;
    } while (!__atomic_compare_exchange(p, &old, &nw, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED));
#endif
}
__device__ __forceinline__ void min_u64(unsigned long long *p, unsigned long long v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(p, v);
#else
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
#endif
}

// ------------------------------------------------------------------- open-addressing table
// A table groups hits by a key without sorting or densifying it: a slot holds "first hit + 1" of its
// group (0 = empty), so the key of a slot is read from the arrays of that hit and keys of any size fit
// an int32 slot.  Linear probing from the hash; a slot is claimed by compare-and-swap and never
// released, so a probe that meets its own key or an empty slot is final.  Termination: the table has
// more slots than there are hits (table_size), so a probe always meets an empty slot at the latest.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {   // (murmur3's finaliser)
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

inline uint64_t table_size(int64_t n) {   // power of two, at least twice the hits: load factor <= 1/2
    uint64_t s = 64;
    while (s < 2 * (uint64_t)n) s <<= 1;
    return s;
}

// the slot of hit i's group, claimed for it if the group is new.  same(h)...: hit h has the key of hit i; a key
// of several parts gives one predicate per part, tested left to right (a later part is read only where the
// earlier ones agree)
template <class... Same>
__device__ __forceinline__ uint64_t table_claim(int32_t *tab, uint64_t mask, uint64_t hash, int64_t i, Same... same) {
    uint64_t s = hash & mask;
    for (;;) {
        const int32_t h = cas_i32(&tab[s], 0, (int32_t)(i + 1));
        if (h == 0 || (same(h - 1) && ...)) break;
        s = (s + 1) & mask;
    }
    return s;
}

// the slot of the group with the key that same(h) tests for, or the empty slot that ends its probe
template <class Same>
__device__ __forceinline__ uint64_t table_find(const int32_t *tab, uint64_t mask, uint64_t hash, Same same) {
    uint64_t s = hash & mask;
    for (;;) {
        const int32_t h = tab[s];
        if (h == 0 || same(h - 1)) return s;
        s = (s + 1) & mask;
    }
}

// ------------------------------------------------------------------------ block reduction
// block-wide: adds the per-thread counts v[0..NV) into dst[0..NV) with one global atomic per value
template <int NV>
__device__ __forceinline__ void block_add(const uint32_t (&v)[NV], unsigned long long *dst) {
    __shared__ unsigned long long acc[NV];
    if (threadIdx.x < NV) acc[threadIdx.x] = 0ull;
    __syncthreads();
    for (int k = 0; k < NV; ++k) {
        const uint32_t s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[k], (unsigned long long)s);
    }
    __syncthreads();
    if (threadIdx.x < NV && acc[threadIdx.x]) atomicAdd(&dst[threadIdx.x], acc[threadIdx.x]);
}

// ------------------------------------------------------------------- events of a collated batch
// Hits [ptr[s], ptr[s + 1]) are event s, every event its own problem.  The kernels' BATCH = false instantiations
// (one event) never read it.  With BATCH a particle is the pair (event, particle id).
struct Events {
    const int64_t *ptr;
    int32_t n;
};
// the rows [lo, hi) of the event of hit i (one event: all rows) and its number
template <bool BATCH>
__device__ __forceinline__ int event_rows(const Events &ev, int64_t n, int64_t i, int64_t &lo, int64_t &hi) {
    lo = 0;
    hi = n;
    if (!BATCH) return 0;
    const int e = segment_of(ev.ptr, ev.n, i);
    lo = ev.ptr[e];
    hi = ev.ptr[e + 1];
    return e;
}
// hash of a particle: its id, with BATCH combined with its event
template <bool BATCH>
__device__ __forceinline__ uint64_t particle_hash(int64_t key, int e) {
    return mix64(BATCH ? (uint64_t)key + 0x9e3779b97f4a7c15ull * (uint64_t)(e + 1) : (uint64_t)key);
}

// wave-wide, every lane of the wave calls it: adds the per-lane counts v[0..NV) into dst[e * stride + 0..NV), e the
// lane's event, and clears them.  Hits are sorted by event, so the lanes of a wave that walks consecutive hits have
// one event unless an event edge falls among them: then a wave sum and one int64 atomic per value; otherwise every
// lane adds its own counts.  The event of a lane without counts is not looked at.
template <int NV>
__device__ __forceinline__ void event_add(uint32_t (&v)[NV], int e, unsigned long long *dst, size_t stride) {
    uint32_t any = 0u;
    for (int k = 0; k < NV; ++k) any |= v[k];
    const unsigned long long live = __ballot(any != 0u);
    if (live == 0ull) return;   // (uniform in the wave, as the branch below)
    const int lead = __builtin_ctzll(live);
    const int e0 = __shfl(e, lead);
    if (__ballot(any != 0u && e != e0) == 0ull) {
        for (int k = 0; k < NV; ++k) {
            const uint32_t s = wave_sum(v[k]);
            if ((int)(threadIdx.x & 63) == lead && s) atomicAdd(&dst[(size_t)e0 * stride + k], (unsigned long long)s);
        }
    } else {
        for (int k = 0; k < NV; ++k)
            if (v[k]) atomicAdd(&dst[(size_t)e * stride + k], (unsigned long long)v[k]);
    }
    for (int k = 0; k < NV; ++k) v[k] = 0u;
}

// ----------------------------------------------------------------------------- edge labels
// positive iff int(y) == 1 (BinaryClassificationStats: y.int() == 1), for labels held as bytes or as float32
template <class Y> __device__ __forceinline__ uint32_t is_positive(const Y *y, int64_t i);
template <> __device__ __forceinline__ uint32_t is_positive<uint8_t>(const uint8_t *y, int64_t i) { return y[i] == 1; }
// int(v) == 1 (truncation toward zero) for every finite v; NaN compares false
template <> __device__ __forceinline__ uint32_t is_positive<float>(const float *y, int64_t i) {
    const float v = y[i];
    return v >= 1.f && v < 2.f;
}

// -------------------------------------------------------------------------------- pt cuts
struct Cuts {   // (a kernel argument by value: nothing to upload)
    float v[GNNTRK_METRICS_MAX_CUTS];
    int32_t n;
};

// c = the n_cuts ascending values of cuts (NULL: zeros); refuses NaN and descending values as "<prefix>: ..."
inline int fill_cuts(Cuts &c, const float *cuts, int32_t n_cuts, const char *prefix) {
    c = Cuts{};
    c.n = n_cuts;
    for (int j = 0; cuts && j < n_cuts; ++j) {
        c.v[j] = cuts[j];
        if (!(cuts[j] == cuts[j]) || (j > 0 && !(cuts[j] >= cuts[j - 1]))) {
            char msg[96];
            snprintf(msg, sizeof(msg), "%s: the pt cuts must be ascending numbers", prefix);
            return fail(GNNTRK_EINVAL, msg);
        }
    }
    return GNNTRK_OK;
}

}  // namespace gnntrk
