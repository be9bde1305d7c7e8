// Helpers shared by the units that count over the particles and segments of a built graph (track_graph.hip,
// ec_scan.hip): the 64-bit maximum, the rows of a hit's event, the key that ranks the segments of a particle, and the
// check of the events argument of their entries.
#pragma once

#include <stdio.h>

#include "count_util.h"

namespace gnntrk {

__device__ __forceinline__ void max_u64(unsigned long long *p, unsigned long long v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicMax(p, v);
#else
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
#endif
}

// the rows [lo, hi) of the event of hit i, clipped to [0, n): whatever seg_ptr holds, an index inside them is a hit
__device__ __forceinline__ int tg_event_rows(const Events &ev, int64_t n, int64_t i, int64_t &lo, int64_t &hi) {
    const int e = event_rows<true>(ev, n, i, lo, hi);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    return e;
}

__device__ __forceinline__ unsigned long long seg_key(uint32_t size, int64_t label) {
    return ((unsigned long long)size << 32) | (unsigned long long)(0xffffffffu - (uint32_t)label);
}
__device__ __forceinline__ int64_t key_label(unsigned long long key) { return (int64_t)(0xffffffffu - (uint32_t)key); }

inline int check_events(const char *entry, const int64_t *seg_ptr, int32_t n_seg) {
    char msg[160];
    if (!seg_ptr || n_seg < 1) {
        snprintf(msg, sizeof(msg), "%s: seg_ptr needs n_seg >= 1 events", entry);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n_seg > GNNTRK_KSCAN_MAX_EVENTS) {
        snprintf(msg, sizeof(msg), "%s: n_seg = %d, at most %d events per call", entry, (int)n_seg,
                 GNNTRK_KSCAN_MAX_EVENTS);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    return GNNTRK_OK;
}

}  // namespace gnntrk
