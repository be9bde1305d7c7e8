// The lock-free union-find of the component kernels (kscan.hip, ec_scan.hip): parent[] holds hit indices, roots are
// only ever hooked under SMALLER roots, so parent[x] <= x always holds and the root of a tree is its minimum - the
// label of a component is unique and does not depend on the order in which atomics land.
//
// Memory-order argument of the union-find (ks_find / ks_unite): parent[] is read with relaxed
// agent-scope atomic loads and written with compare-and-swap (hooking a root) or relaxed atomic stores
// (path halving, which stores an ancestor of x into parent[x]).  The ancestors of a hit stay its
// ancestors for the rest of the launch (a non-root is never re-hooked, only moved up its own path), so a
// stale read is an older ancestor in the same component and costs extra steps, never a wrong answer.  A
// failed compare-and-swap continues from the value it returned.  Termination: parent[x] never increases
// and every failed compare-and-swap saw a strict decrease of one entry; the sum of all entries is
// bounded below.
#pragma once

#include "count_util.h"

namespace gnntrk {

// root of x with path halving (see the argument at the top)
__device__ __forceinline__ int32_t ks_find(int32_t *parent, int32_t x) {
    int32_t p = load_i32(&parent[x]);
    while (p != x) {
        const int32_t g = load_i32(&parent[p]);
        if (g == p) return p;
        store_i32(&parent[x], g);
        x = g;
        p = load_i32(&parent[x]);
    }
    return x;
}

__device__ __forceinline__ void ks_unite(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = ks_find(parent, a);
        b = ks_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = cas_i32(&parent[a], a, b);   // hook the larger root under the smaller
        if (old == a) return;
        a = old;   // a was hooked by someone else meanwhile: go on from its new parent
    }
}

}  // namespace gnntrk
