// Lock-free union-find over parent[N] (uint32), the merge structure of revo_gallery_clusters (clusters.hip; DESIGN.md
// section 4p).  Device code and, for tests/native/unionfind_host_check.cpp, host code: one source, the atomics behind UF_*.
//
//   invariant   parent[x] <= x at every instant; a root is an x with parent[x] == x.  Only two writes exist: the link
//               (compare-and-swap of a root's own index to a LOWER index) and the halving store (an ancestor of x, which is
//               <= parent[x] <= x, into a non-root x).  A non-root never becomes a root again.
//   root        the higher root is linked under the lower one, so a component's root is its lowest member.
//   stale reads a value read from parent[x] may be out of date; it is then an older ancestor of x, in x's component (links are
//               never removed), and lower than x: the walk still ends, and "same root" once seen stays true.
//   accesses    every access is a relaxed atomic at agent scope: L1 is per CU, and a line another XCD wrote is seen only by
//               such accesses.  parent[] is the only shared data and carries no payload: no fences.
//   bounds      every loop has a trip limit (UfLimits); past it the caller's error word is set and the operation gives up.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UF_FN __host__ __device__ __forceinline__
#else
#define UF_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define UF_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define UF_CAS(p, expected, desired) \
    __hip_atomic_compare_exchange_strong((p), (expected), (desired), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define UF_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define UF_STORE(p, v) __atomic_store_n((p), (v), __ATOMIC_RELAXED)
#define UF_CAS(p, expected, desired) __atomic_compare_exchange_n((p), (expected), (desired), false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)
#endif

namespace revo {

// trip limits of one call: walk = steps of one find (indices decrease strictly: N always suffices), retries = rounds of one
// unite.  A round fails only when another unite linked, in between, the very root this one was about to link, and the next
// round starts from a strictly lower node: 1024 + 2 * 32 rounds (N < 2^32) are far more than contention produces and still
// end a wave that a bug would otherwise leave spinning.
struct UfLimits { uint32_t walk, retries; };
UF_FN UfLimits uf_limits(long N) {
    UfLimits l;
    l.walk = (uint32_t)(N > 1 ? N : 1);
    l.retries = 1024u + 2u * 32u;
    return l;
}

// The root of x (as of some instant during the call), halving the path on the way.  *err is set when the walk's limit is hit;
// the node reached is returned.
UF_FN uint32_t uf_walk(uint32_t* parent, uint32_t x, uint32_t walk, bool& failed) {
    for (uint32_t s = 0; s < walk; ++s) {
        const uint32_t p = UF_LOAD(parent + x);
        if (p == x) return x;
        const uint32_t gp = UF_LOAD(parent + p);
        if (gp == p) return p;
        UF_STORE(parent + x, gp);                           // gp < p < x: an ancestor of x
        x = gp;
    }
    failed = true;
    return x;
}
UF_FN uint32_t uf_find(uint32_t* parent, uint32_t x, uint32_t walk, uint32_t* err) {
    bool failed = false;
    x = uf_walk(parent, x, walk, failed);
    if (failed) UF_STORE(err, 1u);
    return x;
}

// Joins the components of a and b; returns their common root as of the join (the lower of the two roots), or a node of a's
// component with *err set when a limit was hit.
UF_FN uint32_t uf_unite(uint32_t* parent, uint32_t a, uint32_t b, UfLimits lim, uint32_t* err) {
    bool failed = false;
    for (uint32_t t = 0; t < lim.retries && !failed; ++t) {
        a = uf_walk(parent, a, lim.walk, failed);
        b = uf_walk(parent, b, lim.walk, failed);
        if (failed) break;
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        uint32_t seen = hi;
        if (UF_CAS(parent + hi, &seen, lo)) return lo;
        a = seen;                                           // hi is no root any more: seen (< hi) is its parent, the truth
        b = lo;
    }
    UF_STORE(err, 1u);
    return a;
}

}  // namespace revo
