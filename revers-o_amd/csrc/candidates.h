// Device-side pieces of the candidate pipeline (pairs, range and recommend searches, and the large-k
// count pass): the rounding slack of a bf16-score bound, the wave's column mask of a 256 x 256 tile, the wave-aggregated
// append, the group-of-four fp32 re-score.  Exactness rests on these: a fix is made here, once.
#pragma once
#include "topk_util.h"

namespace revo {

// x moved down / up by more than the rounding of the one or two fp32 operations that made it from values of magnitude <= |ref| + 1
__device__ __forceinline__ float score_down(float x, float ref) { return x - 4e-7f * (1.f + fabsf(ref)); }
__device__ __forceinline__ float score_up(float x, float ref) { return x + 4e-7f * (1.f + fabsf(ref)); }

// The wave's 64 columns cw .. cw + 63 of gallery tile n0: bit c is set when row n0 + cw + c exists (< N) and is allowed
// (allow: optional bitmap, zero-padded to whole 256-row tiles; the wave's bits are two whole words of it).  Wave-uniform.
__device__ __forceinline__ uint64_t tile_column_mask(long N, long n0, int cw, const uint32_t* allow) {
    const long left = N - n0 - cw;                          // rows of the gallery from the wave's first column on
    uint64_t fm = left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
    if (allow) {
        const long w0 = (n0 + cw) >> 5;
        fm &= (uint64_t)allow[w0] | ((uint64_t)allow[w0 + 1] << 32);
    }
    return fm;
}

// The bf16-score bound of the pairs join (pairs.hip, clusters.hip).  A row's bf16 copy gb_i has ||gb_i|| <= ||g_i|| + ||gb_i - g_i|| <= G + Eg, so a row used
// as the query of cert_eps has e_q <= Eg and n_qb <= G + Eg; cert_eps increases in both, so this eps bounds the error of
// every row-against-row score.  fl(thr - eps) lowered by its rounding: every pair with fp32 score >= thr has bf16 score >= lb.
__device__ __forceinline__ float pairs_lb(const uint32_t* gstat, float thr, int D) {
    const float G = __uint_as_float(gstat[0]), Eg = __uint_as_float(gstat[1]);
    const float eps = cert_eps(Eg, G + Eg, G, Eg, D);
    return score_down(thr - eps, thr);
}
// The other side of that bound (clusters.hip): fl(thr + eps) raised by its rounding: every pair with bf16 score >= ub has fp32
// score >= ub - eps >= thr.
__device__ __forceinline__ float pairs_ub(const uint32_t* gstat, float thr, int D) {
    const float G = __uint_as_float(gstat[0]), Eg = __uint_as_float(gstat[1]);
    const float eps = cert_eps(Eg, G + Eg, G, Eg, D);
    return score_up(thr + eps, thr);
}

// first tile pair of row tile ti in the row-major linearisation of the upper triangle (ti <= tj < T)
__device__ __forceinline__ long pairs_row_start(long ti, long T) { return ti * T - ti * (ti - 1) / 2; }

// Wave-aggregated append: mk = __ballot(take), not zero (the caller leaves, wave-uniformly, when no lane takes).  The lanes
// of mk get consecutive slots of the buffer *counter counts, one atomic per wave instruction.  The counter counts past the
// buffer's end: the caller bounds its store (take && pos < cap).  below = lanes_below(lane), computed outside unrolled loops.
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ unsigned long long wave_append(unsigned long long mk, unsigned long long* counter, int lane,
                                                          unsigned long long below) {
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(counter, (unsigned long long)__popcll(mk));
    base = readlane_u64(base, 0);
    return base + (unsigned long long)__popcll(mk & below);
}

// One wave re-scores candidates c0 .. c0 + m - 1 of cand[0 .. n), m = min(4, n - c0) (returned): rows(key, q, g) names the
// two fp32 rows of a candidate key, pairs_dot4 gives the four scores (loads past m repeat the last candidate), and lane
// u < m leaves with candidate u's score v and key k.
template <class Rows>
__device__ __forceinline__ int rescore_group4(const uint64_t* __restrict__ cand, long n, long c0, int D, int lane, Rows rows,
                                              float& v, uint64_t& k) {
    const int m = n - c0 < 4 ? (int)(n - c0) : 4;
    const float* qr[4];
    const float* gr[4];
    uint64_t key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        key[u] = cand[c0 + (u < m ? u : m - 1)];
        rows(key[u], qr[u], gr[u]);
    }
    float t[4];
    pairs_dot4(qr, gr, D, lane, t);
    v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
    k = lane == 0 ? key[0] : (lane == 1 ? key[1] : (lane == 2 ? key[2] : key[3]));
    return m;
}

}  // namespace revo
