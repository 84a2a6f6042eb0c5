// Near-duplicate pairs of one gallery (revo_gallery_pairs, include/revo.h): every pair (i, j), i < j,
// of allowed rows whose fp32 score reaches a threshold, sorted by (i, j).  eps is the certificate's rigorous bound of
// |bf16 score - fp32 score| (cert_eps, kernels.h), here for a gallery row against a gallery row.
//
//   join     the 256 x 256 main loop over the upper triangle of row-tile pairs (ti <= tj; tile_walk.h), both operands the
//            gallery's bf16 rows; every score v >= lb = fl(thr - eps) lowered by its rounding is a candidate; keys (i << 32) | j are
//            appended (candidates.h wave_append)
//   rescore  the fp32 score of every candidate (the exact_dot4 chain); those >= thr are kept, as (i << b) | j, b = the bits
//            of the largest row index
//   sort     radix_sort.hip over the 2 b bits of the kept keys
//   emit     keys -> [n][2] int64 row pairs
// The host side of the pipeline (counts read back, the workspace's one regrow) is search.hip's CandidateWs.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

// (the join's bf16-score bound pairs_lb and the triangle's linearisation pairs_row_start: candidates.h, shared with clusters.hip)
// -------------------------------------------------------------------------- join ----
// tile_walk.h's tile-pair frame over the triangle; rows past N read as zeros and are never appended.
__global__ __launch_bounds__(G256_THREADS, 2) void pairs_join_kernel(PairsJoinArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float lb = pairs_lb(p.gstat, p.thr, p.D);
    tile_pair_frame(p, TriangleWalk{p.T}, smem, [&](int ci, int cj, long n0, bool diag, int wave, int lane, const f32x4 (&acc)[8][4]) {
        const TileLane t = tile_lane(wave, lane);
        const int lq = t.lq, rbase = t.rbase, cw = t.cw;
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        if (fm == 0ull) return;                             // wave-uniform: no allowed column
        const uint64_t bits = fm >> (lq * 4);
        const unsigned long long below = lanes_below(lane);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int row = rbase + m * 16;
            const float mx = tile_row_max(acc, m);
            if (__ballot(mx >= lb) == 0ull) continue;      // wave-uniform
            const long gi = (long)ci * 256 + row;
            const bool rok = gi < p.N && (!p.allow || ((p.allow[gi >> 5] >> (gi & 31)) & 1u));
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = cw + n * 16 + lq * 4 + j;
                    const bool take = rok && acc[m][n][j] >= lb && ((bits >> (n * 16 + j)) & 1ull) && (!diag || col > row);
                    const unsigned long long mk = __ballot(take);
                    if (mk == 0ull) continue;               // wave-uniform
                    const unsigned long long pos = wave_append(mk, p.cnt, lane, below);
                    if (take && pos < (unsigned long long)p.cap) p.keys[pos] = ((uint64_t)gi << 32) | (uint64_t)(n0 + col);
                }
        }
    });
}

// ----------------------------------------------------------------------- rescore ----
// wave g re-scores candidates 4 g .. 4 g + 3 (grid-stride); kept pairs are appended with one atomic per wave
__global__ __launch_bounds__(256) void pairs_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Gf,
                                                            long ldg, int D, float thr, int b, unsigned long long* __restrict__ kept,
                                                            uint64_t* __restrict__ out_keys, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const unsigned long long below = lanes_below(lane);
    for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < n; g += waves) {
        float v;
        uint64_t k;
        const int m = rescore_group4(cand, n, g * 4, D, lane, [&](uint64_t key, const float*& q, const float*& r) {
            q = Gf + (long)(key >> 32) * ldg;
            r = Gf + (long)(uint32_t)key * ldg;
        }, v, k);
        const bool take = lane < m && v >= thr;
        const unsigned long long mk = __ballot(take);
        if (mk == 0ull) continue;
        const unsigned long long pos = wave_append(mk, kept, lane, below);
        if (take) {
            out_keys[pos] = ((k >> 32) << b) | (k & 0xffffffffull);
            out_scores[pos] = v;
        }
    }
}

// -------------------------------------------------------------------------- emit ----
__global__ __launch_bounds__(256) void pairs_emit_kernel(const uint64_t* __restrict__ keys, const float* __restrict__ vals, long n,
                                                         int b, long long* __restrict__ pairs, float* __restrict__ scores) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint64_t k = keys[e];
    pairs[2 * e] = (long long)(k >> b);
    pairs[2 * e + 1] = (long long)(k & ((1ull << b) - 1ull));
    scores[e] = vals[e];
}

// ------------------------------------------------------------------------ launchers ----
// T, pairs and the grid of a join (`who`: the caller's name in the messages; no rows: a grid of 0): shared with clusters.hip
int pairs_join_plan(PairsJoinArgs& a, const char* who, long* wgs_out) {
    if (int rc = g256_check_operands(who, a.D, a.ldg)) return rc;
    REVO_REQUIRE(a.N < (1ll << 31), std::string(who) + ": row indices must fit in 31 bits");
    *wgs_out = 0;
    if (a.N <= 0) return 0;
    a.T = (a.N + 255) / 256;
    a.pairs = a.T * (a.T + 1) / 2;
    int dev = 0, cus = 0;
    REVO_HIP_CHECK(hipGetDevice(&dev));
    REVO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // one workgroup per CU (the LDS image takes the CU), each a contiguous range of < 2^30 tile pairs
    long wgs = cus > 0 ? cus : 256;
    if (wgs < (a.pairs >> 30) + 1) wgs = (a.pairs >> 30) + 1;
    if (wgs > a.pairs) wgs = a.pairs;
    *wgs_out = wgs;
    return 0;
}
int launch_pairs_join(const PairsJoinArgs& a_in, hipStream_t st) {
    PairsJoinArgs a = a_in;
    long wgs = 0;
    { const int rc = pairs_join_plan(a, "gallery_pairs", &wgs); if (rc) return rc; }
    if (wgs == 0) return 0;
    REVO_FUNC_LDS(pairs_join_kernel, G256_LDS);
    hipLaunchKernelGGL(pairs_join_kernel, dim3((unsigned)wgs), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_pairs_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, int b,
                         unsigned long long* kept, uint64_t* out_keys, float* out_scores, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(pairs_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Gf, ldg,
                       D, thr, b, kept, out_keys, out_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_pairs_emit(const uint64_t* keys, const float* vals, long n, int b, long long* pairs, float* scores, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pairs_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, vals, n, b, pairs, scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
