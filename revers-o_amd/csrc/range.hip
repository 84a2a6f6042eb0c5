// Range search (revo_search_range, include/revo.h): for each query every allowed gallery row whose fp32
// score reaches a threshold, ordered by (score desc, row asc).  eps(q) is the certificate's rigorous bound of |bf16 score -
// fp32 score| for query q (cert_eps with the query's own rounding norms, as topk_large.hip uses it).
//
//   join     the scan's 256 x 256 main loop and work plan (scan_plan.h: XCD-aware phases of query tiles x gallery slices,
//            the 64 / 128 / 192-row forms for a chunk of one query tile, non-temporal gallery DMA when there is one query
//            tile); every score v >= lb(q) = fl(thr - eps(q)) lowered by its rounding is a candidate; keys (q << 32) | row
//            are appended (candidates.h wave_append)
//   rescore  the fp32 score of every candidate (the chain of every re-score, pairs_dot4); those >= thr are kept as
//            (q << (32 + b)) | (~order-preserving score << b) | row, b = the bits of the largest row index, and counted per
//            query (agent-scope atomics)
//   sort     radix_sort.hip over those keys: (query, score desc, row asc)
//   emit     keys -> row + index_offset, scores;  offsets: inclusive prefix sums of the per-query counts (radix_sort.hip)
// The host side of the pipeline (counts read back, the workspace's one regrow) is search.hip's CandidateWs.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "scan_plan.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

static_assert(RANGE_PHASES == S256_PHASES, "the range join runs the scan's phases");
constexpr int RANGE_LDS = G256_LDS + 256 * 4;     // main loop | the tile's 256 query bounds

// -------------------------------------------------------------------------- join ----
// Block b of phase i -> query tile ph_q0[i] + j % ph_qn[i], slice j / ph_qn[i] of ph_ns[i] (j = b - ph_first[i]), as in the
// scan (topk_scan256_kernel, topk256.hip; the lookup is typed out in both kernels: see the comment there).  ROWS: the scan's row forms (0, or the chunk's queries fit in 64 / 128 / 192 rows of one tile);
// BAUX = 2: the gallery tiles are requested non-temporally (one query tile: every gallery row is read once).
template <int ROWS, int BAUX>
__global__ __launch_bounds__(G256_THREADS, 2) void range_join_kernel(RangeJoinArgs p) {
    constexpr bool DEEP = ROWS == 64 || ROWS == 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lbs = (float*)(smem + G256_LDS);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    // (constant indices only: a run-time index into the by-value argument block makes hipcc copy it to scratch)
    int ph_first = p.ph_first[0], ph_q0 = p.ph_q0[0], ph_qn = p.ph_qn[0], nsl = p.ph_ns[0];
#pragma unroll
    for (int i = 1; i < RANGE_PHASES; ++i)
        if (i < p.nph && (int)blockIdx.x >= p.ph_first[i]) { ph_first = p.ph_first[i]; ph_q0 = p.ph_q0[i]; ph_qn = p.ph_qn[i]; nsl = p.ph_ns[i]; }
    const int jloc = (int)blockIdx.x - ph_first;
    const int sp = __builtin_amdgcn_readfirstlane(jloc / ph_qn);
    const int q0 = (ph_q0 + (jloc - sp * ph_qn)) * 256;
    if (q0 >= p.Q) return;
    const int qvalid = (p.Q - q0) < 256 ? (p.Q - q0) : 256;
    int t0, t1;
    if (!tile_slice((int)((p.N + 255) / 256), nsl, sp, t0, t1)) return;
    if (tid < 256) {
        // lb(q): every row with fp32 score >= thr has bf16 score >= fl(thr - eps(q)) lowered by its rounding; +inf: no query
        float lb = INFINITY;
        if (tid < qvalid) {
            const long q = q0 + tid;
            const float eps = cert_eps(p.qstat[q * 2], p.qstat[q * 2 + 1], __uint_as_float(p.gstat[0]),
                                       __uint_as_float(p.gstat[1]), p.D);
            lb = score_down(p.thr - eps, p.thr);
        }
        lbs[tid] = lb;
    }
    __syncthreads();

    G256Operand A;
    g256_operand_init(A, p.Qb, p.ldq, p.Q, q0, wave, lane);
    // (the query bounds sit past the main loop's LDS image)
    tile_slice_frame<ROWS, DEEP, BAUX>(A, p.Gb, p.ldg, p.N, t0, t1, smem, p.D, wave, lane, [&](long n0, int lane, const f32x4 (&acc)[8][4]) {
        const int lr = lane & 15, lq = lane >> 4;
        const int wrow = (wave >> 2) * 128;                 // the wave's first query row of the tile
        const int cw = (wave & 3) * 64;                     // the wave's 64 columns: bits of one 64-bit word of the bitmap
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        if (fm == 0ull) return;                             // wave-uniform: no allowed column
        const uint64_t bits = fm >> (lq * 4);
        const unsigned long long below = lanes_below(lane);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (ROWS != 0 && wrow + m * 16 >= ROWS) continue;   // rows the row form never computed (no query there)
            const int row = wrow + m * 16 + lr;
            const float lb = lbs[row];
            const float mx = tile_row_max(acc, m);
            if (__ballot(mx >= lb) == 0ull) continue;      // wave-uniform: no score of these 16 queries reaches its bound
            const uint64_t qk = (uint64_t)(q0 + row) << 32;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = cw + n * 16 + lq * 4 + j;
                    const bool take = acc[m][n][j] >= lb && ((bits >> (n * 16 + j)) & 1ull);
                    const unsigned long long mk = __ballot(take);
                    if (mk == 0ull) continue;               // wave-uniform
                    const unsigned long long pos = wave_append(mk, p.cnt, lane, below);
                    if (take && pos < (unsigned long long)p.cap) p.keys[pos] = qk | (uint64_t)(n0 + col);
                }
        }
    });
}

// ----------------------------------------------------------------------- rescore ----
// Wave g re-scores candidates 4 g .. 4 g + 3 (grid-stride); kept entries are appended with one atomic per wave, and each
// query among the four is counted with one agent-scope atomic (exact whichever XCD runs the wave).
__global__ __launch_bounds__(256) void range_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Qf,
                                                            long ldq, const float* __restrict__ Gf, long ldg, int D, float thr, int b,
                                                            unsigned long long* __restrict__ kept,
                                                            unsigned long long* __restrict__ counts,
                                                            uint64_t* __restrict__ out_keys, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const unsigned long long below = lanes_below(lane);
    const int qshift = 32 + b;                              // <= 64; 64 only for a one-query chunk (query 0)
    for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < n; g += waves) {
        float v;
        uint64_t k;
        const int m = rescore_group4(cand, n, g * 4, D, lane, [&](uint64_t key, const float*& q, const float*& r) {
            q = Qf + (long)(key >> 32) * ldq;
            r = Gf + (long)(uint32_t)key * ldg;
        }, v, k);
        const bool take = lane < m && v >= thr;
        const unsigned long long mk = __ballot(take);
        if (mk == 0ull) continue;
        const unsigned long long pos = wave_append(mk, kept, lane, below);
        const uint32_t q = (uint32_t)(k >> 32);
        // the kept entries of this query among lanes 0..3; the first of them adds the count
        unsigned long long same = 0ull;
        bool first = true;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t qu = (uint32_t)__shfl((int)q, u, 64);
            if (((mk >> u) & 1ull) && qu == q) { ++same; if (u < lane) first = false; }
        }
        if (take) {
            const uint64_t qkey = qshift < 64 ? (uint64_t)q << qshift : 0ull;
            out_keys[pos] = qkey | ((uint64_t)(~f32_orderable(v)) << b) | (k & 0xffffffffull);
            out_scores[pos] = v;
            if (first) (void)__hip_atomic_fetch_add(counts + q, same, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// -------------------------------------------------------------------------- emit ----
__global__ __launch_bounds__(256) void range_emit_kernel(const uint64_t* __restrict__ keys, const float* __restrict__ vals, long n,
                                                         int b, long idx_offset, long long* __restrict__ idx,
                                                         float* __restrict__ scores) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    idx[e] = (long long)(keys[e] & ((1ull << b) - 1ull)) + idx_offset;
    scores[e] = vals[e];
}

// ------------------------------------------------------------------------ launchers ----
int launch_range_join(const RangeJoinArgs& a_in, hipStream_t st) {
    RangeJoinArgs a = a_in;
    if (int rc = g256_check_operands("search_range", a.D, a.ldg, a.ldq)) return rc;
    REVO_REQUIRE(a.N < (1ll << 32), "search_range: row indices must fit in 32 bits");
    if (a.Q <= 0 || a.N <= 0) return 0;
    const long tiles = (a.N + 255) / 256;
    const int qtiles = (a.Q + 255) / 256;
    Scan256Plan pl;
    scan256_plan(qtiles, tiles, pl);
    a.nph = pl.nph;
    const long blocks = scan256_phase_table(pl, a.ph_first, a.ph_q0, a.ph_qn, a.ph_ns);
    REVO_REQUIRE(blocks < (1l << 31), "search_range: too many workgroups");
    const dim3 grid((unsigned)blocks), block(G256_THREADS);
#define RANGE_LAUNCH(RW, AUX)                                                                 \
    do {                                                                                      \
        REVO_FUNC_LDS((range_join_kernel<RW, AUX>), RANGE_LDS);                               \
        hipLaunchKernelGGL((range_join_kernel<RW, AUX>), grid, block, RANGE_LDS, st, a);      \
    } while (0)
    // one query tile: the row form that covers the chunk, and every gallery row is read by one workgroup once
    if (a.Q <= 64) RANGE_LAUNCH(64, 2);
    else if (a.Q <= 128) RANGE_LAUNCH(128, 2);
    else if (a.Q <= 192) RANGE_LAUNCH(192, 2);
    else if (a.Q <= 256) RANGE_LAUNCH(0, 2);
    else RANGE_LAUNCH(0, 0);
#undef RANGE_LAUNCH
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_range_rescore(const uint64_t* cand, long n, const float* Qf, long ldq, const float* Gf, long ldg, int D, float thr,
                         int b, unsigned long long* kept, unsigned long long* counts, uint64_t* out_keys, float* out_scores,
                         hipStream_t st) {
    if (n <= 0) return 0;
    REVO_REQUIRE(b >= 1 && b <= 32, "search_range: bad key width");
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(range_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Qf, ldq,
                       Gf, ldg, D, thr, b, kept, counts, out_keys, out_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_range_emit(const uint64_t* keys, const float* vals, long n, int b, long idx_offset, long long* idx, float* scores,
                      hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, vals, n, b, idx_offset, idx,
                       scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
