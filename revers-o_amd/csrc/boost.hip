// Boosted search (revo_search_boosted, include/revo.h): one query, and per gallery row a multiplier
// m[r] >= 0 and a bias b[r]; final(r) = fmaf(m[r], s(r), b[r]) with s(r) the fp32 score of the one re-score chain; the best k
// allowed rows with s(r) >= min_similarity and final(r) >= threshold by (final desc, row asc).  a = a row's bf16 scan score,
// e = the query's cert_eps: s lies in [lo, hi] = [score_down(a - e), score_up(a + e)], and a correctly rounded fma is monotone
// in each argument, so with m >= 0 final lies in [fmaf(m, lo, b), fmaf(m, hi, b)]: no further widening.
//
//   sample   the pass below over 256-row tiles strided evenly over the gallery (boosts grow with the row index where they
//            come from timestamps: a prefix of the gallery would hold no good row), writing the lower bound of every allowed
//            row that certainly passes the minimum similarity (-inf otherwise)
//   level    recommend.hip's kernel: tau = the k-th largest of those, raised to the threshold: proven for ANY sample
//   pass     recommend.hip's pass with the one query row as A and no reduction over examples; per column it has m and b
//            (requested before the main loop starts: 8 bytes per row against 2 D), forms the upper bound and appends the
//            rows that can pass the minimum similarity and have an upper bound >= tau; it counts the allowed rows whose m
//            or b is outside the domain
//   rescore  four candidate rows per wave (pairs_dot4: every row its own chain), the two cuts, the fma; kept as
//            (~order-preserving final << b) | row, the similarity by row
//   sort, emit as in recommend.hip; the emit also delivers the similarities
// Candidates are rows: at most N of them, the workspace is sized once.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

constexpr int BOOST_LDS = G256_LDS + 256 + 4 * 64 * 4;   // main loop | e, tau | the query row's 64 scores of waves 0..3

// gallery tile of the pass's tile t: the sample's S tiles are the gallery tiles floor(t T / S), S <= T
template <bool SAMPLE>
__device__ __forceinline__ long boost_tile(int t, int T, int S) { return SAMPLE ? (long)t * T / S : (long)t; }

// m and b of row r (1 and 0 for a null array or a row past the gallery's end)
__device__ __forceinline__ void boost_load(const BoostPassArgs& p, long r, float& m, float& b) {
    const bool in = r < p.N;
    m = (p.mult && in) ? p.mult[r] : 1.f;
    b = (p.bias && in) ? p.bias[r] : 0.f;
}

// -------------------------------------------------------------------------- pass ----
// Workgroup s takes slice s of the tiles; waves 0..3 hold the query row's scores of their 64 columns (row 0 of the tile:
// fragment 0 of the lanes with lr == 0), waves 4..7 only move data.  The scores go through 64 floats of LDS per wave so that
// lane c holds column c: m and b are then one coalesced request each, made for the NEXT tile before that tile's prologue is
// issued (older than every DMA request the main loop counts, so its vmcnt waits stay right; its last wait covers them).
template <bool SAMPLE>
__global__ __launch_bounds__(G256_THREADS, 2) void boost_pass_kernel(BoostPassArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* par = (float*)(smem + G256_LDS);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nsl = (int)gridDim.x, sl = (int)blockIdx.x;
    const int T = (int)((p.N + 255) / 256), S = SAMPLE ? (int)(p.n_sample / 256) : T;
    int t0, t1;
    if (!tile_slice(S, nsl, sl, t0, t1)) return;
    if (tid == 0) {
        par[0] = cert_eps(p.qstat[0], p.qstat[1], __uint_as_float(p.gstat[0]), __uint_as_float(p.gstat[1]), p.D);
        par[1] = SAMPLE ? 0.f : p.tau[0];
    }
    __syncthreads();

    G256Operand A, B;
    g256_operand_init(A, p.Qb, p.ldq, 1, 0, wave, lane);
    long g0 = boost_tile<SAMPLE>(t0, T, S) * 256;
    float mv = 1.f, bv = 0.f;
    if (wave < 4) boost_load(p, g0 + wave * 64 + lane, mv, bv);
    asm volatile("" ::: "memory");
    g256_operand_init(B, p.Gb + g0 * p.ldg, p.ldg, p.N - g0, 0, wave, lane);
    g256_issue_prologue_deep<2>(A, B, smem, p.D, wave);
    unsigned long long n_allowed = 0ull, n_bad = 0ull;      // wave-uniform: allowed rows met, those outside the domain
    for (int t = t0; t < t1; ++t) {
        const long n0 = g0;
        f32x4 acc[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm256_mainloop<64, false, true, 0, 2>(A, B, smem, p.D, wave, lane, acc);
        // (the main loop's last wait was vmcnt(0): this tile's m and b have arrived)
        asm volatile("" : "+v"(mv), "+v"(bv));
        const float m_r = mv, b_r = bv;
        if (t + 1 < t1) {
            g0 = boost_tile<SAMPLE>(t + 1, T, S) * 256;
            if (wave < 4) boost_load(p, g0 + wave * 64 + lane, mv, bv);
            asm volatile("" ::: "memory");
            g256_operand_init(B, p.Gb + g0 * p.ldg, p.ldg, p.N - g0, 0, wave, lane);
            g256_issue_prologue_deep<2>(A, B, smem, p.D, wave);
        }
        if (wave >= 4) continue;                            // the query row is in the first wave-row
        asm volatile("" : "+v"(lane) :: "memory");
        const int lr = lane & 15, lq = lane >> 4;
        const int cw = wave * 64;
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        if (!SAMPLE) {
            if (fm == 0ull) continue;                       // wave-uniform: no allowed column (their m and b are not looked at)
            n_allowed += (unsigned long long)__popcll(fm);
        }
        float* sc = par + 64 + cw;
        if (lr == 0) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) sc[n * 16 + lq * 4 + j] = acc[0][n][j];
        }
        __builtin_amdgcn_wave_barrier();
        const float a = sc[lane];
        __builtin_amdgcn_wave_barrier();
        const bool allowed = (fm >> lane) & 1ull;
        const float e = par[0];
        const float lo = score_down(a - e, a - e), hi = score_up(a + e, a + e);
        const bool plain = !p.mult && !p.bias;              // wave-uniform: final = s, no operation
        if (SAMPLE) {
            const float f_lo = plain ? lo : fmaf(m_r, lo, b_r);
            const bool sure = allowed && (!p.has_min || lo >= p.min_sim) && f_lo == f_lo;   // (a NaN bound never raises the level)
            p.lb_out[(long)t * 256 + cw + lane] = sure ? f_lo : -INFINITY;
        } else {
            const bool bad = allowed && !(fabsf(m_r) < INFINITY && m_r >= 0.f && fabsf(b_r) < INFINITY);
            n_bad += (unsigned long long)__popcll(__ballot(bad));
            const float f_hi = plain ? hi : fmaf(m_r, hi, b_r);
            const bool take = allowed && !(p.has_min && hi < p.min_sim) && !(f_hi < par[1]);   // (a NaN bound keeps the row)
            const unsigned long long mk = __ballot(take);
            if (mk == 0ull) continue;                       // wave-uniform
            const unsigned long long pos = wave_append(mk, p.cnt, lane, lanes_below(lane));
            if (take && pos < (unsigned long long)p.cap) p.rows[pos] = (uint32_t)(n0 + cw + lane);
        }
    }
    if (!SAMPLE && wave < 4 && lane == 0) {
        if (n_allowed != 0ull) atomicAdd(p.cnt + 2, n_allowed);
        if (n_bad != 0ull) atomicAdd(p.cnt + 3, n_bad);
    }
}

// ----------------------------------------------------------------------- rescore ----
// Wave w re-scores candidate rows 4 w .. 4 w + 3, then 4 (w + waves) ...: pairs_dot4 with the query as every pair's first row
// (a row's score keeps its own chain: the bits every other search gives it); lane u < 4 finishes row u: the minimum-similarity
// cut on s, final = fmaf(m, s, b) (s itself when both arrays are null), the threshold cut on final.  Kept rows are appended
// with one atomic per wave; the key orders -0 with +0 (equal finals: the row index decides); s goes to sim[row].
__global__ __launch_bounds__(256) void boost_rescore_kernel(BoostRescoreArgs r) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const unsigned long long below = lanes_below(lane);
    const float* qr[4] = {r.Qf, r.Qf, r.Qf, r.Qf};
    for (long c0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4; c0 < r.n; c0 += waves * 4) {
        const int m = r.n - c0 < 4 ? (int)(r.n - c0) : 4;
        uint32_t rows[4];
        const float* gr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rows[u] = r.cand[c0 + (u < m ? u : m - 1)];
            gr[u] = r.Gf + (long)rows[u] * r.ldg;
        }
        float t[4];
        pairs_dot4(qr, gr, r.D, lane, t);
        const float s = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
        const uint32_t row = lane == 0 ? rows[0] : (lane == 1 ? rows[1] : (lane == 2 ? rows[2] : rows[3]));
        bool keep = lane < m && !(r.has_min && !(s >= r.min_sim));
        float f = s;
        if (r.mult || r.bias) f = fmaf(r.mult ? r.mult[row] : 1.f, s, r.bias ? r.bias[row] : 0.f);
        if (r.has_thr && !(f >= r.thr)) keep = false;
        const unsigned long long mk = __ballot(keep);
        if (mk == 0ull) continue;                           // wave-uniform
        const unsigned long long pos = wave_append(mk, r.kept, lane, below);
        if (keep) {
            const float fk = f == 0.f ? 0.f : f;
            r.out_keys[pos] = ((uint64_t)(~f32_orderable(fk)) << r.b) | (uint64_t)row;
            r.out_scores[pos] = f;
            r.sim[row] = s;
        }
    }
}

// -------------------------------------------------------------------------- emit ----
// recommend.hip's emit, and sims[i] = sim[row of entry i] (-inf in the padding)
__global__ __launch_bounds__(256) void boost_emit_kernel(const uint64_t* __restrict__ keys, const float* __restrict__ vals, long n, int k,
                                                         int b, long idx_offset, const float* __restrict__ sim,
                                                         float* __restrict__ scores, float* __restrict__ sims,
                                                         long long* __restrict__ idx, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) counts[0] = (int)(n < k ? n : k);
    if (i >= k) return;
    if (i < n) {
        const long long row = (long long)(keys[i] & ((1ull << b) - 1ull));
        scores[i] = vals[i];
        sims[i] = sim[row];
        idx[i] = row + idx_offset;
    } else {
        scores[i] = -INFINITY;
        sims[i] = -INFINITY;
        idx[i] = -1;
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_boost_pass(const BoostPassArgs& a, int sample, hipStream_t st) {
    if (int rc = g256_check_operands("search_boosted", a.D, a.ldg, a.ldq)) return rc;
    REVO_REQUIRE(a.N < (1ll << 32), "search_boosted: row indices must fit in 32 bits");
    if (a.N <= 0) return 0;
    const long T = (a.N + 255) / 256, tiles = sample ? a.n_sample / 256 : T;
    REVO_REQUIRE(!sample || (a.n_sample % 256 == 0 && tiles >= 1 && tiles <= T && a.lb_out), "search_boosted: bad sample");
    REVO_REQUIRE(sample || (a.tau && a.cnt && a.rows), "search_boosted: null pass argument");
    const dim3 grid((unsigned)pass256_slices(tiles)), block(G256_THREADS);
    if (sample) {
        REVO_FUNC_LDS((boost_pass_kernel<true>), BOOST_LDS);
        hipLaunchKernelGGL((boost_pass_kernel<true>), grid, block, BOOST_LDS, st, a);
    } else {
        REVO_FUNC_LDS((boost_pass_kernel<false>), BOOST_LDS);
        hipLaunchKernelGGL((boost_pass_kernel<false>), grid, block, BOOST_LDS, st, a);
    }
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_boost_rescore(const BoostRescoreArgs& a, hipStream_t st) {
    if (a.n <= 0) return 0;
    REVO_REQUIRE(a.b >= 1 && a.b <= 32, "search_boosted: bad key width");
    const long blocks = (a.n + 15) / 16;
    hipLaunchKernelGGL(boost_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_boost_emit(const uint64_t* keys, const float* vals, long n, int k, int b, long idx_offset, const float* sim,
                      float* scores, float* sims, long long* idx, int* counts, hipStream_t st) {
    hipLaunchKernelGGL(boost_emit_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, keys, vals, n, k, b, idx_offset, sim,
                       scores, sims, idx, counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
