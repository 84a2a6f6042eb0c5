// Search by examples (revo_search_recommend, include/revo.h): P positive and Nn negative example
// vectors, score(r) = sp if sp > sn else -(sn * sn) with sp / sn the largest fp32 score of row r against a positive / a
// negative example; the best k allowed rows by (score desc, row asc).  e is the largest cert_eps over the examples: the
// rigorous bound of |bf16 score - fp32 score| (kernels.h), so with a / b the largest bf16 scores of a row over the
// positives / negatives, sp lies in [a - e, a + e] and sn in [b - e, b + e].
//
//   sample   the pass below over the first n_s rows, writing lb(r) <= score(r) of every allowed row (-inf otherwise)
//   level    tau = the k-th largest lb of the sample (-inf with fewer than k), raised to the threshold if there is one:
//            k rows score at least tau, so every row of the answer has ub(r) >= score(r) >= tau
//   pass     the 64- / 128-row form of the 256 x 256 main loop (deep DMA schedule, non-temporal gallery requests, the next
//            tile's prologue issued before the epilogue) with A = the example rows; its epilogue
//            reduces each score column over the example rows (all of them live in ONE wave: registers, then DPP row
//            rotations), computes ub(r) and appends the rows with ub(r) >= tau (candidates.h wave_append, once per tile)
//   rescore  one wave per candidate row: the P + Nn fp32 scores (the chain of every re-score, pairs_dot4), score(r), the
//            threshold cut; kept as (~order-preserving score << b) | row, b = the bits of the largest row index
//   sort     radix_sort.hip over those keys: (score desc, row asc)
//   emit     the first k -> row + index_offset, scores; the rest padded
// Candidates are rows: at most N of them, the workspace is sized once.  The host reads the candidate count before the
// re-score and the kept count before the sort: the call is synchronous.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

constexpr int REC_LDS = G256_LDS + 256;           // main loop | e, tau

// Bounds of score(r) from the bf16 maxima a (positives) and b (negatives; unused when there is no negative).
// Branch A (sp > sn) is possible iff a + e > b - e and gives [a - e, a + e]; branch B iff a - e <= b + e and gives
// [-M^2, -m^2], m / M the smallest / largest |x| on [b - e, b + e].  The interval ends are moved outward first (score_down /
// score_up, each end its own reference), which only makes a branch possible more often and its interval wider; one of the
// two is always possible.
__device__ __forceinline__ void rec_bounds(float a, float b, float e, bool has_neg, float& lb, float& ub) {
    const float a_lo = score_down(a - e, a - e), a_hi = score_up(a + e, a + e);
    if (!has_neg) { lb = a_lo; ub = a_hi; return; }
    const float b_lo = score_down(b - e, b - e), b_hi = score_up(b + e, b + e);
    const bool br_a = a_hi >= b_lo, br_b = a_lo <= b_hi;
    const float x0 = fabsf(b_lo), x1 = fabsf(b_hi);
    const float M = fmaxf(x0, x1);
    const float m = (b_lo <= 0.f && b_hi >= 0.f) ? 0.f : fminf(x0, x1);
    const float nM2 = -(M * M), nm2 = -(m * m);
    const float nb_lo = score_down(nM2, nM2), nb_hi = score_up(nm2, nm2);
    lb = br_a ? (br_b ? fminf(a_lo, nb_lo) : a_lo) : nb_lo;
    ub = br_a ? (br_b ? fmaxf(a_hi, nb_hi) : a_hi) : nb_hi;
}

// max over the 16 lanes of a DPP row (the lanes that share lane >> 4), in every lane of the row
__device__ __forceinline__ float rec_row_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)));   // row_ror:8
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false)));   // row_ror:4
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false)));   // row_ror:2
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false)));   // row_ror:1
    return v;
}

// -------------------------------------------------------------------------- pass ----
// Workgroup s takes slice s of the gallery tiles [0, ceil(N / 256)).  ROWS = 64 / 128: the example rows fit in that many rows
// of the tile; in both forms waves 0..3 hold every example row of their 64 columns (gemm256_mainloop: the second wave-row
// computes nothing), waves 4..7 only move data.  SAMPLE: write lb of every row instead of appending candidates.
// (The tile loop is tile_walk.h's slice frame, typed out: see there.)
template <int ROWS, bool SAMPLE>
__global__ __launch_bounds__(G256_THREADS, 2) void recommend_pass_kernel(RecommendPassArgs p) {
    static_assert(ROWS == 64 || ROWS == 128, "one wave holds every example row of a column");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* par = (float*)(smem + G256_LDS);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nsl = (int)gridDim.x, sl = (int)blockIdx.x;
    int t0, t1;
    if (!tile_slice((int)((p.N + 255) / 256), nsl, sl, t0, t1)) return;
    const int E = p.P + p.Nn;
    if (wave == 0) {
        // e: the largest error bound over the examples
        float e = 0.f;
        for (int q = lane; q < E; q += 64)
            e = fmaxf(e, cert_eps(p.qstat[q * 2], p.qstat[q * 2 + 1], __uint_as_float(p.gstat[0]), __uint_as_float(p.gstat[1]), p.D));
        e = wave_max(e);
        if (lane == 0) { par[0] = e; par[1] = SAMPLE ? 0.f : p.tau[0]; }
    }
    __syncthreads();

    G256Operand A, B;
    g256_operand_init(A, p.Qb, p.ldq, E, 0, wave, lane);
    g256_operand_init(B, p.Gb + (long)t0 * 256 * p.ldg, p.ldg, p.N - (long)t0 * 256, 0, wave, lane);
    g256_issue_prologue_deep<2>(A, B, smem, p.D, wave);
    unsigned long long n_allowed = 0ull;                    // wave-uniform: allowed rows this wave has met
    for (int t = t0; t < t1; ++t) {
        const long n0 = (long)t * 256;
        f32x4 acc[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm256_mainloop<ROWS, false, true, 0, 2>(A, B, smem, p.D, wave, lane, acc);
        if (t + 1 < t1) {
            // next gallery tile: DMA in flight during the epilogue (e and tau sit past the main loop's LDS image)
            g256_operand_init(B, p.Gb + (n0 + 256) * p.ldg, p.ldg, p.N - (n0 + 256), 0, wave, lane);
            g256_issue_prologue_deep<2>(A, B, smem, p.D, wave);
        }
        if (wave >= 4) continue;                            // no example rows in the second wave-row
        asm volatile("" : "+v"(lane) :: "memory");
        const int lr = lane & 15, lq = lane >> 4;
        const int cw = wave * 64;                           // the wave's 64 columns: bits of one 64-bit word of the bitmap
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        // this lane's column after the reduction: fragment n = lr >> 2, element j = lr & 3 of its 16-lane row
        const int cbit = (lr >> 2) * 16 + lq * 4 + (lr & 3);
        const bool allowed = (fm >> cbit) & 1ull;
        if (SAMPLE) {
            if (p.N - n0 - cw <= 0) continue;               // wave-uniform: past the gallery's end
        } else {
            if (fm == 0ull) continue;                       // wave-uniform: no allowed column
            n_allowed += (unsigned long long)__popcll(fm);
        }
        // a / b: the maxima over the positive / negative example rows of the 16 columns this lane holds a share of.  A
        // block of 16 rows that lies inside one class is folded without a select (wave-uniform tests on P and Nn).
        float av[4][4], bv[4][4];
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) { av[n][j] = -INFINITY; bv[n][j] = -INFINITY; }
#pragma unroll
        for (int m = 0; m < ROWS / 16; ++m) {
            const int r0 = m * 16;
            if (r0 >= E) continue;
            if (r0 + 16 <= p.P) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[n][j] = fmaxf(av[n][j], acc[m][n][j]);
            } else if (r0 >= p.P && r0 + 16 <= E) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[n][j] = fmaxf(bv[n][j], acc[m][n][j]);
            } else {
                const int row = r0 + lr;
                const bool pos = row < p.P, neg = !pos && row < E;
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        av[n][j] = fmaxf(av[n][j], pos ? acc[m][n][j] : -INFINITY);
                        bv[n][j] = fmaxf(bv[n][j], neg ? acc[m][n][j] : -INFINITY);
                    }
            }
        }
        // across the 16 lanes of the row; lane lr keeps column (n, j) = (lr >> 2, lr & 3): one column per lane
        float a = -INFINITY, b = -INFINITY;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ra = rec_row_max(av[n][j]);
                a = lr == n * 4 + j ? ra : a;
            }
        if (p.Nn > 0) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float rb = rec_row_max(bv[n][j]);
                    b = lr == n * 4 + j ? rb : b;
                }
        }
        float lb, ub;
        rec_bounds(a, b, par[0], p.Nn > 0, lb, ub);
        const long grow = n0 + cw + cbit;
        if (SAMPLE) {
            // (a NaN bound -- non-finite rows -- counts as -inf: it never raises the level)
            if (grow < p.N) p.lb_out[grow] = (allowed && lb == lb) ? lb : -INFINITY;
        } else {
            const bool take = allowed && !(ub < par[1]);    // (a NaN bound keeps the row)
            const unsigned long long mk = __ballot(take);
            if (mk == 0ull) continue;                       // wave-uniform
            const unsigned long long pos = wave_append(mk, p.cnt, lane, lanes_below(lane));
            if (take && pos < (unsigned long long)p.cap) p.rows[pos] = (uint32_t)grow;
        }
    }
    if (!SAMPLE && wave < 4 && lane == 0 && n_allowed != 0ull) atomicAdd(p.cnt + 2, n_allowed);
}

// ------------------------------------------------------------------------- level ----
// tau[0] = the k-th largest of v[0 .. n) (-inf when n < k), raised to thr when has_thr.  One workgroup; radix selection over
// the order-preserving keys, 8 bits per round.
__global__ __launch_bounds__(1024) void recommend_level_kernel(const float* __restrict__ v, int n, int k, int has_thr, float thr,
                                                               float* __restrict__ tau) {
    __shared__ uint32_t h[256];
    __shared__ uint32_t sel[2];                             // chosen digit, rank left inside it
    const int t = threadIdx.x;
    float out = -INFINITY;
    if (n >= k) {
        uint32_t prefix = 0u, want = (uint32_t)k;           // the want-th largest among the keys whose high bits equal prefix
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (t < 256) h[t] = 0u;
            __syncthreads();
            const uint32_t hi_mask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (int i = t; i < n; i += 1024) {
                const uint32_t key = f32_orderable(v[i]);
                if ((key & hi_mask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (t == 0) {
                uint32_t left = want;
                int d = 255;
                for (; d > 0; --d) { if (h[d] >= left) break; left -= h[d]; }
                sel[0] = (uint32_t)d; sel[1] = left;
            }
            __syncthreads();
            prefix |= sel[0] << shift; want = sel[1];
            __syncthreads();
        }
        out = orderable_f32(prefix);
    }
    if (t == 0) tau[0] = (has_thr && !(out >= thr)) ? thr : out;
}

// ----------------------------------------------------------------------- rescore ----
// Wave w re-scores candidate rows w, w + waves, ...: four examples at a time against the row (pairs_dot4: every score keeps
// its own chain, so it has the bits every other search gives it), sp / sn, score(r); kept rows are appended with one atomic
// per wave.  The key orders -0 with +0 (equal scores: the row index decides).
__global__ __launch_bounds__(256) void recommend_rescore_kernel(const uint32_t* __restrict__ cand, long n, const float* __restrict__ Qf,
                                                                long ldq, int P, int Nn, const float* __restrict__ Gf, long ldg, int D,
                                                                int has_thr, float thr, int b, unsigned long long* __restrict__ kept,
                                                                uint64_t* __restrict__ out_keys, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const int E = P + Nn;
    for (long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += waves) {
        const uint32_t row = cand[c];
        const float* g = Gf + (long)row * ldg;
        const float* gr[4] = {g, g, g, g};
        float sp = -INFINITY, sn = -INFINITY;
        for (int e0 = 0; e0 < E; e0 += 4) {
            const float* qr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) qr[u] = Qf + (long)(e0 + u < E ? e0 + u : E - 1) * ldq;
            float t[4];
            pairs_dot4(qr, gr, D, lane, t);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u;
                if (e < P) sp = fmaxf(sp, t[u]);
                else if (e < E) sn = fmaxf(sn, t[u]);
            }
        }
        float v = sp;
        if (Nn > 0 && !(sp > sn)) v = -__fmul_rn(sn, sn);
        if (has_thr && !(v >= thr)) continue;               // wave-uniform
        if (lane == 0) {
            const unsigned long long pos = atomicAdd(kept, 1ull);
            const float vk = v == 0.f ? 0.f : v;
            out_keys[pos] = ((uint64_t)(~f32_orderable(vk)) << b) | (uint64_t)row;
            out_scores[pos] = v;
        }
    }
}

// -------------------------------------------------------------------------- emit ----
// the first min(n, k) sorted entries -> scores / row + idx_offset, the rest padded (-inf / -1); counts[0] = min(n, k)
__global__ __launch_bounds__(256) void recommend_emit_kernel(const uint64_t* __restrict__ keys, const float* __restrict__ vals, long n,
                                                             int k, int b, long idx_offset, float* __restrict__ scores,
                                                             long long* __restrict__ idx, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) counts[0] = (int)(n < k ? n : k);
    if (i >= k) return;
    if (i < n) {
        scores[i] = vals[i];
        idx[i] = (long long)(keys[i] & ((1ull << b) - 1ull)) + idx_offset;
    } else {
        scores[i] = -INFINITY;
        idx[i] = -1;
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_recommend_pass(const RecommendPassArgs& a, int sample, hipStream_t st) {
    if (int rc = g256_check_operands("search_recommend", a.D, a.ldg, a.ldq)) return rc;
    REVO_REQUIRE(a.N < (1ll << 32), "search_recommend: row indices must fit in 32 bits");
    REVO_REQUIRE(a.P >= 1 && a.Nn >= 0 && a.P + a.Nn <= RECOMMEND_MAX_EXAMPLES, "search_recommend: bad example counts");
    if (a.N <= 0) return 0;
    const long tiles = (a.N + 255) / 256;
    const dim3 grid((unsigned)pass256_slices(tiles)), block(G256_THREADS);
#define REC_LAUNCH(RW, SM)                                                                      \
    do {                                                                                        \
        REVO_FUNC_LDS((recommend_pass_kernel<RW, SM>), REC_LDS);                                \
        hipLaunchKernelGGL((recommend_pass_kernel<RW, SM>), grid, block, REC_LDS, st, a);       \
    } while (0)
    if (a.P + a.Nn <= 64) { if (sample) REC_LAUNCH(64, true); else REC_LAUNCH(64, false); }
    else { if (sample) REC_LAUNCH(128, true); else REC_LAUNCH(128, false); }
#undef REC_LAUNCH
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_recommend_level(const float* lb, int n, int k, int has_thr, float thr, float* tau, hipStream_t st) {
    hipLaunchKernelGGL(recommend_level_kernel, dim3(1), dim3(1024), 0, st, lb, n, k, has_thr, thr, tau);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_recommend_rescore(const uint32_t* cand, long n, const float* Qf, long ldq, int P, int Nn, const float* Gf, long ldg,
                             int D, int has_thr, float thr, int b, unsigned long long* kept, uint64_t* out_keys, float* out_scores,
                             hipStream_t st) {
    if (n <= 0) return 0;
    REVO_REQUIRE(b >= 1 && b <= 32, "search_recommend: bad key width");
    const long blocks = (n + 3) / 4;
    hipLaunchKernelGGL(recommend_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Qf, ldq,
                       P, Nn, Gf, ldg, D, has_thr, thr, b, kept, out_keys, out_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_recommend_emit(const uint64_t* keys, const float* vals, long n, int k, int b, long idx_offset, float* scores,
                          long long* idx, int* counts, hipStream_t st) {
    hipLaunchKernelGGL(recommend_emit_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, keys, vals, n, k, b, idx_offset,
                       scores, idx, counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
