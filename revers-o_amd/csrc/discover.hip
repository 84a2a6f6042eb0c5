// Discovery and context search (revo_search_discover, include/revo.h DISCOVER): n context pairs
// (positive_i, negative_i) and an optional target.  With sp_i / sn_i / st the fp32 scores of row r against positive i /
// negative i / the target:
//   discovery  score(r) = (float)R + sig,  R = sum of (sp_i > sn_i ? +1 : -1),  sig = 0.5 * (fs(st) + 1),  fs(x) = x / (1 + |x|)
//   context    score(r) = loss_0 + loss_1 + ...,  loss_i = fs(min((sp_i - sn_i) - FLT_EPSILON, 0))
// every operation one fp32 operation rounded to nearest; the best k allowed rows by (score desc, row asc).  The plan is the
// recommend search's (recommend.hip: sample, level, pass, rescore, sort, emit; its level and emit kernels serve here as they
// are).  New here: the layout of the example tile, the epilogue of the pass, the bounds and the re-score formula.
//
// Example tile (ROWS = 64 / 128 rows, HALF = ROWS / 2): positive i in row i, negative i in row HALF + i, the target in row
// HALF - 1 (discovery has at most HALF - 1 pairs, so no pair uses it); every other row is zero.  In the main loop's
// accumulators a lane holds rows 16 m + (lane & 15), so a pair's two scores sit in acc[m] and acc[m + ROWS / 32] of ONE lane.
//
// Bounds.  e is the largest cert_eps over the example rows: every bf16 scan score is within e of the fp32 score.  With a, b
// the scan scores of a pair and d = a - b, the fp32 difference sp - sn lies within 2 e of d.
//   discovery  a pair is surely +1 when (d - 2 e) moved down is > 0, surely -1 when (d + 2 e) moved up is < 0 (sp > sn is an
//              exact comparison of two fp32 numbers, so only the three roundings that made the end count: at most
//              3.6e-7 for |d| < 4, below score_down's 4e-7), else open.  R_ub counts open pairs +1, R_lb -1.  The computed
//              sig is not monotone in st to the last bit; it is within 7.5e-8 of the real function g (denominator
//              rounding 6e-8 on the quotient, the division 3e-8, the addition 6e-8, halved), g' <= 0.5, and the end t +- e
//              is rounded once (6e-8 on g): the computed sig of the end is within 2.1e-7 of every computed sig inside,
//              which score_down / score_up (at least 4e-7) cover.  fl(R + sig) is monotone in both, so the sum of the ends
//              bounds the score; it is moved outward once more (score_up with the sum as reference: 2.6e-5 at |R| = 63,
//              where an ulp is 3.8e-6).
//   context    the computed loss is within 3.5e-7 of f(delta) = fs(min(delta - eps, 0)) of the real difference delta (two
//              subtractions 2.4e-7, the denominator 8e-8, the division 3e-8; f' <= 1).  The ends of x = d -+ 2 e - eps are
//              made by three roundings (3.6e-7) and moved outward by CTX_X (2e-6 (1 + |d|)); the epilogue takes fs of an
//              end as x * rcp(1 + |x|) (v_rcp_f32: 1 ulp; 2.1e-7 in all) and moves it outward by CTX_F (1e-6).  An end
//              x >= 0 gives exactly 0: the lower end then proves the computed x >= 0 and the loss +0.  The pair sums are
//              formed in another order than the contract's: every partial sum has the total's sign, so either sequence is
//              within n * 2^-24 * |sum| of the real sum; both ends are moved by CTX_SUM * n * |lower sum| (1.5e-7 > 2 * 2^-24).
//              A row with every pair surely positive has lb = ub = +0, the score itself.
// tau = the k-th largest lb over the sample (raised to the threshold): k rows score at least tau, so a row of the answer has
// ub >= tau.  No certificate can fail and there is no fallback; loose bounds cost candidates, never exactness.
#include <cfloat>

#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

constexpr int DISC_LDS = G256_LDS + 256;          // main loop | e, tau
constexpr float CTX_X = 2e-6f, CTX_F = 1e-6f, CTX_SUM = 1.5e-7f;

// the contract's operations, each rounded to nearest (the _rn intrinsics are plain operators to the compiler, hence the
// pragma).  The one fusion the code generator still makes, R + 0.5 * y as v_fmac, has the contract's bits: y = fs + 1 lies in
// [0.5, 1.5], so 0.5 * y is exact and the fma rounds the same real number once.  The division is the correctly rounded
// sequence (v_div_scale / v_div_fmas / v_div_fixup).
__device__ __forceinline__ float disc_fs(float x) {
#pragma clang fp contract(off)
    return __fdiv_rn(x, __fadd_rn(1.f, fabsf(x)));
}
__device__ __forceinline__ float disc_sig(float x) {
#pragma clang fp contract(off)
    return __fmul_rn(0.5f, __fadd_rn(disc_fs(x), 1.f));
}
__device__ __forceinline__ float disc_score(int R, float st) {
#pragma clang fp contract(off)
    return __fadd_rn((float)R, disc_sig(st));
}
__device__ __forceinline__ float disc_loss(float sp, float sn) {
#pragma clang fp contract(off)
    const float x = __fsub_rn(__fsub_rn(sp, sn), FLT_EPSILON);
    return disc_fs(x < 0.f ? x : (x != x ? x : 0.f));      // min(x, 0) that keeps a NaN, as numpy's minimum does
}
// fs of an end of the loss argument (x < 0), 1 ulp reciprocal: bounds only
__device__ __forceinline__ float disc_fs_approx(float x) { return x * __builtin_amdgcn_rcpf(1.f - x); }

// sum over the 16 lanes of a DPP row (the lanes that share lane >> 4), in every lane of the row
__device__ __forceinline__ int disc_row_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);   // row_ror:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);   // row_ror:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false);   // row_ror:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false);   // row_ror:1
    return v;
}
// lane 15 of a DPP row, in every lane of the row
__device__ __forceinline__ float disc_row_last(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x15f, 0xf, 0xf, false));   // row_newbcast:15
}
__device__ __forceinline__ float disc_row_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
    return v;
}

// is row q of the example tile an example?
__device__ __forceinline__ bool disc_row_used(int q, int half, int n_pairs, int has_target) {
    return q < n_pairs || (q >= half && q - half < n_pairs) || (has_target && q == half - 1);
}

// -------------------------------------------------------------------------- pass ----
// recommend_pass_kernel's tile loop: workgroup s takes slice s of the gallery tiles; waves 0..3 hold every example row of their
// 64 columns, waves 4..7 only move data.  SAMPLE: write lb of every row instead of appending candidates.  TARGET: discovery
// (integer counts and the target's score cross the lanes), else context (two float sums do).
template <int ROWS, bool SAMPLE, bool TARGET>
__global__ __launch_bounds__(G256_THREADS, 2) void discover_pass_kernel(DiscoverPassArgs p) {
    static_assert(ROWS == 64 || ROWS == 128, "one wave holds every example row of a column");
    constexpr int HB = ROWS / 32;                           // 16-row blocks per half of the tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* par = (float*)(smem + G256_LDS);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nsl = (int)gridDim.x, sl = (int)blockIdx.x;
    int t0, t1;
    if (!tile_slice((int)((p.N + 255) / 256), nsl, sl, t0, t1)) return;
    const int np = p.n_pairs;
    if (wave == 0) {
        // e: the largest error bound over the examples
        float e = 0.f;
        for (int q = lane; q < ROWS; q += 64)
            if (disc_row_used(q, ROWS / 2, np, TARGET))
                e = fmaxf(e, cert_eps(p.qstat[q * 2], p.qstat[q * 2 + 1], __uint_as_float(p.gstat[0]), __uint_as_float(p.gstat[1]), p.D));
        e = wave_max(e);
        if (lane == 0) { par[0] = e; par[1] = SAMPLE ? 0.f : p.tau[0]; }
    }
    __syncthreads();

    G256Operand A, B;
    g256_operand_init(A, p.Qb, p.ldq, ROWS, 0, wave, lane);
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
        const float e = par[0], e2 = 2.f * e;
        float lb, ub;
        if (TARGET) {
            // per column: pairs surely +1 (low half word) and surely -1 (high half word) among this lane's rows
            int cn[4][4];
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) cn[n][j] = 0;
#pragma unroll
            for (int m = 0; m < HB; ++m) {
                if (m * 16 >= np) continue;                 // wave-uniform
                const bool valid = m * 16 + lr < np;
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = acc[m][n][j] - acc[m + HB][n][j];
                        const int c = (score_down(d - e2, d) > 0.f ? 1 : 0) | (score_up(d + e2, d) < 0.f ? 0x10000 : 0);
                        cn[n][j] += valid ? c : 0;
                    }
            }
            // across the 16 lanes of the row; lane lr keeps column (n, j) = (lr >> 2, lr & 3): one column per lane.  The
            // target's scores sit in lane 15 of the row (row HALF - 1 = 16 (HB - 1) + 15): one row broadcast per column.
            int c = 0;
            float ts = 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rc = disc_row_sum(cn[n][j]);
                    const float rt = disc_row_last(acc[HB - 1][n][j]);
                    c = lr == n * 4 + j ? rc : c;
                    ts = lr == n * 4 + j ? rt : ts;
                }
            const float r_lb = (float)(2 * (c & 0xffff) - np), r_ub = (float)(np - 2 * (c >> 16));
            const float s_lo = disc_sig(ts - e), s_hi = disc_sig(ts + e);
            const float lo = __fadd_rn(r_lb, score_down(s_lo, s_lo)), hi = __fadd_rn(r_ub, score_up(s_hi, s_hi));
            lb = score_down(lo, lo);
            ub = score_up(hi, hi);
        } else {
            float lo[4][4], hi[4][4];
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) { lo[n][j] = 0.f; hi[n][j] = 0.f; }
#pragma unroll
            for (int m = 0; m < HB; ++m) {
                if (m * 16 >= np) continue;                 // wave-uniform
                const bool valid = m * 16 + lr < np;
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = acc[m][n][j] - acc[m + HB][n][j];
                        const float w = CTX_X * (1.f + fabsf(d));
                        const float xl = ((d - e2) - FLT_EPSILON) - w, xh = ((d + e2) - FLT_EPSILON) + w;
                        // (a NaN difference: both ends NaN, and so the row's bounds -- the row is kept, see below)
                        const float fl = xl >= 0.f ? 0.f : disc_fs_approx(xl) - CTX_F;
                        const float fh = xh >= 0.f ? 0.f : fminf(disc_fs_approx(xh) + CTX_F, 0.f);
                        lo[n][j] += valid ? fl : 0.f;
                        hi[n][j] += valid ? fh : 0.f;
                    }
            }
            float sl_ = 0.f, sh_ = 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float rl = disc_row_sum(lo[n][j]);
                    const float rh = disc_row_sum(hi[n][j]);
                    sl_ = lr == n * 4 + j ? rl : sl_;
                    sh_ = lr == n * 4 + j ? rh : sh_;
                }
            const float w = CTX_SUM * (float)np * fabsf(sl_);
            lb = sl_ - w;
            ub = fminf(sh_ + w, 0.f);
            ub = sh_ != sh_ ? sh_ : ub;                     // (fminf drops a NaN: keep it, the row is kept)
        }
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

// ----------------------------------------------------------------------- rescore ----
// Wave w re-scores candidate rows w, w + waves, ...: two pairs at a time against the row (pairs_dot4: every score keeps its
// own chain, so it has the bits every other search gives it), R or the loss sum in pair order, the target's score (in the
// spare slots of an odd pair count's last call, else a call of its own), score(r);
// kept rows are appended with one atomic per wave.  The key orders -0 with +0 (equal scores: the row index decides).
__global__ __launch_bounds__(256) void discover_rescore_kernel(const uint32_t* __restrict__ cand, long n, const float* __restrict__ Qf,
                                                               long ldq, int half, int n_pairs, int has_target,
                                                               const float* __restrict__ Gf, long ldg, int D, int has_thr, float thr,
                                                               int b, unsigned long long* __restrict__ kept,
                                                               uint64_t* __restrict__ out_keys, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += waves) {
        const uint32_t row = cand[c];
        const float* g = Gf + (long)row * ldg;
        const float* gr[4] = {g, g, g, g};
        int R = 0;
        float sum = 0.f, st = 0.f;
        const float* qt = Qf + (long)(half - 1) * ldq;      // the target's row (discovery)
        for (int i0 = 0; i0 < n_pairs; i0 += 2) {
            const bool two = i0 + 1 < n_pairs;              // (an odd count's last call: the target, or the pair again, in the spare slots)
            const float* q2 = two ? Qf + (long)(i0 + 1) * ldq : (has_target ? qt : Qf + (long)i0 * ldq);
            const float* q3 = two ? Qf + (long)(half + i0 + 1) * ldq : (has_target ? qt : Qf + (long)(half + i0) * ldq);
            const float* qr[4] = {Qf + (long)i0 * ldq, Qf + (long)(half + i0) * ldq, q2, q3};
            float t[4];
            pairs_dot4(qr, gr, D, lane, t);
            if (has_target) {
                R += t[0] > t[1] ? 1 : -1;
                if (two) R += t[2] > t[3] ? 1 : -1;
                else st = t[2];
            } else {
                const float l0 = disc_loss(t[0], t[1]);
                sum = i0 == 0 ? l0 : __fadd_rn(sum, l0);
                if (i0 + 1 < n_pairs) sum = __fadd_rn(sum, disc_loss(t[2], t[3]));
            }
        }
        float v = sum;
        if (has_target) {
            if ((n_pairs & 1) == 0) {                       // wave-uniform: no spare slot carried the target
                const float* qr[4] = {qt, qt, qt, qt};
                float t[4];
                pairs_dot4(qr, gr, D, lane, t);
                st = t[0];
            }
            v = disc_score(R, st);
        }
        if (has_thr && !(v >= thr)) continue;               // wave-uniform
        if (lane == 0) {
            const unsigned long long pos = atomicAdd(kept, 1ull);
            const float vk = v == 0.f ? 0.f : v;
            out_keys[pos] = ((uint64_t)(~f32_orderable(vk)) << b) | (uint64_t)row;
            out_scores[pos] = v;
        }
    }
}

// ------------------------------------------------------------------------ launchers ----
int discover_tile_rows(int n_pairs, int has_target) { return n_pairs + (has_target ? 1 : 0) <= 32 ? 64 : 128; }
int launch_discover_pass(const DiscoverPassArgs& a, int sample, hipStream_t st) {
    if (int rc = g256_check_operands("search_discover", a.D, a.ldg, a.ldq)) return rc;
    REVO_REQUIRE(a.N < (1ll << 32), "search_discover: row indices must fit in 32 bits");
    REVO_REQUIRE(a.n_pairs >= (a.has_target ? 0 : 1) && a.n_pairs + (a.has_target ? 1 : 0) <= DISCOVER_MAX_PAIRS,
                 "search_discover: bad pair count");
    if (a.N <= 0) return 0;
    const long tiles = (a.N + 255) / 256;
    const dim3 grid((unsigned)pass256_slices(tiles)), block(G256_THREADS);
#define DISC_LAUNCH(RW, SM, TG)                                                                     \
    do {                                                                                            \
        REVO_FUNC_LDS((discover_pass_kernel<RW, SM, TG>), DISC_LDS);                                \
        hipLaunchKernelGGL((discover_pass_kernel<RW, SM, TG>), grid, block, DISC_LDS, st, a);       \
    } while (0)
#define DISC_FORM(RW)                                                                               \
    do {                                                                                            \
        if (a.has_target) { if (sample) DISC_LAUNCH(RW, true, true); else DISC_LAUNCH(RW, false, true); }        \
        else { if (sample) DISC_LAUNCH(RW, true, false); else DISC_LAUNCH(RW, false, false); }      \
    } while (0)
    if (discover_tile_rows(a.n_pairs, a.has_target) == 64) DISC_FORM(64); else DISC_FORM(128);
#undef DISC_FORM
#undef DISC_LAUNCH
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_discover_rescore(const uint32_t* cand, long n, const float* Qf, long ldq, int half, int n_pairs, int has_target,
                            const float* Gf, long ldg, int D, int has_thr, float thr, int b, unsigned long long* kept,
                            uint64_t* out_keys, float* out_scores, hipStream_t st) {
    if (n <= 0) return 0;
    REVO_REQUIRE(b >= 1 && b <= 32, "search_discover: bad key width");
    const long blocks = (n + 3) / 4;
    hipLaunchKernelGGL(discover_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Qf, ldq,
                       half, n_pairs, has_target, Gf, ldg, D, has_thr, thr, b, kept, out_keys, out_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
