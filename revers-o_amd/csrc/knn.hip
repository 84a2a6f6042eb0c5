// Exact kNN graph of one gallery (revo_gallery_knn, include/revo.h KNN): for every allowed row i its
// best k allowed rows j != i by (PAIRS score desc, index asc), cut at a threshold if one is given.  The pairs join (pairs.hip)
// with a level PER ROW instead of one threshold:
//
//   sample   rows 0, stride, 2 stride, ... (at most 8 192) are copied to a contiguous bf16 tile set; the allowed rows of the
//            gallery and of the sample are counted
//   level    one MFMA pass of all rows against the sample; the epilogue keeps, per row, the sum and the sum of squares of its
//            bf16 scores against the allowed sample rows other than itself.  t_i = mu_i + z sigma_i with z the normal
//            quantile that leaves about 2 k + 16 of the allowed rows above it -- an ESTIMATE of a level that a few times k
//            rows reach, raised to the threshold if one is given.  No more allowed rows than the sample holds: t_i = the
//            floor (the threshold, or -inf), every pair is a candidate.  A second pass counts the sample rows that reach
//            the row's bound: a row with far too many (a block of near-identical rows) gets t_i = +inf and goes to the
//            fallback without flooding the workspace; it also leaves the sample, and a third pass estimates the other
//            rows' levels again without the block's weight in their sigma.
//   join     the pairs join's walk over the upper triangle of 256 x 256 tiles (tile_walk.h).  Pair (i, j) is a candidate when its bf16
//            score reaches min(lb_i, lb_j), lb_r = fl(t_r - eps) lowered by its rounding, eps the row-against-row cert_eps of
//            pairs_lb.  A key that finds no room in the workspace is dropped and BOTH its rows are marked lost.
//   rescore  the fp32 PAIRS score v of every candidate (rescore_group4, the pairs row functor): a directed entry for row i
//            when v >= t_i and one for row j when v >= t_j
//   sort     radix_sort.hip by (row, score desc)
//   select   one wave per row: the best k of its segment, ties by index ascending
//   fallback rows without a certificate: exhaustive fp32 scoring of the allowed rows in PAIRS bits and an exact selection
//            (topk_large.hip's fallback kernels; the row itself is left out by index)
//
// THE CERTIFICATE.  Row i is complete when no key of it was lost and either (a) its segment holds >= k entries, or (b) t_i is
// the floor.  Why that is exact: |bf16 score - fp32 score| <= eps for every pair, so every j with v(i, j) >= t_i has a bf16
// score >= t_i - eps >= lb_i >= min(lb_i, lb_j) and was a candidate of the join; not lost, it was re-scored and became an entry
// of row i.  So row i's segment is EXACTLY {j allowed, j != i : v(i, j) >= t_i}.  (a) With k or more entries, every row outside
// the segment scores below t_i, hence below all of them: the best k of the segment by (score desc, index asc) are the best k
// of all rows, ties included.  (b) With t_i the floor the segment is everything the contract admits.  Nothing here depends on
// how t_i was chosen: a level that is too high sends the row to the fallback, one that is too low costs candidates.  The
// level estimate, the workspace size and the order of the device's appends therefore change speed only, never a byte.
//
// A gallery of mostly identical rows (every one of n duplicates has n - 1 partners at one score) overflows the workspace and
// is answered by the fallback, one pass over the fp32 rows per row: slow, but correct.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

// ------------------------------------------------------------------------ sample ----
// workgroup s < ST * 256: sample row s (zeros past S); the workgroups behind them count the allowed rows of the gallery
__global__ __launch_bounds__(256) void knn_sample_kernel(const bf16_t* __restrict__ Gb, long ldg, long N, int D, long S, long stride,
                                                         long sample_rows, const uint32_t* __restrict__ allow,
                                                         bf16_t* __restrict__ Sb, uint32_t* __restrict__ sallow,
                                                         unsigned long long* __restrict__ ctr) {
    const long s = blockIdx.x;
    if (s < sample_rows) {
        const long r = s * stride;
        const bool live = s < S && r < N;
        const uint4* src = (const uint4*)(Gb + (live ? r : 0) * ldg);
        uint4* dst = (uint4*)(Sb + s * (long)D);
        for (int c = threadIdx.x; c < D / 8; c += 256) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (live) v = src[c];
            dst[c] = v;
        }
        if (threadIdx.x == 0 && live && (!allow || ((allow[r >> 5] >> (r & 31)) & 1u))) {
            atomicOr(&sallow[s >> 5], 1u << (s & 31));
            atomicAdd(&ctr[3], 1ull);
        }
        return;
    }
    // the allowed rows, 32 per lane and trip
    const long words = (N + 31) >> 5;
    const long w0 = (s - sample_rows) * 256 + threadIdx.x, step = (long)(gridDim.x - sample_rows) * 256;
    unsigned long long n = 0;
    for (long w = w0; w < words; w += step) {
        const long left = N - (w << 5);
        uint32_t m = left >= 32 ? ~0u : (1u << left) - 1u;
        if (allow) m &= allow[w];
        n += (unsigned long long)__popc(m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned long long)__shfl_xor((int)n, o, 64);   // (< 2^31 rows: one word)
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctr[2], n);
}

// ------------------------------------------------------------------------- level ----
// Workgroup ti: row tile ti against every sample tile (tile_walk.h's slice frame, B the sample).  Per tile a lane folds its
// 8 x 16 scores into sum / sum of squares per row, the four lanes of a row meet, and the wave adds its share to the slot
// (wave column, row) of the zeroed sum / sq arrays (no atomics, no registers held across the main loop: launch_knn_levels
// adds the four wave columns in a fixed order).  With p.lb (the second pass) it counts instead, into `sum`: the allowed sample
// rows other than the row itself whose bf16 score reaches the row's bound.
__global__ __launch_bounds__(G256_THREADS, 2) void knn_level_kernel(KnnLevelArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const long ti = blockIdx.x;
    const int ST = (int)((p.S + 255) / 256);
    const bool counting = p.lb != nullptr;
    G256Operand A;
    g256_operand_init(A, p.Gb + ti * 256 * p.ldg, p.ldg, p.N - ti * 256, 0, wave, lane);
    tile_slice_frame<0, false, 0>(A, p.Sb, p.D, p.S, 0, ST, smem, p.D, wave, lane, [&](long n0, int lane, const f32x4 (&acc)[8][4]) {
        const TileLane tl = tile_lane(wave, lane);
        const int lq = tl.lq, rbase = tl.rbase, cw = tl.cw;
        const uint64_t fm = tile_column_mask(p.S, n0, cw, p.sallow);
        if (fm == 0ull) return;                             // wave-uniform: no allowed sample row
        const uint64_t bits = fm >> (lq * 4);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const long gi = ti * 256 + rbase + m * 16;
            // the sample column that is row gi itself (-1: none)
            const long q = gi / p.stride;
            const long selfc = q * p.stride == gi ? q - n0 - cw - lq * 4 : -1;
            const float lbr = counting ? p.lb[gi] : 0.f;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = ((bits >> (n * 16 + j)) & 1ull) && selfc != (long)(n * 16 + j);
                    if (counting) {                         // wave-uniform
                        a += ok && acc[m][n][j] >= lbr ? 1.f : 0.f;
                    } else {
                        const float v = ok ? acc[m][n][j] : 0.f;
                        a += v;
                        b = fmaf(v, v, b);
                    }
                }
            // the four lanes of the row meet; the slot (wave column, row) is this wave's alone: a plain add, in tile order
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
            if (lq == 0) {
                const long slot = (long)(wave & 3) * p.rows + gi;   // gi < rows: rows is whole tiles
                p.sum[slot] += a;
                p.sq[slot] += b;
            }
        }
    });
}

// the upper normal quantile of p in (0, 0.5] (Abramowitz & Stegun 26.2.23, |error| < 4.5e-4)
__device__ __forceinline__ float knn_normal_quantile(float p) {
    const float t = sqrtf(-2.f * logf(p));
    return t - (2.515517f + t * (0.802853f + t * 0.010328f)) / (1.f + t * (1.432788f + t * (0.189269f + t * 0.001308f)));
}
// level[r], lb[r] of every row of the padded tiles
__global__ __launch_bounds__(256) void knn_levels_kernel(KnnLevelArgs p, const uint32_t* __restrict__ allow,
                                                         const uint32_t* __restrict__ gstat,
                                                         const unsigned long long* __restrict__ ctr, int k, int has_thr, float thr,
                                                         int level_mode, int have_pass, int keep_dense,
                                                         const int* __restrict__ pruned, float* __restrict__ level,
                                                         float* __restrict__ lb) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.rows) return;
    const bool ok = r < p.N && (!allow || ((allow[r >> 5] >> (r & 31)) & 1u));
    if (!ok) { level[r] = INFINITY; lb[r] = INFINITY; return; }
    if (keep_dense && level[r] == INFINITY) return;         // a dense row of the first round (knn_dense_rows_kernel) stays one
    const float floor_level = has_thr ? thr : -INFINITY;
    float t = floor_level;
    if (level_mode == 2) {
        t = fmaxf(2.0f, floor_level);
    } else if (level_mode != 1 && have_pass) {
        const float M = (float)ctr[2];                      // allowed rows
        const bool in_sample = r % p.stride == 0 && r / p.stride < p.S;
        const float n = (float)ctr[3] - (float)pruned[0] - (in_sample ? 1.f : 0.f);   // allowed sample rows other than r
        const float want = (float)(2 * k + 16);
        if (M > (float)KNN_SAMPLE && n >= 64.f && want < 0.5f * (M - 1.f)) {
            const float a = ((p.sum[r] + p.sum[p.rows + r]) + p.sum[2 * p.rows + r]) + p.sum[3 * p.rows + r];
            const float b = ((p.sq[r] + p.sq[p.rows + r]) + p.sq[2 * p.rows + r]) + p.sq[3 * p.rows + r];
            const float mu = a / n;
            const float var = fmaxf(b / n - mu * mu, 0.f);
            float e = mu + knn_normal_quantile(want / (M - 1.f)) * sqrtf(var);
            if (level_mode == 3) e += 0.05f;
            if (e == e) t = fmaxf(e, floor_level);          // (a NaN estimate: the floor)
        }
    }
    level[r] = t;
    const float G = __uint_as_float(gstat[0]), Eg = __uint_as_float(gstat[1]);
    const float eps = cert_eps(Eg, G + Eg, G, Eg, p.D);     // pairs_lb's eps
    lb[r] = t > -INFINITY ? score_down(t - eps, t) : -INFINITY;
}

// Behind the counting pass: a row whose bound so many sample rows reach that its share of the gallery would be hundreds of
// candidates -- a member of a block of near-identical rows, where no level between "too few" and "all of the block" exists --
// gets level = lb = +inf: it starts no candidate (its partners still take it by their own bounds) and, with no entry of its
// own, takes the fallback.  The limit: three times the expected count of a row with 2 (2 k + 16) candidates, and 8.  A dense
// row also leaves the sample (its bit of sallow is cleared, pruned[0] counts them): a block of equal sample rows inflates the
// sigma of every row that is two or three sigma away from it, and the levels are estimated once more without them.
__global__ __launch_bounds__(256) void knn_dense_rows_kernel(KnnLevelArgs p, const unsigned long long* __restrict__ ctr, int k,
                                                             uint32_t* __restrict__ sallow, int* __restrict__ pruned,
                                                             float* __restrict__ level, float* __restrict__ lb) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.N || !(level[r] < INFINITY)) return;
    const float M = (float)ctr[2];
    const bool in_sample = r % p.stride == 0 && r / p.stride < p.S;
    const float n = (float)ctr[3] - (in_sample ? 1.f : 0.f);
    if (!(M > (float)KNN_SAMPLE) || n < 64.f) return;      // (no estimate was made: launch_knn_levels)
    const float c = ((p.sum[r] + p.sum[p.rows + r]) + p.sum[2 * p.rows + r]) + p.sum[3 * p.rows + r];
    if (c > 8.f + 6.f * (float)(2 * k + 16) * n / M) {
        level[r] = INFINITY; lb[r] = INFINITY;
        if (in_sample) {
            const long s = r / p.stride;
            atomicAnd(&sallow[s >> 5], ~(1u << (s & 31)));
            atomicAdd(pruned, 1);
        }
    }
}

// -------------------------------------------------------------------------- join ----
// pairs_join_kernel (tile_walk.h's tile-pair frame over the triangle) with the bound min(lb_i, lb_j).  Per tile a lane reads the lb of ONE of the wave's 64 columns (the others
// come by a lane shuffle where a row gets past the wave-uniform test) and of its 8 rows; the test per 16-row block is the
// block's best score against min(lb of the lane's row, the smallest lb of the wave's columns).
__global__ __launch_bounds__(G256_THREADS, 2) void knn_join_kernel(KnnJoinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PairsJoinArgs& p = a.j;
    tile_pair_frame(p, TriangleWalk{p.T}, smem, [&](int ci, int cj, long n0, bool diag, int wave, int lane, const f32x4 (&acc)[8][4]) {
        const TileLane t = tile_lane(wave, lane);
        const int lq = t.lq, rbase = t.rbase, cw = t.cw;
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        if (fm == 0ull) return;                             // wave-uniform: no allowed column
        const float lbc = a.lb[n0 + cw + lane];             // column cw + lane (lb holds whole tiles: +inf past N)
        float cmin = lbc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
        const uint64_t bits = fm >> (lq * 4);
        const unsigned long long below = lanes_below(lane);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int row = rbase + m * 16;
            const long gi = (long)ci * 256 + row;
            const float lbr = a.lb[gi];
            float mx = -INFINITY;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = fmaxf(mx, acc[m][n][j]);
            if (__ballot(mx >= fminf(lbr, cmin)) == 0ull) continue;      // wave-uniform
            const bool rok = gi < p.N && (!p.allow || ((p.allow[gi >> 5] >> (gi & 31)) & 1u));
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int cl = n * 16 + lq * 4 + j;     // the column inside the wave's 64
                    const int col = cw + cl;
                    const float lbj = __shfl(lbc, cl, 64);
                    const bool take = rok && acc[m][n][j] >= fminf(lbr, lbj) && ((bits >> (n * 16 + j)) & 1ull) &&
                                      (!diag || col > row);
                    const unsigned long long mk = __ballot(take);
                    if (mk == 0ull) continue;               // wave-uniform
                    const unsigned long long pos = wave_append(mk, p.cnt, lane, below);
                    if (take) {
                        const long gj = n0 + col;
                        if (pos < (unsigned long long)p.cap) {
                            p.keys[pos] = ((uint64_t)gi << 32) | (uint64_t)gj;
                        } else {                            // no room: neither row's list can be certified
                            atomicOr(&a.lost[gi >> 5], 1u << (gi & 31));
                            atomicOr(&a.lost[gj >> 5], 1u << (gj & 31));
                        }
                    }
                }
        }
    });
}

// ----------------------------------------------------------------------- rescore ----
// wave g re-scores candidates 4 g .. 4 g + 3 (grid-stride); the directed entries are appended with one atomic per wave and end
__global__ __launch_bounds__(256) void knn_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Gf,
                                                          long ldg, int D, const float* __restrict__ level,
                                                          unsigned long long* __restrict__ kept, uint64_t* __restrict__ out_keys,
                                                          float* __restrict__ out_partner) {
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
        const uint32_t i = (uint32_t)(k >> 32), j = (uint32_t)k;
        const uint64_t sbits = (uint64_t)(0xffffffffu - f32_orderable(v));     // ascending keys: best score first
#pragma unroll
        for (int end = 0; end < 2; ++end) {
            const uint32_t row = end == 0 ? i : j, other = end == 0 ? j : i;
            const bool take = lane < m && v >= level[row];
            const unsigned long long mk = __ballot(take);
            if (mk == 0ull) continue;
            const unsigned long long pos = wave_append(mk, kept, lane, below);
            if (take) {
                out_keys[pos] = ((uint64_t)row << 32) | sbits;
                out_partner[pos] = __uint_as_float(other);  // (the sort moves a float with every key: the partner's bits)
            }
        }
    }
}

// ------------------------------------------------------------------------ select ----
// first entry of keys[lo, hi) that is >= x (wave-uniform)
__device__ __forceinline__ long knn_lower_bound(const uint64_t* __restrict__ keys, long lo, long hi, uint64_t x) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// one wave per row (grid-stride).  The row's segment is sorted by score, best first; inside a run of equal scores the partners
// are taken by index ascending: the smallest index above the last one taken, one wave-wide minimum each.
__global__ __launch_bounds__(256) void knn_select_kernel(const uint64_t* __restrict__ keys, const float* __restrict__ partner, long n,
                                                         long N, int k, float floor_level, const float* __restrict__ level,
                                                         const uint32_t* __restrict__ lost, const uint32_t* __restrict__ allow,
                                                         int* __restrict__ fb_q, int* __restrict__ fb_ctr,
                                                         float* __restrict__ scores, long long* __restrict__ idx,
                                                         int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < N; r += waves) {
        const bool ok = !allow || ((allow[r >> 5] >> (r & 31)) & 1u);
        int out = 0;
        if (ok) {
            const long s = knn_lower_bound(keys, 0, n, (uint64_t)r << 32);
            const long e = knn_lower_bound(keys, s, n, (uint64_t)(r + 1) << 32);
            const bool is_lost = (lost[r >> 5] >> (r & 31)) & 1u;
            const bool complete = !is_lost && (e - s >= (long)k || level[r] == floor_level);
            if (!complete) {
                if (lane == 0) fb_q[atomicAdd(&fb_ctr[1], 1)] = (int)r;
            } else {
                long at = s;
                while (out < k && at < e) {
                    const uint64_t key0 = keys[at];
                    const long ge = knn_lower_bound(keys, at + 1, e, key0 + 1ull);   // the end of the run of key0's score
                    const float v = orderable_f32(0xffffffffu - (uint32_t)key0);
                    long last = -1;
                    const long take = ge - at < (long)(k - out) ? ge - at : (long)(k - out);
                    for (long t = 0; t < take; ++t) {
                        long best = ge - at == 1 ? (long)__float_as_uint(partner[at]) : (1l << 40);
                        if (ge - at > 1) {
                            for (long c = at + lane; c < ge; c += 64) {
                                const long pj = (long)__float_as_uint(partner[c]);
                                if (pj > last && pj < best) best = pj;
                            }
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) {
                                const long other = (long)shfl_xor_u64((uint64_t)best, o);
                                best = other < best ? other : best;
                            }
                        }
                        if (lane == 0) { scores[r * k + out] = v; idx[r * k + out] = (long long)best; }
                        last = best;
                        ++out;
                    }
                    at = ge;
                }
            }
        }
        for (int c = out + lane; c < k; c += 64) { scores[r * k + c] = -INFINITY; idx[r * k + c] = -1ll; }
        if (lane == 0) counts[r] = out;
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_knn_sample(const bf16_t* Gb, long ldg, long N, int D, long S, long stride, const uint32_t* allow, bf16_t* Sb,
                      uint32_t* sallow, unsigned long long* ctr, hipStream_t st) {
    REVO_REQUIRE(D % 64 == 0 && ldg % 8 == 0, "gallery_knn: D must be a multiple of 64");
    if (N <= 0) return 0;
    const long sample_rows = (S + 255) / 256 * 256;
    REVO_HIP_CHECK(hipMemsetAsync(sallow, 0, (size_t)(sample_rows / 32) * 4, st));
    long count_blocks = ((N + 31) / 32 + 255) / 256;
    if (count_blocks > 1024) count_blocks = 1024;
    hipLaunchKernelGGL(knn_sample_kernel, dim3((unsigned)(sample_rows + count_blocks)), dim3(256), 0, st, Gb, ldg, N, D, S, stride,
                       sample_rows, allow, Sb, sallow, ctr);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_level_pass(const KnnLevelArgs& a, hipStream_t st) {
    if (int rc = g256_check_operands("gallery_knn", a.D, a.ldg)) return rc;
    REVO_REQUIRE(a.rows % 256 == 0 && a.rows >= a.N && a.stride >= 1 && a.S >= 1 && (a.S - 1) * a.stride < a.N,
                 "gallery_knn: internal: inconsistent sample");
    if (a.N <= 0) return 0;
    REVO_HIP_CHECK(hipMemsetAsync(a.sum, 0, (size_t)a.rows * 16, st));
    REVO_HIP_CHECK(hipMemsetAsync(a.sq, 0, (size_t)a.rows * 16, st));
    REVO_FUNC_LDS(knn_level_kernel, G256_LDS);
    hipLaunchKernelGGL(knn_level_kernel, dim3((unsigned)(a.rows / 256)), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_levels(const KnnLevelArgs& a, const uint32_t* allow, const uint32_t* gstat, const unsigned long long* ctr, int k,
                      int has_thr, float thr, int level_mode, int have_pass, int keep_dense, const int* pruned, float* level,
                      float* lb, hipStream_t st) {
    if (a.rows <= 0) return 0;
    hipLaunchKernelGGL(knn_levels_kernel, dim3((unsigned)(a.rows / 256)), dim3(256), 0, st, a, allow, gstat, ctr, k, has_thr, thr,
                       level_mode, have_pass, keep_dense, pruned, level, lb);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_dense_rows(const KnnLevelArgs& a, const unsigned long long* ctr, int k, uint32_t* sallow, int* pruned, float* level,
                          float* lb, hipStream_t st) {
    if (a.N <= 0) return 0;
    hipLaunchKernelGGL(knn_dense_rows_kernel, dim3((unsigned)(a.rows / 256)), dim3(256), 0, st, a, ctr, k, sallow, pruned, level, lb);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_join(const KnnJoinArgs& a_in, hipStream_t st) {
    KnnJoinArgs a = a_in;
    long wgs = 0;                                           // the pairs join's plan and grid
    { const int rc = pairs_join_plan(a.j, "gallery_knn", &wgs); if (rc) return rc; }
    if (wgs == 0) return 0;
    REVO_FUNC_LDS(knn_join_kernel, G256_LDS);
    hipLaunchKernelGGL(knn_join_kernel, dim3((unsigned)wgs), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, const float* level,
                       unsigned long long* kept, uint64_t* out_keys, float* out_partner, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(knn_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Gf, ldg, D,
                       level, kept, out_keys, out_partner);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_knn_select(const uint64_t* keys, const float* partner, long n, long N, int k, float floor_level, const float* level,
                      const uint32_t* lost, const uint32_t* allow, int* fb_q, int* fb_ctr, float* scores, long long* idx,
                      int* counts, hipStream_t st) {
    if (N <= 0) return 0;
    const long blocks = (N + 3) / 4;
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, keys, partner, n, N, k,
                       floor_level, level, lost, allow, fb_q, fb_ctr, scores, idx, counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
