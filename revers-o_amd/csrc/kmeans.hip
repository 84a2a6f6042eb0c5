// Exact spherical k-means over one gallery (revo_gallery_kmeans, include/revo.h KMEANS).  A step is an
// ASSIGNMENT of every allowed row to its best centroid under the fp32 score, and an UPDATE of the centroids from the labels.
//
//   rows     once per call, one wave per row: inv_i, the factor the query normalisation of every search gives the row (the
//            score of the contract is the fma chain over q_i = fl(g_i * inv_i) and the centroid's fp32 row: what
//            revo_search_topk returns for the master row as a query), and the row's two rounding norms against its OWN bf16
//            scan row gb_i:  e_i = ||inv_i gb_i - q_i||,  n_i = inv_i ||gb_i||
//   best     row tile ti against every centroid tile (tile_walk.h's slice frame, B the centroids' bf16 copy): each row's
//            largest bf16 score over the centroids, per wave column (no atomics, nothing held across the main loop)
//   bound    thr_i = best_i - 2 eps_i / inv_i lowered by its rounding, eps_i = cert_eps(e_i, n_i, max ||c||, max ||cb - c||, D);
//            +inf for a row that is past N or not allowed
//   decide   the same walk: every (row, centroid) whose bf16 score reaches thr_i is appended as a candidate key, one atomic
//            per wave and tile
//   rescore  the fp32 chain of every candidate, folded per row with a 64-bit atomic max on make_key(score, centroid): the
//            maximum of a set -- order-independent -- under (score desc, centroid asc)
//   finish   label / score of every row from its key, the labels that changed, the rows with more than one candidate, sizes
//
// WHY THE BAND IS EXACT.  With s(i, c) the MFMA score of gb_i against cb_c and v(i, c) the fp32 chain of q_i against c_c,
// |inv_i s(i, c) - v(i, c)| <= eps_i for every centroid (cert_eps with the row in the query's place: the products of bf16
// values are exact in fp32, inv_i scales the MFMA chain's error with the score).  Let c* maximise v(i, .) -- any of them
// when several tie -- and b the centroid of the best bf16 score.  Then inv_i s(i, c*) + eps_i >= v(i, c*) >= v(i, b) >=
// inv_i s(i, b) - eps_i, so s(i, c*) >= s(i, b) - 2 eps_i / inv_i >= thr_i: every maximiser of the fp32 score is a candidate,
// the fold over the candidates is the fold over all centroids.  The bound costs candidates, never a byte.
//
//   update   keys (label << b) | row sorted by radix_sort.hip (a row without a label sorts behind the last centroid); the
//            centroids' member and chunk offsets by two prefix sums; one workgroup per (centroid, chunk of 256 members) adds
//            its members' fp32 master rows in row order into a partial, plain fp32 adds from +0; one workgroup per centroid
//            adds its partials in chunk order; the append's normalisation kernel; a centroid without members, or whose sum
//            has a squared norm (the normalisation's own) that is zero or not finite, gets its previous rows back
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

// What the two tile kernels take of KmeansAssignArgs (kernels.h): as few scalar registers as their walk needs -- they run at 256
// VGPRs, and a scalar that finds no register takes a lane of one more.  Rows are D elements apart in both operands.
struct KmeansBestArgs { const bf16_t* Gb; const bf16_t* Cb; long N, C, rows; float* best; int D; };
struct KmeansDecideArgs {
    const bf16_t* Gb; const bf16_t* Cb; long N, C; const float* thr; unsigned long long* cnt; uint64_t* keys; long cap; int D;
};

// the squared norm the normalisation kernel (elementwise.hip l2norm_rows_kernel) computes for a row: the same element order
// per lane, the same tree -- the same bits
__device__ __forceinline__ float kmeans_row_sq(const float* __restrict__ s, int D, int lane) {
    float q = 0.f;
    for (int c = lane; c < D; c += 64) q = fmaf(s[c], s[c], q);
    return wave_sum(q);
}

// -------------------------------------------------------------------------- rows ----
__global__ __launch_bounds__(256) void kmeans_rows_kernel(const float* __restrict__ Gf, const bf16_t* __restrict__ Gb, long ldg,
                                                          long N, int D, float* __restrict__ inv_out,
                                                          float* __restrict__ rstat) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < N; r += waves) {
        const float* s = Gf + r * ldg;
        const bf16_t* sb = Gb + r * ldg;
        const float q = kmeans_row_sq(s, D, lane);
        const float inv = q > 0.f ? 1.0f / sqrtf(q) : 1.0f;
        float e2 = 0.f, n2 = 0.f;
        for (int c = lane; c < D; c += 64) {
            const float y = s[c] * inv;
            const float fb = bf16_to_f32(sb[c]);
            const float d = fmaf(inv, fb, -y), t = inv * fb;
            e2 = fmaf(d, d, e2);
            n2 = fmaf(t, t, n2);
        }
        e2 = wave_sum(e2); n2 = wave_sum(n2);
        if (lane == 0) {
            inv_out[r] = inv;
            rstat[r * 2] = sqrtf(e2);
            rstat[r * 2 + 1] = sqrtf(n2);
        }
    }
}

// -------------------------------------------------------------------------- best ----
// Workgroup ti: row tile ti against every centroid tile.  Per tile a lane folds its 8 x 16 scores into the maximum per row
// over the columns that are centroids, the four lanes of a row meet, and the wave folds it into the slot (wave column, row)
// of `best` (preset to -inf; the slot is this wave's alone: a plain read-modify-write, as knn_level_kernel's sums).
__global__ __launch_bounds__(G256_THREADS, 2) void kmeans_best_kernel(KmeansBestArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const long ti = blockIdx.x;
    const int CT = (int)((p.C + 255) / 256);
    G256Operand A;
    g256_operand_init(A, p.Gb + ti * 256 * p.D, p.D, p.N - ti * 256, 0, wave, lane);
    tile_slice_frame<0, false, 0>(A, p.Cb, p.D, p.C, 0, CT, smem, p.D, wave, lane, [&](long n0, int lane, const f32x4 (&acc)[8][4]) {
        const TileLane tl = tile_lane(wave, lane);
        const int lq = tl.lq, rbase = tl.rbase, cw = tl.cw;
        const uint64_t fm = tile_column_mask(p.C, n0, cw, nullptr);
        if (fm == 0ull) return;                             // wave-uniform: no centroid in the wave's columns
        const uint64_t bits = fm >> (lq * 4);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            float mx = -INFINITY;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = fmaxf(mx, ((bits >> (n * 16 + j)) & 1ull) ? acc[m][n][j] : -INFINITY);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (lq == 0) {
                const long slot = (long)(wave & 3) * p.rows + ti * 256 + rbase + m * 16;   // (rows is whole tiles)
                p.best[slot] = fmaxf(p.best[slot], mx);
            }
        }
    });
}

// ------------------------------------------------------------------------- bound ----
__global__ __launch_bounds__(256) void kmeans_bound_kernel(const float* __restrict__ best, long rows, long N,
                                                           const uint32_t* __restrict__ allow, const float* __restrict__ inv,
                                                           const float* __restrict__ rstat, const uint32_t* __restrict__ cstat,
                                                           int D, float* __restrict__ thr) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const bool ok = r < N && (!allow || ((allow[r >> 5] >> (r & 31)) & 1u));
    if (!ok) { thr[r] = INFINITY; return; }
    const float b = fmaxf(fmaxf(best[r], best[rows + r]), fmaxf(best[2 * rows + r], best[3 * rows + r]));
    const float Nc = __uint_as_float(cstat[0]), Ec = __uint_as_float(cstat[1]);
    const float eps = cert_eps(rstat[r * 2], rstat[r * 2 + 1], Nc, Ec, D);
    const float band = 2.f * eps / inv[r] * 1.000001f;      // (the division's and the doubling's rounding)
    // a band that is not a number, or infinite: every centroid is a candidate
    const float t = band == band ? score_down(b - band, fabsf(b) + band) : -INFINITY;
    thr[r] = t == t ? t : -INFINITY;
}

// ------------------------------------------------------------------------ decide ----
// The walk of kmeans_best_kernel.  A lane classifies its 8 x 16 scores against its rows' bounds into two bit masks without a
// branch per score (tile_walk.h, the top of the file), the wave counts its candidates with one prefix sum and takes their
// slots with one atomic; a key that finds no room is dropped, the count says so (join_until_it_fits).
__global__ __launch_bounds__(G256_THREADS, 2) void kmeans_decide_kernel(KmeansDecideArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const long ti = blockIdx.x;
    const int CT = (int)((p.C + 255) / 256);
    G256Operand A;
    g256_operand_init(A, p.Gb + ti * 256 * p.D, p.D, p.N - ti * 256, 0, wave, lane);
    tile_slice_frame<0, false, 0>(A, p.Cb, p.D, p.C, 0, CT, smem, p.D, wave, lane, [&](long n0, int lane, const f32x4 (&acc)[8][4]) {
        const TileLane tl = tile_lane(wave, lane);
        const int lq = tl.lq, rbase = tl.rbase, cw = tl.cw;
        const uint64_t fm = tile_column_mask(p.C, n0, cw, nullptr);
        if (fm == 0ull) return;                             // wave-uniform: no centroid in the wave's columns
        const uint64_t bits = fm >> (lq * 4);
        uint32_t colm = 0u;                                 // bit n * 4 + j: this lane's column cw + n * 16 + lq * 4 + j is a centroid
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) colm |= ((uint32_t)(bits >> (n * 16 + j)) & 1u) << (n * 4 + j);
        uint64_t take0 = 0ull, take1 = 0ull;                // bit (m & 3) * 16 + c: score [m][c] is a candidate
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const float t = p.thr[ti * 256 + rbase + m * 16];
            const float mx = tile_row_max(acc, m);
            if (__ballot(mx >= t) == 0ull) continue;        // wave-uniform
            uint32_t ge = 0u;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) ge |= acc[m][n][j] >= t ? 1u << (n * 4 + j) : 0u;
            ge &= colm;
            if (m < 4) take0 |= (uint64_t)ge << (m * 16); else take1 |= (uint64_t)ge << ((m - 4) * 16);
        }
        const int mine = __popcll(take0) + __popcll(take1);
        if (__ballot(mine != 0) == 0ull) return;            // wave-uniform
        int upto = mine;                                    // inclusive prefix sum over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(upto, o, 64);
            if (lane >= o) upto += v;
        }
        const int total = __builtin_amdgcn_readlane(upto, 63);
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(p.cnt, (unsigned long long)total);
        base = readlane_u64(base, 0);
        // (scalar: the wave's slots start at keys + base, `room` of them exist)
        const long left = p.cap - (long)base;
        const int room = left <= 0 ? 0 : (left > (long)total ? total : (int)left);
        uint2* out = (uint2*)(p.keys + (base < (unsigned long long)p.cap ? base : 0ull));
        int pos = upto - mine;
        const uint32_t row0 = (uint32_t)(ti * 256 + rbase), col0 = (uint32_t)(n0 + cw + lq * 4);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            uint64_t mk = h ? take1 : take0;
            while (mk != 0ull) {
                const int bit = __ffsll((long long)mk) - 1;
                mk &= mk - 1ull;
                const int m = h * 4 + (bit >> 4), c = bit & 15;
                if (pos < room) out[pos] = make_uint2(col0 + (uint32_t)((c >> 2) * 16 + (c & 3)), row0 + (uint32_t)(m * 16));   // (row << 32) | centroid
                ++pos;
            }
        }
    });
}

// ----------------------------------------------------------------------- rescore ----
// pairs_dot4's chain (per-lane fma chain over the elements lane * 4 + 256 i, + 0 .. 3 in that order, then wave_sum) over
// q = fl(g * inv) and the centroid's row: the bits a search's re-score gives the master row as a query
__device__ __forceinline__ void kmeans_dot4(const float* const (&gr)[4], const float (&inv)[4], const float* const (&cr)[4], int D,
                                            int lane, float (&out)[4]) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = *(const f32x4*)(gr[u] + c); b[u] = *(const f32x4*)(cr[u] + c); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[u] = fmaf(__fmul_rn(a[u][0], inv[u]), b[u][0], acc[u]);
            acc[u] = fmaf(__fmul_rn(a[u][1], inv[u]), b[u][1], acc[u]);
            acc[u] = fmaf(__fmul_rn(a[u][2], inv[u]), b[u][2], acc[u]);
            acc[u] = fmaf(__fmul_rn(a[u][3], inv[u]), b[u][3], acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) out[u] = wave_sum(acc[u]);
}
// wave g re-scores candidates 4 g .. 4 g + 3 (grid-stride) and folds each into its row's key
__global__ __launch_bounds__(256) void kmeans_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Gf,
                                                             long ldg, const float* __restrict__ inv, const float* __restrict__ Cf,
                                                             int D, unsigned long long* __restrict__ rowkey,
                                                             uint32_t* __restrict__ ncand) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < n; g += waves) {
        const long c0 = g * 4;
        const int m = n - c0 < 4 ? (int)(n - c0) : 4;
        const float* gr[4];
        const float* cr[4];
        float iv[4];
        uint64_t key[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            key[u] = cand[c0 + (u < m ? u : m - 1)];
            const long row = (long)(key[u] >> 32);
            gr[u] = Gf + row * ldg;
            iv[u] = inv[row];
            cr[u] = Cf + (long)(uint32_t)key[u] * D;
        }
        float t[4];
        kmeans_dot4(gr, iv, cr, D, lane, t);
        if (lane < m) {
            const float v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
            const uint64_t k = lane == 0 ? key[0] : (lane == 1 ? key[1] : (lane == 2 ? key[2] : key[3]));
            const long row = (long)(k >> 32);
            atomicMax(&rowkey[row], (unsigned long long)make_key(v, (uint32_t)k));
            atomicAdd(&ncand[row], 1u);
        }
    }
}

// ------------------------------------------------------------------------ finish ----
// ctr[0] += labels that changed, ctr[1] += rows with more than one candidate, ctr[2] += rows with a label; sizes[c] += 1 per
// member (the lanes of a wave that share a label add once)
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const unsigned long long* __restrict__ rowkey,
                                                            const uint32_t* __restrict__ ncand, long N, long C,
                                                            int* __restrict__ labels, float* __restrict__ scores,
                                                            unsigned long long* __restrict__ sizes,
                                                            unsigned long long* __restrict__ ctr) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int lab = -1;
    float sc = -INFINITY;
    bool changed = false, amb = false;
    if (r < N) {
        const unsigned long long k = rowkey[r];
        if (k != 0ull && (long)key_index(k) < C) { lab = (int)key_index(k); sc = key_score(k); }
        changed = labels[r] != lab;
        amb = ncand[r] > 1u;
        labels[r] = lab;
        scores[r] = sc;
    }
    const unsigned long long mc = __ballot(changed), ma = __ballot(amb), ml = __ballot(lab >= 0);
    if (lane == 0) {
        if (mc) atomicAdd(&ctr[0], (unsigned long long)__popcll(mc));
        if (ma) atomicAdd(&ctr[1], (unsigned long long)__popcll(ma));
        if (ml) atomicAdd(&ctr[2], (unsigned long long)__popcll(ml));
    }
    unsigned long long left = ml;
    while (left != 0ull) {                                  // wave-uniform: one trip per distinct label of the wave
        const int first = __ffsll((long long)left) - 1;
        const int l = __shfl(lab, first, 64);
        const unsigned long long same = __ballot(lab == l);
        if (lane == first) atomicAdd(&sizes[l], (unsigned long long)__popcll(same));
        left &= ~same;
    }
}

// ------------------------------------------------------------------------ update ----
__global__ __launch_bounds__(256) void kmeans_keys_kernel(const int* __restrict__ labels, long N, long C, int b,
                                                          uint64_t* __restrict__ keys) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int l = labels[r];
    keys[r] = ((uint64_t)(l >= 0 ? (long)l : C) << b) | (uint64_t)r;
}
// moff[c] = members of centroid c, coff[c] = its chunks of 256 (the two prefix sums follow)
__global__ __launch_bounds__(256) void kmeans_counts_kernel(const unsigned long long* __restrict__ sizes, long C,
                                                            unsigned long long* __restrict__ moff,
                                                            unsigned long long* __restrict__ coff) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const unsigned long long s = sizes[c];
    moff[c] = s;
    coff[c] = (s + 255ull) / 256ull;
}
// Workgroup w: chunk w of the chunks of all centroids in (centroid, chunk) order.  Thread t owns the columns t, t + 256, ...:
// a plain fp32 add chain over the chunk's members in row order, from +0.  The loads of four members are requested together;
// the adds stay in order.
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const uint64_t* __restrict__ keys, int b, const float* __restrict__ Gf,
                                                             long ldg, int D, long C, const unsigned long long* __restrict__ moff,
                                                             const unsigned long long* __restrict__ coff,
                                                             float* __restrict__ part) {
    const unsigned long long w = blockIdx.x;
    if (w >= coff[C - 1]) return;
    long lo = 0, hi = C - 1;                                // the first centroid whose inclusive chunk count passes w
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (coff[mid] > w) hi = mid; else lo = mid + 1;
    }
    const long c = lo;
    const unsigned long long j = w - (c > 0 ? coff[c - 1] : 0ull);
    const long m0 = (long)((c > 0 ? moff[c - 1] : 0ull) + j * 256ull);
    const long m1 = (long)moff[c] < m0 + 256 ? (long)moff[c] : m0 + 256;
    const uint64_t rmask = (1ull << b) - 1ull;
    for (int col = threadIdx.x; col < D; col += 256) {
        float s = 0.f;
        long m = m0;
        for (; m + 4 <= m1; m += 4) {
            const float v0 = Gf[(long)(keys[m] & rmask) * ldg + col], v1 = Gf[(long)(keys[m + 1] & rmask) * ldg + col];
            const float v2 = Gf[(long)(keys[m + 2] & rmask) * ldg + col], v3 = Gf[(long)(keys[m + 3] & rmask) * ldg + col];
            s = __fadd_rn(s, v0); s = __fadd_rn(s, v1); s = __fadd_rn(s, v2); s = __fadd_rn(s, v3);
        }
        for (; m < m1; ++m) s = __fadd_rn(s, Gf[(long)(keys[m] & rmask) * ldg + col]);
        part[(long)w * D + col] = s;
    }
}
// workgroup c: the centroid's partials added in chunk order, from +0
__global__ __launch_bounds__(256) void kmeans_sum_kernel(const float* __restrict__ part, int D,
                                                         const unsigned long long* __restrict__ coff, float* __restrict__ sums) {
    const long c = blockIdx.x;
    const long w0 = c > 0 ? (long)coff[c - 1] : 0, w1 = (long)coff[c];
    for (int col = threadIdx.x; col < D; col += 256) {
        float s = 0.f;
        for (long w = w0; w < w1; ++w) s = __fadd_rn(s, part[w * D + col]);
        sums[c * D + col] = s;
    }
}
// one wave per centroid, behind the normalisation of `sums` into (Cf, Cb): a centroid without members, or whose sum has a
// squared norm -- the normalisation's own -- that is zero or not finite, gets its previous rows back
__global__ __launch_bounds__(256) void kmeans_keep_kernel(const float* __restrict__ sums, const unsigned long long* __restrict__ sizes,
                                                          long C, int D, const float* __restrict__ Cf_old,
                                                          const bf16_t* __restrict__ Cb_old, float* __restrict__ Cf,
                                                          bf16_t* __restrict__ Cb) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const float q = kmeans_row_sq(sums + c * D, D, lane);
    if (sizes[c] != 0ull && q > 0.f && q < INFINITY) return;
    for (int k = lane; k < D; k += 64) {
        Cf[c * D + k] = Cf_old[c * D + k];
        Cb[c * D + k] = Cb_old[c * D + k];
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_kmeans_rows(const float* Gf, const bf16_t* Gb, long ldg, long N, int D, float* inv, float* rstat, hipStream_t st) {
    if (N <= 0) return 0;
    const long blocks = (N + 3) / 4;
    hipLaunchKernelGGL(kmeans_rows_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, Gf, Gb, ldg, N, D, inv,
                       rstat);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
static int kmeans_assign_check(const KmeansAssignArgs& a) {
    if (int rc = g256_check_operands("gallery_kmeans", a.D, a.ldg, a.D)) return rc;
    REVO_REQUIRE(a.rows % 256 == 0 && a.rows >= a.N && a.C >= 1 && a.ldg == a.D, "gallery_kmeans: internal: inconsistent tiles");
    return 0;
}
int launch_kmeans_best(const KmeansAssignArgs& a, hipStream_t st) {
    if (int rc = kmeans_assign_check(a)) return rc;
    if (a.N <= 0) return 0;
    REVO_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)a.best, (int)0xff800000u, (size_t)4 * a.rows, st));   // 4 x rows words of -inf
    REVO_FUNC_LDS(kmeans_best_kernel, G256_LDS);
    const KmeansBestArgs k{a.Gb, a.Cb, a.N, a.C, a.rows, a.best, a.D};
    hipLaunchKernelGGL(kmeans_best_kernel, dim3((unsigned)(a.rows / 256)), dim3(G256_THREADS), G256_LDS, st, k);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_kmeans_bound(const KmeansAssignArgs& a, const float* inv, const float* rstat, const uint32_t* cstat, hipStream_t st) {
    if (a.N <= 0) return 0;
    hipLaunchKernelGGL(kmeans_bound_kernel, dim3((unsigned)(a.rows / 256)), dim3(256), 0, st, a.best, a.rows, a.N, a.allow, inv, rstat,
                       cstat, a.D, a.thr);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_kmeans_decide(const KmeansAssignArgs& a, hipStream_t st) {
    if (int rc = kmeans_assign_check(a)) return rc;
    if (a.N <= 0) return 0;
    REVO_FUNC_LDS(kmeans_decide_kernel, G256_LDS);
    const KmeansDecideArgs k{a.Gb, a.Cb, a.N, a.C, a.thr, a.cnt, a.keys, a.cap, a.D};
    hipLaunchKernelGGL(kmeans_decide_kernel, dim3((unsigned)(a.rows / 256)), dim3(G256_THREADS), G256_LDS, st, k);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_kmeans_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, const float* inv, const float* Cf, int D,
                          unsigned long long* rowkey, uint32_t* ncand, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(kmeans_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Gf, ldg, inv,
                       Cf, D, rowkey, ncand);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_kmeans_finish(const unsigned long long* rowkey, const uint32_t* ncand, long N, long C, int* labels, float* scores,
                         unsigned long long* sizes, unsigned long long* ctr, hipStream_t st) {
    REVO_HIP_CHECK(hipMemsetAsync(sizes, 0, (size_t)C * 8, st));
    if (N <= 0) return 0;
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rowkey, ncand, N, C, labels, scores,
                       sizes, ctr);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_kmeans_update(const KmeansUpdateArgs& a, hipStream_t st) {
    const long N = a.N, C = a.C;
    const int D = a.D;
    if (N > 0) {
        hipLaunchKernelGGL(kmeans_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a.labels, N, C, a.b, a.keys);
        REVO_HIP_CHECK(hipGetLastError());
    }
    uint64_t* sk = nullptr; float* sv = nullptr;
    int cbits = 1;
    while ((1l << cbits) <= C) ++cbits;                     // the label field holds 0 .. C
    if (int rc = launch_sort_keys_u64(a.keys, a.vals, a.keys_alt, a.vals_alt, N, a.b + cbits, a.hist, &sk, &sv, st)) return rc;
    REVO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, a.sizes, C, a.moff, a.coff);
    REVO_HIP_CHECK(hipGetLastError());
    if (int rc = launch_inclusive_sums_u64(a.moff, C, st)) return rc;
    if (int rc = launch_inclusive_sums_u64(a.coff, C, st)) return rc;
    const long max_chunks = N / 256 + C;                    // every centroid leaves less than one chunk unfilled
    REVO_REQUIRE(max_chunks <= a.part_chunks, "gallery_kmeans: internal: the partial sums' workspace is too small");
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)max_chunks), dim3(256), 0, st, sk, a.b, a.Gf, a.ldg, D, C, a.moff, a.coff,
                       a.part);
    REVO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_sum_kernel, dim3((unsigned)C), dim3(256), 0, st, a.part, D, a.coff, a.sums);
    REVO_HIP_CHECK(hipGetLastError());
    if (int rc = launch_l2norm_rows(a.sums, D, a.Cf_new, D, a.Cb_new, D, C, D, st, 1, nullptr, a.cstat)) return rc;
    hipLaunchKernelGGL(kmeans_keep_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, a.sums, a.sizes, C, D, a.Cf_old, a.Cb_old,
                       a.Cf_new, a.Cb_new);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
