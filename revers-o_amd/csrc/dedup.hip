// Deduplicating append (revo_gallery_append_unique, include/revo.h DEDUP): the batch rows are decided in
// order -- a row with a PAIRS score >= thr against a gallery row or an earlier KEPT batch row is dropped -- after they were
// written provisionally to rows N0 .. N0 + n - 1 by the ordinary row writer.
//
//   join     the pairs join (pairs.hip: operands, main loop, column mask, diagonal rule) over the tile pairs whose column tile
//            holds a batch row (dedup_plan.h), with the three-way scores of clusters.hip: a certain edge (i, j), i < j, j a batch
//            row, is applied in place -- atomicMin(first_old[j - N0], i) for a gallery row i, bit (j - N0, i - N0) of the n x n
//            bit matrix for a batch row i -- and only the pairs inside the rounding bound are appended as keys (i << 32) | j
//   rescore  the fp32 score of every ambiguous pair; those >= thr are applied in the same way.  Nothing is stored per edge
//   select   the sequential part, one workgroup: the kept bitmap in LDS, 64 rows per step (each row's matrix words ANDed with
//            the kept bits in front of the block, then one wave resolves the block's own 64 x 64 dependencies in order)
//   scores   one fp32 score per dropped row (the bits revo_gallery_pairs reports for the row and its representative)
//   bits     the remove-bitmap of the dropped rows in the layout of revo_gallery_remove, for the rows from N0 & ~31 on
// Both edge forms are idempotent (min, or): a second join pass (workspace regrow) repeats them, which changes nothing.
#include "candidates.h"
#include "dedup_plan.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

namespace {
// edge (gi, gj), gi < gj, gj a batch row.  edges: first_old [n_pad] | mat [n][W] (DedupJoinArgs, kernels.h); every word
// offset fits 32 bits (n_pad + n W <= 16384 * 513)
__device__ __forceinline__ void dedup_edge(uint32_t* __restrict__ edges, uint32_t N0, uint32_t n_pad, uint32_t W, uint32_t gi,
                                           uint32_t gj) {
    const uint32_t j = gj - N0;
    if (gi < N0) {
        atomicMin(edges + j, gi);
    } else {
        const uint32_t i = gi - N0;
        atomicOr(edges + (n_pad + j * W + (i >> 5)), 1u << (i & 31));
    }
}
__device__ __forceinline__ uint32_t dedup_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t < v ? t : v; }
    return v;
}
}  // namespace

// -------------------------------------------------------------------------- join ----
// tile_walk.h's tile-pair frame on dedup_plan.h's walk, with its three-way classification: A is the row tile ti (it changes
// with every pair), B the column tile tj (the same rows across a column's pairs, from L2), so both operands are set up
// again for every pair (tests/test_dedup_host.py holds the kernel to 0 spilled VGPRs).
// The wave's columns are those of [N0, N): a tile that straddles N0 ignores its old columns.
struct DedupWalk {
    static constexpr bool kInitBoth = true;
    long tj0, T;
    __device__ __forceinline__ void locate(long p0, int& ti, int& tj) const { dedup_locate(p0, tj0, T, ti, tj); }
    __device__ __forceinline__ void next(int& ti, int& tj) const { dedup_next(ti, tj); }
};
__global__ __launch_bounds__(G256_THREADS, 2) void dedup_join_kernel(DedupJoinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PairsJoinArgs& p = a.j;
    const float lb = pairs_lb(p.gstat, p.thr, p.D), ub = pairs_ub(p.gstat, p.thr, p.D);
    tile_pair_frame(p, DedupWalk{(long)(a.N0 >> 8), p.T}, smem, [&](int ci, int cj, long n0, bool diag, int wave, int lane, const f32x4 (&acc)[8][4]) {
        const int cw = (wave & 3) * 64;
        // columns that exist (< N) and are batch rows (>= N0)
        const uint64_t fm = tile_column_mask(p.N, n0, cw, nullptr) & ~tile_column_mask((long)a.N0, n0, cw, nullptr);
        const uint32_t n_pad = dedup_pad(p.N - a.N0), W = dedup_words(p.N - a.N0);
        classify_tile3(p, fm, lb, ub, ci, n0, diag, wave, lane, acc, [](long) { return true; },
                       [&](uint32_t gi, uint32_t gj, bool) { dedup_edge(a.edges, a.N0, n_pad, W, gi, gj); return true; });
    });
}

// ----------------------------------------------------------------------- rescore ----
// wave g re-scores ambiguous pairs 4 g .. 4 g + 3 (grid-stride) with the one fma chain; those that reach thr become edges
__global__ __launch_bounds__(256) void dedup_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Gf,
                                                            long ldg, int D, float thr, uint32_t* __restrict__ edges,
                                                            long N0, long nb) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < n; g += waves) {
        float v;
        uint64_t k;
        const int m = rescore_group4(cand, n, g * 4, D, lane, [&](uint64_t key, const float*& q, const float*& r) {
            q = Gf + (long)(key >> 32) * ldg;
            r = Gf + (long)(uint32_t)key * ldg;
        }, v, k);
        if (lane < m && v >= thr) dedup_edge(edges, (uint32_t)N0, dedup_pad(nb), dedup_words(nb), (uint32_t)(k >> 32), (uint32_t)k);
    }
}

// ------------------------------------------------------------------------ select ----
// One workgroup of 16 waves.  s_kept: the kept flags of the batch rows decided so far; s_pos[i]: kept rows in front of batch
// row i (the new row of a kept row i is N0 + s_pos[i]).  Per block of 64 rows, two barriers:
//   (a) a wave per row (four rows each): a row no gallery row dropped ANDs its matrix words in front of the block with s_kept;
//       the lowest bit left is its lowest kept neighbour of an earlier block.  The block's own word goes to LDS as it is
//   (b) wave 0, lane = row: a row without a gallery row and without an earlier-block neighbour is kept unless a kept row of
//       the block in front of it is its neighbour -- 64 ballots, row r's flag final at step r
// representative, in order of the final row index: the gallery row, the earlier-block row, the row of this block.
__global__ __launch_bounds__(1024) void dedup_select_kernel(DedupSelectArgs a) {
    __shared__ uint64_t s_kept[DEDUP_MAX_BATCH / 64];
    __shared__ uint16_t s_pos[DEDUP_MAX_BATCH];
    __shared__ uint32_t s_pre[64], s_old[64];
    __shared__ uint64_t s_in[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t NONE = DEDUP_NONE;
    const long n = a.n;
    const uint32_t n_pad = dedup_pad(n), W = dedup_words(n);
    for (int i = threadIdx.x; i < DEDUP_MAX_BATCH / 64; i += 1024) s_kept[i] = 0ull;
    __syncthreads();
    const int nb = (int)((n + 63) / 64);
    uint32_t base = 0u;                                     // kept rows in front of the block (wave 0's)
    for (int b = 0; b < nb; ++b) {
        const long j0 = (long)b * 64;
        for (int r = wave; r < 64; r += 16) {
            const long j = j0 + r;
            uint32_t pre = NONE, old = NONE;
            uint64_t in = 0ull;
            if (j < n) {
                old = a.edges[j];
                if (old == NONE) {
                    const uint64_t* row = (const uint64_t*)(a.edges + n_pad + (size_t)j * W);
                    for (int w = lane; w < b; w += 64) {
                        const uint64_t x = row[w] & s_kept[w];
                        if (x != 0ull) { pre = (uint32_t)(w * 64 + __ffsll((long long)x) - 1); break; }   // (w ascends: the lane's lowest)
                    }
                    pre = dedup_wave_min(pre);
                    in = row[b];
                }
            }
            if (lane == 0) { s_pre[r] = pre; s_old[r] = old; s_in[r] = in; }
        }
        __syncthreads();
        if (wave == 0) {
            const long j = j0 + lane;
            const bool valid = j < n;
            const uint32_t old = s_old[lane], pre = s_pre[lane];
            const unsigned long long below = lanes_below(lane);
            const uint64_t in = s_in[lane] & below;         // (the join sets only bits of rows in front of the row)
            const bool free_row = valid && old == NONE && pre == NONE;
            uint64_t km = 0ull;
#pragma unroll 8
            for (int r = 0; r < 64; ++r) {
                const uint64_t mk = __ballot(free_row && (in & km) == 0ull);
                km |= mk & (1ull << r);
            }
            const bool kept = (km >> lane) & 1ull;
            const uint32_t mypos = base + (uint32_t)__popcll(km & below);
            if (valid) {
                s_pos[j] = (uint16_t)mypos;
                uint32_t rep = NONE;
                long long row = (long long)a.N0 + mypos;
                if (!kept) {
                    if (old != NONE) { rep = old; row = (long long)old; }
                    else if (pre != NONE) { rep = (uint32_t)a.N0 + pre; row = (long long)a.N0 + s_pos[pre]; }
                    else {
                        const int i = __ffsll((long long)(in & km)) - 1;
                        rep = (uint32_t)(a.N0 + j0 + i);
                        row = (long long)a.N0 + base + __popcll(km & ((1ull << i) - 1ull));
                    }
                }
                a.rep[j] = rep;
                a.rows[j] = row;
            }
            if (lane == 0) s_kept[b] = km;
            base += (uint32_t)__popcll(km);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_kept[0] = base;
}

// ------------------------------------------------------------------------ finish ----
// wave g: the scores of batch rows 4 g .. 4 g + 3 -- -inf for a kept row, else the PAIRS score of the row and its representative
// (both still at their provisional rows)
__global__ __launch_bounds__(256) void dedup_scores_kernel(const uint32_t* __restrict__ rep, long n, long N0,
                                                           const float* __restrict__ Gf, long ldg, int D,
                                                           float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const long j0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (j0 >= n) return;
    const int m = n - j0 < 4 ? (int)(n - j0) : 4;
    const float* qr[4];
    const float* gr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long j = j0 + (u < m ? u : m - 1);
        const uint32_t rp = rep[j];
        gr[u] = Gf + (N0 + j) * ldg;
        qr[u] = rp == DEDUP_NONE ? gr[u] : Gf + (long)rp * ldg;
    }
    float t[4];
    pairs_dot4(qr, gr, D, lane, t);
    if (lane < m) {
        const float v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
        scores[j0 + lane] = rep[j0 + lane] == DEDUP_NONE ? -INFINITY : v;
    }
}
// the remove-bitmap over the rows from R0 = N0 & ~31 on: position p is row R0 + p; the s = N0 - R0 gallery rows in front stay,
// batch row p - s leaves when it has a representative.  One thread per position, a wave's ballot is two words.
__global__ __launch_bounds__(256) void dedup_bits_kernel(const uint32_t* __restrict__ rep, long n, int s, uint32_t* __restrict__ bits,
                                                         long nwords) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const long j = p - s;
    const bool drop = j >= 0 && j < n && rep[j] != DEDUP_NONE;
    const unsigned long long mk = __ballot(drop);
    if ((threadIdx.x & 63) == 0) {
        const long w = p >> 5;
        if (w < nwords) bits[w] = (uint32_t)mk;
        if (w + 1 < nwords) bits[w + 1] = (uint32_t)(mk >> 32);
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_dedup_join(const DedupJoinArgs& a_in, hipStream_t st) {
    DedupJoinArgs a = a_in;
    PairsJoinArgs& p = a.j;
    if (int rc = g256_check_operands("gallery_append_unique", p.D, p.ldg)) return rc;
    REVO_REQUIRE(p.N < (1ll << 31), "gallery_append_unique: row indices must fit in 31 bits");
    REVO_REQUIRE((long)a.N0 <= p.N && p.N - (long)a.N0 <= DEDUP_MAX_BATCH, "gallery_append_unique: internal: bad join arguments");
    const DedupPlan pl = dedup_plan((long)a.N0, p.N - (long)a.N0);
    if (pl.pairs <= 0) return 0;
    p.T = pl.T; p.pairs = pl.pairs;
    int dev = 0, cus = 0;
    REVO_HIP_CHECK(hipGetDevice(&dev));
    REVO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // one workgroup per CU (the LDS image takes the CU), each a contiguous range of < 2^30 tile pairs
    long wgs = cus > 0 ? cus : 256;
    if (wgs < (p.pairs >> 30) + 1) wgs = (p.pairs >> 30) + 1;
    if (wgs > p.pairs) wgs = p.pairs;
    REVO_FUNC_LDS(dedup_join_kernel, G256_LDS);
    hipLaunchKernelGGL(dedup_join_kernel, dim3((unsigned)wgs), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_dedup_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, uint32_t* edges, long N0,
                         long nb, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(dedup_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Gf, ldg,
                       D, thr, edges, N0, nb);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_dedup_select(const DedupSelectArgs& a, hipStream_t st) {
    REVO_REQUIRE(a.n >= 1 && a.n <= DEDUP_MAX_BATCH, "gallery_append_unique: internal: bad select arguments");
    hipLaunchKernelGGL(dedup_select_kernel, dim3(1), dim3(1024), 0, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_dedup_finish(const uint32_t* rep, long n, long N0, const float* Gf, long ldg, int D, float* scores, uint32_t* bits,
                        long nwords, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4;
    hipLaunchKernelGGL(dedup_scores_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, st, rep, n, N0, Gf, ldg, D, scores);
    const int s = (int)(N0 & 31);
    REVO_REQUIRE(nwords * 32 >= s + n, "gallery_append_unique: internal: remove-bitmap too short");
    hipLaunchKernelGGL(dedup_bits_kernel, dim3((unsigned)((nwords * 32 + 255) / 256)), dim3(256), 0, st, rep, n, s, bits, nwords);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
