// Exact diverse search: top-k by maximal marginal relevance (revo_search_mmr, include/revo.h).  The
// candidates of a query are the result lists of revo_search_topk_large at k = C (search.hip runs it into a workspace);
//
//   gram     per query the n x n matrix sim(i, j) of its n <= C candidates' fp32 master rows: the bits revo_gallery_pairs
//            reports for the pair (pairs_dot4: per-lane fma chain over the elements lane*4 + 256*i, then wave_sum's tree).
//            A wave owns a T x T tile of the upper triangle of candidate tiles: every lane loads its f32x4 slice of the 2 T
//            gathered rows once per 256-element step and runs T * T independent fma chains on it (pairs_dot4 runs 4 chains
//            on 8 slices); the cross-lane sums go through wave_sum_transposed (common.h: wave_sum's tree, T * T sums in
//            T * T - 1 + a few shuffles).  fmaf's product is commutative, so the value is written to (i, j) and (j, i).
//   select   one workgroup per query, thread t owns candidate t (relevance, running maximum m of its similarity to the
//            picked ones, a picked flag: registers).  k steps of: v = fl(fl(lam * rel) - fl(diversity * m)), workgroup
//            arg-max of a 64-bit key (order-preserving v with -0 = +0, then the lower position), emit, m = max(m, row of
//            the picked candidate in the query's matrix).  Its tail writes the padding and the count.
// Both kernels read the list lengths on the device: the call has no host round trip.
#include "kernels.h"
#include "topk_util.h"

namespace revo {

// first tile pair of tile row ta in the row-major linearisation of the upper triangle (ta <= tb < T)
__device__ __forceinline__ int mmr_row_start(int ta, int T) { return ta * T - ta * (ta - 1) / 2; }

// -------------------------------------------------------------------------- gram ----
// Block b -> (query, workgroup of the query's tile pairs).  Blocks b and b + 8 are observed to land on the same XCD, so the
// first 8 * (Q / 8) queries go eight at a time, query 8 g + (b & 7) to the blocks of one residue: the <= 4 MB of a query's
// candidate rows are then gathered through one XCD's L2.  The remaining Q % 8 queries (a single query above all) take their
// workgroups in block order, over every XCD: eight copies of a few MB cost less than seven idle XCDs.  Placement changes
// speed only.  Wave w of a workgroup takes tile pair 4 * wg + w of the query's own triangle (n candidates: the tiles a short
// list does not reach belong to no pair, their waves leave).
template <int T>
__global__ __launch_bounds__(256) void mmr_gram_kernel(MmrGramArgs p) {
    constexpr int NV = T * T, NG = NV < 32 ? NV : 32, DUP = 64 / NG;   // sums per wave_sum_transposed call; lanes per sum
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long b = blockIdx.x;
    const long grouped = (long)(p.Q / 8) * 8 * p.W;
    int q, wg;
    if (b < grouped) {
        const long slot = b >> 3;
        q = (int)(slot / p.W) * 8 + (int)(b & 7);
        wg = (int)(slot % p.W);
    } else {
        q = p.Q / 8 * 8 + (int)((b - grouped) / p.W);
        wg = (int)((b - grouped) % p.W);
    }
    int n = p.counts[q];
    n = n < p.C ? n : p.C;
    const int Tn = (n + T - 1) / T;
    const int pair = wg * 4 + wave;
    if (pair >= Tn * (Tn + 1) / 2) return;                  // wave-uniform (n = 0: every wave)
    int lo = 0, hi = Tn - 1;                                // the tile row of `pair`: the largest ta with row_start(ta) <= pair
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mmr_row_start(mid, Tn) <= pair) lo = mid; else hi = mid - 1;
    }
    const int ta = lo, tb = lo + (pair - mmr_row_start(lo, Tn));
    const long long* cand = p.cand + (long)q * p.C;
    const float* ra[T];
    const float* rb[T];
#pragma unroll
    for (int u = 0; u < T; ++u) {
        // positions past the list's end read its last row (computed, never written); a row outside the gallery reads row 0
        const int ia = ta * T + u < n ? ta * T + u : n - 1, ib = tb * T + u < n ? tb * T + u : n - 1;
        const long long ga = cand[ia], gb = cand[ib];
        ra[u] = p.Gf + ((unsigned long long)ga < (unsigned long long)p.N ? (long)ga : 0l) * p.ldg;
        rb[u] = p.Gf + ((unsigned long long)gb < (unsigned long long)p.N ? (long)gb : 0l) * p.ldg;
    }
    float acc[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = 0.f;
    for (int c = lane * 4; c < p.D; c += 256) {
        f32x4 a[T], bb[T];
#pragma unroll
        for (int u = 0; u < T; ++u) { a[u] = *(const f32x4*)(ra[u] + c); bb[u] = *(const f32x4*)(rb[u] + c); }
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                float s = acc[i * T + j];
                s = fmaf(a[i][0], bb[j][0], s);
                s = fmaf(a[i][1], bb[j][1], s);
                s = fmaf(a[i][2], bb[j][2], s);
                s = fmaf(a[i][3], bb[j][3], s);
                acc[i * T + j] = s;
            }
    }
    float* gq = p.gram + (long)q * p.C * p.C;
#pragma unroll
    for (int g = 0; g < NV / NG; ++g) {
        float v[NG];
#pragma unroll
        for (int e = 0; e < NG; ++e) v[e] = acc[g * NG + e];
        int idx;
        const float s = wave_sum_transposed<NG>(v, lane, idx);
        // DUP lanes hold the same sum: one of them writes it, a different one for each group
        if ((lane & (DUP - 1)) != (g & (DUP - 1))) continue;
        const int e = g * NG + idx;
        const int ci = ta * T + e / T, cj = tb * T + e % T;
        if (ci < n && cj < n) {
            gq[(long)ci * p.C + cj] = s;
            gq[(long)cj * p.C + ci] = s;
        }
    }
}

// ------------------------------------------------------------------------ select ----
// blockDim = C rounded up to whole waves.  One barrier per step: the waves' maxima alternate between two LDS rows, so a
// wave that is a step ahead writes the row nobody reads any more.
__global__ __launch_bounds__(1024) void mmr_select_kernel(MmrSelectArgs p) {
    __shared__ uint64_t wmax[2][16];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = (blockDim.x + 63) >> 6;
    int n = p.counts[q];
    n = n < p.C ? n : p.C;
    const int steps = p.k < n ? p.k : n;
    bool alive = t < n;
    const float rel = alive ? p.rel[(long)q * p.C + t] : 0.f;
    const long long row = alive ? p.cand[(long)q * p.C + t] : -1ll;
    // v is three separately rounded operations.  __fmul_rn / __fsub_rn are plain * and - to hipcc, whose back end contracts
    // them into one fma (one rounding less: other bits whenever diversity is not a power of two), so each product is pinned
    // in a register before the subtraction sees it
    float lr = __fmul_rn(p.lam, rel);
    asm volatile("" : "+v"(lr));
    float m = -INFINITY;
    const float* gq = p.gram + (long)q * p.C * p.C;
    float* o_s = p.scores + (long)q * p.k;
    float* o_v = p.mmr ? p.mmr + (long)q * p.k : nullptr;
    long long* o_i = p.idx + (long)q * p.k;
    for (int s = 0; s < steps; ++s) {
        float dm = __fmul_rn(p.diversity, m);
        asm volatile("" : "+v"(dm));
        const float v = s == 0 ? lr : __fsub_rn(lr, dm);
        // (a candidate's key is never 0: its low word is ~t)
        uint64_t key = alive ? make_key(v == 0.f ? 0.f : v, (uint32_t)t) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint64_t x = shfl_xor_u64(key, o); key = key > x ? key : x; }
        if (lane == 0) wmax[s & 1][wave] = key;
        __syncthreads();
        uint64_t best = 0ull;
        for (int w = 0; w < nw; ++w) { const uint64_t x = wmax[s & 1][w]; best = best > x ? best : x; }
        const int pk = (int)key_index(best);
        if (t == pk) {
            o_s[s] = rel;
            if (o_v) o_v[s] = v;
            o_i[s] = row + p.idx_offset;
            alive = false;
        }
        if (alive) m = fmaxf(m, gq[(long)pk * p.C + t]);
    }
    for (int s = steps + t; s < p.k; s += blockDim.x) {
        o_s[s] = -INFINITY;
        if (o_v) o_v[s] = -INFINITY;
        o_i[s] = -1;
    }
    if (t == 0) p.out_counts[q] = steps;
}

// ------------------------------------------------------------------------ launchers ----
int launch_mmr_gram(const MmrGramArgs& a_in, hipStream_t st) {
    MmrGramArgs a = a_in;
    REVO_REQUIRE(a.D % 64 == 0 && a.ldg % 4 == 0, "search_mmr: D must be a multiple of 64");
    REVO_REQUIRE(a.C >= 1 && a.C <= LARGE_K_MAX && a.Q >= 0, "search_mmr: bad workspace shape");
    if (a.Q == 0 || a.N <= 0) return 0;
    const int T = a.tile == 4 ? 4 : 8;
    const long Tm = (a.C + T - 1) / T;
    a.W = (int)((Tm * (Tm + 1) / 2 + 3) / 4);
    const long blocks = (long)a.Q * a.W;
    REVO_REQUIRE(blocks < (1l << 31), "search_mmr: too many queries in one chunk");
    if (T == 4) hipLaunchKernelGGL(mmr_gram_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(mmr_gram_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_mmr_select(const MmrSelectArgs& a, int Q, hipStream_t st) {
    REVO_REQUIRE(a.C >= 1 && a.C <= LARGE_K_MAX && a.k >= 1 && a.k <= a.C, "search_mmr: 1 <= k <= candidates <= 1024");
    if (Q <= 0) return 0;
    hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)Q), dim3((unsigned)((a.C + 63) / 64 * 64)), 0, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
