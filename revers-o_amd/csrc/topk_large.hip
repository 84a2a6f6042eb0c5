// Exact top-k for 51 <= k <= 1024 (revo_search_topk_large, include/revo.h).  The k <= 50 search keeps
// 32 or 64 candidates per query and cannot be widened; this is a second selection path with its own exactness argument.
// eps(q) is the certificate's rigorous bound of |bf16 score - fp32 score| (cert_eps, kernels.h), for any bf16 MFMA pass.
//
//   sample   the k-th best allowed bf16 score s_b of the first n_s rows (pre-pass GEMM, radix select): at least k rows
//            score >= s_b - eps in fp32, so every row of the answer has bf16 score >= lo = s_b - 2 eps (threshold:
//            max(lo, thr - eps)); fewer than k allowed sample rows: lo = -inf
//   count    one MFMA pass over the gallery (the 256 x 256 main loop): a histogram of the bf16 scores >= lo in LARGE_NB
//            linear buckets of about eps / 4, one non-returning atomic per counted row
//   level    h = the lower edge of the highest bucket with >= k counted rows at or above it (t_k >= h - eps); the band
//            {bf16 >= b = max(h - 2 eps, lo)} holds every row scoring >= t_k in fp32, ties included, and the histogram
//            bounds its size.  Bound <= LARGE_CAP: the query is a band entry; otherwise an entry of the exhaustive fallback
//   collect  launch_topk_collect256 (topk256.hip) with lb = b appends the band's rows
//   finish   fp32 re-score of the band (exact_dot4: the chain of every other re-score, so the scores are the bits
//            revo_search_topk returns), bitonic sort of the (score, index) keys in LDS, threshold cut, first k written
//   fallback every allowed row scored in fp32 into a per-entry buffer, radix select of the k-th best 64-bit key, the k
//            keys at or above it sorted in LDS.  Entries run in rounds of LargeWs::F (bounded scratch)
// Every launch past the sample reads its entry count from the device: no host round trip.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

// bucket of a counted score (monotone in v: fp32 subtraction, multiplication by a positive constant and the clamp all are)
__device__ __forceinline__ int lk_bucket(float v, float base, float inv) {
    float t = __fmul_rn(__fsub_rn(v, base), inv);
    t = fminf(fmaxf(t, 0.f), (float)(LARGE_NB - 1));
    return (int)t;
}
__device__ __forceinline__ float lk_lds_f32(uint32_t off) { return *(__attribute__((address_space(3))) const float*)(uintptr_t)off; }

// ---------------------------------------------------------------- block-wide selection ----
// The k-th largest of the n keys key_of(0 .. n-1) (0 = absent) over their top 8 * passes bits, radix 256: the key with its
// remaining low bits cleared.  0 if fewer than k keys are present.  Every thread of the block calls it; hist: 256 LDS words,
// sh: 2.  passes = 8: the exact key; passes = 4: the exact score of the k-th best (make_key keys).
template <class KeyOf>
__device__ uint64_t lk_kth_largest(KeyOf key_of, long n, int k, int passes, uint32_t* hist, uint32_t* sh) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint64_t prefix = 0ull, mask = 0ull;
    uint32_t need = (uint32_t)k;
    for (int p = 0; p < passes; ++p) {
        const int shift = 56 - 8 * p;
        for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0u;
        __syncthreads();
        for (long r = tid; r < n; r += blockDim.x) {
            const uint64_t key = key_of(r);
            if (key != 0ull && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            uint32_t h[4], c = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) { h[d] = hist[lane * 4 + d]; c += h[d]; }
            uint32_t S = c;                                   // keys in digits >= 4 lane
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_down(S, o, 64);
                if (lane + o < 64) S += t;
            }
            const uint32_t X = S - c;                         // keys in digits above this lane's four
            if (X < need && need <= S) {
                uint32_t cum = X;
                for (int d = 3; d >= 0; --d) {
                    if (cum + h[d] >= need) { sh[0] = (uint32_t)(lane * 4 + d); sh[1] = need - cum; break; }
                    cum += h[d];
                }
            }
            if (lane == 0 && S < need) sh[0] = 0xffffffffu;   // fewer than k keys at all
        }
        __syncthreads();
        const uint32_t digit = sh[0];
        need = sh[1];
        __syncthreads();                                      // everyone has read sh before the next pass writes it
        if (digit == 0xffffffffu) return 0ull;
        prefix |= (uint64_t)digit << shift;
        mask |= 255ull << shift;
    }
    return prefix;
}

// (the block-wide LDS sort lk_sort_desc: topk_util.h, shared with fusion.hip)
// keys[0 .. P) sorted best first (0 = empty; entries past P count as empty) -> output row `orow` (k <= blockDim.x)
__device__ __forceinline__ void lk_write(const uint64_t* keys, int P, long orow, int k, int has_thr, float thr, long idx_offset,
                                         float* __restrict__ out_scores, long long* __restrict__ out_idx,
                                         int* __restrict__ out_counts) {
    const int i = threadIdx.x;
    const uint64_t key = i < k && i < P ? keys[i] : 0ull;
    const bool ok = key != 0ull && (!has_thr || key_score(key) >= thr);
    if (i < k) {
        out_scores[orow * k + i] = ok ? key_score(key) : -INFINITY;
        out_idx[orow * k + i] = ok ? (long long)key_index(key) + idx_offset : -1ll;
    }
    const int cnt = __syncthreads_count(ok);                 // the valid keys are a prefix: sorted, threshold monotone
    if (i == 0) out_counts[orow] = cnt;
}

// ------------------------------------------------------------------------- sample ----
// One workgroup per query: lo, the bucket origin and step, eps (LargeWs::lvl).  pre: [Q][ld] bf16-GEMM scores of rows [0, n_s).
__global__ __launch_bounds__(256) void topk_large_sample_kernel(const float* __restrict__ pre, long ld, int n_s,
                                                                const uint32_t* __restrict__ allow,
                                                                const float* __restrict__ qstat,
                                                                const uint32_t* __restrict__ gstat, int D, int k,
                                                                int has_thr, float thr, float* __restrict__ lvl) {
    __shared__ uint32_t hist[256], sh[2];
    const int q = blockIdx.x;
    const float eps = cert_eps(qstat[(long)q * 2], qstat[(long)q * 2 + 1], __uint_as_float(gstat[0]), __uint_as_float(gstat[1]), D);
    const float* row = pre + (long)q * ld;
    auto key_of = [&](long r) -> uint64_t {
        if (allow && !((allow[r >> 5] >> (r & 31)) & 1u)) return 0ull;
        return make_key(row[r], (uint32_t)r);
    };
    const uint64_t kth = n_s > 0 ? lk_kth_largest(key_of, n_s, k, 4, hist, sh) : 0ull;
    if (threadIdx.x != 0) return;
    float lo = -INFINITY;
    if (kth != 0ull) { const float sb = key_score(kth); lo = score_down(sb - 2.f * eps, sb); }
    if (has_thr) lo = fmaxf(lo, score_down(thr - eps, thr));
    // the buckets cover [base, 1 + 2 eps] (every bf16 score of unit rows lies below it; anything above lands in the last)
    const float base = lo > -INFINITY ? lo : -1.f - 2.f * eps;
    const float span = (1.f + 2.f * eps) - base;
    float step = 0.25f * eps;
    if (span > step * (float)(LARGE_NB - 2)) step = span / (float)(LARGE_NB - 2);
    float* o = lvl + (long)q * LARGE_LVL;
    o[0] = lo; o[1] = base; o[2] = 1.f / step; o[3] = step; o[4] = eps;
}

// -------------------------------------------------------------------------- count ----
// The collect pass's main loop and slicing (topk256.hip topk_collect256_kernel) with the append replaced by a histogram
// count: a score v of query row q, column c, is counted when v >= lo(q) and c is an allowed row of the gallery.
// (The tile loop inside the query-tile loop is tile_walk.h's slice frame, typed out: see there.)
template <int ROWS>
__global__ __launch_bounds__(G256_THREADS, 2) void topk_large_count_kernel(LargeCountArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lv = (float*)(smem + G256_LDS);                  // [256][3] lo, base, inv of the tile's query rows
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nq = p.nq;
    const int sp = blockIdx.x;
    long t0, t1;
    if (!tile_slice<long>((p.N + 255) / 256, p.splits, sp, t0, t1)) return;
    const long row_begin = t0 * 256;
    for (int q0 = 0; q0 < nq; q0 += 256) {
        const int qvalid = (nq - q0) < 256 ? (nq - q0) : 256;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                    // the previous query tile's last reads of lv / the stage
        if (tid < 256) {
            const float* l = p.lvl + (long)(q0 + tid) * LARGE_LVL;
            lv[tid * 3 + 0] = tid < qvalid ? l[0] : INFINITY;    // rows past the queries never count
            lv[tid * 3 + 1] = tid < qvalid ? l[1] : 0.f;
            lv[tid * 3 + 2] = tid < qvalid ? l[2] : 0.f;
        }
        __syncthreads();
        G256Operand A, B;
        g256_operand_init(A, p.Qb, p.ldq, nq, q0, wave, lane);
        g256_operand_init(B, p.Gb + row_begin * p.ldg, p.ldg, p.N - row_begin, 0, wave, lane);
        g256_issue_prologue(A, B, smem, p.D, wave);
        for (long t = t0; t < t1; ++t) {
            const long n0 = t * 256;
            f32x4 acc[8][4];
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
            gemm256_mainloop<ROWS>(A, B, smem, p.D, wave, lane, acc);
            if (t + 1 < t1) {
                g256_operand_init(B, p.Gb + (n0 + 256) * p.ldg, p.ldg, p.N - (n0 + 256), 0, wave, lane);
                g256_issue_prologue(A, B, smem, p.D, wave);
            }
            asm volatile("" : "+v"(lane) :: "memory");
            const int lr = lane & 15, lq = lane >> 4;
            const int rbase = (wave >> 2) * 128 + lr;
            const int cw = (wave & 3) * 64;                 // the wave's 64 columns: bits of one 64-bit word of the bitmap
            const uint64_t bits = tile_column_mask(p.N, n0, cw, p.allow) >> (lq * 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int row = rbase + m * 16;
                const float lo = lk_lds_f32(G256_LDS + row * 12);
                const float mx = tile_row_max(acc, m);
                if (__ballot(mx >= lo) == 0ull) continue;   // wave-uniform
                const float base = lk_lds_f32(G256_LDS + row * 12 + 4), inv = lk_lds_f32(G256_LDS + row * 12 + 8);
                uint32_t* h = p.hist + (long)(q0 + row) * LARGE_NB;
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = acc[m][n][j];
                        if (v >= lo && ((bits >> (n * 16 + j)) & 1ull))
                            __hip_atomic_fetch_add(h + lk_bucket(v, base, inv), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
            }
        }
    }
}

// -------------------------------------------------------------------------- level ----
// One workgroup per query (thread i: buckets 16 i .. 16 i + 15): the band bound, its size bound, and the entry the query becomes.
__global__ __launch_bounds__(256) void topk_large_level_kernel(LargeWs ws, const bf16_t* __restrict__ Qb, long ldq, int D, int k,
                                                               int force_fallback) {
    __shared__ uint32_t suf[256];
    __shared__ int top_b, entry;
    __shared__ uint32_t band_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint32_t* h = ws.hist + (long)q * LARGE_NB;
    uint32_t c[16], T = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { c[i] = h[tid * 16 + i]; T += c[i]; }
    suf[tid] = T;
    if (tid == 0) { top_b = -1; band_n = 0u; }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                // suf[i] := sum of T over threads >= i
        const uint32_t v = tid + off < 256 ? suf[tid + off] : 0u;
        __syncthreads();
        suf[tid] += v;
        __syncthreads();
    }
    if (suf[tid] >= (uint32_t)k) {
        uint32_t cum = suf[tid] - T;
        for (int i = 15; i >= 0; --i) {
            cum += c[i];
            if (cum >= (uint32_t)k) { atomicMax(&top_b, tid * 16 + i); break; }
        }
    }
    __syncthreads();
    const float* l = ws.lvl + (long)q * LARGE_LVL;
    const float lo = l[0], base = l[1], inv = l[2], step = l[3], eps = l[4];
    const int b = top_b;
    // rows of bucket >= b >= 1 score >= base + (b - 1) step (a whole bucket below the edge: covers the rounding of lk_bucket)
    float hh = b < 0 ? -INFINITY : (b == 0 ? lo : base + (float)(b - 1) * step);
    const float lb = fmaxf(hh > -INFINITY ? score_down(hh - 2.f * eps, hh) : -INFINITY, lo);
    const int bb = lk_bucket(lb, base, inv);                 // every row >= lb was counted in a bucket >= bb
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) mine += tid * 16 + i >= bb ? c[i] : 0u;
    atomicAdd(&band_n, mine);
    __syncthreads();
    if (tid == 0) {
        if (!force_fallback && band_n <= (uint32_t)LARGE_CAP) {
            const int j = atomicAdd(ws.ctr + 0, 1);
            ws.band_q[j] = q; ws.band_lb[j] = lb; ws.band_cnt[j] = 0;
            entry = j;
        } else {
            ws.fb_q[atomicAdd(ws.ctr + 1, 1)] = q;
            atomicAdd(ws.stats + CTR_LARGE_FALLBACK, 1);
            entry = -1;
        }
    }
    __syncthreads();
    if (entry >= 0) {                                        // the collect pass reads whole query tiles: compacted rows
        const uint32_t* src = (const uint32_t*)(Qb + (long)q * ldq);
        uint32_t* dst = (uint32_t*)(ws.band_qb + (long)entry * D);
        for (int i = tid; i < D / 2; i += 256) dst[i] = src[i];
    }
}

// ------------------------------------------------------------------------- finish ----
// grid (LARGE_CAP / 256, entries): wave w of workgroup (s, y) re-scores keys s * 256 + 64 w .. + 63 of band entries y, y + gy, ...
// in place (bf16 key -> fp32 key), four rows in flight (the exact_finish pattern, topk_exact.hip)
__global__ __launch_bounds__(256) void topk_large_rescore_kernel(LargeWs ws, const float* __restrict__ Qf, long ldqf,
                                                                 const float* __restrict__ Gf, long ldgf, int D) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int entries = ws.ctr[0];
    for (int j = blockIdx.y; j < entries; j += gridDim.y) {
        const int n = ws.band_cnt[j];
        const int c0 = blockIdx.x * 256 + w * 64;
        if (n > LARGE_CAP || c0 >= n) continue;              // (an overflowed band goes to the fallback: sort kernel)
        const int m = (n - c0) < 64 ? (n - c0) : 64;
        const float* qr = Qf + (long)ws.band_q[j] * ldqf;
        uint64_t* col = ws.band_col + (long)j * LARGE_CAP + c0;
        const uint32_t idx = key_index(lane < m ? col[lane] : 0ull);
        float score = -INFINITY;
        for (int e0 = 0; e0 < m; e0 += 4) {
            const float* gr[4];
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cn = e0 + u < m ? e0 + u : m - 1;
                gr[u] = Gf + (long)__shfl(idx, cn, 64) * ldgf;
            }
            exact_dot4(qr, gr, D, lane, t);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (lane == e0 + u) score = t[u];
        }
        if (lane < m) col[lane] = make_key(score, idx);
    }
}
// one workgroup per band entry: sort its re-scored keys in LDS, write the first k; an overflowed band becomes a fallback entry
__global__ __launch_bounds__(1024) void topk_large_sort_kernel(LargeWs ws, int k, int has_thr, float thr, long idx_offset,
                                                               float* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                               int* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = (uint64_t*)smem;                        // [LARGE_CAP]
    const int entries = ws.ctr[0];
    for (int j = blockIdx.x; j < entries; j += gridDim.x) {
        const int n = ws.band_cnt[j], q = ws.band_q[j];
        if (n > LARGE_CAP) {                                 // (the count's size bound held for the count pass's own scores)
            if (threadIdx.x == 0) { ws.fb_q[atomicAdd(ws.ctr + 1, 1)] = q; atomicAdd(ws.stats + CTR_LARGE_FALLBACK, 1); }
            continue;
        }
        if (threadIdx.x == 0) atomicAdd(ws.stats + CTR_COLLECTED, n);
        int P = 64;
        while (P < n) P <<= 1;
        const uint64_t* col = ws.band_col + (long)j * LARGE_CAP;
        for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = i < n ? col[i] : 0ull;
        __syncthreads();
        lk_sort_desc(keys, P);
        lk_write(keys, P, q, k, has_thr, thr, idx_offset, out_scores, out_idx, out_counts);
        __syncthreads();                                     // `keys` is reused by the next entry
    }
}

// ----------------------------------------------------------------------- fallback ----
// grid (LARGE_FB_SLICES, F): the fp32 score of every row of slice s for fallback entry round * F + y (NaN: not allowed)
__global__ __launch_bounds__(1024) void topk_large_fb_score_kernel(LargeWs ws, int round, const float* __restrict__ Qf, long ldqf,
                                                                   const float* __restrict__ Gf, long ldgf, long N, int D,
                                                                   const uint32_t* __restrict__ allow, int skip_self) {
    const int i = round * ws.F + blockIdx.y;
    if (i >= ws.ctr[1]) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* qr = Qf + (long)ws.fb_q[i] * ldqf;
    const long self = skip_self ? (long)ws.fb_q[i] : -1;    // the kNN graph: the query is gallery row fb_q[i], never its own neighbour
    float* out = ws.fb_scores + (long)blockIdx.y * N;
    const long per = (N + LARGE_FB_SLICES - 1) / LARGE_FB_SLICES;
    const long r0 = (long)blockIdx.x * per;
    const long r1 = r0 + per < N ? r0 + per : N;
    for (long r = r0 + (long)w * 4; r < r1; r += 16 * 4) {
        const float* gr[4];
        float t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) gr[u] = Gf + (r + u < r1 ? r + u : r1 - 1) * ldgf;
        exact_dot4(qr, gr, D, lane, t);
        if (lane < 4 && r + lane < r1) {
            const long row = r + lane;
            const float v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
            const bool ok = (!allow || ((allow[row >> 5] >> (row & 31)) & 1u)) && row != self;
            out[row] = ok ? v : __builtin_nanf("");
        }
    }
}
// one workgroup per fallback entry of the round: the k-th best key of its N scores, the keys at or above it sorted, k written
__global__ __launch_bounds__(1024) void topk_large_fb_select_kernel(LargeWs ws, int round, long N, int k, int has_thr, float thr,
                                                                    long idx_offset, float* __restrict__ out_scores,
                                                                    long long* __restrict__ out_idx, int* __restrict__ out_counts) {
    __shared__ uint64_t keys[LARGE_K_MAX];
    __shared__ uint32_t hist[256], sh[2], n_kept;
    const int i = round * ws.F + blockIdx.x;
    if (i >= ws.ctr[1]) return;
    const float* s = ws.fb_scores + (long)blockIdx.x * N;
    auto key_of = [&](long r) -> uint64_t {
        const float v = s[r];
        return v != v ? 0ull : make_key(v, (uint32_t)r);
    };
    const uint64_t kth = lk_kth_largest(key_of, N, k, 8, hist, sh);
    for (int t = threadIdx.x; t < LARGE_K_MAX; t += blockDim.x) keys[t] = 0ull;
    if (threadIdx.x == 0) n_kept = 0u;
    __syncthreads();
    // kth != 0: exactly k keys are >= kth (keys are distinct); kth == 0: fewer than k keys at all
    for (long r = threadIdx.x; r < N; r += blockDim.x) {
        const uint64_t key = key_of(r);
        if (key != 0ull && key >= kth) {
            const uint32_t pos = atomicAdd(&n_kept, 1u);
            if (pos < (uint32_t)LARGE_K_MAX) keys[pos] = key;
        }
    }
    __syncthreads();
    lk_sort_desc(keys, LARGE_K_MAX);
    lk_write(keys, LARGE_K_MAX, ws.fb_q[i], k, has_thr, thr, idx_offset, out_scores, out_idx, out_counts);
}

// ------------------------------------------------------------------------ launchers ----
int launch_topk_large_sample(const float* pre, long ld, int n_s, const uint32_t* allow, const float* qstat, const uint32_t* gstat,
                             int D, int Q, int k, int has_thr, float thr, const LargeWs& ws, hipStream_t st) {
    if (Q <= 0) return 0;
    hipLaunchKernelGGL(topk_large_sample_kernel, dim3((unsigned)Q), dim3(256), 0, st, pre, ld, n_s, allow, qstat, gstat, D, k,
                       has_thr, thr, ws.lvl);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_topk_large_count(const bf16_t* Qb, long ldq, const bf16_t* Gb, long ldg, long N, int D, int Q, const LargeWs& ws,
                            const uint32_t* allow, hipStream_t st) {
    if (int rc = g256_check_operands("search", D, ldg, ldq)) return rc;
    REVO_REQUIRE(N < (1ll << 32), "search: a gallery holds at most 2^32 rows");
    if (Q <= 0 || N <= 0) return 0;
    LargeCountArgs a{};
    a.Qb = Qb; a.ldq = ldq; a.Gb = Gb; a.ldg = ldg; a.N = N; a.D = D; a.nq = Q; a.splits = topk_collect256_splits(N);
    a.lvl = ws.lvl; a.hist = ws.hist; a.allow = allow;
    constexpr int LDS = G256_LDS + 256 * 12;
    const dim3 grid((unsigned)a.splits), block(G256_THREADS);
#define LK_COUNT(RW)                                                                        \
    do {                                                                                    \
        REVO_FUNC_LDS((topk_large_count_kernel<RW>), LDS);                                  \
        hipLaunchKernelGGL((topk_large_count_kernel<RW>), grid, block, LDS, st, a);         \
    } while (0)
    if (Q <= 64) LK_COUNT(64);
    else if (Q <= 128) LK_COUNT(128);
    else LK_COUNT(0);
#undef LK_COUNT
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_topk_large_level(const LargeWs& ws, const bf16_t* Qb, long ldq, int D, int Q, int k, int force_fallback, hipStream_t st) {
    if (Q <= 0) return 0;
    hipLaunchKernelGGL(topk_large_level_kernel, dim3((unsigned)Q), dim3(256), 0, st, ws, Qb, ldq, D, k, force_fallback);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_topk_large_finish(const LargeWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf, int D,
                             int k, int has_thr, float thr, long idx_offset, float* out_scores, long long* out_idx,
                             int* out_counts, hipStream_t st) {
    if (max_entries <= 0) return 0;
    REVO_REQUIRE(Gf && k >= 1 && k <= LARGE_K_MAX, "large-k finish: needs the fp32 master rows and 1 <= k <= 1024");
    const int ny = max_entries < 1024 ? max_entries : 1024;
    hipLaunchKernelGGL(topk_large_rescore_kernel, dim3(LARGE_CAP / 256, (unsigned)ny), dim3(256), 0, st, ws, Qf, ldqf, Gf, ldgf, D);
    constexpr int LDS = LARGE_CAP * 8;
    REVO_FUNC_LDS(topk_large_sort_kernel, LDS);
    hipLaunchKernelGGL(topk_large_sort_kernel, dim3((unsigned)ny), dim3(1024), LDS, st, ws, k, has_thr, thr, idx_offset,
                       out_scores, out_idx, out_counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_topk_large_fallback(const LargeWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf, long N,
                               int D, int k, int has_thr, float thr, long idx_offset, float* out_scores, long long* out_idx,
                               int* out_counts, const uint32_t* allow, hipStream_t st, int skip_self) {
    if (max_entries <= 0 || N <= 0) return 0;
    REVO_REQUIRE(Gf && ws.F >= 1 && k >= 1 && k <= LARGE_K_MAX && N < (1ll << 32),
                 "large-k fallback: needs the fp32 master rows, 1 <= k <= 1024, N < 2^32");
    // rounds of F entries: the score buffer holds F rows of N; a round past the device's entry count exits at once
    for (int round = 0; round * ws.F < max_entries; ++round) {
        hipLaunchKernelGGL(topk_large_fb_score_kernel, dim3(LARGE_FB_SLICES, (unsigned)ws.F), dim3(1024), 0, st, ws, round, Qf,
                           ldqf, Gf, ldgf, N, D, allow, skip_self);
        hipLaunchKernelGGL(topk_large_fb_select_kernel, dim3((unsigned)ws.F), dim3(1024), 0, st, ws, round, N, k, has_thr, thr,
                           idx_offset, out_scores, out_idx, out_counts);
    }
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
