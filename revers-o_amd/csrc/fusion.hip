// Hybrid queries (revo_search_fusion, revo_topk_fuse; include/revo.h FUSION): m result lists of one
// search fused into one by reciprocal rank fusion (RRF) or distribution-based score fusion (DBSF).  One workgroup per fused
// search, everything in LDS:
//   stats    DBSF only: the scores are staged in LDS; lane j walks list j twice in fp64 (sum, then squared deviations), in
//            position order
//   gather   a member (row, list j, position r - 1) becomes the 64-bit word (row << 16) | (j << 10) | (r - 1); the LDS sort is
//            descending, so the COMPLEMENT is stored: equal rows end up as one run, lists ascending inside it, positions
//            ascending inside a list, and 0 (the empty slot) sorts behind every member
//   sum      the thread at a run's head adds the run's contributions one after the other in fp32: j ascending, the contract's
//            order; it emits (order-preserving F) << 32 | ~(run position) << 16 | (F is -0)
//   order    the second LDS sort: F descending with -0 = +0, then the run position ascending = the row ascending
//   write    threshold cut, the first k with their ranks (one walk along the run per output row)
// The sort is topk_large.hip's (topk_util.h lk_sort_desc), at the power of two the launch needs: 64 .. 8192 keys.
#include "kernels.h"
#include "topk_util.h"

namespace revo {

constexpr int FK_POS_BITS = 10, FK_LIST_BITS = 6;     // position < 1024, list < 64; the row sits above both
constexpr int FK_ROW_SHIFT = FK_POS_BITS + FK_LIST_BITS;

__device__ __forceinline__ uint64_t fk_row(uint64_t member) { return member >> FK_ROW_SHIFT; }
__device__ __forceinline__ int fk_list(uint64_t member) { return (int)(member >> FK_POS_BITS) & (FUSION_MAX_LISTS - 1); }
__device__ __forceinline__ int fk_pos(uint64_t member) { return (int)member & ((1 << FK_POS_BITS) - 1); }

// DBSF statistics of one list over its kept entries in position order (fp64, every operation rounded on its own):
// lo = mu - 3 sd and span = 6 sd; span = 0 when !(sd > 0) (every member then contributes v = 0.5)
__device__ __forceinline__ void fk_list_stats(const float* __restrict__ s, int cnt, float t, double& lo, double& span) {
#pragma clang fp contract(off)
    double S = 0.0;
    int nm = 0;
    for (int r = 0; r < cnt; ++r) {
        const float v = s[r];
        if (v < t) continue;
        S = nm ? S + (double)v : (double)v;
        ++nm;
    }
    lo = 0.0; span = 0.0;
    if (nm == 0) return;
    const double mu = S / (double)nm;
    double V = 0.0;
    bool first = true;
    for (int r = 0; r < cnt; ++r) {
        const float v = s[r];
        if (v < t) continue;
        const double d = (double)v - mu;
        const double dd = d * d;
        V = first ? dd : V + dd;
        first = false;
    }
    const double sd = sqrt(V / (double)nm);
    if (!(sd > 0.0)) return;
    const double three = 3.0 * sd;
    lo = mu - three;
    span = 6.0 * sd;
}
__device__ __forceinline__ float fk_dbsf(float s, double lo, double span, float w) {
#pragma clang fp contract(off)
    float v = 0.5f;
    if (span > 0.0) {
        const double num = (double)s - lo;
        v = (float)(num / span);
    }
    return __fmul_rn(w, v);
}
__device__ __forceinline__ float fk_rrf(int r, float rrf_k, float w) {
#pragma clang fp contract(off)
    return __fdiv_rn(w, __fadd_rn(rrf_k, (float)r));
}
__device__ __forceinline__ float fk_add(float F, float c) {
#pragma clang fp contract(off)
    return __fadd_rn(F, c);
}

// grid: one workgroup per fused search; blockDim = P / 2 clamped to [64, 1024]; dynamic LDS: 2 * P keys
__global__ __launch_bounds__(1024) void fusion_fuse_kernel(FusionArgs p, int P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = (uint64_t*)smem;                        // [P] the members, complemented (0 = empty)
    uint64_t* heads = keys + P;                              // [P] one word per run, at the run's first position
    __shared__ double s_lo[FUSION_MAX_LISTS], s_span[FUSION_MAX_LISTS];
    __shared__ float s_w[FUSION_MAX_LISTS], s_t[FUSION_MAX_LISTS];
    __shared__ int s_cnt[FUSION_MAX_LISTS];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int m = p.m, C = p.C, k = p.k;
    const long base = (long)i * m * C;
    const float* sc = p.scores + base;
    const long long* ix = p.idx + base;
    const int total = m * C;
    const float* stage = (const float*)heads;                // DBSF: the lists' scores, staged where the run words go later
    if (p.method == 1) {                                     // (one lane walking a list twice reads LDS, not global memory)
        for (int e = tid; e < total; e += blockDim.x) ((float*)heads)[e] = sc[e];
        __syncthreads();
    }
    if (tid < m) {
        int c = p.counts[(long)i * m + tid];
        c = c < 0 ? 0 : (c < C ? c : C);
        s_cnt[tid] = c;
        s_w[tid] = p.w[tid];
        s_t[tid] = p.t[tid];
        if (p.method == 1) {
            double lo, span;
            fk_list_stats(stage + tid * C, c, p.t[tid], lo, span);
            s_lo[tid] = lo; s_span[tid] = span;
        }
    }
    __syncthreads();
    // ---- gather
    for (int e = tid; e < P; e += blockDim.x) {
        uint64_t key = 0ull;
        if (e < total) {
            const int j = e / C, pos = e - j * C;
            if (pos < s_cnt[j] && !(sc[e] < s_t[j]))
                key = ~(((uint64_t)ix[e] << FK_ROW_SHIFT) | ((uint64_t)j << FK_POS_BITS) | (uint64_t)pos);
        }
        keys[e] = key;
    }
    __syncthreads();
    lk_sort_desc(keys, P);
    // ---- sum: the head of each run
    for (int e = tid; e < P; e += blockDim.x) {
        const uint64_t k0 = keys[e];
        uint64_t out = 0ull;
        if (k0 != 0ull) {
            const uint64_t row = fk_row(~k0);
            if (e == 0 || fk_row(~keys[e - 1]) != row) {
                float F = 0.f;
                for (int x = e; x < P; ++x) {
                    const uint64_t kk = keys[x];
                    if (kk == 0ull) break;
                    const uint64_t mem = ~kk;
                    if (fk_row(mem) != row) break;
                    const int j = fk_list(mem), pos = fk_pos(mem);
                    const float c = p.method == 1 ? fk_dbsf(sc[(long)j * C + pos], s_lo[j], s_span[j], s_w[j])
                                                  : fk_rrf(pos + 1, p.rrf_k, s_w[j]);
                    F = x == e ? c : fk_add(F, c);
                }
                const bool zero = F == 0.f;                  // -0 orders as +0; its sign rides below the run position
                const uint32_t neg0 = zero && (__float_as_uint(F) >> 31) ? 1u : 0u;
                out = ((uint64_t)f32_orderable(zero ? 0.f : F) << 32) | ((uint64_t)(~(uint32_t)e & 0xffffu) << 16) | neg0;
            }
        }
        heads[e] = out;
    }
    __syncthreads();
    lk_sort_desc(heads, P);
    // ---- write (the kept words are a prefix: sorted, and the cut is monotone in F)
    int cnt = 0;
    for (int o0 = 0; o0 < k; o0 += blockDim.x) {
        const int o = o0 + tid;
        const uint64_t h = o < k && o < P ? heads[o] : 0ull;
        float F = orderable_f32((uint32_t)(h >> 32));
        const bool ok = h != 0ull && !(p.has_thr && F < p.thr);
        if (h & 1ull) F = -0.f;
        const int e = (int)(~(uint32_t)(h >> 16) & 0xffffu);
        const uint64_t row = ok ? fk_row(~keys[e]) : 0ull;
        if (o < k) {
            p.out_scores[(long)i * k + o] = ok ? F : -INFINITY;
            p.out_idx[(long)i * k + o] = ok ? (long long)row + p.idx_offset : -1ll;
            if (p.out_ranks) {
                int* rr = p.out_ranks + ((long)i * k + o) * m;
                int x = e;
                for (int j = 0; j < m; ++j) {
                    int r = 0;
                    while (ok && x < P) {                    // the run's entries of list j: the first one is the rank
                        const uint64_t kk = keys[x];
                        if (kk == 0ull) break;
                        const uint64_t mem = ~kk;
                        if (fk_row(mem) != row || fk_list(mem) > j) break;
                        if (r == 0) r = fk_pos(mem) + 1;
                        ++x;
                    }
                    rr[j] = r;
                }
            }
        }
        cnt += __syncthreads_count(ok);
    }
    if (tid == 0) p.out_counts[i] = cnt;
}

// grid: one workgroup per (fused search, list); wave w scores result rows 4 w .. 4 w + 3, then 16 further on
__global__ __launch_bounds__(256) void fusion_list_scores_kernel(const float* __restrict__ Qf, long ldq, const float* __restrict__ Gf,
                                                                  long ldg, int D, const long long* __restrict__ out_idx,
                                                                  const int* __restrict__ out_counts, long idx_offset, int m, int k,
                                                                  float* __restrict__ list_scores) {
    const int ij = blockIdx.x, i = ij / m, j = ij - i * m;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cnt = out_counts[i];
    cnt = cnt < 0 ? 0 : (cnt < k ? cnt : k);
    const float* qr = Qf + (long)ij * ldq;
    const long long* oi = out_idx + (long)i * k;
    for (int e0 = w * 4; e0 < k; e0 += 16) {
        float v = -INFINITY;
        if (e0 < cnt) {
            const float* gr[4];
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) gr[u] = Gf + (long)(oi[e0 + u < cnt ? e0 + u : cnt - 1] - idx_offset) * ldg;
            exact_dot4(qr, gr, D, lane, t);
            if (e0 + lane < cnt) v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
        }
        if (lane < 4 && e0 + lane < k) list_scores[((long)i * k + e0 + lane) * m + j] = v;
    }
}

// ------------------------------------------------------------------------ launchers ----
int launch_fusion_fuse(const FusionArgs& a, int n, hipStream_t st) {
    REVO_REQUIRE(a.m >= 1 && a.m <= FUSION_MAX_LISTS && a.C >= 1 && a.C <= LARGE_K_MAX && a.m * a.C <= FUSION_MAX_KEYS &&
                     a.k >= 1 && a.k <= LARGE_K_MAX && (a.method == 0 || a.method == 1),
                 "fusion: 1 <= lists <= 64, 1 <= limit <= 1024, lists * limit <= 8192, 1 <= k <= 1024, method 0 or 1");
    if (n <= 0) return 0;
    int P = 64;
    while (P < a.m * a.C) P <<= 1;
    const int threads = P / 2 < 64 ? 64 : (P / 2 > 1024 ? 1024 : P / 2);
    REVO_FUNC_LDS(fusion_fuse_kernel, FUSION_MAX_KEYS * 16);
    hipLaunchKernelGGL(fusion_fuse_kernel, dim3((unsigned)n), dim3((unsigned)threads), (size_t)P * 16, st, a, P);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_fusion_list_scores(const float* Qf, long ldq, const float* Gf, long ldg, int D, const long long* out_idx,
                              const int* out_counts, long idx_offset, int n, int m, int k, float* list_scores, hipStream_t st) {
    REVO_REQUIRE(D % 4 == 0 && ldq % 4 == 0 && ldg % 4 == 0, "fusion: D must be a multiple of 4");
    if (n <= 0) return 0;
    REVO_REQUIRE((long)n * m < (1l << 31), "fusion: too many lists in one call");
    hipLaunchKernelGGL(fusion_list_scores_kernel, dim3((unsigned)((long)n * m)), dim3(256), 0, st, Qf, ldq, Gf, ldg, D, out_idx,
                       out_counts, idx_offset, m, k, list_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
