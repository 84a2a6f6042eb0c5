// Multi-vector search (revo_search_maxsim, include/revo.h): n query vectors against the GROUPS of the
// gallery's rows (revo_search_set_groups).  With s(i, r) the fp32 score of query vector i against row r, A(G) the allowed
// rows of group G and M_i(G) = max of s(i, r) over A(G),  score(G) = (((M_0 + M_1) + M_2) + ...) + M_{n-1}; the best k
// groups by (score desc, group id asc).  e_i is the certificate's bound of |bf16 score - fp32 score| for vector i
// (cert_eps, kernels.h), m_i(G) the max of the bf16 scan scores over A(G): |M_i - m_i| <= e_i.
//
//   index    once per set of group ids: keys (group << 32) | row sorted -> CSR of the distinct ids (ascending) and their rows
//   pass     RECOMMEND's 64-row form of the 256 x 256 main loop with A = the query vectors; the epilogue stores the bf16
//            scan score of every (allowed row, vector) into S[N][n_pad]
//   bounds   one wave per group: m_i over the group's allowed rows, a = sum m_i, lb / ub = a -+ (sum e_i + rounding slack)
//   level    tau = the k-th largest lb over ALL groups (recommend_level_kernel), raised to the threshold if there is one:
//            k groups score at least tau, so every group of the answer has ub >= tau
//   select   the groups with ub >= tau and an allowed row; their allowed rows are the candidate rows
//   rescore  one wave per (candidate row, four query vectors): the fp32 chains (pairs_dot4) overwrite the row's slots in S
//   reduce   one wave per candidate group: M_i with the lowest-row tie rule, the ordered sum, the threshold cut; kept as
//            (~order-preserving score << 32) | dense group position (ascending in the group id)
//   sort     radix_sort.hip over those keys: (score desc, group id asc)
//   emit     the first k; M_i and its row are reduced once more from S for those k groups only
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"

namespace revo {

constexpr uint64_t MAXSIM_NO_KEY = ~0ull;          // key of a row without a group: sorts behind every group
constexpr uint32_t MAXSIM_NO_ROW = 0xffffffffu;

// -------------------------------------------------------------------------- index ----
__global__ __launch_bounds__(256) void maxsim_keys_kernel(const int32_t* __restrict__ groups, long N, uint64_t* __restrict__ keys) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int32_t gr = groups[r];
    keys[r] = gr >= 0 ? ((uint64_t)(uint32_t)gr << 32) | (uint64_t)r : MAXSIM_NO_KEY;
}
// flags[i] = 1 where sorted key i starts a group
__global__ __launch_bounds__(256) void maxsim_heads_kernel(const uint64_t* __restrict__ keys, long N,
                                                           unsigned long long* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = keys[i];
    flags[i] = (key != MAXSIM_NO_KEY && (i == 0 || (keys[i - 1] >> 32) != (key >> 32))) ? 1ull : 0ull;
}
// sums: the inclusive prefix sums of the flags.  Position i of the sorted keys belongs to dense group sums[i] - 1.
// meta[0] = groups, meta[1] = grouped rows (both stay 0 when no row has a group).
__global__ __launch_bounds__(256) void maxsim_csr_kernel(const uint64_t* __restrict__ keys, const unsigned long long* __restrict__ sums,
                                                         long N, int32_t* __restrict__ gid, uint32_t* __restrict__ off,
                                                         uint32_t* __restrict__ rows, uint32_t* __restrict__ pos_group,
                                                         unsigned long long* __restrict__ meta) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = keys[i];
    if (key == MAXSIM_NO_KEY) return;
    const uint32_t p = (uint32_t)(sums[i] - 1ull);
    rows[i] = (uint32_t)key;
    pos_group[i] = p;
    if (i == 0 || (keys[i - 1] >> 32) != (key >> 32)) { gid[p] = (int32_t)(key >> 32); off[p] = (uint32_t)i; }
    if (i == N - 1 || keys[i + 1] == MAXSIM_NO_KEY) {
        off[p + 1] = (uint32_t)(i + 1);
        meta[0] = (unsigned long long)p + 1ull; meta[1] = (unsigned long long)(i + 1);
    }
}

// --------------------------------------------------------------------------- pass ----
// Workgroup s takes slice s of the gallery tiles [0, ceil(N / 256)).  Waves 0..3 hold every query vector of their 64 columns
// (gemm256_mainloop<64>: the second wave-row computes nothing), waves 4..7 only move data.  acc[m][n][j] of lane (lr, lq) is
// vector m * 16 + lr against column n * 16 + lq * 4 + j: the 16 lanes of a DPP row store 64 consecutive bytes of one S row.
__global__ __launch_bounds__(G256_THREADS, 2) void maxsim_pass_kernel(MaxsimPassArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nsl = (int)gridDim.x, sl = (int)blockIdx.x;
    int t0, t1;
    if (!tile_slice((int)((p.N + 255) / 256), nsl, sl, t0, t1)) return;

    G256Operand A;
    g256_operand_init(A, p.Qb, p.ldq, p.n, 0, wave, lane);
    tile_slice_frame<64, true, 2>(A, p.Gb, p.ldg, p.N, t0, t1, smem, p.D, wave, lane, [&](long n0, int lane, const f32x4 (&acc)[8][4]) {
        if (wave >= 4) return;                              // no query vectors in the second wave-row
        const int lr = lane & 15, lq = lane >> 4;
        const int cw = wave * 64;                           // the wave's 64 columns: bits of one 64-bit word of the bitmap
        const uint64_t fm = tile_column_mask(p.N, n0, cw, p.allow);
        if (fm == 0ull) return;                             // wave-uniform: no allowed column inside the gallery
        // bit c of fm set: row n0 + cw + c is below N (and allowed), so its S row exists; v < n_pad: the slot exists
        float* srow = p.S + (n0 + cw + lq * 4) * (long)p.n_pad + lr;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (m * 16 >= p.n_pad) continue;                // wave-uniform
            if (m * 16 + lr >= p.n_pad) continue;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((fm >> (n * 16 + lq * 4 + j)) & 1ull) srow[(long)(n * 16 + j) * p.n_pad + m * 16] = acc[m][n][j];
        }
    });
}

// ------------------------------------------------------------------ group reduction ----
// One wave reduces the rows [j0, j1) of a group (CSR positions; rows ascending): W = n_pad rounded up to a power of two
// lanes per row, 64 / W rows at a time.  Lane l works on vector i = l & (W - 1).  Returns, in EVERY lane with i < n, the
// largest S[row][i] over the allowed rows (fp32 comparison, -0 equal to +0; among equal values the lowest row, with that
// row's own bits) and the row; `allowed` = the group's allowed rows (every lane).  No allowed row: MAXSIM_NO_ROW.
__device__ __forceinline__ void maxsim_group_max(const MaxsimGroupArgs& a, uint32_t j0, uint32_t j1, int lane, float& best,
                                                 uint32_t& brow, uint32_t& allowed) {
    const int W = a.lanes, i = lane & (W - 1), sub = lane / W, R = 64 / W;
    best = -INFINITY; brow = MAXSIM_NO_ROW; allowed = 0u;
    for (uint32_t j = j0 + (uint32_t)sub; j < j1; j += (uint32_t)R) {
        const uint32_t r = a.rows[j];
        if (a.allow && !((a.allow[r >> 5] >> (r & 31u)) & 1u)) continue;
        ++allowed;
        if (i < a.n) {
            const float s = a.S[(long)r * a.n_pad + i];
            if (brow == MAXSIM_NO_ROW || s > best) { best = s; brow = r; }
        }
    }
    for (int o = W; o < 64; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const uint32_t orow = __shfl_xor(brow, o, 64);
        allowed += __shfl_xor(allowed, o, 64);
        if (orow != MAXSIM_NO_ROW && (brow == MAXSIM_NO_ROW || ov > best || (ov == best && orow < brow))) { best = ov; brow = orow; }
    }
}

// ------------------------------------------------------------------------- bounds ----
// Wave w takes groups w, w + waves, ...  With a = sum m_i, A1 = sum |m_i| and E = sum e_i (wave_sum's tree, fp32):
//   |score(G) - a| <= E + g (A1 + E) + g A1,  g = (n - 1) 2^-24 (1 + tiny): the rounding of the contract's ordered sum of the
// M_i (|M_i| <= |m_i| + e_i) and of the sum of the m_i.  T below exceeds that (n 2^-22 instead of 2 g; the 1.001 absorbs the
// rounding of E and A1 themselves), and lb / ub are then moved outward past the rounding of a -+ T (score_down / score_up).
__global__ __launch_bounds__(256) void maxsim_bounds_kernel(MaxsimGroupArgs a, float* __restrict__ lb, float* __restrict__ ub,
                                                            uint32_t* __restrict__ acnt, unsigned long long* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const bool mine = lane < a.n;                           // lanes 0 .. n - 1: sub 0, vector = lane (W >= n)
    const float e = mine ? cert_eps(a.qstat[lane * 2], a.qstat[lane * 2 + 1], __uint_as_float(a.gstat[0]),
                                    __uint_as_float(a.gstat[1]), a.D) : 0.f;
    const float E = wave_sum(e);
    unsigned long long live = 0ull;                         // wave-uniform: groups with an allowed row this wave has met
    for (long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.G; p += waves) {
        float best; uint32_t brow, allowed;
        maxsim_group_max(a, a.off[p], a.off[p + 1], lane, best, brow, allowed);
        const float m = (mine && allowed > 0u) ? best : 0.f;
        const float s = wave_sum(m), A1 = wave_sum(fabsf(m));
        const float T = E * 1.001f + (float)a.n * 2.4e-7f * (A1 + E) + 1e-30f;
        float lo = score_down(s - T, fabsf(s) + T), hi = score_up(s + T, fabsf(s) + T);
        if (allowed == 0u) { lo = -INFINITY; hi = -INFINITY; }
        else ++live;
        if (lane == 0) {
            lb[p] = lo == lo ? lo : -INFINITY;              // (a NaN bound -- non-finite rows -- never raises the level ...
            ub[p] = hi;                                     //  ... and keeps the group: the select tests !(ub < tau))
            acnt[p] = allowed;
        }
    }
    if (lane == 0 && live != 0ull) atomicAdd(cnt + 2, live);
}

// ------------------------------------------------------------------------- select ----
// Over the CSR positions: the allowed rows of the groups with an allowed row and ub >= tau are the candidate rows (cnt[0]);
// each such group is appended once, by its first position (cnt[3]).
__global__ __launch_bounds__(256) void maxsim_select_kernel(MaxsimGroupArgs a, long n_grouped, const uint32_t* __restrict__ pos_group,
                                                            const float* __restrict__ ub, const uint32_t* __restrict__ acnt,
                                                            const float* __restrict__ tau, unsigned long long* __restrict__ cnt,
                                                            uint32_t* __restrict__ crows, uint32_t* __restrict__ cgroups) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lanes_below(lane);
    const float level = tau[0];
    const long stride = (long)gridDim.x * 256;
    const long rounds = (n_grouped + stride - 1) / stride;
    for (long it = 0; it < rounds; ++it) {
        const long j = it * stride + (long)blockIdx.x * 256 + threadIdx.x;
        bool take_row = false, take_group = false;
        uint32_t r = 0u, p = 0u;
        if (j < n_grouped) {
            p = pos_group[j];
            if (acnt[p] > 0u && !(ub[p] < level)) {
                r = a.rows[j];
                take_row = !a.allow || ((a.allow[r >> 5] >> (r & 31u)) & 1u);
                take_group = (uint32_t)j == a.off[p];
            }
        }
        const unsigned long long mr = __ballot(take_row);
        if (mr != 0ull) {
            const unsigned long long pos = wave_append(mr, cnt, lane, below);
            if (take_row) crows[pos] = r;
        }
        const unsigned long long mg = __ballot(take_group);
        if (mg != 0ull) {
            const unsigned long long pos = wave_append(mg, cnt + 3, lane, below);
            if (take_group) cgroups[pos] = p;
        }
    }
}

// ------------------------------------------------------------------------ rescore ----
// Item (c, b): candidate row c against query vectors 4 b .. 4 b + 3 (pairs_dot4: every score keeps its own chain, the bits
// every other search gives it); the four scores replace the row's bf16 scan scores in S (slots past n repeat vector n - 1).
__global__ __launch_bounds__(256) void maxsim_rescore_kernel(const uint32_t* __restrict__ crows, long n_rows, const float* __restrict__ Qf,
                                                             long ldq, int n, int n_pad, const float* __restrict__ Gf, long ldg, int D,
                                                             float* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const int nb = n_pad / 4;
    const long items = n_rows * nb;
    for (long it = (long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += waves) {
        const long c = it / nb;
        const int b = (int)(it - c * nb);
        const uint32_t row = crows[c];
        const float* gp = Gf + (long)row * ldg;
        const float* gr[4] = {gp, gp, gp, gp};
        const float* qr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) qr[u] = Qf + (long)(b * 4 + u < n ? b * 4 + u : n - 1) * ldq;
        float t[4];
        pairs_dot4(qr, gr, D, lane, t);
        if (lane == 0) *(f32x4*)(S + (long)row * n_pad + b * 4) = (f32x4){t[0], t[1], t[2], t[3]};
    }
}

// ------------------------------------------------------------------------- reduce ----
// Wave w takes candidate groups w, w + waves, ...: M_i from the re-scored slots, the contract's ordered sum, the threshold
// cut.  The key orders -0 with +0 (equal scores: the dense group position, ascending in the group id, decides).
__global__ __launch_bounds__(256) void maxsim_reduce_kernel(MaxsimGroupArgs a, const uint32_t* __restrict__ cgroups, long n_groups,
                                                            int has_thr, float thr, unsigned long long* __restrict__ kept,
                                                            uint64_t* __restrict__ out_keys, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6); c < n_groups; c += waves) {
        const uint32_t p = cgroups[c];
        float best; uint32_t brow, allowed;
        maxsim_group_max(a, a.off[p], a.off[p + 1], lane, best, brow, allowed);
        float v = __shfl(best, 0, 64);
        for (int i = 1; i < a.n; ++i) v = __fadd_rn(v, __shfl(best, i, 64));
        if (has_thr && !(v >= thr)) continue;               // wave-uniform
        if (lane == 0) {
            const unsigned long long pos = atomicAdd(kept, 1ull);
            const float vk = v == 0.f ? 0.f : v;
            out_keys[pos] = ((uint64_t)(~f32_orderable(vk)) << 32) | (uint64_t)p;
            out_scores[pos] = v;
        }
    }
}

// --------------------------------------------------------------------------- emit ----
// Wave i < k: sorted entry i -> scores, group_ids, and (optional) M_v / its lowest attaining row + idx_offset per query
// vector, reduced once more from S; entries past n_kept are padding (-inf, -1, -inf, -1).  counts[0] = min(n_kept, k).
__global__ __launch_bounds__(256) void maxsim_emit_kernel(MaxsimGroupArgs a, const uint64_t* __restrict__ keys,
                                                          const float* __restrict__ vals, long n_kept, int k, int n_vec,
                                                          long idx_offset, float* __restrict__ scores, int32_t* __restrict__ group_ids,
                                                          int32_t* __restrict__ counts, float* __restrict__ part_scores,
                                                          long long* __restrict__ part_rows) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i == 0 && lane == 0) counts[0] = (int32_t)(n_kept < k ? n_kept : k);
    if (i >= k) return;
    if (i < n_kept) {
        const uint32_t p = (uint32_t)keys[i];
        if (lane == 0) { scores[i] = vals[i]; group_ids[i] = a.gid[p]; }
        if (!part_scores && !part_rows) return;
        float best; uint32_t brow, allowed;
        maxsim_group_max(a, a.off[p], a.off[p + 1], lane, best, brow, allowed);
        if (lane < n_vec) {
            if (part_scores) part_scores[(long)i * n_vec + lane] = best;
            if (part_rows) part_rows[(long)i * n_vec + lane] = (long long)brow + idx_offset;
        }
    } else {
        if (lane == 0) { scores[i] = -INFINITY; group_ids[i] = -1; }
        if (lane < n_vec) {
            if (part_scores) part_scores[(long)i * n_vec + lane] = -INFINITY;
            if (part_rows) part_rows[(long)i * n_vec + lane] = -1;
        }
    }
}

// ------------------------------------------------------------------------ launchers ----
int maxsim_group_lanes(int n_pad) {
    int w = 4;
    while (w < n_pad) w <<= 1;
    return w;
}
int launch_maxsim_index(const int32_t* groups, long N, uint64_t* keys, uint64_t* keys_alt, float* vals, float* vals_alt,
                        uint32_t* hist, unsigned long long* flags, unsigned long long* meta, int32_t* gid, uint32_t* off,
                        uint32_t* rows, uint32_t* pos_group, hipStream_t st) {
    REVO_REQUIRE(N >= 1 && N < (1ll << 32), "search_maxsim: row indices must fit in 32 bits");
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    REVO_HIP_CHECK(hipMemsetAsync(meta, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(maxsim_keys_kernel, grid, block, 0, st, groups, N, keys);
    uint64_t* sk = nullptr; float* sv = nullptr;
    if (int rc = launch_sort_keys_u64(keys, vals, keys_alt, vals_alt, N, 64, hist, &sk, &sv, st)) return rc;
    hipLaunchKernelGGL(maxsim_heads_kernel, grid, block, 0, st, sk, N, flags);
    if (int rc = launch_inclusive_sums_u64(flags, N, st)) return rc;
    hipLaunchKernelGGL(maxsim_csr_kernel, grid, block, 0, st, sk, flags, N, gid, off, rows, pos_group, meta);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_maxsim_pass(const MaxsimPassArgs& a, hipStream_t st) {
    if (int rc = g256_check_operands("search_maxsim", a.D, a.ldg, a.ldq)) return rc;
    REVO_REQUIRE(a.N < (1ll << 32), "search_maxsim: row indices must fit in 32 bits");
    REVO_REQUIRE(a.n >= 1 && a.n <= MAXSIM_MAX_VECTORS && a.n_pad == (a.n + 3) / 4 * 4, "search_maxsim: bad vector count");
    if (a.N <= 0) return 0;
    const long tiles = (a.N + 255) / 256;
    REVO_FUNC_LDS(maxsim_pass_kernel, G256_LDS);
    hipLaunchKernelGGL(maxsim_pass_kernel, dim3((unsigned)pass256_slices(tiles)), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
static unsigned maxsim_wave_blocks(long waves) {
    const long blocks = (waves + 3) / 4;
    return (unsigned)(blocks < 1 ? 1 : (blocks < 8192 ? blocks : 8192));
}
int launch_maxsim_bounds(const MaxsimGroupArgs& a, float* lb, float* ub, uint32_t* acnt, unsigned long long* cnt, hipStream_t st) {
    REVO_REQUIRE(a.lanes == maxsim_group_lanes(a.n_pad) && a.n <= a.n_pad && a.n_pad <= 64, "search_maxsim: bad lane geometry");
    if (a.G <= 0) return 0;
    hipLaunchKernelGGL(maxsim_bounds_kernel, dim3(maxsim_wave_blocks(a.G)), dim3(256), 0, st, a, lb, ub, acnt, cnt);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_maxsim_select(const MaxsimGroupArgs& a, long n_grouped, const uint32_t* pos_group, const float* ub, const uint32_t* acnt,
                         const float* tau, unsigned long long* cnt, uint32_t* crows, uint32_t* cgroups, hipStream_t st) {
    if (n_grouped <= 0) return 0;
    const long blocks = (n_grouped + 255) / 256;
    hipLaunchKernelGGL(maxsim_select_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a, n_grouped, pos_group,
                       ub, acnt, tau, cnt, crows, cgroups);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_maxsim_rescore(const uint32_t* crows, long n_rows, const float* Qf, long ldq, int n, int n_pad, const float* Gf, long ldg,
                          int D, float* S, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(maxsim_rescore_kernel, dim3(maxsim_wave_blocks(n_rows * (n_pad / 4))), dim3(256), 0, st, crows, n_rows, Qf, ldq,
                       n, n_pad, Gf, ldg, D, S);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_maxsim_reduce(const MaxsimGroupArgs& a, const uint32_t* cgroups, long n_groups, int has_thr, float thr,
                         unsigned long long* kept, uint64_t* out_keys, float* out_scores, hipStream_t st) {
    if (n_groups <= 0) return 0;
    hipLaunchKernelGGL(maxsim_reduce_kernel, dim3(maxsim_wave_blocks(n_groups)), dim3(256), 0, st, a, cgroups, n_groups, has_thr, thr,
                       kept, out_keys, out_scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_maxsim_emit(const MaxsimGroupArgs& a, const uint64_t* keys, const float* vals, long n_kept, int k, int n_vec,
                       long idx_offset, float* scores, int32_t* group_ids, int32_t* counts, float* part_scores, long long* part_rows,
                       hipStream_t st) {
    hipLaunchKernelGGL(maxsim_emit_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, a, keys, vals, n_kept, k, n_vec, idx_offset,
                       scores, group_ids, counts, part_scores, part_rows);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
