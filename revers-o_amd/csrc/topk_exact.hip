// The fallback behind the search's exactness certificate (kernels.h): what makes
// "the top-k of an exhaustive fp32 scoring of the gallery" (the reference's brute-force  G @ q ; argsort,
// core_system.py:659-664 -> qdrant local mode) a guarantee and not a likelihood of the bf16 scan.
//
//   finish (topk.hip)     re-scores the scan's ksel candidates in fp32 and checks the certificate; a query that fails
//                         it becomes entry j of the fallback workspace (query index, collect bound, bf16 query row)
//   collect (topk256.hip) one more MFMA pass over the gallery for those entries: every row whose bf16 score reaches
//                         the bound is appended to the entry's list
//   exact_finish          fp32 re-score of every collected row, running best-64 list, the entry's k results; an entry
//                         whose list overflowed is passed on
//   bruteforce            for those: the fp32 score of EVERY row of the gallery (the same fma chain as every other
//                         re-score), per-wave best-64 lists, merged per slice; bruteforce_final merges the slices
//
// Every launch is sized for the worst case and reads the entry count from device memory: workgroups past it exit, so a
// search in which every query is certified pays four empty launches and no host round trip.
#include "kernels.h"
#include "topk_util.h"

namespace revo {

// write one entry's results: `run` = its best keys (fp32 score, row), best first, 0 = empty
__device__ __forceinline__ void exact_write(uint64_t run, int lane, long orow, int k, int has_thr, float thr,
                                            long idx_offset, float* __restrict__ out_scores,
                                            long long* __restrict__ out_idx, int* __restrict__ out_counts) {
    const bool ok = run != 0ull && lane < k && (!has_thr || key_score(run) >= thr);
    const int cnt = __popcll(__ballot(ok));
    if (lane < k) {
        out_scores[orow * k + lane] = ok ? key_score(run) : -INFINITY;
        out_idx[orow * k + lane] = ok ? (long long)key_index(run) + idx_offset : -1ll;
    }
    if (lane == 0) out_counts[orow] = cnt;
}

// ------------------------------------------------------------ exact finish ----
// One workgroup of four waves per entry.  Wave w takes the 64-key chunks w, w + 4, ... of the entry's collect
// list, re-scores them (exact_dot4: four rows in flight) and folds them into its best-64 list; the four lists meet in
// LDS.  The collect list holds every row that can be in the result, each exactly once.
constexpr int XF_WAVES = 4;
__global__ __launch_bounds__(XF_WAVES * 64) void topk_exact_finish_kernel(ExactWs ws, const float* __restrict__ Qf, long ldqf,
                                                                          const float* __restrict__ Gf, long ldgf, int D,
                                                                          int k, int has_thr, float thr, long idx_offset,
                                                                          int force_bruteforce, int out_compact,
                                                                          float* __restrict__ out_scores,
                                                                          long long* __restrict__ out_idx,
                                                                          int* __restrict__ out_counts) {
    __shared__ uint64_t partial[XF_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // entries 0 .. nfront - 1 were filled by the collect pass, cap - 1 .. cap - ctr[CTR_FROM_SEGS] by the finish step from the
    // scan's segments
    const int nfront = ws.ctr[CTR_UNCERTIFIED], entries = nfront + ws.ctr[CTR_FROM_SEGS];
    for (int jj = blockIdx.x; jj < entries; jj += gridDim.x) {
    const int j = jj < nfront ? jj : ws.cap - 1 - (jj - nfront);
    const int n = ws.col_cnt[j];
    if (n > EXACT_COL_CAP || force_bruteforce) {
        if (threadIdx.x == 0) ws.over_j[atomicAdd(ws.ctr + CTR_BRUTEFORCE, 1)] = j;
        continue;
    }
    if (threadIdx.x == 0) atomicAdd(ws.ctr + CTR_COLLECTED, n);
    const int q = ws.unc_q[j];
    const float* qr = Qf + (long)q * ldqf;
    const uint64_t* col = ws.col + (long)j * EXACT_COL_CAP;
    uint64_t run = 0ull;
    for (int c0 = w * 64; c0 < n; c0 += XF_WAVES * 64) {
        const int m = (n - c0) < 64 ? (n - c0) : 64;
        const uint64_t key = lane < m ? col[c0 + lane] : 0ull;
        const uint32_t idx = key_index(key);
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
                if (lane == e0 + u && e0 + u < m) score = t[u];
        }
        run = wave_fold_best64(run, lane < m ? make_key(score, idx) : 0ull, lane);
    }
    partial[w][lane] = run;
    __syncthreads();
    if (w == 0) {
#pragma unroll 1
        for (int o = 1; o < XF_WAVES; ++o) {
            const uint64_t rev = partial[o][63 - lane];
            run = wave_bitonic_merge_desc(run > rev ? run : rev, lane);
        }
        exact_write(run, lane, out_compact ? (long)ws.orow[j] : (long)q, k, has_thr, thr, idx_offset, out_scores, out_idx, out_counts);
    }
    __syncthreads();                           // `partial` is reused by the next entry
    }
}
int launch_topk_exact_finish(const ExactWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf,
                             int D, int k, int has_thr, float thr, long idx_offset, int force_bruteforce, int out_compact,
                             float* out_scores, long long* out_idx, int* out_counts, hipStream_t st) {
    if (max_entries <= 0) return 0;
    REVO_REQUIRE(Gf && k >= 1 && k <= 64, "exact finish: needs the fp32 master rows and 1 <= k <= 64");
    // a bounded launch whatever the search's size (workgroups stride over the entries): an idle pass costs microseconds
    hipLaunchKernelGGL(topk_exact_finish_kernel, dim3((unsigned)(max_entries < 2048 ? max_entries : 2048)), dim3(XF_WAVES * 64), 0, st, ws, Qf, ldqf, Gf,
                       ldgf, D, k, has_thr, thr, idx_offset, force_bruteforce, out_compact, out_scores, out_idx, out_counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------- brute force ----
// grid (EXACT_L3_SLICES, up to 64); workgroup (s, y) scores slice s of the gallery for overflowed entries y, y + 64, ...
// 16 waves per workgroup, four rows per wave in flight (16 KB per wave: the pass runs at the rate a CU can pull HBM);
// each wave keeps its best 64 (score, row) keys sorted in one register per lane and inserts a row only if it beats
// the 64th.  The slice's 16 lists meet in LDS; its best 64 go to slot s of the entry's (now useless) collect buffer.
constexpr int BF_WAVES = 16;
// Grouped search (GroupWs, kernels.h): `run` holds keys best first (0 = empty), `grp` each key's group (-1 = empty).
// Insert `key` of group `gr` (>= 0) keeping at most `cap` keys per group: a group that already holds `cap` keys gives up
// its worst one if `key` beats it, otherwise the list's last entry is dropped if `key` beats it.  Wave-uniform arguments.
__device__ __forceinline__ void group_insert(uint64_t& run, int& grp, uint64_t key, int gr, int cap, int lane) {
    const uint64_t m = __ballot(grp == gr);
    const int e = __popcll(m) < cap ? 63 : 63 - __clzll(m);           // the entry that leaves (or is overtaken)
    if (key <= readlane_u64(run, e)) return;
    const int pos = __popcll(__ballot(run > key));                     // <= e: run[e] < key
    const uint64_t prev = shfl_up1_u64(run);
    const int prevg = __shfl_up(grp, 1, 64);
    if (lane >= pos && lane <= e) { run = lane == pos ? key : prev; grp = lane == pos ? gr : prevg; }
}
// fold another such list (best first) into run/grp.  Once one of its keys cannot enter, none of the later ones can
// (they are smaller, and the last entry of run only grows).
__device__ __forceinline__ void group_fold(uint64_t& run, int& grp, uint64_t other, int other_grp, int cap, int lane) {
#pragma unroll 1
    for (int t = 0; t < 64; ++t) {
        const uint64_t key = readlane_u64(other, t);
        if (key <= readlane_u64(run, 63)) break;
        group_insert(run, grp, key, __builtin_amdgcn_readlane(other_grp, t), cap, lane);
    }
}
__device__ __forceinline__ int group_of_key(const int* __restrict__ group_of_row, uint64_t key) {
    return key ? group_of_row[key_index(key)] : -1;
}

// FILTER: rows whose allow-bit is clear are skipped (the test is wave-uniform: one row per step of the insertion).
// GROUP: the grouped fallback's entries (ws.ctr[CTR_GROUPED], gw.gq) instead of the overflowed ones.  Pass A (gw.hits == 0) keeps
// the best 64 GROUPS, each with its best key; pass B (gw.hits = group_size) only the rows of the entry's chosen groups, at
// most gw.hits per group.  Rows of no group and rows below the threshold never enter.
template <bool FILTER, bool GROUP>
__device__ __forceinline__ void bruteforce_body(const ExactWs& ws, const float* __restrict__ Qf, long ldqf,
                                                const float* __restrict__ Gf, long ldgf, long N, int D,
                                                const uint32_t* __restrict__ allow, const GroupWs& gw) {
    __shared__ uint64_t partial[BF_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int over = GROUP ? ws.ctr[CTR_GROUPED] : ws.ctr[CTR_BRUTEFORCE];
    for (int i = blockIdx.y; i < over; i += gridDim.y) {
    const int j = GROUP ? i : ws.over_j[i];
    const float* qr = Qf + (long)(GROUP ? gw.gq[i] : ws.unc_q[j]) * ldqf;
    const long per = (N + EXACT_L3_SLICES - 1) / EXACT_L3_SLICES;
    const long r0 = (long)blockIdx.x * per;
    const long r1 = r0 + per < N ? r0 + per : N;
    uint64_t run = 0ull;                       // lane l: the wave's (l+1)-th best key so far
    int grp = -1, chosen = -1, cap = 1;        // GROUP: run's groups; pass B: lane l holds the entry's l-th chosen group
    if constexpr (GROUP) {
        if (gw.hits) { chosen = gw.chosen[(long)i * 64 + lane]; cap = gw.hits; }
    }
    for (long r = r0 + (long)w * 4; r < r1; r += BF_WAVES * 4) {
        int gu[4];                             // GROUP: the rows' groups, -1 = the row cannot enter
        if constexpr (GROUP) {
            bool any = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int gr = r + u < r1 ? __builtin_amdgcn_readfirstlane(gw.group_of_row[r + u]) : -1;
                if (gr >= 0 && gw.hits && __ballot(chosen == gr) == 0ull) gr = -1;
                gu[u] = gr;
                any = any || gr >= 0;
            }
            if (!any) continue;                // nothing to score: pass B reads only the chosen groups' rows
        }
        const float* gr[4];
        float t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) gr[u] = Gf + (r + u < r1 ? r + u : r1 - 1) * ldgf;
        exact_dot4(qr, gr, D, lane, t);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + u >= r1) break;                                        // wave-uniform
            if constexpr (FILTER) { if (!((allow[(r + u) >> 5] >> ((r + u) & 31)) & 1u)) continue; }   // wave-uniform
            const uint64_t key = make_key(t[u], (uint32_t)(r + u));       // wave-uniform value
            if constexpr (GROUP) {
                if (gu[u] < 0 || (gw.has_thr && !(t[u] >= gw.thr))) continue;
                group_insert(run, grp, key, gu[u], cap, lane);
                continue;
            }
            const uint64_t worst = readlane_u64(run, 63);
            if (key <= worst) continue;
            const int pos = __popcll(__ballot(run > key));                 // entries that stay ahead of it
            const uint64_t prev = shfl_up1_u64(run);
            run = lane < pos ? run : (lane == pos ? key : prev);
        }
    }
    partial[w][lane] = run;
    __syncthreads();
    if (w == 0) {
#pragma unroll 1
        for (int o = 1; o < BF_WAVES; ++o) {
            if constexpr (GROUP) {
                const uint64_t other = partial[o][lane];
                group_fold(run, grp, other, group_of_key(gw.group_of_row, other), cap, lane);
            } else {
                const uint64_t rev = partial[o][63 - lane];
                run = wave_bitonic_merge_desc(run > rev ? run : rev, lane);
            }
        }
        ws.col[(long)j * EXACT_COL_CAP + (long)blockIdx.x * 64 + lane] = run;
    }
    __syncthreads();
    }
}
__global__ __launch_bounds__(BF_WAVES * 64) void topk_exact_bruteforce_kernel(ExactWs ws, const float* __restrict__ Qf,
                                                                              long ldqf, const float* __restrict__ Gf,
                                                                              long ldgf, long N, int D) {
    bruteforce_body<false, false>(ws, Qf, ldqf, Gf, ldgf, N, D, nullptr, GroupWs{});
}
__global__ __launch_bounds__(BF_WAVES * 64) void topk_exact_bruteforce_filtered_kernel(ExactWs ws, const float* __restrict__ Qf,
                                                                                       long ldqf, const float* __restrict__ Gf,
                                                                                       long ldgf, long N, int D,
                                                                                       const uint32_t* __restrict__ allow) {
    bruteforce_body<true, false>(ws, Qf, ldqf, Gf, ldgf, N, D, allow, GroupWs{});
}
// one wave per overflowed entry: merge the slices' lists, write the results
__global__ __launch_bounds__(256) void topk_exact_bruteforce_final_kernel(ExactWs ws, int k, int has_thr, float thr,
                                                                          long idx_offset, int out_compact,
                                                                          float* __restrict__ out_scores,
                                                                          long long* __restrict__ out_idx,
                                                                          int* __restrict__ out_counts) {
    const int lane = threadIdx.x & 63;
    const int over = ws.ctr[CTR_BRUTEFORCE];
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < over; i += gridDim.x * 4) {
    const int j = ws.over_j[i];
    const uint64_t* lists = ws.col + (long)j * EXACT_COL_CAP;
    uint64_t run = lists[lane];
#pragma unroll 1
    for (int s = 1; s < EXACT_L3_SLICES; ++s) {
        const uint64_t rev = lists[s * 64 + 63 - lane];
        run = wave_bitonic_merge_desc(run > rev ? run : rev, lane);
    }
    exact_write(run, lane, out_compact ? (long)ws.orow[j] : (long)ws.unc_q[j], k, has_thr, thr, idx_offset, out_scores, out_idx,
                out_counts);
    }
}
int launch_topk_exact_bruteforce(const ExactWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf,
                                 long N, int D, int k, int has_thr, float thr, long idx_offset, int out_compact,
                                 float* out_scores, long long* out_idx, int* out_counts, hipStream_t st,
                                 const uint32_t* allow) {
    if (max_entries <= 0 || N <= 0) return 0;
    REVO_REQUIRE(Gf && k >= 1 && k <= 64 && N < (1ll << 32), "exact brute force: needs the fp32 master rows, 1 <= k <= 64, N < 2^32");
    const int ny = max_entries < 64 ? max_entries : 64;
    if (allow)
        hipLaunchKernelGGL(topk_exact_bruteforce_filtered_kernel, dim3(EXACT_L3_SLICES, (unsigned)ny), dim3(BF_WAVES * 64), 0,
                           st, ws, Qf, ldqf, Gf, ldgf, N, D, allow);
    else
        hipLaunchKernelGGL(topk_exact_bruteforce_kernel, dim3(EXACT_L3_SLICES, (unsigned)ny), dim3(BF_WAVES * 64), 0, st,
                           ws, Qf, ldqf, Gf, ldgf, N, D);
    hipLaunchKernelGGL(topk_exact_bruteforce_final_kernel, dim3((unsigned)((ny + 3) / 4)), dim3(256), 0, st, ws, k,
                       has_thr, thr, idx_offset, out_compact, out_scores, out_idx, out_counts);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------ grouped search ----
// (include/revo.h, revo_search_groups)  One wave writes one query's grouped result.  Lane l holds
// key (its hit, 0 = none), r / h (the hit's group rank and its rank within the group) and, for group rank l: gid_l (the
// group, -1 = none) and hc_l (hits of that group in the result, <= group_size); ngroups = groups in the result.
__device__ __forceinline__ void group_write(const GroupOut& o, long orow, uint64_t key, int r, int h, int gid_l, int hc_l,
                                            int ngroups, int lane) {
    const int L = o.limit, S = o.group_size;
    if (key != 0ull && r < L && h < S) {
        o.scores[(orow * L + r) * S + h] = key_score(key);
        o.idx[(orow * L + r) * S + h] = (long long)key_index(key) + o.idx_offset;
    }
    const int rr = lane / S, hh = lane - rr * S;        // the slot lane l pads if nobody holds it (L * S <= 50)
    const int hc = __shfl(hc_l, rr, 64);
    if (lane < L * S && hh >= hc) {
        o.scores[orow * L * S + lane] = -INFINITY;
        o.idx[orow * L * S + lane] = -1ll;
    }
    if (lane < L) {
        o.hit_counts[orow * L + lane] = hc_l;
        o.group_ids[orow * L + lane] = gid_l;
    }
    if (lane == 0) o.group_counts[orow] = ngroups;
}

// Fast path: one wave per query over the exact top-GROUP_K1 rows of the ungrouped search (lane i: entry i).  The first
// occurrence of each group is found with ballots; as the list is in key order, so are the groups' first occurrences.
// Certified: the list is complete (fewer than GROUP_K1 entries: every allowed row at or above the threshold is in it), or it
// holds >= limit groups and each of the first limit groups holds >= group_size of its entries (a row outside the list
// scores at most the last entry's score and, on a tie, has a larger index: it can neither found a group that outranks a
// listed group nor displace a listed hit).  Otherwise the query becomes an entry of the grouped fallback (ws.ctr[CTR_GROUPED]).
__global__ __launch_bounds__(256) void topk_group_select_kernel(const float* __restrict__ s1, const long long* __restrict__ i1,
                                                                const int* __restrict__ c1, int Q, ExactWs ws, GroupWs gw,
                                                                int force_fallback, GroupOut o) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int cnt = c1[q];
    const bool in = lane < cnt && lane < GROUP_K1;
    const long long row = in ? i1[(long)q * GROUP_K1 + lane] : -1ll;
    const int gid = in ? gw.group_of_row[row] : -1;
    const uint64_t key = gid >= 0 ? make_key(s1[(long)q * GROUP_K1 + lane], (uint32_t)row) : 0ull;
    const unsigned long long below = (1ull << lane) - 1ull;
    int r = 64, h = 0, gid_l = -1, hc_l = 0, it = 0;
    for (unsigned long long rem = __ballot(gid >= 0); rem != 0ull; ++it) {
        const int lead = __ffsll((long long)rem) - 1;
        const int g = __builtin_amdgcn_readlane(gid, lead);
        const unsigned long long m = __ballot(gid == g);
        if (gid == g) { r = it; h = __popcll(m & below); }
        if (lane == it) { gid_l = g; hc_l = __popcll(m); }
        rem &= ~m;
    }
    const int L = o.limit, S = o.group_size;
    const bool full_groups = it >= L && __ballot(lane < L && hc_l < S) == 0ull;
    if (force_fallback || (cnt >= GROUP_K1 && !full_groups)) {
        if (lane == 0) gw.gq[atomicAdd(ws.ctr + CTR_GROUPED, 1)] = q;
        return;
    }
    if (lane >= L) { gid_l = -1; hc_l = 0; }
    group_write(o, q, key, r, h, gid_l, hc_l < S ? hc_l : S, it < L ? it : L, lane);
}

// fallback, after the slices of a pass: merge entry i's 32 slice lists (deduplicated by group) and, pass A, record its
// chosen groups (and write the result if group_size == 1), pass B, write the result.  One wave per entry.
__global__ __launch_bounds__(256) void topk_group_final_kernel(ExactWs ws, GroupWs gw, GroupOut o) {
    const int lane = threadIdx.x & 63;
    const int over = ws.ctr[CTR_GROUPED];
    const int cap = gw.hits ? gw.hits : 1;
    const int L = o.limit;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < over; i += gridDim.x * 4) {
    const uint64_t* lists = ws.col + (long)i * EXACT_COL_CAP;
    uint64_t run = lists[lane];
    int grp = group_of_key(gw.group_of_row, run);
#pragma unroll 1
    for (int s = 1; s < EXACT_L3_SLICES; ++s) {
        const uint64_t other = lists[s * 64 + lane];
        group_fold(run, grp, other, group_of_key(gw.group_of_row, other), cap, lane);
    }
    const long orow = gw.gq[i];
    if (!gw.hits) {                                // pass A: lane l holds the l-th best group with its best row
        const bool has = run != 0ull && lane < L;
        gw.chosen[(long)i * 64 + lane] = has ? grp : -1;
        if (o.group_size == 1)
            group_write(o, orow, has ? run : 0ull, lane, 0, has ? grp : -1, has ? 1 : 0, __popcll(__ballot(has)), lane);
        continue;
    }
    // pass B: run holds each chosen group's best rows (at most group_size each, so at most 50 keys)
    const int chosen = gw.chosen[(long)i * 64 + lane];
    const unsigned long long below = (1ull << lane) - 1ull;
    int r = 64, h = 0, hc_l = 0, ng = 0;
#pragma unroll 1
    for (; ng < L; ++ng) {
        const int g = __builtin_amdgcn_readlane(chosen, ng);
        if (g < 0) break;
        const unsigned long long m = __ballot(run != 0ull && grp == g);
        if (run != 0ull && grp == g) { r = ng; h = __popcll(m & below); }
        if (lane == ng) hc_l = __popcll(m);
    }
    group_write(o, orow, run, r, h, lane < ng ? chosen : -1, hc_l, ng, lane);
    }
}

int launch_topk_group_select(const float* s1, const long long* i1, const int* c1, int Q, const ExactWs& ws, const GroupWs& gw,
                             int force_fallback, const GroupOut& o, hipStream_t st) {
    if (Q <= 0) return 0;
    hipLaunchKernelGGL(topk_group_select_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, s1, i1, c1, Q, ws, gw,
                       force_fallback, o);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
__global__ __launch_bounds__(BF_WAVES * 64) void topk_group_bruteforce_kernel(ExactWs ws, const float* __restrict__ Qf,
                                                                            long ldqf, const float* __restrict__ Gf, long ldgf,
                                                                            long N, int D, GroupWs gw) {
    bruteforce_body<false, true>(ws, Qf, ldqf, Gf, ldgf, N, D, nullptr, gw);
}
__global__ __launch_bounds__(BF_WAVES * 64) void topk_group_bruteforce_filtered_kernel(ExactWs ws, const float* __restrict__ Qf,
                                                                                     long ldqf, const float* __restrict__ Gf,
                                                                                     long ldgf, long N, int D,
                                                                                     const uint32_t* __restrict__ allow,
                                                                                     GroupWs gw) {
    bruteforce_body<true, true>(ws, Qf, ldqf, Gf, ldgf, N, D, allow, gw);
}
int launch_topk_group_fallback(const ExactWs& ws, GroupWs gw, int max_entries, const float* Qf, long ldqf, const float* Gf,
                               long ldgf, long N, int D, const uint32_t* allow, const GroupOut& o, hipStream_t st) {
    if (max_entries <= 0 || N <= 0) return 0;
    REVO_REQUIRE(Gf && N < (1ll << 32), "grouped fallback: needs the fp32 master rows and N < 2^32");
    REVO_REQUIRE(o.limit >= 1 && o.group_size >= 1 && o.limit * o.group_size <= GROUP_K1, "grouped fallback: bad limit / group_size");
    const int ny = max_entries < 64 ? max_entries : 64;
    // pass A: best groups; pass B (group_size > 1): the chosen groups' best rows
    for (int pass = 0; pass < (o.group_size > 1 ? 2 : 1); ++pass) {
        gw.hits = pass ? o.group_size : 0;
        if (allow)
            hipLaunchKernelGGL(topk_group_bruteforce_filtered_kernel, dim3(EXACT_L3_SLICES, (unsigned)ny), dim3(BF_WAVES * 64), 0,
                               st, ws, Qf, ldqf, Gf, ldgf, N, D, allow, gw);
        else
            hipLaunchKernelGGL(topk_group_bruteforce_kernel, dim3(EXACT_L3_SLICES, (unsigned)ny), dim3(BF_WAVES * 64), 0, st,
                               ws, Qf, ldqf, Gf, ldgf, N, D, gw);
        hipLaunchKernelGGL(topk_group_final_kernel, dim3((unsigned)((ny + 3) / 4)), dim3(256), 0, st, ws, gw, o);
        REVO_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------- entries from an explicit list ----
__global__ __launch_bounds__(256) void topk_exact_prepare_kernel(ExactWs ws, const int* __restrict__ q_idx,
                                                                 const float* __restrict__ need, int n, CertArgs cert, int D,
                                                                 const uint64_t* __restrict__ cand, long cand_stride, int ksel) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);        // place in the caller's list = output row
    if (i >= n) return;
    const int q = q_idx[i];
    const float G = __uint_as_float(cert.gstat[0]), Eg = __uint_as_float(cert.gstat[1]);
    const float eps = cert_eps(cert.qstat[(long)q * 2], cert.qstat[(long)q * 2 + 1], G, Eg, D);
    const float nd = need[i];
    float lb = nd - eps;
    lb -= fabsf(lb) * 2.4e-7f;
    if (nd == -INFINITY) lb = -INFINITY;
    // the scan's segments answer if they hold every row at or above lb (topk_util.h); U = this shard's ksel-th best scan score
    bool from_seg = false;
    if (cert.mode == 0 && cert.nsegs > 0 && cand) {
        const uint64_t last = cand[(long)q * cand_stride + ksel - 1];
        from_seg = last != 0ull && cert_segments_cover(cert, q, lb, key_score(last));
    }
    int j = 0;
    if (lane == 0) j = atomicAdd(ws.ctr + (from_seg ? CTR_FROM_SEGS : CTR_UNCERTIFIED), 1);
    j = __builtin_amdgcn_readfirstlane(j);
    if (from_seg) j = ws.cap - 1 - j;
    if (lane == 0) {
        ws.unc_q[j] = q;
        ws.unc_lb[j] = lb;
        ws.orow[j] = i;
        if (!from_seg) ws.col_cnt[j] = 0;
    }
    if (from_seg) { cert_fill_from_segments(cert, q, lb, j, lane); return; }
    const bf16_t* qs = cert.Qb + (long)q * cert.ldq;
    bf16_t* qd = ws.qb_u + (long)j * ws.ldqb;
    for (int c = lane * 8; c < D; c += 512) *(uint4*)(qd + c) = *(const uint4*)(qs + c);
}
int launch_topk_exact_prepare(const ExactWs& ws, const int* q_idx, const float* need, int n, const CertArgs& cert, int D,
                              const uint64_t* cand, long cand_stride, int ksel, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(topk_exact_prepare_kernel, dim3((unsigned)(n + 3) / 4), dim3(256), 0, st, ws, q_idx, need, n,
                       cert, D, cand, cand_stride, ksel);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
