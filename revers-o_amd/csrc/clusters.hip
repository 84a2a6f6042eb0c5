// Duplicate clusters of one gallery (revo_gallery_clusters, include/revo.h CLUSTERS): the connected
// components of the graph whose edges are the pairs of revo_gallery_pairs, without storing those pairs.
//
//   join     the pairs join (pairs.hip: same walk over the upper triangle of row-tile pairs, operands, main loop, column mask,
//            diagonal rule; tile_walk.h) with three-way scores: v >= ub = fl(thr + eps) raised by its rounding is certainly an edge (the
//            fp32 score is >= v - eps >= thr) and is merged into the union-find (unionfind.h) in place; lb <= v < ub is
//            ambiguous and appended as the key (i << 32) | j; v < lb is certainly no edge
//   rescore  the fp32 score of every ambiguous pair; those >= thr are merged.  Nothing is kept, nothing is sorted
//   finish   labels[r] = find(r) (the component's lowest row; -1: not allowed), component sizes, the rows of components of two
//            or more rows as keys (label << b) | row, radix sort (radix_sort.hip), label boundaries -> prefix sum -> offsets
// The result does not depend on the order of the merges: the components are those of the edge set, and a component's root
// is its lowest row whatever the order.  A second join pass (workspace regrow) repeats merges, which changes nothing.
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"
#include "tile_walk.h"
#include "topk_util.h"
#include "unionfind.h"

namespace revo {

// parent[r] = r, sizes[r] = 0, the counters and the error word (parent[N], in every kernel here) cleared
__global__ __launch_bounds__(256) void clusters_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ sizes, long N,
                                                            unsigned long long* __restrict__ ctr4) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < 4) ctr4[r] = 0ull;
    if (r < N) { parent[r] = (uint32_t)r; sizes[r] = 0u; }
    if (r == N) parent[N] = 0u;
}

// -------------------------------------------------------------------------- join ----
// tile_walk.h's tile-pair frame over the triangle and its three-way classification; a certain edge is merged: the row's
// root stays in a register across the row's columns, and a column whose parent is that root costs one load.
__global__ __launch_bounds__(G256_THREADS, 2) void clusters_join_kernel(ClustersJoinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PairsJoinArgs& p = a.j;
    const float lb = pairs_lb(p.gstat, p.thr, p.D), ub = pairs_ub(p.gstat, p.thr, p.D);
    tile_pair_frame(p, TriangleWalk{p.T}, smem, [&](int ci, int cj, long n0, bool diag, int wave, int lane, const f32x4 (&acc)[8][4]) {
        const uint64_t fm = tile_column_mask(p.N, n0, (wave & 3) * 64, p.allow);
        const UfLimits lim = uf_limits(p.N);
        uint32_t* const err = a.parent + p.N;               // (the error word sits behind the last row's parent)
        uint32_t ri = 0u;
        classify_tile3(p, fm, lb, ub, ci, n0, diag, wave, lane, acc,
                       [&](long gi) { return !p.allow || ((p.allow[gi >> 5] >> (gi & 31)) & 1u); },
                       [&](uint32_t gi, uint32_t gj, bool new_row) {
                           if (new_row) ri = uf_find(a.parent, gi, lim.walk, err);
                           if (UF_LOAD(a.parent + gj) == ri) return true;   // same component (true whenever seen: links are never removed)
                           ri = uf_unite(a.parent, ri, gj, lim, err);
                           return UF_LOAD(err) == 0u;       // a trip limit was hit somewhere: leave
                       });
    });
}

// ----------------------------------------------------------------------- rescore ----
// wave g re-scores ambiguous pairs 4 g .. 4 g + 3 (grid-stride) with the one fma chain; those that reach thr are merged
__global__ __launch_bounds__(256) void clusters_rescore_kernel(const uint64_t* __restrict__ cand, long n, const float* __restrict__ Gf,
                                                               long ldg, int D, float thr, uint32_t* parent, long N) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    const UfLimits lim = uf_limits(N);
    uint32_t* const err = parent + N;
    for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < n; g += waves) {
        float v;
        uint64_t k;
        const int m = rescore_group4(cand, n, g * 4, D, lane, [&](uint64_t key, const float*& q, const float*& r) {
            q = Gf + (long)(key >> 32) * ldg;
            r = Gf + (long)(uint32_t)key * ldg;
        }, v, k);
        if (lane < m && v >= thr) uf_unite(parent, (uint32_t)(k >> 32), (uint32_t)k, lim, err);
    }
}

// ------------------------------------------------------------------------ finish ----
// labels[r] = root of r, or -1 for a row the filter excludes; sizes[root] counts the component's rows
__global__ __launch_bounds__(256) void clusters_label_kernel(uint32_t* parent, const uint32_t* __restrict__ allow, long N,
                                                             long long* __restrict__ labels, uint32_t* sizes) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const bool ok = !allow || ((allow[r >> 5] >> (r & 31)) & 1u);
    if (!ok) { labels[r] = -1; return; }
    const uint32_t root = uf_find(parent, (uint32_t)r, uf_limits(N).walk, parent + N);
    labels[r] = (long long)root;
    atomicAdd(sizes + root, 1u);
}
// the rows of components of two or more rows -> keys (label << b) | row, counted in ctr4[0]; their roots counted in ctr4[1];
// ctr4[2] = the error word (every launch that can set it has ended)
__global__ __launch_bounds__(256) void clusters_keys_kernel(const long long* __restrict__ labels, const uint32_t* __restrict__ sizes,
                                                            long N, int b, uint64_t* __restrict__ keys,
                                                            unsigned long long* __restrict__ ctr4, const uint32_t* __restrict__ err) {
    // (err = parent + N)
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (r == 0) ctr4[2] = (unsigned long long)err[0];
    const long long lab = r < N ? labels[r] : -1;
    const bool take = lab >= 0 && sizes[lab] >= 2u;
    const unsigned long long mk = __ballot(take);
    if (mk == 0ull) return;                                 // wave-uniform
    const unsigned long long pos = wave_append(mk, ctr4, lane, lanes_below(lane));
    if (take) keys[pos] = ((uint64_t)lab << b) | (uint64_t)r;
    const unsigned long long heads = __ballot(take && lab == (long long)r);
    if (lane == 0 && heads != 0ull) atomicAdd(ctr4 + 1, (unsigned long long)__popcll(heads));
}
// sorted keys: members[e] = row; rank[e] = 1 where entry e starts a cluster (its row is its label), else 0
__global__ __launch_bounds__(256) void clusters_members_kernel(const uint64_t* __restrict__ keys, long n, int b,
                                                               long long* __restrict__ members,
                                                               unsigned long long* __restrict__ rank) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint64_t k = keys[e], row = k & ((1ull << b) - 1ull);
    members[e] = (long long)row;
    rank[e] = row == (k >> b) ? 1ull : 0ull;
}
// rank: the inclusive sums of the starts; cluster c = rank - 1 starts at entry e; offsets[n_clusters] = n
__global__ __launch_bounds__(256) void clusters_offsets_kernel(const uint64_t* __restrict__ keys, long n, long n_clusters, int b,
                                                               const unsigned long long* __restrict__ rank,
                                                               long long* __restrict__ offsets) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) offsets[n_clusters] = (long long)n;
    if (e >= n) return;
    const uint64_t k = keys[e];
    if ((k & ((1ull << b) - 1ull)) != (k >> b)) return;
    const unsigned long long c = rank[e] - 1ull;
    if (c < (unsigned long long)n_clusters) offsets[c] = (long long)e;
}

// ------------------------------------------------------------------------ launchers ----
int launch_clusters_init(uint32_t* parent, uint32_t* sizes, long N, unsigned long long* ctr4, hipStream_t st) {
    const long n = N + 1 > 4 ? N + 1 : 4;
    hipLaunchKernelGGL(clusters_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, parent, sizes, N, ctr4);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_clusters_join(const ClustersJoinArgs& a_in, hipStream_t st) {
    ClustersJoinArgs a = a_in;
    long wgs = 0;                                           // the pairs join's plan and grid
    { const int rc = pairs_join_plan(a.j, "gallery_clusters", &wgs); if (rc) return rc; }
    if (wgs == 0) return 0;
    REVO_FUNC_LDS(clusters_join_kernel, G256_LDS);
    hipLaunchKernelGGL(clusters_join_kernel, dim3((unsigned)wgs), dim3(G256_THREADS), G256_LDS, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_clusters_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, uint32_t* parent,
                            long N, hipStream_t st) {
    if (n <= 0) return 0;
    const long groups = (n + 3) / 4, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(clusters_rescore_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, cand, n, Gf, ldg,
                       D, thr, parent, N);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_clusters_labels(uint32_t* parent, const uint32_t* allow, long N, int b, long long* labels, uint32_t* sizes,
                           uint64_t* keys, unsigned long long* ctr4, hipStream_t st) {
    // (N = 0: the keys kernel still copies the error word)
    const unsigned blocks = (unsigned)(((N > 1 ? N : 1) + 255) / 256);
    if (N > 0) hipLaunchKernelGGL(clusters_label_kernel, dim3(blocks), dim3(256), 0, st, parent, allow, N, labels, sizes);
    hipLaunchKernelGGL(clusters_keys_kernel, dim3(blocks), dim3(256), 0, st, labels, sizes, N, b, keys, ctr4, parent + N);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_clusters_emit(const uint64_t* keys, long n, long n_clusters, int b, unsigned long long* rank, long long* members,
                         long long* offsets, hipStream_t st) {
    const unsigned blocks = (unsigned)(((n > 1 ? n : 1) + 255) / 256);
    if (n > 0) {
        hipLaunchKernelGGL(clusters_members_kernel, dim3(blocks), dim3(256), 0, st, keys, n, b, members, rank);
        REVO_HIP_CHECK(hipGetLastError());
        const int rc = launch_inclusive_sums_u64(rank, n, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(clusters_offsets_kernel, dim3(blocks), dim3(256), 0, st, keys, n, n_clusters, b, rank, offsets);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
