// The device frame under every kernel that runs the 256 x 256 main loop over a LIST of tiles and hands each tile's scores to
// an epilogue of its own (DESIGN.md section 4i "Tile-walk frame"): the joins of pairs, clusters, kNN graph and deduplicating
// append walk tile PAIRS of one gallery (tile_pair_frame); range, MaxSim and the kNN level pass walk a SLICE of gallery
// tiles against one fixed A tile (tile_slice_frame), as do recommend, discover and the large-k count (see there).  Like
// candidates.h, next to which it sits: a fix is made here, once.  A kernel is its frame plus a lambda.
//
// What the frames do per tile, and why in this order:
//   1. zero acc[8][4], run gemm256_mainloop.
//   2. advance to the next tile, set its operands up and issue its prologue BEFORE the epilogue runs: the DMA of the next
//      tile's first K-tiles flies while the epilogue works (the main loop's LDS image is free once the main loop has left
//      it; what a kernel keeps in LDS of its own sits past G256_LDS).
//   3. the lane fence asm volatile("" : "+v"(lane)): behind it the compiler no longer knows `lane`, so nothing the epilogue
//      derives from it (lr, lq, rbase, column numbers, lanes_below) can be computed in front of the main loop and held
//      in vector registers across it -- these kernels run at 256 VGPRs with the accumulators alone taking 128.
//   4. the epilogue, with the fenced lane.  Leaving a tile early is `return` from the lambda.
// The epilogues test wave-uniformly (ballots, bit masks) where they can: a branch per score keeps so many lane masks alive
// that their scalar spills take a second VGPR, and the main loop spills (measured on the clusters join).
#pragma once
#include "candidates.h"
#include "gemm256_core.h"
#include "kernels.h"

namespace revo {

// Slice `slice` of `slices` over `tiles` items: the contiguous range [t0, t1), the first tiles % slices slices one longer.
// false: an empty slice (more slices than tiles).  I is the kernel's own index width (it is part of its register
// allocation: 64-bit bounds live in vector registers); the 32-bit form pins `per` to a scalar register.
template <class I>
__device__ __forceinline__ bool tile_slice(I tiles, I slices, I slice, I& t0, I& t1) {
    I per = tiles / slices;
    if constexpr (sizeof(I) == 4) per = __builtin_amdgcn_readfirstlane(per);
    const I rem = tiles - per * slices;
    t0 = slice * per + (slice < rem ? slice : rem);
    t1 = t0 + per + (slice < rem ? 1 : 0);
    return t0 < t1;
}

// The epilogue's view of the accumulators: acc[m][n][j] of lane (lr, lq) is row rbase + m * 16 of the tile against column
// cw + n * 16 + lq * 4 + j; the wave's 64 columns cw .. cw + 63 are the bits of one tile_column_mask word.
struct TileLane { int lr, lq, rbase, cw; };
__device__ __forceinline__ TileLane tile_lane(int wave, int lane) {
    const int lr = lane & 15;
    return {lr, lane >> 4, (wave >> 2) * 128 + lr, (wave & 3) * 64};
}

// The largest of this lane's 16 scores of row fragment m (NaN scores are ignored: fmaxf).  Every epilogue asks first whether
// any lane of the wave has a score that reaches the row's bound, `__ballot(tile_row_max(acc, m) >= bound)`: most fragments
// of most tiles have none.  (knn_join_kernel types the loop out: with this call its listing moved, 14 638 -> 14 534 lines.)
__device__ __forceinline__ float tile_row_max(const f32x4 (&acc)[8][4], int m) {
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, acc[m][n][j]);
    return mx;
}

// ------------------------------------------------------------------ tile pairs ----
// The pairs join's walk: the upper triangle ti <= tj < T in row-major order (pairs_row_start, candidates.h), so that
// consecutive pairs share the A tile: A is set up again only when ti changed.
struct TriangleWalk {
    static constexpr bool kInitBoth = false;
    long T;
    __device__ __forceinline__ void locate(long p0, int& ti, int& tj) const {
        // the row tile of p0: the largest ti with pairs_row_start(ti) <= p0
        int lo = 0, hi = (int)T - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pairs_row_start(mid, T) <= p0) lo = mid; else hi = mid - 1;
        }
        ti = lo;
        tj = (int)(lo + (p0 - pairs_row_start(lo, T)));
    }
    __device__ __forceinline__ void next(int& ti, int& tj) const {
        if (++tj == (int)T) { ++ti; tj = ti; }
    }
};

// row tile t of the gallery as an operand.  (This and slice_issue below are free functions, not lambdas inside the frames: a
// lambda that captures `lane` takes the address of the fenced variable, and the clusters join then spills two vector
// registers inside the main loop.)
__device__ __forceinline__ void pair_row_tile(G256Operand& op, const PairsJoinArgs& p, int t, int wave, int lane) {
    g256_operand_init(op, p.Gb + (long)t * 256 * p.ldg, p.ldg, p.N - (long)t * 256, 0, wave, lane);
}

// Workgroup w takes the contiguous range [p0, p1) of the p.pairs tile pairs that `walk` numbers (equal counts: every pair
// is one full tile of MFMA work); both operands are row tiles of the one gallery p.Gb, rows past p.N read as zeros.
//   walk.locate(p0, ti, tj), walk.next(ti, tj); Walk::kInitBoth: set BOTH operands up for every pair.  That is a
//   compile-time property because the run-time test costs registers where the A tile changes with every pair anyway:
//   behind `if (tj != cj)` B's set-up cost the dedup join 8 spilled VGPRs.
//   epilogue(ci, cj, n0, diag, wave, lane, acc): tile pair (ci, cj), n0 = cj * 256 its first column, diag = ci == cj.
template <class Walk, class Epilogue>
__device__ __forceinline__ void tile_pair_frame(const PairsJoinArgs& p, const Walk walk, char* smem, Epilogue epilogue) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    long p0, p1;
    if (!tile_slice<long>(p.pairs, gridDim.x, blockIdx.x, p0, p1)) return;
    const int n_my = (int)(p1 - p0);
    int ti, tj;
    walk.locate(p0, ti, tj);
    G256Operand A, B;
    pair_row_tile(A, p, ti, wave, lane);
    pair_row_tile(B, p, tj, wave, lane);
    g256_issue_prologue(A, B, smem, p.D, wave);
    for (int it = 0; it < n_my; ++it) {
        f32x4 acc[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm256_mainloop(A, B, smem, p.D, wave, lane, acc);
        const int ci = ti, cj = tj;
        walk.next(ti, tj);
        if (it + 1 < n_my) {
            if (Walk::kInitBoth || ti != ci) pair_row_tile(A, p, ti, wave, lane);
            pair_row_tile(B, p, tj, wave, lane);
            g256_issue_prologue(A, B, smem, p.D, wave);
        }
        asm volatile("" : "+v"(lane) :: "memory");
        epilogue(ci, cj, (long)cj * 256, ci == cj, wave, lane, acc);
    }
}

// ---------------------------------------------------------------------- slices ----
// B = the tile of 256 rows from row0 on, and the prologue of (A, B)
template <bool DEEP, int BAUX>
__device__ __forceinline__ void slice_issue(const G256Operand& A, G256Operand& B, const bf16_t* Bb, long ldb, long nb, long row0,
                                            char* smem, int D, int wave, int lane) {
    g256_operand_init(B, Bb + row0 * ldb, ldb, nb - row0, 0, wave, lane);
    if constexpr (DEEP) g256_issue_prologue_deep<BAUX>(A, B, smem, D, wave); else g256_issue_prologue<BAUX>(A, B, smem, D, wave);
}
// Tiles [t0, t1) of the B side (Bb: rows of ldb elements, nb of them; tile t is rows t * 256 ...) against the fixed A the
// kernel has set up.  <ROWS, DEEP, BAUX>: gemm256_mainloop's row form, its deep prologue, B's cache policy.  T: the
// kernel's index width (tile_slice).  `lane` is the KERNEL's variable: the fence covers what the kernel does with it
// behind the frame (a query-tile loop around the frame sets A up again with it).  epilogue(n0, lane, acc): n0 = t * 256,
// the tile's first B row.  A kernel whose waves 4 .. 7 hold no rows leaves them in its epilogue's first line.
// Not on this frame, because hipcc's register allocation did not survive the move (their tile loops are this text, typed
// out): recommend_pass_kernel and discover_pass_kernel (the allowed-row count they carry across the tiles costs a scalar
// spill as a by-reference capture), topk_large_count_kernel (one spilled vector register inside its query-tile loop).
template <int ROWS, bool DEEP, int BAUX, class T, class Epilogue>
__device__ __forceinline__ void tile_slice_frame(const G256Operand& A, const bf16_t* Bb, long ldb, long nb, T t0, T t1,
                                                 char* smem, int D, int wave, int& lane, Epilogue epilogue) {
    G256Operand B;
    slice_issue<DEEP, BAUX>(A, B, Bb, ldb, nb, (long)t0 * 256, smem, D, wave, lane);
    for (T t = t0; t < t1; ++t) {
        const long n0 = (long)t * 256;
        f32x4 acc[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm256_mainloop<ROWS, false, DEEP, 0, BAUX>(A, B, smem, D, wave, lane, acc);
        // (a next tile exists.  Written as a distance: `t + 1 < t1` is the loop's own test of the next trip, hipcc keeps the one
        //  result in a scalar pair across the epilogue, and the 64-row range join spills one more scalar)
        if (t1 - t > 1) slice_issue<DEEP, BAUX>(A, B, Bb, ldb, nb, n0 + 256, smem, D, wave, lane);
        asm volatile("" : "+v"(lane) :: "memory");
        epilogue(n0, lane, acc);
    }
}

// -------------------------------------------------------- three-way classification ----
// The epilogue of a join that applies its certain edges in place (clusters.hip, dedup.hip).  fm: the wave's allowed columns
// (tile_column_mask); lb / ub = pairs_lb / pairs_ub.  A pair (gi, gj) of tile pair (ci, cj) counts when gi < p.N, row_ok(gi),
// column gj is in fm and, on the diagonal, gj > gi.  Its bf16 score v then decides: v >= ub is certainly an edge, lb <= v < ub
// is ambiguous and appended to p.keys as (gi << 32) | gj (as the pairs join appends its candidates), v < lb is no edge.
// A lane classifies its 8 x 16 scores into bit masks without a branch per score (see the top of the file); the certain
// edges are applied in one loop behind the rows, per lane and rows in order: keep = edge(gi, gj, new_row), new_row: the
// first edge of its row in this lane (a functor may keep per-row state in a register); keep == false leaves the tile.
template <class RowOk, class Edge>
__device__ __forceinline__ void classify_tile3(const PairsJoinArgs& p, uint64_t fm, float lb, float ub, int ci, long n0,
                                               bool diag, int wave, int lane, const f32x4 (&acc)[8][4], RowOk row_ok,
                                               Edge edge) {
    if (fm == 0ull) return;                                 // wave-uniform: no column counts
    const TileLane t = tile_lane(wave, lane);
    const int lq = t.lq, rbase = t.rbase, cw = t.cw;
    const uint64_t bits = fm >> (lq * 4);
    // the rows of the tile with a score that reaches lb (wave-uniform): most tiles have none
    uint32_t hot = 0u;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const float mx = tile_row_max(acc, m);
        if (__ballot(mx >= lb) != 0ull) hot |= 1u << m;
    }
    if (hot == 0u) return;
    // bit c = n * 4 + j of the masks below: this lane's column cw + n * 16 + lq * 4 + j
    uint32_t colm = 0u;                                     // columns that count
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) colm |= ((uint32_t)(bits >> (n * 16 + j)) & 1u) << (n * 4 + j);
    const int dl = rbase - cw - lq * 4;                     // row - column = dl + m * 16 - (n * 16 + j)
    const unsigned long long below = lanes_below(lane);
    uint64_t sure0 = 0ull, sure1 = 0ull;                    // bit (m & 3) * 16 + c: score [m][c] is a certain edge
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        if (!((hot >> m) & 1u)) continue;                   // wave-uniform
        const int row = rbase + m * 16;
        const long gi = (long)ci * 256 + row;
        const bool rok = gi < p.N && row_ok(gi);
        uint32_t pm = rok ? colm : 0u;                      // the pairs of this row that count: on the diagonal, column > row
        if (diag) {
            uint32_t gt = 0u;
#pragma unroll
            for (int c = 0; c < 16; ++c) gt |= ((uint32_t)(dl + m * 16 - ((c >> 2) * 16 + (c & 3))) >> 31) << c;
            pm &= gt;
        }
        uint32_t ge_lb = 0u, ge_ub = 0u;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc[m][n][j];
                ge_lb |= v >= lb ? 1u << (n * 4 + j) : 0u;
                ge_ub |= v >= ub ? 1u << (n * 4 + j) : 0u;
            }
        const uint32_t sure = pm & ge_lb & ge_ub, amb = pm & ge_lb & ~ge_ub;
        if (m < 4) sure0 |= (uint64_t)sure << (m * 16); else sure1 |= (uint64_t)sure << ((m - 4) * 16);
        if (__ballot(amb != 0u) == 0ull) continue;          // wave-uniform
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const bool take = (amb >> c) & 1u;
            const unsigned long long mk = __ballot(take);
            if (mk == 0ull) continue;                       // wave-uniform
            const unsigned long long pos = wave_append(mk, p.cnt, lane, below);
            if (take && pos < (unsigned long long)p.cap)
                p.keys[pos] = ((uint64_t)gi << 32) | (uint64_t)(n0 + cw + (c >> 2) * 16 + lq * 4 + (c & 3));
        }
    }
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        uint64_t mk = h ? sure1 : sure0;
        int last = -1;
        while (mk != 0ull) {
            const int bit = __ffsll((long long)mk) - 1;
            mk &= mk - 1ull;
            const int m = h * 4 + (bit >> 4), c = bit & 15;
            const uint32_t gi = (uint32_t)(ci * 256 + rbase + m * 16);
            const uint32_t gj = (uint32_t)(n0 + cw + (c >> 2) * 16 + lq * 4 + (c & 3));
            const bool keep = edge(gi, gj, m != last);
            last = m;
            if (!keep) { mk = 0ull; h = 2; }
        }
    }
}

}  // namespace revo
