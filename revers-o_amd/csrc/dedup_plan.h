// The tile-pair walk of the deduplicating append's join (dedup.hip).  Device code and, for
// tests/native/dedup_plan_check.cpp, host code: one source.
//
// The gallery holds rows 0 .. N0 - 1, the batch rows N0 .. N0 + n - 1; T = ceil((N0 + n) / 256) row tiles.  The join takes the
// tile pairs (ti <= tj) of the pairs join's upper triangle whose COLUMN tile tj holds a batch row: tj0 = floor(N0 / 256) <= tj < T
// (tile tj0 straddles N0 unless N0 is a multiple of 256; the kernel masks its columns below N0).  They are numbered column by
// column -- all ti = 0 .. tj of tj0, then of tj0 + 1, ... -- so consecutive pairs share the batch-side tile.
#pragma once

#if defined(__HIPCC__)
#define DEDUP_FN __host__ __device__ __forceinline__
#else
#define DEDUP_FN inline
#endif

namespace revo {

struct DedupPlan { long tj0, T, pairs; };

// number of the first tile pair of column tile tj (tj0 <= tj <= T)
DEDUP_FN long dedup_col_start(long tj, long tj0) { return tj * (tj + 1) / 2 - tj0 * (tj0 + 1) / 2; }

DEDUP_FN DedupPlan dedup_plan(long N0, long n) {
    DedupPlan p;
    p.tj0 = 0; p.T = 0; p.pairs = 0;
    if (n <= 0) return p;
    p.tj0 = N0 / 256;
    p.T = (N0 + n + 255) / 256;
    p.pairs = dedup_col_start(p.T, p.tj0);
    return p;
}

// tile pair number q (0 <= q < pairs) -> (ti, tj): the largest tj with dedup_col_start(tj) <= q
DEDUP_FN void dedup_locate(long q, long tj0, long T, int& ti, int& tj) {
    long lo = tj0, hi = T - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (dedup_col_start(mid, tj0) <= q) lo = mid; else hi = mid - 1;
    }
    tj = (int)lo;
    ti = (int)(q - dedup_col_start(lo, tj0));
}
// the pair behind (ti, tj) in the numbering
DEDUP_FN void dedup_next(int& ti, int& tj) {
    if (++ti > tj) { ++tj; ti = 0; }
}

}  // namespace revo
