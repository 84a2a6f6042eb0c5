// Host check of dedup_plan.h, the tile-pair walk of the deduplicating append's join (dedup.hip): for gallery sizes around a
// tile boundary and batch sizes around one tile, the numbering visits exactly the tile pairs (ti <= tj) whose column tile tj
// holds a batch row, each once, column by column, and dedup_locate / dedup_next agree with it.
#include <cstdio>
#include <set>
#include <utility>

#include "../../revers-o_amd/csrc/dedup_plan.h"

int main() {
    int failed = 0;
    const long Ns[] = {0, 255, 256, 257, 1000}, ns[] = {1, 256, 257, 16384};
    for (long N0 : Ns)
        for (long n : ns) {
            const revo::DedupPlan p = revo::dedup_plan(N0, n);
            // brute force: tile tj holds a batch row when [256 tj, 256 tj + 256) meets [N0, N0 + n)
            std::set<std::pair<int, int>> want;
            const long T = (N0 + n + 255) / 256;
            for (long tj = 0; tj < T; ++tj)
                if (tj * 256 + 256 > N0 && tj * 256 < N0 + n)
                    for (long ti = 0; ti <= tj; ++ti) want.insert({(int)ti, (int)tj});
            bool ok = p.T == T && p.pairs == (long)want.size() && p.tj0 == N0 / 256;
            std::set<std::pair<int, int>> seen;
            int wi = 0, wj = 0, pj = -1, pi = -1;
            for (long q = 0; ok && q < p.pairs; ++q) {
                int ti, tj;
                revo::dedup_locate(q, p.tj0, p.T, ti, tj);
                if (q == 0) { wi = ti; wj = tj; }
                ok = ok && ti == wi && tj == wj;                               // the walk from the first pair gives the same
                ok = ok && ti <= tj && want.count({ti, tj}) && seen.insert({ti, tj}).second;
                ok = ok && (tj > pj || (tj == pj && ti == pi + 1));           // column by column, rows ascending
                pj = tj; pi = ti;
                revo::dedup_next(wi, wj);
            }
            ok = ok && seen.size() == want.size();
            std::printf("N0 %ld n %ld: T %ld tj0 %ld pairs %ld %s\n", N0, n, p.T, p.tj0, p.pairs, ok ? "ok" : "FAILED");
            failed += !ok;
        }
    const revo::DedupPlan e = revo::dedup_plan(300, 0);
    if (e.pairs != 0) { std::printf("n = 0: FAILED\n"); ++failed; }
    std::printf(failed ? "FAILED\n" : "ALL OK\n");
    return failed != 0;
}
