// The work plan of a 256 x 256 query x gallery scan (host only): which query tiles and gallery slices each workgroup of the
// launch takes, in phases.  Shared by the top-k scan (topk256.hip) and the range search's candidate pass (range.hip).
#pragma once

namespace revo {

constexpr int S256_PHASES = 8;

// Slices per query tile for up to 7 query tiles (and for the last, unpinned phase of a larger launch).  Workgroups run
// one per CU in rounds; a slice costs its tiles plus about one tile time of fixed work (pipeline fill, refreshes, the
// tail), and the slices are dealt out evenly, so the phase takes about  rounds x (ceil(tiles / s) + 1)  tile times.
// Fewer, longer slices on a tie.
static int scan256_best_splits(int qtiles, long tiles, double* cost_out) {
    int best = 1;
    double best_cost = 1e300;
    for (int s = 1; s <= 512; ++s) {
        if (s > tiles) break;
        const long per = (tiles + s - 1) / s;
        if (s > 1 && per < 3) break;
        const long rounds = ((long)qtiles * s + 255) / 256;
        const double cost = (double)rounds * ((double)per + 1.0);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = s; }
    }
    if (cost_out) *cost_out = best_cost;
    return best;
}
// The phases of a scan launch.  With 8 query tiles and more, query tiles are pinned to XCDs (kernel comment) and the
// slices of an XCD's query tiles have to line up, so an XCD's 32 CUs are all busy only when it holds a = 1, 2, 4, 8, 16 or
// 32 query tiles (32 / a slices each).  The query tiles are therefore taken in phases of 8 a, largest first -- 39 query
// tiles: 32 as 4 per XCD x 8 slices, then the other 7 with the slices of a small launch -- each phase one even round of
// workgroups; the hardware starts a phase's blocks as the previous phase's end.  (Rounds 2-4 ran all query tiles in one
// phase, 5 per XCD x 6 slices = 30 of 32 CUs and 24 on the eighth XCD: 615 tile times where 39 x 3 875 / 256 = 590 is even,
// 78 against 69.5 on a shard of an eighth.)
struct Scan256Plan { int nph, splits; int q0[S256_PHASES], qn[S256_PHASES], ns[S256_PHASES]; double cost; };
static void scan256_plan(int qtiles, long tiles, Scan256Plan& pl) {
    pl = Scan256Plan{};
    int q = 0;
    auto add = [&](int qn, int ns, double cost) {
        pl.q0[pl.nph] = q; pl.qn[pl.nph] = qn; pl.ns[pl.nph] = ns; ++pl.nph;
        pl.splits = ns > pl.splits ? ns : pl.splits;
        pl.cost += cost;
        q += qn;
    };
    while (qtiles - q >= 8 && pl.nph < S256_PHASES - 1) {
        int a = 1;
        while (a < 32 && 16 * a <= qtiles - q) a *= 2;                 // the largest power of two with 8 a <= what is left
        int rounds = 1;
        if (a == 32) rounds = (qtiles - q) / 256;                       // whole rounds of one query tile per CU
        long ns = 32 / a;
        if (ns > tiles) ns = tiles;
        while (ns > 1 && (tiles + ns - 1) / ns < 3) --ns;               // (a gallery of a few tiles: fewer, longer slices)
        add(8 * a * rounds, (int)ns, (double)rounds * ((double)((tiles + ns - 1) / ns) + 1.0));
    }
    if (q < qtiles) {
        double c = 0.0;
        const int ns = scan256_best_splits(qtiles - q, tiles, &c);
        add(qtiles - q, ns, c);
    }
}
// The plan as the kernels' argument blocks hold it (Scan256Args, RangeJoinArgs: plain arrays, read with constant indices):
// phase i is the blocks [first[i], first[i + 1]) of a 1-D grid, block first[i] + j = (query tile q0[i] + j % qn[i], slice
// j / qn[i] of ns[i]).  Every phase starts at a multiple of 8 blocks (the XCD pinning above; pinned phases are multiples of
// 8 blocks anyway).  first has pl.nph + 1 entries.  Returns the number of blocks; the caller checks that it fits its grid.
static long scan256_phase_table(const Scan256Plan& pl, int* first, int* q0, int* qn, int* ns) {
    long blocks = 0;
    for (int i = 0; i < pl.nph; ++i) {
        first[i] = (int)blocks; q0[i] = pl.q0[i]; qn[i] = pl.qn[i]; ns[i] = pl.ns[i];
        blocks += (long)pl.qn[i] * pl.ns[i];
        if (i + 1 < pl.nph) blocks = (blocks + 7) / 8 * 8;
    }
    first[pl.nph] = (int)blocks;
    return blocks;
}

}  // namespace revo
