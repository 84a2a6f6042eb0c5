// The launch plan of launch_gemm (host only): which kernel form a problem gets, over which rows, on which grid.  gemm_plan()
// is the only place that decides; gemm.hip executes what it returns, gemm_resid_folds() and revo_debug_gemm_plan read the
// same answer (tests/test_gemm_plan.py checks it on the CPU tier).  No HIP calls, no device pointers.
#pragma once
#include "kernels.h"

namespace revo {

// Every switch of the launcher.  The defaults are the product's; all but force_tile exist for timing experiments and tests
// of forced forms (revo_op_set_variant and friends), and none changes a result.
struct GemmKnobs {
    int force_tile = 0;         // 0 = heuristic, 128 / 256 = forced (tests, A/B timing)
    int force_gy = 0;           // force the XCD arrangement (1, 2, 4, 8)
    int min_tiles256 = 100;     // fewest 256 x 256 tiles for the big tile (use_256)
    int persistent = 1;         // 0 = one workgroup per tile
    int qstores = 1;            // 0 = gemm256p_kernel for every epilogue (bits 0-2: 2 stores dropped, 3 also RoPE; + 8 stamps)
    int qtail = 1;              // 0 = the leftover rows behind the queued-stores kernel as a launch of their own
    int ring = 1;               // the ring kernel on (0: off) ...
    int ring_max_tiles = 256;   // ... and its largest problem: one tile per CU
    int tail_split = 1;         // 0 disables the tail split
    int splitk = 1;             // 0 disables the split-K forms
    int rows192 = 1;            // 0 disables the 192-row form
    int lnf = 1;                // 0 = never fold a LayerNorm into the residual GEMMs (the caller runs the kernel)
    int ln_planes = 1;          // 0 = folded, but the residual stream stays fp32 rows (+ a bf16 copy)
#ifdef REVO_EXPERIMENTS
    int dbg = 0;                // EPI_BF16 only (results are wrong): 1 = no epilogue stores, 2 = no main loop, 3 = both
    int phase_groups = 0;       // phase groups of the persistent kernel (gemm256pp_kernel): 0 / 1 = off, 2..4 forced
    int stagger_cycles = 0, stagger_groups = 2;
#endif
};

// What the decision reads of a GemmArgs, as plain values.
struct GemmProblem {
    int epi;
    int M, N, K;
    long lda, ldb, ldc;
    int prefer256;
    long ws_elems;              // 0: no split-K workspace
    bool ln_offered;            // a LayerNorm behind the GEMM is offered for fusing (ln_out && ln_fused) ...
    long ln_ldo;
    bool fold_offered;          // the folded producer is offered (lnf_xb && lnf_stats && lnf_done) ...
    long lnf_ldxb;
    int xp_in, xp_out;          // the residual stream in planes, asked for ...
    bool planes_valid;          // ... and usable: xp_hi, xp_lo, xp_ld % 8 == 0, for xp_out xp_hi == lnf_xb
    int rope_S, rope_hd, rope_cols;
    bool lnc;                   // lnc_stats present (folded consumer)
};
static GemmProblem gemm_problem(int epi, const GemmArgs& a) {
    GemmProblem p{};
    p.epi = epi; p.M = a.M; p.N = a.N; p.K = a.K; p.lda = a.lda; p.ldb = a.ldb; p.ldc = a.ldc; p.prefer256 = a.prefer256;
    p.ws_elems = a.ws ? a.ws_elems : 0;
    p.ln_offered = a.ln_out && a.ln_fused; p.ln_ldo = a.ln_ldo;
    p.fold_offered = a.lnf_xb && a.lnf_stats && a.lnf_done; p.lnf_ldxb = a.lnf_ldxb;
    p.xp_in = a.xp_in; p.xp_out = a.xp_out;
    p.planes_valid = a.xp_hi && a.xp_lo && a.xp_ld % 8 == 0 && (!a.xp_out || a.xp_hi == a.lnf_xb);
    p.rope_S = a.rope_S; p.rope_hd = a.rope_hd; p.rope_cols = a.rope_cols;
    p.lnc = a.lnc_stats != nullptr;
    return p;
}

// One launch (the split-K forms: the GEMM on K parts plus its reduce) over rows [row0, row0 + rows).  Fields a form does
// not use stay 0.
struct GemmStep {
    unsigned form;              // the kernel's GemmForm bit (GF_SKINNY_444 .. GF_SPLITK_256)
    int row0, rows;
    int gy;                     // XCD arrangement of the 256 x 256 kernels
    int nslot;                  // persistent kernels: workgroups per XCD
    int grid_x, grid_y;
    int t192_tiles, t192_tall;  // 192-row form: tile rows, how many of the last are 208 rows tall
    int qtail_rows;             // queued-stores kernel: the rows [row0 + rows, + qtail_rows) done by the same launch
    int S;                      // split-K: K parts ...
    bool reduce_ln;             // ... and whether the reduce normalises the rows (sets *ln_fused)
    int xp;                     // residual stream format pair (gemm256_epilogue XP): 0 fp32 rows, 1 planes out, 2 in and out, 3 in
    bool fold;                  // writes bf16(x) and the row statistics (sets *lnf_done)
    int dbg;                    // experiment build, GF_256_TILE only: the work-skipping variant
};
struct GemmPlan {
    const char* error;          // non-null: no plan
    int nsteps;                 // 1, or 2: main rows and leftover rows
    GemmStep step[2];
    unsigned forms;             // GemmForm bits of the whole call
};

#ifdef REVO_EXPERIMENTS
constexpr bool G256Q_ROPE_BUILT = true;       // the RoPE form of the queued-stores kernel: measured, not adopted; experiment build only
#else
constexpr bool G256Q_ROPE_BUILT = false;
#endif

static const char* gemm_shape_error(int M, int N, int K, long lda, long ldb, long ldc) {
    if (K <= 0 || K % 64) return "gemm: K must be a positive multiple of 64";
    if (N % 4) return "gemm: N must be a multiple of 4";
    if (M <= 0 || N <= 0) return "gemm: empty problem";
    if (lda % 8 || ldb % 8) return "gemm: lda/ldb must be multiples of 8 (16-byte rows)";
    if (ldc % 4) return "gemm: ldc must be a multiple of 4";
    return nullptr;
}

// ---- the pieces every form shares ---------------------------------------------------------------------------------------
// a 256-row tile window (or `rows` leftover rows) of an operand with this row stride fits 32-bit DMA offsets
static bool gemm_window_ok(long ld, long rows = 256) { return rows * ld * 2 < (1l << 31); }
static long gemm_tiles256(int M, int N) { return (long)((M + 255) / 256) * ((N + 255) / 256); }
// the persistent 256 x 256 kernels: more than one round of tiles, and a K loop long enough for their pipeline
static bool gemm_persistent(const GemmKnobs& k, int M, int N, int K) { return k.persistent && K >= 128 && gemm_tiles256(M, N) > 256; }

// XCD arrangement of the 256 x 256 kernels: N stripes per 8 XCDs (the other factor of 8 = M stripes).  Re-measured in round 6 with
// the current kernels, alternated per layer shape (scripts/gemm_gy_sweep.py, profiles/r06_gemm_gy_sweep.json): up to 7 column
// tiles every XCD sweeps all of N for its M stripe; from 8 on two N stripes (L14 qkv, 12 tiles: -2.9 % against the four
// stripes round 4 chose; fc1, 16: -1.8 %; G14 qkv, 18: -3.4 %); four only from 24 on (G14 fc1, 35 tiles: -1.7 %).
static int gemm_xcd_stripes(int tiles_n) { return tiles_n >= 24 ? 4 : (tiles_n >= 8 ? 2 : 1); }
// tiles of one XCD's region under gy N stripes
static int gemm_xcd_region(int tiles_m, int tiles_n, int gy) { return ((tiles_m + 8 / gy - 1) / (8 / gy)) * ((tiles_n + gy - 1) / gy); }
static void gemm_xcd_grid(GemmStep& s, int tiles_m, int tiles_n, const GemmKnobs& k, bool persistent) {
    s.gy = k.force_gy ? k.force_gy : gemm_xcd_stripes(tiles_n);
    const int region = gemm_xcd_region(tiles_m, tiles_n, s.gy);
    if (persistent) s.nslot = region < 32 ? region : 32;                // 32 CUs per XCD
    s.grid_x = 8 * (persistent ? s.nslot : region);
    s.grid_y = 1;
}

// Whole rounds plus remainder.  The 256 x 256 kernel runs one workgroup per CU, so its tiles go in rounds of 256; a last
// round that is mostly empty costs a full tile time (PE-L14 at batch 64: out-proj and fc2 have 580 tiles = 2.27 rounds,
// fc1 2320 = 9.06).  When the last round would be less than ~60 % full (rem <= 160), the rows that make whole rounds can
// be split from the rest.
struct GemmRounds { long tm, tn, full, rem; };      // tile rows and columns; whole rounds; tiles of the last, partial round
static GemmRounds gemm_rounds(int M, int N) {
    const long tm = (M + 255) / 256, tn = (N + 255) / 256;
    return {tm, tn, tm * tn / 256, tm * tn % 256};
}
static bool gemm_tail_splits(const GemmRounds& r, const GemmKnobs& k) { return k.tail_split && r.full > 0 && r.rem > 0 && r.rem <= 160; }

static bool gemm_use_skinny(const GemmKnobs& k, int M, int N, int K) { return k.force_tile == 0 && M <= 64 && K % 256 == 0 && N >= 256; }
static bool gemm_use_256(const GemmProblem& p, const GemmKnobs& k) {
    if (!gemm_window_ok(p.lda) || !gemm_window_ok(p.ldb)) return false;   // 32-bit DMA offsets per tile window
    if (k.force_tile == 256) return true;
    if (k.force_tile == 128) return false;
    // the big tile needs enough tiles to occupy the chip: below ~100 of them (a couple of images) the
    // 128-row kernels spread the same work over more CUs
    return p.M >= 1024 && p.N >= 256 && gemm_tiles256(p.M, p.N) >= k.min_tiles256;
}
// the persistent kernel with queued stores (gemm256q_kernel): bf16 epilogues on whole 256-column tiles
static bool gemm_use_256q(const GemmProblem& p, const GemmKnobs& k) {
    const int e = p.epi;
    if (!(e == EPI_BF16 || e == EPI_BF16_GELU || (e == EPI_BF16_ROPE && G256Q_ROPE_BUILT)) || !k.qstores) return false;
    if (p.N % 256 || p.K < 128 || (p.ldc & 7) || !gemm_window_ok(p.ldc)) return false;
    if (e == EPI_BF16_ROPE && (p.rope_cols % 64 || (long)p.rope_S * (p.rope_hd >> 1) * 8 >= (1l << 31))) return false;
    // RoPE: measured, not adopted (profiles/r06_gemm_queued_stores.json): the rotation's 32 table loads per lane must be
    // waited for behind the next tile's DMA requests, and hipcc's wait counts leave LDS-DMA out -- every such wait is a
    // wait for the DMA too; and with its short arithmetic the form gains nothing from stores issued early (the plain
    // bf16 form: +-0).  qkv stays on gemm256p_kernel unless the switch says 3.
    if (e == EPI_BF16_ROPE && (k.qstores & 7) != 3) return false;
    return true;
}

// 192-row tiles.  The 256 x 256 kernel's tiles go in rounds of 256 (one workgroup per CU); PE-L14 at batch 64 has
// 36 928 rows = 144.25 tile rows, which for the two residual GEMMs (four tile columns) is 2.27 rounds: two whole ones
// and leftover rows that cost small-tile kernels more than half a round.  With 192-row tiles the same rows are
// 192 tile rows x 4 = exactly three rounds of 3/4 the work each (gemm256_mainloop<192>); the 64 rows that are still
// left make the last four tile rows 208 rows tall (1/16 of a tile's work more for 16 of the 768 workgroup-tiles: a
// launch of their own cost 10-17 us).  Returns the number of tile rows (and how many are tall), or 0 when the 256-row
// plan is no worse.
static int gemm_plan_rows192(const GemmProblem& p, const GemmKnobs& k, int* tall) {
    if (!k.rows192 || k.force_tile || p.K < 128 || p.M % 16) return 0;
    // T tile rows of 192, the last e of them 16 rows taller: M = 192 T + 16 e
    const long tn = (p.N + 255) / 256, T = p.M / 192, e = (p.M - T * 192) / 16;
    if (e > T || e > 8) return 0;
    const long tiles192 = T * tn, rounds192 = (tiles192 + 255) / 256;
    if (tiles192 <= 256 || rounds192 * 256 - tiles192 > tiles192 / 32) return 0;      // whole rounds only
    // the 256-row plan in tile times: its whole rounds, plus a last round or what the tail split makes of it
    const GemmRounds r = gemm_rounds(p.M, p.N);
    double cost256 = (double)r.full;
    if (r.rem) cost256 += gemm_tail_splits(r, k) ? (r.rem > 77 ? r.rem / 128.0 : 0.6) : 1.0;
    const double cost192 = rounds192 * 0.75 * 1.06 + (e ? 0.0625 : 0.0);
    if (cost192 >= cost256) return 0;
    *tall = (int)e;
    return (int)T;
}

// ---- the forms ------------------------------------------------------------------------------------------------------------
static GemmStep& gemm_add_step(GemmPlan& pl, unsigned form, int row0, int rows) {
    GemmStep& s = pl.step[pl.nsteps++];
    s = GemmStep{};
    s.form = form; s.row0 = row0; s.rows = rows;
    pl.forms |= form;
    return s;
}

// the 256 x 256 kernels on rows [row0, row0 + rows) (+ qtail_rows fused leftover rows, which the caller has checked)
static void gemm_plan_256(const GemmProblem& p, const GemmKnobs& k, GemmPlan& pl, int row0, int rows, int qtail_rows) {
    const int tiles_m = (rows + 255) / 256, tiles_n = (p.N + 255) / 256;
#ifdef REVO_EXPERIMENTS
    if (p.epi == EPI_BF16 && k.dbg) {
        GemmStep& s = gemm_add_step(pl, GF_256_TILE, row0, rows);
        s.dbg = k.dbg;
        gemm_xcd_grid(s, tiles_m, tiles_n, k, false);
        return;
    }
#endif
    if (gemm_persistent(k, rows, p.N, p.K)) {
        bool queued = gemm_use_256q(p, k);
#ifdef REVO_EXPERIMENTS
        queued = queued && (qtail_rows > 0 || (k.phase_groups <= 1 && k.stagger_cycles == 0));   // (the phased kernel has its own stamps)
#endif
        GemmStep& s = gemm_add_step(pl, queued ? (qtail_rows > 0 ? GF_256Q_QTAIL : GF_256Q) : GF_256P, row0, rows);
        s.qtail_rows = queued ? qtail_rows : 0;
        gemm_xcd_grid(s, tiles_m, tiles_n, k, true);
        return;
    }
    // one workgroup per tile
    gemm_xcd_grid(gemm_add_step(pl, GF_256_TILE, row0, rows), tiles_m, tiles_n, k, false);
}

static void gemm_plan_128(const GemmProblem& p, const GemmKnobs& k, GemmPlan& pl, int row0, int rows) {
    const int tiles = ((rows + 127) / 128) * ((p.N + 127) / 128);
    // at most about one 128 x 128 tile per CU: one latency-bound workgroup each; 128 x 64 tiles halve the work per
    // K step of a workgroup and put two or three of them on a CU
    if (k.force_tile == 0 && tiles <= 384 && p.K >= 512 && p.N % 64 == 0) {
        const int tiles64 = ((rows + 127) / 128) * ((p.N + 63) / 64);
        // about one tile per CU: the K loop is a chain of DMA latencies -- six-deep ring, one workgroup per CU
        GemmStep& s = gemm_add_step(pl, k.ring && tiles64 <= k.ring_max_tiles ? GF_128R : GF_128_64, row0, rows);
        s.grid_x = tiles64; s.grid_y = 1;
        return;
    }
    GemmStep& s = gemm_add_step(pl, GF_128_128, row0, rows);
    s.grid_x = tiles; s.grid_y = 1;
}

static void gemm_plan_skinny(const GemmProblem& p, GemmPlan& pl, int row0, int rows) {
    // few output columns (N / 16 workgroups would leave most CUs idle, each pulling all of A through one L2 port): one
    // workgroup per 16 x 16 fragment, all loads of 256 k per wave in flight -- 64 x 1024 x 4096: 21 -> 9 us, x 1024: 8 -> 6
    // (same bits: per element the same K order and the same fixed-order sum of the waves' parts)
    // (not for fc1's 64 x 4096 x 1024 leftover rows: measured in the step, round 5: fc1 7.70 -> 7.79 ms with the fragment form)
    const bool frag = p.K % 1024 == 0 && p.N <= 2048;
    GemmStep& s = gemm_add_step(pl, frag ? GF_SKINNY_444 : GF_SKINNY_411, row0, rows);
    s.grid_x = (p.N + 15) / 16; s.grid_y = frag ? (rows + 15) / 16 : 1;
}

// Split-K of the residual GEMMs.  The rows the whole rounds of the 256 x 256 kernel leave over (PE-L14 at batch 64, fc2:
// 68 tiles) occupy a quarter of the CUs for a full tile time: the K loop is a latency chain (~1.3 us per K-tile), so
// what helps is fewer K-tiles per CU, not smaller tiles.  Each tile's K range is cut in S parts that run on different CUs
// and write fp32 partial sums; a second kernel adds them in a fixed order (deterministic, unlike atomics) and applies
// bias, LayerScale and the residual add.  Returns false when the caller should use the ordinary path.
static bool gemm_plan_splitk(const GemmProblem& p, const GemmKnobs& k, GemmPlan& pl, int row0, int rows, bool ln_offered) {
    if (!k.splitk || p.ws_elems <= 0 || p.N % 4 || p.K < 1024) return false;
    const int tiles_m = (rows + 255) / 256, tiles_n = (p.N + 255) / 256, nt = p.K / 64;
    const long plane = (long)rows * p.N;
    {
        // one image: so few tiles that even 128 x 64 ones leave most CUs idle -- the ring kernel on K thirds (80 tiles x 3);
        // with the LayerNorm that follows folded into the reduce this also pays at K = 1024 (out-proj: 5 K-steps per part)
        const int tiles64 = ((rows + 127) / 128) * ((p.N + 63) / 64);
        const bool with_ln = ln_offered && p.N % 8 == 0 && p.N <= 2048 && p.ln_ldo % 8 == 0;     // (ln_w / ln_b null: no affine)
        int S = k.ring && p.N % 64 == 0 ? 256 / tiles64 : 0;
        S = S > 8 ? 8 : S;
        while (S > 1 && nt / S < (with_ln ? 4 : 8)) --S;
        if (p.K < 2048 && !with_ln) S = 0;
        if (S >= 2 && plane * S <= p.ws_elems) {
            GemmStep& s = gemm_add_step(pl, with_ln ? GF_SPLITK_RING_LN : GF_SPLITK_RING, row0, rows);
            s.S = S; s.reduce_ln = with_ln;
            s.grid_x = tiles64; s.grid_y = S;
            return true;
        }
    }
    if (p.K < 2048) return false;
    // XCD arrangement that spreads these few tiles most evenly (an XCD has 32 CUs: its tiles x S must fit)
    int gy = 1, per = 1 << 30;
    for (int g : {1, 2, 4, 8}) {
        const int r = gemm_xcd_region(tiles_m, tiles_n, g);
        if (r < per) { per = r; gy = g; }
    }
    int S = 32 / per;
    S = S > 8 ? 8 : S;
    while (S > 1 && nt / S < 8) --S;
    if (S < 2 || plane * S > p.ws_elems) return false;
    GemmStep& s = gemm_add_step(pl, GF_SPLITK_256, row0, rows);
    s.S = S; s.gy = gy;
    s.grid_x = 8 * per; s.grid_y = S;
    return true;
}

// The plan of a problem without the folded LayerNorm and the planes (gemm_plan adds them to a plan that can carry them).
static void gemm_plan_rows(const GemmProblem& p, const GemmKnobs& k, GemmPlan& pl) {
    const int e = p.epi;
    const bool windows = gemm_window_ok(p.lda) && gemm_window_ok(p.ldb);
    if (p.prefer256 && k.force_tile == 0 && windows) return gemm_plan_256(p, k, pl, 0, p.M, 0);
    // a few tiles with a long K (fc2 of one to a few images): the K loop is a latency chain, cut it across CUs
    if (e == EPI_RESID_F32 && k.force_tile == 0 && p.M > 64 && (p.K >= 2048 || (p.K >= 1024 && p.ln_offered)) &&
        gemm_tiles256(p.M, p.N) <= 96 && windows && gemm_plan_splitk(p, k, pl, 0, p.M, p.ln_offered))
        return;
    const bool splittable = e != EPI_PATCH && e != EPI_BF16_ROPE;       // (those two: never the skinny kernel, never main + leftover rows)
    if (splittable && gemm_use_skinny(k, p.M, p.N, p.K)) return gemm_plan_skinny(p, pl, 0, p.M);
    if (!gemm_use_256(p, k)) return gemm_plan_128(p, k, pl, 0, p.M);
    if (e == EPI_RESID_F32) {
        int tall = 0;
        if (const int t192 = gemm_plan_rows192(p, k, &tall)) {
            GemmStep& s = gemm_add_step(pl, GF_256P_192, 0, p.M);
            s.t192_tiles = t192; s.t192_tall = tall;
            return gemm_xcd_grid(s, t192, (p.N + 255) / 256, k, true);
        }
    }
    // Tail split: the 256 x 256 kernel takes the M rows that make whole rounds and the remaining rows go to a small-tile
    // form (two workgroups per CU, 4x shorter tiles)
    const GemmRounds r = gemm_rounds(p.M, p.N);
    const long m_tiles_main = r.full * 256 / r.tn;
    if (!(gemm_tail_splits(r, k) && k.force_tile == 0 && splittable && m_tiles_main >= 1 && m_tiles_main < r.tm))
        return gemm_plan_256(p, k, pl, 0, p.M, 0);
    const int m_main = (int)(m_tiles_main * 256), m_left = p.M - m_main;
    // at most 64 leftover rows behind whole rounds of the queued-stores kernel: done by that launch (qtail_rows)
    if ((e == EPI_BF16 || e == EPI_BF16_GELU) && m_left <= 64 && p.K % 256 == 0 && p.N % 16 == 0 && k.qtail && gemm_use_256q(p, k) &&
        gemm_persistent(k, m_main, p.N, p.K) && gemm_window_ok(p.lda, m_left))
        return gemm_plan_256(p, k, pl, 0, m_main, m_left);
    gemm_plan_256(p, k, pl, 0, m_main, 0);
    if (gemm_use_skinny(k, m_left, p.N, p.K)) return gemm_plan_skinny(p, pl, m_main, m_left);      // fc1 at batch 64: 64 rows are left over
    if (e == EPI_RESID_F32 && gemm_plan_splitk(p, k, pl, m_main, m_left, false)) return;     // (a LayerNorm is only fused into a form that covers ALL rows)
    gemm_plan_128(p, k, pl, m_main, m_left);
}

// The plan of launch_gemm(epi, args): gemm_problem(epi, args) under these knobs.
//
// The folded LayerNorm (kernels.h lnf_*) and the residual stream in planes (xp_*): only a plan that covers ALL rows with one
// launch of the persistent 256-row kernel -- whole rounds of 192-row tiles, or of 256-row tiles -- has the row-coalesced
// epilogue that writes bf16(x), the row statistics and the planes.  Such a plan carries them when they are offered; every
// other plan leaves *lnf_done alone (the caller runs the LayerNorm kernel), and planes asked of it are an error.
static GemmPlan gemm_plan(const GemmProblem& p, const GemmKnobs& k) {
    GemmPlan pl{};
    if ((pl.error = gemm_shape_error(p.M, p.N, p.K, p.lda, p.ldb, p.ldc))) return pl;
    gemm_plan_rows(p, k, pl);
    if (p.lnc) pl.forms |= GF_LN_CONSUMED;
    if (p.epi != EPI_RESID_F32) return pl;
    GemmStep& s = pl.step[0];
    const bool shape_folds = k.lnf && k.force_tile == 0 && p.N % LNF_SLICE == 0 && p.N / LNF_SLICE <= 6 && (p.ldc & 7) == 0;
    const bool can_fold = shape_folds && !p.prefer256 && pl.nsteps == 1 && (s.form == GF_256P || s.form == GF_256P_192);
    const bool fold = can_fold && p.fold_offered && p.lnf_ldxb % 8 == 0;
    if (p.xp_in || p.xp_out) {
        if (!can_fold || !p.planes_valid || (p.xp_out && !fold)) {
            pl.error = "gemm: the residual stream in planes needs a launch form that folds (gemm_resid_folds) and, for xp_out, "
                       "the folded LayerNorm's outputs with xp_hi == lnf_xb";
            return pl;
        }
        s.xp = p.xp_in ? (p.xp_out ? 2 : 3) : 1;
        pl.forms |= (p.xp_in ? GF_PLANES_IN : 0u) | (p.xp_out ? GF_PLANES_OUT : 0u);
    }
    if (fold) { s.fold = true; pl.forms |= GF_LN_FOLDED; }
    return pl;
}

}  // namespace revo
