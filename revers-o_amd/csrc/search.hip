// C ABI of the certified top-k search (include/revo.h): the search pipeline with its exactness fallback, large k, grouped
// search, the row-sharded protocol's entry points, the merges and the stats.  The handle: gallery_internal.h.
#include <cmath>
#include <cstdlib>

#include "gallery_internal.h"

#ifdef REVO_EXPERIMENTS
// experiment (bound exchange between shards): raise the scan's admission bounds to values handed in
__global__ void seed_bounds_kernel(uint32_t* tau, const uint32_t* seed, int Q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Q && seed[i] > tau[i]) tau[i] = seed[i];
}
#endif
// Rows of the pre-pass of the 256 x 256 scan: about one round of GEMM tiles, at most a quarter of the gallery
static long search_prepass_rows(int Q, long N) {
#ifdef REVO_EXPERIMENTS
    // (sweep of the pre-pass size, scripts/: 2048 / 4096 / 8192 / 16384 rows at 10 000 queries -> 4.22 / 3.43 / 3.36 /
    //  3.50 ms per search of a 125 k-row shard: 8192 it is)
    if (const char* e = getenv("REVO_NPRE")) { const long v = atol(e) / 256 * 256; if (v >= 1024 && v <= N / 4) return v; }
#endif
    // (few queries, 1 M rows, whole search in ms at 1 / 64 queries: 8192 rows 0.557 / 0.600, 16 384 0.555 / 0.596, 32 768
    //  0.529 / 0.566, 65 536 0.564 / 0.596: a weaker seed costs the HBM-rate scan more survivors than the rows save)
    const long qtiles = (Q + 255) / 256;
    long n_pre = (65536 / qtiles) / 256 * 256;
    n_pre = n_pre > 32768 ? 32768 : (n_pre < 8192 ? 8192 : n_pre);
    if (n_pre > N / 4) n_pre = (N / 4) / 256 * 256;
    const long cap_pre = ((512l << 20) / (4l * Q)) / 256 * 256;
    if (n_pre > cap_pre) n_pre = cap_pre;
    if (n_pre < 1024) n_pre = 1024;
    return n_pre;
}

// z with P(standard normal > z) = p (Acklam's rational approximation, |relative error| < 1.2e-9; 0 < p < 0.5 here)
static double upper_normal_quantile(double p) {
    static const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
                               -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
                               -1.328068155288572e+01};
    static const double c[] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
                               4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
    if (p < 0.02425) {
        const double q = std::sqrt(-2.0 * std::log(p));
        return -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
    }
    const double q = (1.0 - p) - 0.5, r = q * q;
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
           (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

// The handle's per-query arrays, grown to hold Q queries (every search that normalises queries into the handle)
int search_grow_queries(revo_gallery* g, int Q, hipStream_t st) {
    using namespace revo;
    const int D = g->D;
    if (g->q_cap < Q) {
        g->q_cap = 0; g->xw = ExactWs{};
        CHECK_RC(g->qf.grow((size_t)Q * D * 4, st)); CHECK_RC(g->qb.grow((size_t)Q * D * 2, st));
        CHECK_RC(g->tau0.grow((size_t)Q * 4 * 2, st)); CHECK_RC(g->qstat.grow((size_t)Q * 8, st));   // tau0: pre-pass | live bounds
        CHECK_RC(g->marg.grow((size_t)Q * 4, st)); CHECK_RC(g->dropflag.grow((size_t)Q * 4, st));
        if (g->keep_f32) {
            // fallback workspace of the exactness certificate; the counters come first, zeroed here and by every search
            ExactWs xw{};
            CHECK_RC(carve_buffer(g->xbuf, st, [&](Layout& l) {
                xw.ctr = l.take<int>(CTR_SLOTS);
                xw.unc_q = l.take<int>(Q); xw.unc_lb = l.take<float>(Q); xw.col_cnt = l.take<int>(Q);
                xw.over_j = l.take<int>(Q); xw.orow = l.take<int>(Q); xw.qb_u = l.take<bf16_t>((size_t)Q * D); xw.ldqb = D;
                xw.col = l.take<uint64_t>((size_t)Q * EXACT_COL_CAP); xw.cap = Q;
            }));
            REVO_HIP_CHECK(hipMemsetAsync(xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
            g->xw = xw;
        }
        g->q_cap = Q;
    }
    return 0;
}

// Phase 1 of a search: normalise the queries, scan the gallery (bf16 MFMA scores) and leave each query's best
// ksel candidates, sorted best first, in the handle (cand / cand_stride).  The gallery must not be empty.
static int search_candidates(revo_gallery* g, const float* queries, int Q, int ksel, const uint32_t* allow, hipStream_t st,
                             uint32_t* bounds = nullptr, int top_m = 0, bool margin = false) {
    using namespace revo;
    const int D = g->D;
    const long N = g->size;
    g->drop_two_phase();
    CHECK_RC(search_grow_queries(g, Q, st));
    // the admission margin only pays where the certificate is expected to fail (see revo_search_topk) and only the
    // 256 x 256 scan has segments; it needs the fp32 rows (no certificate without them)
    margin = margin && g->keep_f32 && N >= SEARCH_SMALL_ROWS;
    // (a filtered scan of more than 128 queries has no margin form: launch_topk_scan256; its uncertified queries take the
    //  collect pass instead -- exact either way)
    if (allow && Q > 128) margin = false;
    // query normalisation (+ rounding norms); the same kernel clears the certificate's counters and -- 256 x 256 scan -- the
    // score histograms (two memset launches fewer per search: a quarter of a one-query search is launches)
    auto prep = [&](uint32_t* hist, long hist_words) -> int {
        ProfScope ps("search_prep", st);
        CHECK_RC(launch_l2norm_rows(queries, D, g->qf.p, D, g->qb.p, D, Q, D, st, 1, g->qstat.p, nullptr,
                                    (uint32_t*)g->xw.ctr, g->xw.ctr ? CTR_SLOTS : 0, hist, hist_words));
        if (margin) CHECK_RC(launch_cert_margin(g->qstat.p, g->gstat.p, D, Q, g->marg.p, g->dropflag.p, st));
        return 0;
    };

    if (N >= SEARCH_SMALL_ROWS) {
        // ---- 256 x 256 scan.  Pre-pass: a plain GEMM of the queries against the first n_pre rows and a
        // per-row selection seed the admission scores; the fused scan covers rows [n_pre, N).
        // Pre-pass size: about one round of 256 x 256 GEMM tiles; with few queries (short gallery slices
        // per CU) up to 32 k rows, which seed the 0.1 % quantile.
        const long n_pre = search_prepass_rows(Q, N);
        // the scan runs as one launch, or as a main launch of whole query tiles plus one for a ragged tail of queries
        const int q_main = topk_scan256_main_queries(Q, N - n_pre);
        struct Part { int q0, nq, splits; uint64_t* seg; int* cnt; } parts[2] = {{0, q_main, 0}, {q_main, Q - q_main, 0}};
        const int nparts = q_main < Q ? 2 : 1;
        for (int i = 0; i < nparts; ++i) parts[i].splits = topk_scan256_splits(parts[i].nq, N - n_pre);
        const int NB = topk_scan256_hist_buckets();
        // workspace: histograms (zeroed) | per part: segment counts, segments | pre-pass lists | final lists | pre-pass scores
        uint32_t* hist; uint64_t *prelist, *final_lists; float* pre_scores;
        CHECK_RC(carve_buffer(g->part, st, [&](Layout& l) {
            hist = l.take<uint32_t>((size_t)Q * NB);
            for (int i = 0; i < nparts; ++i) {
                Part& pt = parts[i];
                pt.cnt = l.take<int>((size_t)pt.nq * pt.splits);
                pt.seg = l.take<uint64_t>((size_t)pt.nq * pt.splits * (2 * ksel));
            }
            prelist = l.take<uint64_t>((size_t)Q * ksel);
            final_lists = l.take<uint64_t>((size_t)Q * ksel);
            pre_scores = l.take<float>((size_t)Q * n_pre);
        }));
        uint32_t* tau_base = g->tau0.p, *tau_live = g->tau0.p + g->q_cap;
        CHECK_RC(prep(hist, (long)Q * NB));
        {
            ProfScope ps("topk_prepass", st);
            GemmArgs ga{};
            ga.A = g->qb.p; ga.lda = D; ga.B = g->gb.p; ga.ldb = D; ga.M = Q; ga.N = (int)n_pre; ga.K = D;
            ga.C = pre_scores; ga.ldc = n_pre; ga.prefer256 = 1;
            // (few queries: the skinny form instead -- measured: pre-pass 48 -> 37 us at one query, 50 -> 57 at 64; nothing in the search)
            // Up to 128 queries: 128 x 64 tiles on the six-deep ring (two rounds of workgroups with five K-steps of loads in
            // flight; one 256 x 256 tile per CU is a chain of sixteen DMA latencies): pre-pass 48 -> 40 us at one query,
            // 49 -> 42 at 64, 52 -> 46 at 128
            bool ring = Q <= 128 && n_pre % 64 == 0;
#ifdef REVO_EXPERIMENTS
            if (getenv("REVO_PREPASS_256")) ring = false;
#endif
            if (ring) CHECK_RC(launch_gemm_f32_ring(ga, st));
            else CHECK_RC(launch_gemm(EPI_F32, ga, st));
            // One shard of a larger gallery, in the two-phase search: what its candidates have to reach is decided by ALL
            // shards' rows (the finish step re-scores only candidates among the best min(64, 2 ksel) of the whole gallery),
            // but its scan can only learn its own rows' scores -- at an eighth of the rows its admission bound sits at an
            // 8 x higher quantile and a third of its tile fragments still hold a survivor.  So it
            // starts from an ESTIMATE of the whole gallery's level, extrapolated from its own pre-pass scores
            // (topk_select_rows_kernel); an estimate, not a bound: the protocol's certificate and second round cover it.
            float est_z = 0.f;
            // (not under a filter: the estimate extrapolates from ALL of the whole gallery's rows, a filtered search needs the
            //  level of the allowed ones -- the bound exchange decides instead)
            if (bounds && !margin && g->total_rows > N && !allow) {
                int j = 2 * ksel < 64 ? 2 * ksel : 64;
#ifdef REVO_EXPERIMENTS
                if (const char* e = getenv("REVO_EST_J")) j = atoi(e) > 0 ? atoi(e) : j;      // sweep of the estimate's rank (scripts/)
#endif
                est_z = (float)upper_normal_quantile((double)j / (double)g->total_rows);
                g->two.estimated = true;
            }
            CHECK_RC(launch_topk_select_rows(pre_scores, n_pre, (int)n_pre, Q, prelist, ksel, 0, tau_base, ksel, hist, NB,
                                             topk_scan256_hist_shift(), st, tau_live, est_z, allow));
#ifdef REVO_EXPERIMENTS
            if (g->seed_bounds) hipLaunchKernelGGL(seed_bounds_kernel, dim3((Q + 255) / 256), dim3(256), 0, st, tau_live, g->seed_bounds, Q);
#endif
        }
        { ProfScope ps("topk_scan", st);
          for (int i = 0; i < nparts; ++i) {
              const Part& pt = parts[i];
              CHECK_RC(launch_topk_scan256(g->qb.p + (size_t)pt.q0 * D, D, g->gb.p, D, pt.nq, N, D, n_pre, pt.splits,
                                           pt.seg, pt.cnt, tau_live + pt.q0, tau_base + pt.q0, hist + (size_t)pt.q0 * NB, ksel, st,
                                           margin ? g->marg.p + pt.q0 : nullptr, margin ? g->dropflag.p + pt.q0 : nullptr, allow));
              if (margin) g->two.segs[i] = SegSrc{pt.seg, pt.cnt, pt.splits, pt.q0, pt.nq};
          }
          if (margin) { g->two.nsegs = nparts; g->two.prelist = prelist; } }
        { ProfScope ps("topk_reduce", st);
          for (int i = 0; i < nparts; ++i) {
              const Part& pt = parts[i];
              CHECK_RC(launch_topk_reduce_segs(pt.seg, pt.cnt, pt.splits, prelist + (size_t)pt.q0 * ksel,
                                               final_lists + (size_t)pt.q0 * ksel, pt.nq, ksel, st,
                                               bounds ? bounds + (size_t)pt.q0 * top_m : nullptr, top_m));
          } }
        g->two.cand = final_lists; g->two.stride = ksel;
    } else {
        // ---- small galleries: 128 x 128 scan with per-wave LDS lists
        const int splits = topk_scan_workspace_splits(Q, N);
        CHECK_RC(g->part.grow((size_t)Q * splits * ksel * 8, st));
        uint64_t* part = (uint64_t*)g->part.p;
        CHECK_RC(prep(nullptr, 0));
        ScanArgs a{};
        a.Qb = g->qb.p; a.ldq = D; a.Gb = g->gb.p; a.ldg = D; a.Q = Q; a.N = N; a.D = D; a.ksel = ksel;
        a.splits = splits; a.part = part; a.allow = allow;
        { ProfScope ps("topk_scan", st); CHECK_RC(launch_topk_scan(a, st)); }
        { ProfScope ps("topk_reduce", st); CHECK_RC(launch_topk_reduce(part, Q, splits, ksel, st)); }
        g->two.cand = part; g->two.stride = (long)splits * ksel;
        if (bounds) { ProfScope ps("topk_bounds", st); CHECK_RC(launch_topk_publish(g->two.cand, g->two.stride, Q, top_m, bounds, st)); }
    }
    g->two.Q = Q; g->two.ksel = ksel;
    return 0;
}

// The fallback of the exactness certificate for the entries in the handle's workspace (count on the device): collect
// pass, exact re-score of what it collected, brute force for the entries whose lists overflowed.  Idle passes cost a
// few microseconds each.
static int search_fallback(revo_gallery* g, int max_entries, int k, int has_thr, float thr, long index_offset, int out_compact,
                           float* scores, long long* indices, int* counts, const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    ProfScope ps("topk_exact", st);
    if (g->mode != 2) {
        Collect256Args ca{};
        ca.Qb = g->xw.qb_u; ca.ldq = g->xw.ldqb; ca.Gb = g->gb.p; ca.ldg = g->D; ca.N = g->size; ca.D = g->D;
        ca.n_q = g->xw.ctr + CTR_UNCERTIFIED; ca.lb = g->xw.unc_lb; ca.cnt = g->xw.col_cnt; ca.col = g->xw.col;
        ca.cap = EXACT_COL_CAP; ca.allow = allow;
        CHECK_RC(launch_topk_collect256(ca, max_entries, st));
    }
    CHECK_RC(launch_topk_exact_finish(g->xw, max_entries, g->qf.p, g->D, g->gf.p, g->D, g->D, k, has_thr, thr, index_offset,
                                      g->mode == 2, out_compact, scores, indices, counts, st));
    return launch_topk_exact_bruteforce(g->xw, max_entries, g->qf.p, g->D, g->gf.p, g->D, g->size, g->D, k, has_thr, thr,
                                        index_offset, out_compact, scores, indices, counts, st, allow);
}

// over-selection: the bf16 scan keeps ksel >= k + margin candidates, the fp32 re-score decides
static int search_ksel(int k) { return (k <= 16) ? 32 : 64; }
extern "C" int32_t revo_search_ksel(int32_t k) { return (k >= 1 && k <= 50) ? search_ksel(k) : -1; }
// k > 25: the scan runs with the admission margin (revo_search_topk); a shard's two-phase scan estimates the whole gallery's
// admission level only without it -- one rule, asked for by the host side that decides whether to exchange bounds
static bool search_uses_margin(int k) { return k > 25; }
extern "C" int32_t revo_search_estimates(int32_t k) { return (k >= 1 && k <= 50) ? (search_uses_margin(k) ? 0 : 1) : -1; }
extern "C" int32_t revo_search_plan(const revo_gallery* g, int32_t Q, int32_t k, int64_t* out4) {
    REVO_REQUIRE(g && out4 && Q >= 1 && k >= 1 && k <= 50, "search_plan: bad arguments");
    const long N = g->size;
    const bool big = N >= SEARCH_SMALL_ROWS;
    const long n_pre = big ? search_prepass_rows(Q, N) : 0;
    out4[0] = big ? 1 : 0;
    out4[1] = n_pre;
    out4[2] = big ? revo::topk_scan256_splits(revo::topk_scan256_main_queries(Q, N - n_pre), N - n_pre)
                  : revo::topk_scan_workspace_splits(Q, N);
    out4[3] = N >= SEARCH_WIDE_ROWS ? 64 : search_ksel(k);
    return 0;
}

// revo_search_topk / revo_search_groups after their argument checks (Q >= 1, device current, `allow` = search_filter)
static int search_topk(revo_gallery* g, const float* queries, int Q, int k, int has_thr, float thr, long index_offset,
                       float* scores, long long* indices, int* counts, const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    if (g->size == 0) return launch_topk_fill_empty(scores, indices, counts, Q, k, st);
    // candidates per query: 32 for k <= 16, 64 beyond -- and 64 on very large galleries whatever k is: there a query
    // that fails its certificate costs a whole extra pass over the gallery (10 M x 1536: 5.9 ms next to a 7.7 ms scan),
    // and the wider list all but rules that out (the k-th to 64th score gap is 1.6 x the k-th to 32nd) for 0.1 ms of re-scores
    int ksel = g->size >= SEARCH_WIDE_ROWS ? 64 : search_ksel(k);
#ifdef REVO_EXPERIMENTS
    if (const char* e = getenv("REVO_KSEL")) ksel = atoi(e) == 64 ? 64 : ksel;         // candidate-list width study (scripts/)
#endif
    // k > 25: 64 candidates leave the certificate less room than its error bound on ordinary data (the 50th-to-64th score
    // gap of a random 1 M gallery is half of eps), so nearly every query fails it.  The scan then runs with an admission
    // margin of 2 eps: what an uncertified query needs is in its segments, and no second pass over the gallery is made
    // (Not for smaller k, not even on very large galleries where a second pass costs most of a search: measured on 10 M x
    //  1536 with 256 queries, the margin's extra survivors cost the scan 18 % on EVERY search -- 7.5 -> 8.9 ms -- to save a
    //  pass that the 64-candidate lists kept there for every k already make a rarity.)
    CHECK_RC(search_candidates(g, queries, Q, ksel, allow, st, nullptr, 0, search_uses_margin(k)));
    const CertArgs ca = g->cert_args(nullptr);
    { ProfScope ps("topk_finish", st);
      CHECK_RC(launch_topk_finish(g->two.cand, g->two.stride, ksel, g->qf.p, g->D, g->keep_f32 ? g->gf.p : nullptr, g->D, g->D, Q, k,
                                  has_thr, thr, index_offset, nullptr, 0, 0, scores, indices, counts,
                                  g->keep_f32 ? &ca : nullptr, st)); }
    if (g->keep_f32 && g->mode != 3)
        CHECK_RC(search_fallback(g, Q, k, has_thr, thr, index_offset, 0, scores, indices, counts, allow, st));
    return 0;
}

extern "C" int32_t revo_search_topk(revo_gallery* g, const float* queries, int32_t Q, int32_t k, int32_t has_thr,
                                    float thr, int64_t index_offset, float* scores, int64_t* indices, int32_t* counts,
                                    void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (queries || Q == 0), "search: null argument");
    REVO_REQUIRE(Q >= 0, "search: negative query count");
    REVO_REQUIRE(k >= 1 && k <= 50, "search: k must be in [1, 50]");
    if (Q == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_topk(g, queries, Q, k, has_thr, thr, index_offset, scores, (long long*)indices, counts, allow,
                       (hipStream_t)stream);
    API_END
}

// ---- large k (include/revo.h revo_search_topk_large; topk_large.hip)
constexpr int LARGE_CHUNK = 1024;   // queries per pass of the pipeline (the workspace is sized for one chunk)
// Rows of the large-k sample: what the pre-pass of the k <= 50 search would take, at least 64 k (the sample's k-th best is then
// about the gallery's (N / n_s) k-th: fewer rows counted and a tighter start for the buckets), at most a quarter of the
// gallery and 512 MB of scores.  None below the small-gallery size: lo = -inf there, the count pass histograms every row.
long large_sample_rows(int Q, long N, int k) {
    if (N < SEARCH_SMALL_ROWS) return 0;
    long n = search_prepass_rows(Q, N);
    const long want = (64l * k + 255) / 256 * 256;
    if (n < want) n = want;
    if (n > N / 4) n = (N / 4) / 256 * 256;
    const long cap = ((512l << 20) / (4l * Q)) / 256 * 256;
    return n < cap ? n : cap;
}
// Fallback entries per round: F score rows of N floats, at most 256 MB (and at least one row, whatever N is)
static int large_fallback_rows(int Qc, long N) {
    long f = (256l << 20) / (4l * (N > 0 ? N : 1));
    f = f < 1 ? 1 : f;
    return (int)(f < Qc ? f : Qc);
}
int search_topk_large(revo_gallery* g, const float* queries, int Q, int k, int has_thr, float thr, long index_offset,
                             float* scores, long long* indices, int* counts, const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    const int QC = Q < LARGE_CHUNK ? Q : LARGE_CHUNK;
    if (g->size == 0) {
        for (int c0 = 0; c0 < Q; c0 += QC)
            CHECK_RC(launch_topk_fill_empty(scores + (size_t)c0 * k, indices + (size_t)c0 * k, counts + c0,
                                            Q - c0 < QC ? Q - c0 : QC, k, st));
        return 0;
    }
    const int D = g->D;
    const long N = g->size;
    g->drop_two_phase();
    CHECK_RC(search_grow_queries(g, QC, st));
    REVO_REQUIRE(g->xw.ctr, "search_topk_large: no certificate workspace");
    const long n_s = large_sample_rows(QC, N, k);
    LargeWs ws{};
    ws.F = large_fallback_rows(QC, N);
    ws.stats = g->xw.ctr;
    float* pre = nullptr; uint32_t* zeroed = nullptr;
    CHECK_RC(carve_buffer(g->lbuf, st, [&](Layout& l) {
        zeroed = l.take<uint32_t>(64 + (size_t)QC * LARGE_NB);       // entry counters | histograms
        ws.lvl = l.take<float>((size_t)QC * LARGE_LVL);
        ws.band_q = l.take<int>(QC); ws.band_lb = l.take<float>(QC); ws.band_cnt = l.take<int>(QC);
        ws.band_qb = l.take<bf16_t>((size_t)QC * D);
        ws.band_col = l.take<uint64_t>((size_t)QC * LARGE_CAP);
        ws.fb_q = l.take<int>(QC);
        ws.fb_scores = l.take<float>((size_t)ws.F * N);
        pre = l.take<float>((size_t)QC * n_s);
    }));
    ws.ctr = (int*)zeroed; ws.hist = zeroed + 64;
    for (int c0 = 0; c0 < Q; c0 += QC) {
        const int Qc = Q - c0 < QC ? Q - c0 : QC;
        float* s_out = scores + (size_t)c0 * k; long long* i_out = indices + (size_t)c0 * k; int* c_out = counts + c0;
        { ProfScope ps("search_prep", st);
          // the first chunk also clears the handle's counters (revo_search_stats: the whole search's)
          CHECK_RC(launch_l2norm_rows(queries + (size_t)c0 * D, D, g->qf.p, D, g->qb.p, D, Qc, D, st, 1, g->qstat.p, nullptr,
                                      c0 == 0 ? (uint32_t*)g->xw.ctr : nullptr, c0 == 0 ? CTR_SLOTS : 0, zeroed,
                                      64 + (long)Qc * LARGE_NB)); }
        { ProfScope ps("large_sample", st);
          if (n_s > 0) {
              GemmArgs ga{};
              ga.A = g->qb.p; ga.lda = D; ga.B = g->gb.p; ga.ldb = D; ga.M = Qc; ga.N = (int)n_s; ga.K = D;
              ga.C = pre; ga.ldc = n_s; ga.prefer256 = 1;
              if (Qc <= 128 && n_s % 64 == 0) CHECK_RC(launch_gemm_f32_ring(ga, st));
              else CHECK_RC(launch_gemm(EPI_F32, ga, st));
          }
          CHECK_RC(launch_topk_large_sample(pre, n_s, (int)n_s, allow, g->qstat.p, g->gstat.p, D, Qc, k, has_thr, thr, ws, st)); }
        { ProfScope ps("large_count", st);
          CHECK_RC(launch_topk_large_count(g->qb.p, D, g->gb.p, D, N, D, Qc, ws, allow, st)); }
        { ProfScope ps("large_level", st);
          CHECK_RC(launch_topk_large_level(ws, g->qb.p, D, D, Qc, k, g->mode == 2, st)); }
        { ProfScope ps("large_collect", st);
          Collect256Args ca{};
          ca.Qb = ws.band_qb; ca.ldq = D; ca.Gb = g->gb.p; ca.ldg = D; ca.N = N; ca.D = D;
          ca.n_q = ws.ctr; ca.lb = ws.band_lb; ca.cnt = ws.band_cnt; ca.col = ws.band_col; ca.cap = LARGE_CAP; ca.allow = allow;
          CHECK_RC(launch_topk_collect256(ca, Qc, st)); }
        { ProfScope ps("large_finish", st);
          CHECK_RC(launch_topk_large_finish(ws, Qc, g->qf.p, D, g->gf.p, D, D, k, has_thr, thr, index_offset, s_out, i_out, c_out,
                                            st)); }
        { ProfScope ps("large_fallback", st);
          CHECK_RC(launch_topk_large_fallback(ws, Qc, g->qf.p, D, g->gf.p, D, N, D, k, has_thr, thr, index_offset, s_out, i_out,
                                              c_out, allow, st)); }
    }
    return 0;
}

extern "C" int32_t revo_search_topk_large(revo_gallery* g, const float* queries, int32_t Q, int32_t k, int32_t has_thr,
                                          float thr, int64_t index_offset, float* scores, int64_t* indices, int32_t* counts,
                                          void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (queries || Q == 0), "search_topk_large: null argument");
    REVO_REQUIRE(Q >= 0, "search_topk_large: negative query count");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_topk_large: k must be in [1, 1024]");
    CHECK_RC(require_f32_rows(g, "search_topk_large"));
    if (Q == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_topk_large(g, queries, Q, k, has_thr, thr, index_offset, scores, (long long*)indices, counts, allow,
                             (hipStream_t)stream);
    API_END
}

// ---- the same search in two phases, for a gallery that is row-sharded over several GPUs (include/revo.h)
extern "C" int32_t revo_search_candidates(revo_gallery* g, const float* queries, int32_t Q, int32_t k, int32_t top_m,
                                          uint32_t* bounds, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && bounds && (queries || Q == 0), "search_candidates: null argument");
    REVO_REQUIRE(Q >= 0, "search_candidates: negative query count");
    REVO_REQUIRE(k >= 1 && k <= 50, "search_candidates: k must be in [1, 50]");
    const int ksel = search_ksel(k);
    REVO_REQUIRE(top_m >= 1 && top_m <= ksel, "search_candidates: top_m must be in [1, revo_search_ksel(k)]");
    if (Q == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    g->two.cand = nullptr; g->two.Q = Q; g->two.ksel = ksel;
    if (g->size == 0) {                                   // an empty shard publishes nothing
        REVO_HIP_CHECK(hipMemsetAsync(bounds, 0, (size_t)Q * top_m * 4, st));
        return 0;
    }
    // (the published scores come out of the final selection kernel: no launch of their own; k > 25: with the admission
    //  margin, so that the second round the merge's certificate then asks for needs no pass over the shard -- revo_search_topk)
    return search_candidates(g, queries, Q, ksel, allow, st, bounds, top_m, search_uses_margin(k));
    API_END
}
extern "C" int32_t revo_search_finish(revo_gallery* g, int32_t Q, int32_t k, int32_t has_thr, float thr,
                                      int64_t index_offset, const uint32_t* all_bounds, int32_t parts, int32_t top_m,
                                      float* scores, int64_t* indices, int32_t* counts, float* cert, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts, "search_finish: null argument");
    REVO_REQUIRE(k >= 1 && k <= 50 && Q >= 0, "search_finish: bad k or query count");
    REVO_REQUIRE(Q == g->two.Q && search_ksel(k) == g->two.ksel,
                 "search_finish: no matching revo_search_candidates call on this handle");
    REVO_REQUIRE(!all_bounds || (parts >= 1 && top_m >= 1 && top_m <= g->two.ksel), "search_finish: bad bounds layout");
    // A scan that started from an ESTIMATED admission level (revo_search_set_total_rows) has dropped rows on the strength of
    // that estimate: only the certificate (cert -> revo_topk_merge_packed -> revo_search_exact) makes the result exhaustive
    REVO_REQUIRE(cert || !g->two.estimated,
                 "search_finish: this shard scanned against an estimated admission level (revo_search_set_total_rows): cert must "
                 "be given and checked by revo_topk_merge_packed, with revo_search_exact as the second round");
    if (Q == 0) return 0;
    { const uint32_t* allow; CHECK_RC(search_filter(g, &allow)); }
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    if (g->size == 0 || !g->two.cand) {
        // an empty shard holds no row that could change a result: its certificate bound is -inf
        if (cert) REVO_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)cert, (int)0xff800000u, (size_t)Q, st));
        return launch_topk_fill_empty(scores, (long long*)indices, counts, Q, k, st);
    }
    ProfScope ps("topk_finish", st);
    const CertArgs ca = g->cert_args(cert);
    return launch_topk_finish(g->two.cand, g->two.stride, g->two.ksel, g->qf.p, g->D, g->keep_f32 ? g->gf.p : nullptr, g->D, g->D,
                              Q, k, has_thr, thr, index_offset, all_bounds, parts, top_m, scores, (long long*)indices,
                              counts, cert ? &ca : nullptr, st);
    API_END
}

// Second round of a row-sharded search: exact local results for the queries the merge step could not certify.
extern "C" int32_t revo_search_exact(revo_gallery* g, int32_t n, const int32_t* q_idx, const float* need, int32_t k,
                                     int32_t has_thr, float thr, int64_t index_offset, float* scores, int64_t* indices,
                                     int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (n == 0 || (q_idx && need)), "search_exact: null argument");
    REVO_REQUIRE(k >= 1 && k <= 50 && n >= 0, "search_exact: bad k or entry count");
    REVO_REQUIRE(n <= g->two.Q, "search_exact: more entries than queries in the last revo_search_candidates call");
    if (n == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    if (g->size == 0) return launch_topk_fill_empty(scores, (long long*)indices, counts, n, k, st);
    REVO_REQUIRE(g->keep_f32 && g->xw.ctr, "search_exact: the gallery was created without the fp32 master copy");
    const CertArgs ca = g->cert_args(nullptr);
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    CHECK_RC(launch_topk_exact_prepare(g->xw, q_idx, need, n, ca, g->D, g->two.cand, g->two.stride, g->two.ksel, st));
    return search_fallback(g, n, k, has_thr, thr, index_offset, 1, scores, (long long*)indices, counts, allow, st);
    API_END
}

// Grouped search (include/revo.h): the certified search at k = GROUP_K1 into the handle's workspace, the groups of each
// query's list (certified, or an entry of the grouped fallback), the fallback's fp32 passes over the gallery.  Every launch
// is sized for Q entries and reads the entry count from the device.
extern "C" int32_t revo_search_groups(revo_gallery* g, const float* queries, int32_t Q, int32_t limit, int32_t group_size,
                                      int32_t has_thr, float thr, int64_t index_offset, float* scores, int64_t* indices,
                                      int32_t* hit_counts, int32_t* group_ids, int32_t* group_counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(Q >= 0, "search_groups: negative query count");
    REVO_REQUIRE(limit >= 1 && limit <= 50 && group_size >= 1 && group_size <= 50 && limit * group_size <= 50,
                 "search_groups: needs 1 <= limit, 1 <= group_size and limit * group_size <= 50");
    REVO_REQUIRE(g, "search_groups: null handle");
    REVO_REQUIRE(scores && indices && hit_counts && group_ids && group_counts && (queries || Q == 0), "search_groups: null argument");
    CHECK_RC(require_f32_rows(g, "search_groups"));
    REVO_REQUIRE(g->groups_rows >= 0, "search_groups: no group ids set (revo_search_set_groups)");
    REVO_REQUIRE(g->groups_rows == g->size,
                 "search_groups: the group ids were set for " + std::to_string(g->groups_rows) + " rows but the gallery holds " +
                     std::to_string(g->size) + " (set them again after appending)");
    if (Q == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    float* s1; long long* i1; int* c1;
    GroupWs gw{};
    CHECK_RC(carve_buffer(g->gbuf, st, [&](Layout& l) {
        s1 = l.take<float>((size_t)Q * GROUP_K1); i1 = l.take<long long>((size_t)Q * GROUP_K1);
        c1 = l.take<int>(Q); gw.gq = l.take<int>(Q);
        gw.chosen = l.take<int>((size_t)Q * 64);
    }));
    CHECK_RC(search_topk(g, queries, Q, GROUP_K1, has_thr, thr, 0, s1, i1, c1, allow, st));
    ProfScope ps("topk_groups", st);
    gw.group_of_row = g->groups.p; gw.has_thr = has_thr ? 1 : 0; gw.thr = thr;
    GroupOut o{};
    o.scores = scores; o.idx = (long long*)indices; o.hit_counts = hit_counts; o.group_ids = group_ids;
    o.group_counts = group_counts; o.limit = limit; o.group_size = group_size; o.idx_offset = (long)index_offset;
    // (an empty gallery: the search wrote empty lists and left the counters alone -- every query is certified)
    if (g->size == 0) return launch_topk_group_select(s1, i1, c1, Q, g->xw, gw, 0, o, st);
    REVO_REQUIRE(g->xw.ctr, "search_groups: no certificate workspace");
    CHECK_RC(launch_topk_group_select(s1, i1, c1, Q, g->xw, gw, g->mode == 2, o, st));
    return launch_topk_group_fallback(g->xw, gw, Q, g->qf.p, g->D, g->gf.p, g->D, g->size, g->D, allow, o, st);
    API_END
}

#ifdef REVO_EXPERIMENTS   // librevo.so cannot be put into a non-exact mode
extern "C" int32_t revo_search_set_mode(revo_gallery* g, int32_t mode) {
    REVO_REQUIRE(g && mode >= 0 && mode <= 3, "search_set_mode: mode must be 0..3");
    g->mode = mode;
    return 0;
}
#endif
extern "C" int32_t revo_search_stats(revo_gallery* g, int32_t* out8, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && out8, "search_stats: null argument");
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!g->xw.ctr) { out8[0] = -1; return 0; }     // no fp32 master rows (or no search yet): nothing was certified
    REVO_ON_DEVICE(g->device);
    using namespace revo;
    int c[CTR_SLOTS];
    REVO_HIP_CHECK(hipMemcpyAsync(c, g->xw.ctr, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));   // on `stream`, like revo_vit_stats
    REVO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    out8[0] = c[CTR_UNCERTIFIED] + c[CTR_MODE3_FAILED] + c[CTR_FROM_SEGS]; out8[1] = c[CTR_BRUTEFORCE];
    out8[2] = c[CTR_CHECKED]; out8[3] = c[CTR_COLLECTED]; out8[4] = c[CTR_FROM_SEGS]; out8[5] = c[CTR_GROUPED];
    out8[6] = c[CTR_LARGE_FALLBACK]; out8[7] = c[CTR_PAIR_PASSES];
    return 0;
    API_END
}

extern "C" int32_t revo_topk_merge(const float* scores, const int64_t* indices, int32_t parts, int32_t Q, int32_t k,
                                   int32_t has_thr, float thr, float* out_scores, int64_t* out_indices,
                                   int32_t* out_counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(scores && indices && out_scores && out_indices && out_counts, "merge: null argument");
    ProfScope ps("topk_merge", (hipStream_t)stream);
    return revo::launch_topk_merge(scores, (const long long*)indices, parts, Q, k, has_thr, thr, out_scores,
                                   (long long*)out_indices, out_counts, (hipStream_t)stream);
    API_END
}

extern "C" int64_t revo_topk_packed_bytes(int32_t Q, int32_t k) {
    return Q < 0 || k < 1 ? -1 : (((int64_t)Q * k * 12 + (int64_t)Q * 4 + 15) / 16) * 16;
}
extern "C" int32_t revo_topk_merge_packed(const void* packed, int32_t parts, int32_t Q, int32_t k, int32_t has_thr, float thr,
                                          float* out_scores, int64_t* out_indices, int32_t* out_counts,
                                          int32_t* unc_count, int32_t* unc_q, float* unc_need, void* stream) {
    API_BEGIN
    REVO_REQUIRE(packed && out_scores && out_indices && out_counts, "merge: null argument");
    REVO_REQUIRE(Q >= 0 && k >= 1, "merge: bad sizes");
    REVO_REQUIRE(!unc_count || (unc_q && unc_need), "merge: the certificate needs all three of unc_count, unc_q, unc_need");
    const int64_t pb = revo_topk_packed_bytes(Q, k);
    ProfScope ps("topk_merge", (hipStream_t)stream);
    // part p: [Q][k] int64 indices, then [Q][k] fp32 scores, then [Q] fp32 certificate bounds
    revo::MergeCert mc{};
    if (unc_count) {
        REVO_HIP_CHECK(hipMemsetAsync(unc_count, 0, 4, (hipStream_t)stream));
        mc.cert = (const float*)((const char*)packed + (size_t)Q * k * 12); mc.cert_part_stride = pb / 4;
        mc.unc_count = unc_count; mc.unc_q = unc_q; mc.unc_need = unc_need;
    }
    return revo::launch_topk_merge_strided((const float*)((const char*)packed + (size_t)Q * k * 8), pb / 4,
                                           (const long long*)packed, pb / 8, parts, Q, k, has_thr, thr, out_scores,
                                           (long long*)out_indices, out_counts, (hipStream_t)stream, unc_count ? &mc : nullptr);
    API_END
}

#ifdef REVO_EXPERIMENTS
// copy bytes [offset, offset + bytes) of the handle's search workspace to the host (debugging the scan's buffers)
extern "C" int64_t revo_debug_read_workspace(revo_gallery* g, int64_t offset, int64_t bytes, void* host_dst) {
    if (!g || !g->part.p) return -1;
    if (!host_dst) return (int64_t)g->part.bytes;
    if (offset < 0 || bytes < 0 || (size_t)(offset + bytes) > g->part.bytes) return -2;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(host_dst, g->part.p + offset, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return bytes;
}
extern "C" int32_t revo_debug_seed_bounds(revo_gallery* g, const uint32_t* bounds) {
    if (!g) return -1;
    g->seed_bounds = bounds;
    return 0;
}
extern "C" int32_t revo_debug_scan_stats(int64_t* out4) {
    REVO_HIP_CHECK(hipDeviceSynchronize());
    REVO_HIP_CHECK(hipMemcpy(out4, revo::topk_scan256_stats(), 64, hipMemcpyDeviceToHost));
    REVO_HIP_CHECK(hipMemset(revo::topk_scan256_stats(), 0, 64));
    return 0;
}
#endif
