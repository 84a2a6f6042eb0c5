// C ABI of the searches on the candidate pipeline (include/revo.h): pairs, clusters, kNN, k-means, range,
// recommend, discover, boosted, MaxSim, MMR and the hybrid queries (fusion), with their _read entry points.  The handle: gallery_internal.h; the certified top-k: search.hip.
#include <algorithm>
#include <vector>

#include "gallery_internal.h"

namespace {
// The host side of the candidate pipeline (pairs, range and recommend searches): its workspace in one
// buffer of the handle and the steps between its kernels (synchronous: the host reads the candidate and the kept count).
struct CandidateWs {
    DeviceBuffer<>& buf;
    long& cap;                           // candidate keys the workspace holds (a handle remembers it: once grown, it stays grown)
    unsigned long long* cnt = nullptr;   // [4] device counters: [0] candidates (counts past cap), [1] kept, [2], [3] the search's own
    uint64_t *cand = nullptr, *kept_k = nullptr;   // [cap] candidate keys (then the sort's second key buffer), kept sort keys
    float *kept_v = nullptr, *alt_v = nullptr;     // [cap] kept scores, the sort's second score buffer
    uint32_t* hist = nullptr;            // the sort's digit counts
    unsigned long long h[4] = {0, 0, 0, 0}, n_cand = 0, n_kept = 0;   // cnt as read behind the join; candidates, kept entries
    int passes = 0;                      // joins run: 1, or 2 after a regrow
    uint64_t* sk = nullptr; float* sv = nullptr;   // the sorted kept entries
    // the layout for n candidate keys; extra(Layout&) takes the arrays a search adds behind it
    template <class Extra> int carve(long n, hipStream_t st, Extra&& extra) {
        CHECK_RC(carve_buffer(buf, st, [&](Layout& l) {
            cnt = l.take<unsigned long long>(4);
            cand = l.take<uint64_t>(n); kept_k = l.take<uint64_t>(n);
            kept_v = l.take<float>(n); alt_v = l.take<float>(n);
            hist = l.take<uint32_t>(256l * revo::SORT_MAX_BLOCKS);
            extra(l);
        }));
        cap = n;
        return 0;
    }
    int carve(long n, hipStream_t st) { return carve(n, st, [](Layout&) {}); }
    // Clears the counters, runs join() and reads them; limit(candidates) is the caller's check.  A count past the workspace's
    // end: carved again for the counted size, joined once more (`changed`: the error text if that does not fit either).
    template <class Join, class Limit> int join_until_it_fits(hipStream_t st, Join&& join, Limit&& limit, const char* changed) {
        for (passes = 0;;) {
            REVO_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(h), st));
            CHECK_RC(join());
            ++passes;
            REVO_HIP_CHECK(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
            REVO_HIP_CHECK(hipStreamSynchronize(st));
            n_cand = h[0];
            CHECK_RC(limit(n_cand));
            if (n_cand <= (unsigned long long)cap) return 0;
            REVO_REQUIRE(passes == 1, changed);
            CHECK_RC(carve((long)n_cand, st));
        }
    }
    // behind the re-score (it counted into cnt[1]): the kept count, the kept entries sorted over key_bits bits -> n_kept, sk, sv
    int sort_kept(const char* prof, int key_bits, hipStream_t st) {
        n_kept = 0;
        if (n_cand > 0) {
            REVO_HIP_CHECK(hipMemcpyAsync(&n_kept, cnt + 1, sizeof(n_kept), hipMemcpyDeviceToHost, st));
            REVO_HIP_CHECK(hipStreamSynchronize(st));
        }
        ProfScope ps(prof, st);
        return revo::launch_sort_keys_u64(kept_k, kept_v, cand, alt_v, (long)n_kept, key_bits, hist, &sk, &sv, st);
    }
};
// revo_search_stats slot 3 = candidates re-scored, slot 7 = candidate passes; the call ends synchronised
int publish_candidate_stats(int* ctr, unsigned long long candidates, int passes, hipStream_t st) {
    const int stats[2] = {(int)candidates, passes};
    REVO_HIP_CHECK(hipMemcpyAsync(ctr + revo::CTR_COLLECTED, &stats[0], sizeof(int), hipMemcpyHostToDevice, st));
    REVO_HIP_CHECK(hipMemcpyAsync(ctr + revo::CTR_PAIR_PASSES, &stats[1], sizeof(int), hipMemcpyHostToDevice, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
// the bits of the largest row index of N rows (at least 1): the row field of a sort key
int row_index_bits(long N) {
    int b = 1;
    while (N > 1 && (1l << b) < N) ++b;
    return b;
}

// The start of a candidate search: the handle's per-query arrays hold `rows` rows, and its counters (revo_search_stats) are
// this call's alone
int begin_counted(revo_gallery* g, int rows, const char* who, hipStream_t st) {
    CHECK_RC(search_grow_queries(g, rows, st));
    REVO_REQUIRE(g->xw.ctr, std::string(who) + ": no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, revo::CTR_SLOTS * sizeof(int), st));
    return 0;
}

// ---- the two joins of the gallery with itself (pairs, clusters) behind their null checks: the remaining argument checks ...
int self_join_checks(const revo_gallery* g, float threshold, const char* who, const uint32_t** allow) {
    CHECK_RC(require_threshold(1, threshold, who));
    CHECK_RC(require_f32_rows(g, who));
    REVO_REQUIRE(g->size < (1ll << 31), std::string(who) + ": row indices must fit in 31 bits");
    return search_filter(g, allow);
}
// ... and, on the handle's device, the counters (the two-phase state stays: these calls do not write the handle's query rows),
// prepare() (what has to be on the stream before the join and survive the workspace's regrow), the candidate workspace and the
// join: launch(PairsJoinArgs) under the profile class <cls>_join; `what` and `advice` are the limit message's two halves
template <class Prepare, class Launch>
int self_join(revo_gallery* g, CandidateWs& ws, float threshold, const uint32_t* allow, const char* who, const char* cls,
              const char* what, const char* advice, hipStream_t st, Prepare&& prepare, Launch&& launch) {
    using namespace revo;
    CHECK_RC(begin_counted(g, 1, who, st));
    CHECK_RC(prepare());
    CHECK_RC(ws.carve(ws.cap > PAIRS_WS_KEYS ? ws.cap : PAIRS_WS_KEYS, st));
    PairsJoinArgs ja{};
    ja.Gb = g->gb.p; ja.ldg = g->D; ja.N = g->size; ja.D = g->D; ja.gstat = g->gstat.p; ja.thr = threshold; ja.allow = allow;
    const std::string name = who, prof = std::string(cls) + "_join";
    return ws.join_until_it_fits(st, [&]() -> int {
        ja.cnt = ws.cnt; ja.keys = ws.cand; ja.cap = ws.cap;
        ProfScope ps(prof.c_str(), st);
        return launch(ja);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)PAIRS_MAX_CAND,
                     name + ": " + std::to_string(n_cand) + what + std::to_string(PAIRS_MAX_CAND) + advice);
        return 0;
    }, (name + ": the candidate count changed between two joins").c_str());
}
}  // namespace

// ---- near-duplicate pairs of one gallery (include/revo.h revo_gallery_pairs; pairs.hip)
extern "C" int32_t revo_gallery_pairs(revo_gallery* g, float threshold, int64_t* n_pairs, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_pairs, "gallery_pairs: null argument");
    const uint32_t* allow; CHECK_RC(self_join_checks(g, threshold, "gallery_pairs", &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    g->pairs.valid = false;
    const long N = g->size;
    const int D = g->D;
    CandidateWs ws{g->pbuf, g->pairs.cap};
    CHECK_RC(self_join(g, ws, threshold, allow, "gallery_pairs", "pairs", " candidate pairs exceed the limit of ",
                       " (raise the threshold)", st, [] { return 0; },
                       [&](const PairsJoinArgs& ja) { return launch_pairs_join(ja, st); }));
    // fp32 re-score; the kept entries as (i << b) | j
    const int b = row_index_bits(N);
    { ProfScope ps("pairs_rescore", st);
      CHECK_RC(launch_pairs_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, threshold, b, ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    CHECK_RC(ws.sort_kept("pairs_sort", 2 * b, st));
    const unsigned long long n_kept = ws.n_kept;
    CHECK_RC(g->pairs.idx.grow((size_t)(n_kept > 0 ? n_kept : 1) * 16, st));
    CHECK_RC(g->pairs.score.grow((size_t)(n_kept > 0 ? n_kept : 1) * 4, st));
    CHECK_RC(launch_pairs_emit(ws.sk, ws.sv, (long)n_kept, b, g->pairs.idx.p, g->pairs.score.p, st));
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.passes, st));
    g->pairs.n = (int64_t)n_kept;
    g->pairs.valid = true;
    *n_pairs = (int64_t)n_kept;
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_pairs_read(revo_gallery* g, int64_t start, int64_t n, int64_t* pairs, float* scores,
                                           int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_pairs_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "gallery_pairs_read: negative start or count");
    REVO_REQUIRE((pairs && scores) || n == 0, "gallery_pairs_read: null argument");
    REVO_REQUIRE(g->pairs.valid, "gallery_pairs_read: no result (call revo_gallery_pairs again after the rows change)");
    REVO_REQUIRE(start + n <= g->pairs.n, "gallery_pairs_read: range past the result's " + std::to_string(g->pairs.n) + " pairs");
    if (n == 0) return 0;
    REVO_ON_DEVICE(g->device);
    CHECK_RC(copy_out(pairs, g->pairs.idx.p + start * 2, (size_t)n * 2, dst_on_device));
    return copy_out(scores, g->pairs.score.p + start, (size_t)n, dst_on_device);
    API_END
}

// ---- duplicate clusters of one gallery (include/revo.h revo_gallery_clusters; clusters.hip)
extern "C" int32_t revo_gallery_clusters(revo_gallery* g, float threshold, int64_t* n_clusters, int64_t* n_members, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_clusters && n_members, "gallery_clusters: null argument");
    const uint32_t* allow; CHECK_RC(self_join_checks(g, threshold, "gallery_clusters", &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    ClustersResult& cl = g->clusters;
    cl.valid = false;
    const long N = g->size;
    const int D = g->D;
    const int b = row_index_bits(N);
    const size_t rows = (size_t)(N > 0 ? N : 1);
    uint32_t *parent = nullptr, *sizes = nullptr, *hist = nullptr;
    unsigned long long *ctr4 = nullptr, *rank = nullptr;
    uint64_t *keys = nullptr, *keys_alt = nullptr;
    float *vals = nullptr, *vals_alt = nullptr;
    // the union-find and the finish step's arrays: a buffer of their own, so the candidate workspace's regrow leaves parent[] be
    auto prepare = [&]() -> int {
        CHECK_RC(carve_buffer(cl.ws, st, [&](Layout& l) {
            ctr4 = l.take<unsigned long long>(4);
            parent = l.take<uint32_t>(rows + 1); sizes = l.take<uint32_t>(rows);      // parent[N]: the error word
            keys = l.take<uint64_t>(rows); keys_alt = l.take<uint64_t>(rows);
            vals = l.take<float>(rows); vals_alt = l.take<float>(rows);       // (the sort moves a value with every key: unused here)
            rank = l.take<unsigned long long>(rows);
            hist = l.take<uint32_t>(256l * SORT_MAX_BLOCKS);
        }));
        CHECK_RC(cl.labels.grow(rows * 8, st));
        return launch_clusters_init(parent, sizes, N, ctr4, st);
    };
    // (a second join repeats the first one's merges: parent[] is not reset between the passes)
    auto join = [&](const PairsJoinArgs& j) -> int {
        ClustersJoinArgs ja{}; ja.j = j; ja.parent = parent;
        return launch_clusters_join(ja, st);
    };
    CandidateWs ws{g->pbuf, g->pairs.cap};
    CHECK_RC(self_join(g, ws, threshold, allow, "gallery_clusters", "clusters", " pairs inside the rounding bound of the threshold "
                       "exceed the limit of ", " (move the threshold)", st, prepare, join));
    { ProfScope ps("clusters_rescore", st);
      CHECK_RC(launch_clusters_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, threshold, parent, N, st)); }
    unsigned long long h[4] = {0, 0, 0, 0};
    { ProfScope ps("clusters_finish", st);
      CHECK_RC(launch_clusters_labels(parent, allow, N, b, cl.labels.p, sizes, keys, ctr4, st)); }
    REVO_HIP_CHECK(hipMemcpyAsync(h, ctr4, sizeof(h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    if (h[2] != 0) {
        revo_set_error("clusters: union-find did not converge");
        return -4;
    }
    const long n_mem = (long)h[0], n_cl = (long)h[1];
    REVO_REQUIRE(n_mem <= N && n_cl <= n_mem / 2, "gallery_clusters: internal: inconsistent counts");
    CHECK_RC(cl.off.grow((size_t)(n_cl + 1) * 8, st));
    CHECK_RC(cl.members.grow((size_t)(n_mem > 0 ? n_mem : 1) * 8, st));
    {
        ProfScope ps("clusters_finish", st);
        uint64_t* sk = nullptr; float* sv = nullptr;
        CHECK_RC(launch_sort_keys_u64(keys, vals, keys_alt, vals_alt, n_mem, 2 * b, hist, &sk, &sv, st));
        CHECK_RC(launch_clusters_emit(sk, n_mem, n_cl, b, rank, cl.members.p, cl.off.p, st));
    }
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.passes, st));
    cl.rows = N; cl.n = n_cl; cl.n_members = n_mem;
    cl.valid = true;
    *n_clusters = n_cl;
    *n_members = n_mem;
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_clusters_read(revo_gallery* g, int64_t* labels, int64_t* offsets, int64_t* members,
                                              int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_clusters_read: null handle");
    const ClustersResult& cl = g->clusters;
    REVO_REQUIRE(cl.valid, "gallery_clusters_read: no result (call revo_gallery_clusters again after the rows change)");
    if (!labels && !offsets && !members) return 0;
    REVO_ON_DEVICE(g->device);
    if (labels && cl.rows > 0) CHECK_RC(copy_out(labels, cl.labels.p, (size_t)cl.rows, dst_on_device));
    if (offsets) CHECK_RC(copy_out(offsets, cl.off.p, (size_t)(cl.n + 1), dst_on_device));
    if (members && cl.n_members > 0) CHECK_RC(copy_out(members, cl.members.p, (size_t)cl.n_members, dst_on_device));
    return 0;
    API_END
}

// ---- deduplicating append (include/revo.h revo_gallery_append_unique; dedup.hip)
extern "C" int32_t revo_gallery_append_unique(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize, int32_t src_on_device,
                                              float threshold, int64_t* rows, float* scores, int32_t dst_on_device,
                                              int64_t* n_kept, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && rows && scores && n_kept && (vecs || n == 0), "gallery_append_unique: null argument");
    REVO_REQUIRE(n >= 0, "gallery_append_unique: negative row count");
    REVO_REQUIRE(n <= revo::DEDUP_MAX_BATCH, "gallery_append_unique: at most " + std::to_string(revo::DEDUP_MAX_BATCH) +
                                                 " rows per call (split the batch: consecutive calls give the same result)");
    CHECK_RC(require_threshold(1, threshold, "gallery_append_unique"));
    REVO_REQUIRE(g->size + n <= g->capacity, "gallery_append_unique: exceeds the capacity given at create (room for every row "
                                             "of the batch is needed, however few are kept)");
    CHECK_RC(require_f32_rows(g, "gallery_append_unique"));
    REVO_REQUIRE(g->size + n < (1ll << 31), "gallery_append_unique: row indices must fit in 31 bits");
    if (n == 0) { *n_kept = 0; return 0; }
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    // what an append invalidates; the gallery's size stays N0 until the last step has been enqueued and waited for: a failure
    // on the way leaves the gallery as it was (the provisional rows lie behind its end)
    g->rows_changed(); g->maxsim.rows = -1;
    const long N0 = g->size, nb = (long)n, R0 = N0 & ~31l, nwords = (N0 - R0 + nb + 63) / 64 * 2;
    const int D = g->D;
    CHECK_RC(begin_counted(g, 1, "gallery_append_unique", st));
    uint32_t *edges = nullptr, *rep = nullptr, *kept_dev = nullptr, *bits = nullptr, *cnt = nullptr, *first = nullptr;
    long long* rows_dev = nullptr;
    float* scores_dev = nullptr;
    CHECK_RC(carve_buffer(g->dedup, st, [&](Layout& l) {
        edges = l.take<uint32_t>(dedup_edge_words(nb));
        rep = l.take<uint32_t>(nb); rows_dev = l.take<long long>(nb); scores_dev = l.take<float>(nb);
        kept_dev = l.take<uint32_t>(1); bits = l.take<uint32_t>(nwords); cnt = l.take<uint32_t>(1); first = l.take<uint32_t>(1);
    }));
    // provisional append: the fp32 master and the bf16 row of every batch row, with the bits an append writes
    CHECK_RC(gallery_write_rows(g, vecs, n, normalize, src_on_device, N0, nullptr, "dedup_write", st));
    REVO_HIP_CHECK(hipMemsetAsync(edges, 0xff, (size_t)dedup_pad(nb) * 4, st));
    REVO_HIP_CHECK(hipMemsetAsync(edges + dedup_pad(nb), 0, (size_t)nb * dedup_words(nb) * 4, st));
    CandidateWs ws{g->pbuf, g->pairs.cap};
    CHECK_RC(ws.carve(ws.cap > PAIRS_WS_KEYS ? ws.cap : PAIRS_WS_KEYS, st));
    DedupJoinArgs ja{};
    ja.j.Gb = g->gb.p; ja.j.ldg = D; ja.j.N = N0 + nb; ja.j.D = D; ja.j.gstat = g->gstat.p; ja.j.thr = threshold;
    ja.N0 = (uint32_t)N0; ja.edges = edges;
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        ja.j.cnt = ws.cnt; ja.j.keys = ws.cand; ja.j.cap = ws.cap;
        ProfScope ps("dedup_join", st);
        return launch_dedup_join(ja, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)PAIRS_MAX_CAND,
                     "gallery_append_unique: " + std::to_string(n_cand) + " pairs inside the rounding bound of the threshold exceed "
                     "the limit of " + std::to_string(PAIRS_MAX_CAND) + " (move the threshold)");
        return 0;
    }, "gallery_append_unique: the candidate count changed between two joins"));
    { ProfScope ps("dedup_rescore", st);
      CHECK_RC(launch_dedup_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, threshold, edges, N0, nb, st)); }
    {
        ProfScope ps("dedup_select", st);
        DedupSelectArgs sa{};
        sa.edges = edges; sa.n = nb; sa.N0 = N0; sa.rep = rep; sa.rows = rows_dev; sa.n_kept = kept_dev;
        CHECK_RC(launch_dedup_select(sa, st));
        CHECK_RC(launch_dedup_finish(rep, nb, N0, g->gf.p, D, D, scores_dev, bits, nwords, st));
    }
    // the tail compacted through the remove path: one chunk (the batch and the at most 31 gallery rows in front of it that
    // share its first bitmap word); only rows >= N0 move
    long kept_rows = 0;
    const long len = N0 - R0 + nb, chunk = (len + 31) / 32 * 32;
    CHECK_RC(gallery_compact_rows(g, bits, R0, len, chunk, cnt, first, "dedup_compact", st, &kept_rows));
    uint32_t kept_h = 0;
    REVO_HIP_CHECK(hipMemcpyAsync(&kept_h, kept_dev, 4, hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    REVO_REQUIRE((long)kept_h == kept_rows - (N0 - R0) && (long)kept_h <= nb, "gallery_append_unique: internal: inconsistent kept counts");
    CHECK_RC(copy_out(rows, rows_dev, (size_t)nb, dst_on_device));
    CHECK_RC(copy_out(scores, scores_dev, (size_t)nb, dst_on_device));
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.passes, st));
    g->size = N0 + (long)kept_h;
    *n_kept = (int64_t)kept_h;
    return 0;
    API_END
}

// ---- exact kNN graph of one gallery (include/revo.h revo_gallery_knn; knn.hip)
#ifdef REVO_EXPERIMENTS
static long g_knn_cap_keys = 0;
static int g_knn_level_mode = 0;
extern "C" int32_t revo_debug_set_knn(int64_t cap_keys, int32_t level_mode) {
    REVO_REQUIRE(cap_keys >= 0 && cap_keys <= revo::KNN_MAX_KEYS, "debug_set_knn: cap_keys must be in [0, 2^28]");
    REVO_REQUIRE(level_mode >= 0 && level_mode <= 3, "debug_set_knn: level_mode must be in [0, 3]");
    g_knn_cap_keys = (long)cap_keys;
    g_knn_level_mode = level_mode;
    return 0;
}
#endif
extern "C" int32_t revo_gallery_knn(revo_gallery* g, int32_t k, int32_t has_threshold, float threshold, int64_t* n_rows,
                                    void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_rows, "gallery_knn: null argument");
    REVO_REQUIRE(k >= 1 && k <= revo::KNN_K_MAX, "gallery_knn: k must be in [1, 64]");
    CHECK_RC(require_threshold(has_threshold, threshold, "gallery_knn"));
    CHECK_RC(require_f32_rows(g, "gallery_knn"));
    REVO_REQUIRE(g->size < (1ll << 31), "gallery_knn: row indices must fit in 31 bits");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    KnnResult& kr = g->knn;
    kr.valid = false;
    const long N = g->size;
    const int D = g->D;
    CHECK_RC(begin_counted(g, 1, "gallery_knn", st));
    if (N == 0) {
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        kr.n = 0; kr.k = k; kr.valid = true;
        *n_rows = 0;
        return 0;
    }
    long cap_keys = 0;
    int level_mode = 0;
#ifdef REVO_EXPERIMENTS
    cap_keys = g_knn_cap_keys; level_mode = g_knn_level_mode;
#endif
    if (cap_keys <= 0) {
        // about 2 k + 16 entries per row and direction and as many again inside the rounding bound; a gallery no larger than
        // the sample has no levels: all its pairs
        cap_keys = 2l * (2 * k + 16) * N;
        if (N <= KNN_SAMPLE && cap_keys < N * (N - 1) / 2) cap_keys = N * (N - 1) / 2;
        cap_keys = std::min(KNN_MAX_KEYS, std::max(KNN_MIN_KEYS, cap_keys));
    }
    const long T = (N + 255) / 256, rows = T * 256;
    const long stride = (N + KNN_SAMPLE - 1) / KNN_SAMPLE, S = (N + stride - 1) / stride, sample_rows = (S + 255) / 256 * 256;
    const bool have_pass = N > KNN_SAMPLE && level_mode != 1 && level_mode != 2;
    CHECK_RC(kr.score.grow((size_t)N * k * 4, st));
    CHECK_RC(kr.idx.grow((size_t)N * k * 8, st));
    CHECK_RC(kr.counts.grow((size_t)N * 4, st));
    // the workspace: 2 cap_keys entries (a candidate key gives at most two directed entries), the per-row arrays, the sample
    long cap = 0;
    CandidateWs ws{g->pbuf, cap};
    float *level = nullptr, *lb = nullptr, *sum = nullptr, *sq = nullptr;
    uint32_t *lost = nullptr, *sallow = nullptr;
    bf16_t* Sb = nullptr;
    int *fb_q = nullptr, *fb_ctr = nullptr;
    CHECK_RC(ws.carve(2 * cap_keys, st, [&](Layout& l) {
        level = l.take<float>(rows); lb = l.take<float>(rows); lost = l.take<uint32_t>(T * 8);
        fb_q = l.take<int>(N); fb_ctr = l.take<int>(2);    // fb_ctr[0]: sample rows pruned; [1]: fallback rows
        if (have_pass) {
            sum = l.take<float>(4 * rows); sq = l.take<float>(4 * rows);
            Sb = l.take<bf16_t>((size_t)sample_rows * D); sallow = l.take<uint32_t>(sample_rows / 32);
        }
    }));
    REVO_HIP_CHECK(hipMemsetAsync(ws.cnt, 0, sizeof(ws.h), st));
    REVO_HIP_CHECK(hipMemsetAsync(lost, 0, (size_t)T * 8 * 4, st));
    REVO_HIP_CHECK(hipMemsetAsync(fb_ctr, 0, 2 * sizeof(int), st));
    KnnLevelArgs la{};
    la.Gb = g->gb.p; la.ldg = D; la.N = N; la.D = D; la.Sb = Sb; la.S = S; la.stride = stride; la.sallow = sallow;
    la.sum = sum; la.sq = sq; la.rows = rows;
    { ProfScope ps("knn_level", st);
      if (have_pass) {
          CHECK_RC(launch_knn_sample(g->gb.p, D, N, D, S, stride, allow, Sb, sallow, ws.cnt, st));
          CHECK_RC(launch_knn_level_pass(la, st));
      }
      CHECK_RC(launch_knn_levels(la, allow, g->gstat.p, ws.cnt, k, has_threshold, threshold, level_mode, have_pass ? 1 : 0, 0, fb_ctr,
                                 level, lb, st));
      if (have_pass) {
          // rows of dense blocks: out of the join, into the fallback, and out of the sample; the levels once more without them
          la.lb = lb;
          CHECK_RC(launch_knn_level_pass(la, st));
          CHECK_RC(launch_knn_dense_rows(la, ws.cnt, k, sallow, fb_ctr, level, lb, st));
          la.lb = nullptr;
          CHECK_RC(launch_knn_level_pass(la, st));
          CHECK_RC(launch_knn_levels(la, allow, g->gstat.p, ws.cnt, k, has_threshold, threshold, level_mode, 1, 1, fb_ctr, level, lb,
                                     st));
      } }
    KnnJoinArgs ja{};
    ja.j.Gb = g->gb.p; ja.j.ldg = D; ja.j.N = N; ja.j.D = D; ja.j.gstat = g->gstat.p; ja.j.allow = allow;
    ja.j.cnt = ws.cnt; ja.j.keys = ws.cand; ja.j.cap = cap_keys; ja.lb = lb; ja.lost = lost;
    { ProfScope ps("knn_join", st);
      CHECK_RC(launch_knn_join(ja, st)); }
    REVO_HIP_CHECK(hipMemcpyAsync(ws.h, ws.cnt, sizeof(ws.h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    // (a count past the workspace: the keys behind it were dropped and their rows marked lost)
    ws.n_cand = std::min<unsigned long long>(ws.h[0], (unsigned long long)cap_keys);
    { ProfScope ps("knn_rescore", st);
      CHECK_RC(launch_knn_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, level, ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    CHECK_RC(ws.sort_kept("knn_sort", 32 + row_index_bits(N), st));
    REVO_REQUIRE(ws.n_kept <= 2 * ws.n_cand, "gallery_knn: internal: more entries than the workspace holds");
    { ProfScope ps("knn_select", st);
      CHECK_RC(launch_knn_select(ws.sk, ws.sv, (long)ws.n_kept, N, k, has_threshold ? threshold : -INFINITY, level, lost, allow, fb_q,
                                 fb_ctr, kr.score.p, kr.idx.p, kr.counts.p, st)); }
    int fb[2] = {0, 0};
    REVO_HIP_CHECK(hipMemcpyAsync(fb, fb_ctr, sizeof(fb), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    const int n_fb = fb[1];
    REVO_REQUIRE(n_fb >= 0 && n_fb <= N, "gallery_knn: internal: more fallback rows than rows");
    if (n_fb > 0) {
        // rows without a certificate: the large-k search's exhaustive fallback, the master row as the query, in rounds
        long F = (long)(KNN_FB_BYTES / ((size_t)N * 4));
        F = std::max(1l, std::min({F, 1024l, (long)n_fb}));
        CHECK_RC(kr.fb.grow((size_t)F * N * 4, st));
        LargeWs lw{};
        lw.ctr = fb_ctr; lw.fb_q = fb_q; lw.fb_scores = kr.fb.p; lw.F = (int)F;
        ProfScope ps("knn_fallback", st);
        CHECK_RC(launch_topk_large_fallback(lw, n_fb, g->gf.p, D, g->gf.p, D, N, D, k, has_threshold, threshold, 0, kr.score.p,
                                            kr.idx.p, kr.counts.p, allow, st, 1));
    }
    REVO_HIP_CHECK(hipMemcpyAsync(g->xw.ctr + CTR_LARGE_FALLBACK, &n_fb, sizeof(int), hipMemcpyHostToDevice, st));
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, 1, st));
    kr.n = N; kr.k = k;
    kr.valid = true;
    *n_rows = N;
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_knn_read(revo_gallery* g, int64_t start, int64_t n, int64_t* indices, float* scores, int32_t* counts,
                                         int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_knn_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "gallery_knn_read: negative start or count");
    const KnnResult& kr = g->knn;
    REVO_REQUIRE(kr.valid, "gallery_knn_read: no result (call revo_gallery_knn again after the rows change)");
    REVO_REQUIRE(start + n <= kr.n, "gallery_knn_read: range past the result's " + std::to_string(kr.n) + " rows");
    if (n == 0 || (!indices && !scores && !counts)) return 0;
    REVO_ON_DEVICE(g->device);
    if (indices) CHECK_RC(copy_out(indices, kr.idx.p + start * kr.k, (size_t)n * kr.k, dst_on_device));
    if (scores) CHECK_RC(copy_out(scores, kr.score.p + start * kr.k, (size_t)n * kr.k, dst_on_device));
    if (counts) CHECK_RC(copy_out(counts, kr.counts.p + start, (size_t)n, dst_on_device));
    return 0;
    API_END
}

// ---- exact spherical k-means over one gallery (include/revo.h revo_gallery_kmeans; kmeans.hip)
#ifdef REVO_EXPERIMENTS
static long g_kmeans_cap_keys = 0;
extern "C" int32_t revo_debug_set_kmeans(int64_t cap_keys) {
    REVO_REQUIRE(cap_keys >= 0 && cap_keys <= revo::KMEANS_MAX_CAND, "debug_set_kmeans: cap_keys must be in [0, 2^28]");
    g_kmeans_cap_keys = (long)cap_keys;
    return 0;
}
#endif
extern "C" int32_t revo_gallery_kmeans(revo_gallery* g, const float* centroids, int32_t n_centroids, int32_t normalize,
                                       int32_t src_on_device, int32_t max_iter, int32_t* n_iter, int32_t* converged,
                                       int64_t* n_rows, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && centroids && n_iter && converged && n_rows, "gallery_kmeans: null argument");
    REVO_REQUIRE(n_centroids >= 1 && n_centroids <= revo::KMEANS_MAX_CENTROIDS, "gallery_kmeans: n_centroids must be in [1, 65536]");
    REVO_REQUIRE(max_iter >= 0 && max_iter <= revo::KMEANS_MAX_ITER, "gallery_kmeans: max_iter must be in [0, 1000]");
    CHECK_RC(require_f32_rows(g, "gallery_kmeans"));
    REVO_REQUIRE(g->size < (1ll << 31), "gallery_kmeans: row indices must fit in 31 bits");
    CHECK_RC(revo::g256_check_operands("gallery_kmeans", g->D, g->D, g->D));
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    KmeansResult& kr = g->kmeans;
    kr.valid = false;
    const long N = g->size, C = n_centroids, Cpad = (C + 255) / 256 * 256;
    const int D = g->D;
    const long T = (N + 255) / 256, rows = T * 256, part_chunks = N / 256 + C;
    const int b = row_index_bits(N);
    CHECK_RC(begin_counted(g, 1, "gallery_kmeans", st));
    const size_t n1 = (size_t)(N > 0 ? N : 1);
    CHECK_RC(kr.labels.grow(n1 * 4, st));
    CHECK_RC(kr.score.grow(n1 * 4, st));
    CHECK_RC(kr.sizes.grow((size_t)C * 8, st));
    for (int i = 0; i < 2; ++i) {
        CHECK_RC(kr.cf[i].grow((size_t)Cpad * D * 4, st));
        CHECK_RC(kr.cb[i].grow((size_t)Cpad * D * 2, st));
        // (the rows past C of the bf16 copies are operand rows of the last centroid tile: zeros)
        if (Cpad > C) REVO_HIP_CHECK(hipMemsetAsync(kr.cb[i].p + (size_t)C * D, 0, (size_t)(Cpad - C) * D * 2, st));
    }
    // the call's own arrays, in a buffer of their own: a regrow of the candidate workspace leaves them be
    unsigned long long *ctr = nullptr, *rowkey = nullptr, *moff = nullptr, *coff = nullptr;
    uint32_t *cstat = nullptr, *ncand = nullptr, *hist = nullptr;
    float *cst = nullptr, *inv = nullptr, *rstat = nullptr, *best = nullptr, *thr = nullptr, *vals = nullptr, *vals_alt = nullptr,
          *part = nullptr, *sums = nullptr;
    uint64_t *keys = nullptr, *keys_alt = nullptr;
    CHECK_RC(carve_buffer(kr.ws, st, [&](Layout& l) {
        ctr = l.take<unsigned long long>(4); cstat = l.take<uint32_t>(2); cst = l.take<float>(2 * C);
        inv = l.take<float>(n1); rstat = l.take<float>(2 * n1);
        best = l.take<float>(4 * (rows > 0 ? rows : 256)); thr = l.take<float>(rows > 0 ? rows : 256);
        rowkey = l.take<unsigned long long>(n1); ncand = l.take<uint32_t>(n1);
        keys = l.take<uint64_t>(n1); keys_alt = l.take<uint64_t>(n1); vals = l.take<float>(n1); vals_alt = l.take<float>(n1);
        hist = l.take<uint32_t>(256l * SORT_MAX_BLOCKS);
        moff = l.take<unsigned long long>(C); coff = l.take<unsigned long long>(C);
        part = l.take<float>((size_t)part_chunks * D); sums = l.take<float>((size_t)C * D);
    }));
    // the initial centroids through the append's kernel: fp32 rows, bf16 copies, the rows' statistics and their maxima
    kr.cur = 0;
    {
        const float* src = centroids;
        if (!src_on_device) {
            CHECK_RC(g->stage.grow((size_t)C * D * 4, st));
            REVO_HIP_CHECK(hipMemcpyAsync(g->stage.p, centroids, (size_t)C * D * 4, hipMemcpyHostToDevice, st));
            src = g->stage.p;
        }
        REVO_HIP_CHECK(hipMemsetAsync(cstat, 0, 8, st));
        ProfScope ps("kmeans_init", st);
        CHECK_RC(launch_l2norm_rows(src, D, kr.cf[0].p, D, kr.cb[0].p, D, C, D, st, normalize ? 1 : 0, cst, cstat));
        if (N > 0) CHECK_RC(launch_kmeans_rows(g->gf.p, g->gb.p, D, N, D, inv, rstat, st));
    }
    {
        std::vector<float> h((size_t)2 * C);
        REVO_HIP_CHECK(hipMemcpyAsync(h.data(), cst, h.size() * 4, hipMemcpyDeviceToHost, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        for (long c = 0; c < C; ++c) {
            REVO_REQUIRE(std::isfinite(h[2 * c]) && std::isfinite(h[2 * c + 1]),
                         "gallery_kmeans: centroid " + std::to_string(c) + " is not finite");
            REVO_REQUIRE(!normalize || h[2 * c + 1] > 0.f, "gallery_kmeans: centroid " + std::to_string(c) + " has zero norm");
        }
    }
    REVO_HIP_CHECK(hipMemsetAsync(kr.labels.p, 0xfe, n1 * 4, st));          // (no label: every row of step 0 counts as changed)
    long cap_keys = 0;
#ifdef REVO_EXPERIMENTS
    cap_keys = g_kmeans_cap_keys;
#endif
    if (cap_keys <= 0) cap_keys = std::max({KMEANS_MIN_KEYS, 2 * N, kr.cap});   // a candidate per row and as many again in the band
    CandidateWs ws{g->pbuf, kr.cap};
    CHECK_RC(ws.carve(cap_keys, st));
    KmeansAssignArgs aa{};
    aa.Gb = g->gb.p; aa.ldg = D; aa.N = N; aa.D = D; aa.C = C; aa.rows = rows; aa.best = best; aa.thr = thr; aa.allow = allow;
    unsigned long long extra = 0, decided = 0;
    int passes = 0, t = 0, conv = 0;
    for (;;) {
        // the assignment against the centroids of step t
        unsigned long long h[4] = {0, 0, 0, 0};
        aa.Cb = kr.cb[kr.cur].p;
        if (N > 0) {
            { ProfScope ps("kmeans_best", st);
              CHECK_RC(launch_kmeans_best(aa, st));
              CHECK_RC(launch_kmeans_bound(aa, inv, rstat, cstat, st)); }
            CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
                aa.cnt = ws.cnt; aa.keys = ws.cand; aa.cap = ws.cap;
                ProfScope ps("kmeans_decide", st);
                return launch_kmeans_decide(aa, st);
            }, [&](unsigned long long n_cand) -> int {
                REVO_REQUIRE(n_cand <= (unsigned long long)KMEANS_MAX_CAND,
                             "gallery_kmeans: " + std::to_string(n_cand) + " (row, centroid) pairs inside the rounding bound of a "
                             "row's best score exceed the limit of " + std::to_string(KMEANS_MAX_CAND));
                return 0;
            }, "gallery_kmeans: the candidate count changed between two passes"));
            passes += ws.passes;
            REVO_HIP_CHECK(hipMemsetAsync(rowkey, 0, (size_t)N * 8, st));
            REVO_HIP_CHECK(hipMemsetAsync(ncand, 0, (size_t)N * 4, st));
            ProfScope ps("kmeans_rescore", st);
            CHECK_RC(launch_kmeans_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, inv, kr.cf[kr.cur].p, D, rowkey, ncand, st));
        }
        REVO_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof(h), st));
        { ProfScope ps("kmeans_finish", st);
          CHECK_RC(launch_kmeans_finish(rowkey, ncand, N, C, kr.labels.p, kr.score.p, kr.sizes.p, ctr, st)); }
        REVO_HIP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        if (N > 0) {
            REVO_REQUIRE(h[2] <= ws.n_cand && h[2] <= (unsigned long long)N, "gallery_kmeans: internal: inconsistent counts");
            extra += ws.n_cand - h[2];
            decided += h[1];
        }
        if (t >= 1 && h[0] == 0) { conv = 1; break; }
        if (t == max_iter) break;
        // the centroids of step t + 1 from the labels of step t
        KmeansUpdateArgs ua{};
        ua.labels = kr.labels.p; ua.N = N; ua.C = C; ua.D = D; ua.b = b; ua.Gf = g->gf.p; ua.ldg = D; ua.sizes = kr.sizes.p;
        ua.keys = keys; ua.keys_alt = keys_alt; ua.vals = vals; ua.vals_alt = vals_alt; ua.hist = hist; ua.moff = moff; ua.coff = coff;
        ua.part = part; ua.part_chunks = part_chunks; ua.sums = sums;
        ua.Cf_old = kr.cf[kr.cur].p; ua.Cb_old = kr.cb[kr.cur].p; ua.Cf_new = kr.cf[1 - kr.cur].p; ua.Cb_new = kr.cb[1 - kr.cur].p;
        ua.cstat = cstat;
        { ProfScope ps("kmeans_update", st);
          CHECK_RC(launch_kmeans_update(ua, st)); }
        kr.cur = 1 - kr.cur;
        ++t;
    }
    const int stats[2] = {(int)std::min<unsigned long long>(decided, 0x7fffffffull), 0};
    REVO_HIP_CHECK(hipMemcpyAsync(g->xw.ctr + CTR_LARGE_FALLBACK, &stats[0], sizeof(int), hipMemcpyHostToDevice, st));
    CHECK_RC(publish_candidate_stats(g->xw.ctr, std::min<unsigned long long>(extra, 0x7fffffffull), passes, st));
    kr.n = N; kr.C = C;
    kr.valid = true;
    *n_iter = t;
    *converged = conv;
    *n_rows = N;
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_kmeans_read(revo_gallery* g, int64_t start, int64_t n, int32_t* labels, float* scores,
                                            int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_kmeans_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "gallery_kmeans_read: negative start or count");
    const KmeansResult& kr = g->kmeans;
    REVO_REQUIRE(kr.valid, "gallery_kmeans_read: no result (call revo_gallery_kmeans again after the rows change)");
    REVO_REQUIRE(start + n <= kr.n, "gallery_kmeans_read: range past the result's " + std::to_string(kr.n) + " rows");
    if (n == 0 || (!labels && !scores)) return 0;
    REVO_ON_DEVICE(g->device);
    if (labels) CHECK_RC(copy_out(labels, kr.labels.p + start, (size_t)n, dst_on_device));
    if (scores) CHECK_RC(copy_out(scores, kr.score.p + start, (size_t)n, dst_on_device));
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_kmeans_centroids(revo_gallery* g, float* centroids, int64_t* sizes, int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_kmeans_centroids: null handle");
    const KmeansResult& kr = g->kmeans;
    REVO_REQUIRE(kr.valid, "gallery_kmeans_centroids: no result (call revo_gallery_kmeans again after the rows change)");
    if (!centroids && !sizes) return 0;
    REVO_ON_DEVICE(g->device);
    if (centroids) CHECK_RC(copy_out(centroids, kr.cf[kr.cur].p, (size_t)kr.C * g->D, dst_on_device));
    if (sizes) CHECK_RC(copy_out(sizes, (const long long*)kr.sizes.p, (size_t)kr.C, dst_on_device));
    return 0;
    API_END
}

// ---- range search (include/revo.h revo_search_range; range.hip)
extern "C" int32_t revo_search_range(revo_gallery* g, const float* queries, int32_t Q, float thr, int64_t index_offset,
                                     int64_t* n_results, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_results && (queries || Q == 0), "search_range: null argument");
    REVO_REQUIRE(Q >= 0, "search_range: negative query count");
    CHECK_RC(require_threshold(1, thr, "search_range"));
    CHECK_RC(require_f32_rows(g, "search_range"));
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    g->range.valid = false;
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    // sort keys (query << (32 + b)) | (score << b) | row in 64 bits: at most 2^(32 - b) queries per chunk
    const int b = row_index_bits(N);
    int QC = Q < RANGE_CHUNK ? Q : RANGE_CHUNK;
    if ((long)QC > (1l << (32 - b))) QC = (int)(1l << (32 - b));
    int qbits = 0;
    while ((1l << qbits) < QC) ++qbits;
    g->drop_two_phase();
    CHECK_RC(begin_counted(g, QC > 0 ? QC : 1, "search_range", st));
    // offsets: off[1 + q] collects query q's count, then the prefix sums make them the CSR offsets (off[0] = 0)
    CHECK_RC(g->range.off.grow((size_t)(Q + 1) * 8, st));
    REVO_HIP_CHECK(hipMemsetAsync(g->range.off.p, 0, (size_t)(Q + 1) * 8, st));
    unsigned long long* off = g->range.off.p;
    CandidateWs ws{g->pbuf, g->range.cap};
    long total = 0;
    unsigned long long cand_total = 0;
    int max_passes = 0;
    if (N > 0 && Q > 0) {
        const long cap0 = (long)QC * RANGE_WS_PER_QUERY;
        CHECK_RC(ws.carve(g->range.cap > cap0 ? g->range.cap : cap0, st));
        for (int c0 = 0; c0 < Q; c0 += QC) {
            const int Qc = Q - c0 < QC ? Q - c0 : QC;
            { ProfScope ps("search_prep", st);
              CHECK_RC(launch_l2norm_rows(queries + (size_t)c0 * D, D, g->qf.p, D, g->qb.p, D, Qc, D, st, 1, g->qstat.p)); }
            RangeJoinArgs ja{};
            ja.Qb = g->qb.p; ja.ldq = D; ja.Gb = g->gb.p; ja.ldg = D; ja.Q = Qc; ja.N = N; ja.D = D;
            ja.qstat = g->qstat.p; ja.gstat = g->gstat.p; ja.thr = thr; ja.allow = allow;
            CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
                ja.cnt = ws.cnt; ja.keys = ws.cand; ja.cap = ws.cap;
                ProfScope ps("range_join", st);
                return launch_range_join(ja, st);
            }, [&](unsigned long long n_cand) -> int {
                REVO_REQUIRE(cand_total + n_cand <= (unsigned long long)RANGE_MAX_CAND,
                             "search_range: " + std::to_string(cand_total + n_cand) + " candidates exceed the limit of " +
                                 std::to_string(RANGE_MAX_CAND) + " (raise the threshold or search fewer queries per call)");
                return 0;
            }, "search_range: the candidate count changed between two passes"));
            cand_total += ws.n_cand;
            max_passes = ws.passes > max_passes ? ws.passes : max_passes;
            { ProfScope ps("range_rescore", st);
              CHECK_RC(launch_range_rescore(ws.cand, (long)ws.n_cand, g->qf.p, D, g->gf.p, D, D, thr, b, ws.cnt + 1, off + 1 + c0,
                                            ws.kept_k, ws.kept_v, st)); }
            CHECK_RC(ws.sort_kept("range_sort", qbits + 32 + b, st));
            const long n_kept = (long)ws.n_kept;
            const size_t need = (size_t)(total + n_kept > 0 ? total + n_kept : 1);
            CHECK_RC(g->range.idx.grow_keep(need * 8, (size_t)total * 8, st));
            CHECK_RC(g->range.score.grow_keep(need * 4, (size_t)total * 4, st));
            CHECK_RC(launch_range_emit(ws.sk, ws.sv, n_kept, b, index_offset, g->range.idx.p + total, g->range.score.p + total, st));
            total += n_kept;
        }
        CHECK_RC(launch_inclusive_sums_u64(off + 1, Q, st));
    }
    CHECK_RC(publish_candidate_stats(g->xw.ctr, cand_total, max_passes, st));
    g->range.n = total;
    g->range.q = Q;
    g->range.valid = true;
    *n_results = total;
    return 0;
    API_END
}
extern "C" int32_t revo_search_range_read(revo_gallery* g, int64_t* offsets, int64_t start, int64_t n, int64_t* indices,
                                          float* scores, int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "search_range_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "search_range_read: negative start or count");
    REVO_REQUIRE((indices && scores) || n == 0, "search_range_read: null argument");
    REVO_REQUIRE(g->range.valid, "search_range_read: no result (call revo_search_range again after the rows change)");
    REVO_REQUIRE(start + n <= g->range.n,
                 "search_range_read: range past the result's " + std::to_string(g->range.n) + " entries");
    REVO_ON_DEVICE(g->device);
    if (offsets) CHECK_RC(copy_out(offsets, g->range.off.p, (size_t)(g->range.q + 1), dst_on_device));
    if (n == 0) return 0;
    CHECK_RC(copy_out(indices, g->range.idx.p + start, (size_t)n, dst_on_device));
    return copy_out(scores, g->range.score.p + start, (size_t)n, dst_on_device);
    API_END
}

// ---- search by examples: one host skeleton under revo_search_recommend (recommend.hip),
// revo_search_discover (discover.hip, section 4m) and revo_search_boosted (boost.hip, section 4z).  name: "recommend" / "discover" /
// "boosted" (messages search_<name>, profile classes <name>_sample, _pass, _rescore, _sort); tile_rows: the rows the example tile
// takes in the handle; n_examples: the example rows
// that size the sample; pa: the pass's arguments (RecommendPassArgs / DiscoverPassArgs / BoostPassArgs) with the search's own
// fields set -- the skeleton sets those they share.  normalise() fills the example tile, pass(pa, sample, st) launches the sample
// or the candidate pass, rescore(cand, n, b, kept, out_keys, out_scores) the fp32 re-score.  ext: what a search adds to these
// steps -- ExamplesPlain, as it is, for recommend and discover.
struct ExamplesPlain {
    void carve(Layout&, long) {}                                            // arrays behind the workspace's own, for N rows
    template <class PassArgs> void sample(PassArgs& pa, long n_s, long) const { pa.N = n_s; }   // the sample: the first n_s rows
    int after_pass(const unsigned long long (&)[4]) const { return 0; }     // the candidate pass's counters, read and synchronised
    int emit(const uint64_t* sk, const float* sv, long n, int k, int b, long index_offset, float* scores, long long* indices,
             int* counts, hipStream_t st) const {
        return revo::launch_recommend_emit(sk, sv, n, k, b, index_offset, scores, indices, counts, st);
    }
};
template <class PassArgs, class Normalise, class Rescore, class Ext>
static int search_by_examples(revo_gallery* g, const char* name, int tile_rows, int n_examples, PassArgs pa, int k, int has_thr,
                              float thr, long index_offset, float* scores, long long* indices, int* counts, const uint32_t* allow,
                              hipStream_t st, Normalise&& normalise, int (*pass)(const PassArgs&, int, hipStream_t), Rescore&& rescore,
                              Ext&& ext) {
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    const std::string cls = name, who = "search_" + cls;
    g->drop_two_phase();
    CHECK_RC(begin_counted(g, tile_rows, who.c_str(), st));
    if (N == 0) {
        CHECK_RC(launch_topk_fill_empty(scores, indices, counts, 1, k, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    // the sample: as many rows as revo_search_topk_large's sample pass covers (none in a small gallery: tau = -inf or the threshold)
    const long n_s = large_sample_rows(n_examples, N, k);
    // candidates are rows (32-bit indices in the key array), at most N: sized once; counter [2] = allowed rows the pass met
    long cap = 0;
    CandidateWs ws{g->pbuf, cap};
    float *tau = nullptr, *lb = nullptr;
    CHECK_RC(ws.carve(N, st, [&](Layout& l) { tau = l.take<float>(1); lb = l.take<float>(n_s > 0 ? n_s : 1); ext.carve(l, N); }));
    uint32_t* cand = (uint32_t*)ws.cand;
    { ProfScope ps("search_prep", st);
      CHECK_RC(normalise()); }
    pa.Qb = g->qb.p; pa.ldq = D; pa.Gb = g->gb.p; pa.ldg = D; pa.D = D;
    pa.qstat = g->qstat.p; pa.gstat = g->gstat.p; pa.allow = allow;
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        { ProfScope ps((cls + "_sample").c_str(), st);
          if (n_s > 0) { pa.N = N; ext.sample(pa, n_s, N); pa.lb_out = lb; CHECK_RC(pass(pa, 1, st)); }
          CHECK_RC(launch_recommend_level(lb, (int)n_s, k, has_thr, thr, tau, st)); }
        ProfScope ps((cls + "_pass").c_str(), st);
        pa.N = N; pa.lb_out = nullptr; pa.tau = tau; pa.cnt = ws.cnt; pa.rows = cand; pa.cap = N;
        return pass(pa, 0, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)N, who + ": more candidates than rows");
        return 0;
    }, (who + ": the candidate count changed between two passes").c_str()));
    CHECK_RC(ext.after_pass(ws.h));
    const int b = row_index_bits(N);
    { ProfScope ps((cls + "_rescore").c_str(), st);
      CHECK_RC(rescore(cand, (long)ws.n_cand, b, ws.cnt + 1, ws.kept_k, ws.kept_v)); }
    CHECK_RC(ws.sort_kept((cls + "_sort").c_str(), 32 + b, st));
    CHECK_RC(ext.emit(ws.sk, ws.sv, (long)ws.n_kept, k, b, index_offset, scores, indices, counts, st));
    return publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.h[2] > 0 ? 1 : 0, st);   // (no allowed row: no candidate pass counted)
}
extern "C" int32_t revo_search_recommend(revo_gallery* g, const float* examples, int32_t P, int32_t Nn, int32_t k, int32_t has_thr,
                                         float thr, int64_t index_offset, float* scores, int64_t* indices, int32_t* counts,
                                         void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && examples && scores && indices && counts, "search_recommend: null argument");
    REVO_REQUIRE(P >= 1, "search_recommend: needs at least one positive example");
    REVO_REQUIRE(Nn >= 0, "search_recommend: negative count of negative examples");
    REVO_REQUIRE((int64_t)P + Nn <= revo::RECOMMEND_MAX_EXAMPLES, "search_recommend: at most 128 examples (n_positive + n_negative)");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_recommend: k must be in [1, 1024]");
    CHECK_RC(require_threshold(has_thr, thr, "search_recommend"));
    CHECK_RC(require_f32_rows(g, "search_recommend"));
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const int D = g->D, E = P + Nn;
    RecommendPassArgs pa{};
    pa.P = P; pa.Nn = Nn;
    auto normalise = [&]() -> int { return launch_l2norm_rows(examples, D, g->qf.p, D, g->qb.p, D, E, D, st, 1, g->qstat.p); };
    auto rescore = [&](const uint32_t* cand, long n, int b, unsigned long long* kept, uint64_t* out_keys, float* out_scores) -> int {
        return launch_recommend_rescore(cand, n, g->qf.p, D, P, Nn, g->gf.p, D, D, has_thr, thr, b, kept, out_keys, out_scores, st);
    };
    return search_by_examples(g, "recommend", E, E, pa, k, has_thr, thr, index_offset, scores, (long long*)indices, counts, allow, st,
                              normalise, launch_recommend_pass, rescore, ExamplesPlain{});
    API_END
}
extern "C" int32_t revo_search_discover(revo_gallery* g, const float* target, const float* positives, const float* negatives,
                                        int32_t n_pairs, int32_t k, int32_t has_thr, float thr, int64_t index_offset, float* scores,
                                        int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts, "search_discover: null argument");
    if (target) REVO_REQUIRE(n_pairs >= 0 && n_pairs <= revo::DISCOVER_MAX_PAIRS - 1,
                             "search_discover: n_pairs must be in [0, 63] with a target");
    else REVO_REQUIRE(n_pairs >= 1 && n_pairs <= revo::DISCOVER_MAX_PAIRS,
                      "search_discover: n_pairs must be in [1, 64] without a target (context search)");
    REVO_REQUIRE(n_pairs == 0 || (positives && negatives), "search_discover: null positives or negatives");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_discover: k must be in [1, 1024]");
    CHECK_RC(require_threshold(has_thr, thr, "search_discover"));
    CHECK_RC(require_f32_rows(g, "search_discover"));
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const int D = g->D;
    const int has_target = target ? 1 : 0;
    const int rows = discover_tile_rows(n_pairs, has_target), half = rows / 2;
    DiscoverPassArgs pa{};
    pa.n_pairs = n_pairs; pa.has_target = has_target;
    auto normalise = [&]() -> int {
        // the example tile: zero rows, then positive i -> row i, negative i -> row half + i, the target -> row half - 1
        REVO_HIP_CHECK(hipMemsetAsync(g->qb.p, 0, (size_t)rows * D * sizeof(bf16_t), st));
        CHECK_RC(launch_l2norm_rows(positives, D, g->qf.p, D, g->qb.p, D, n_pairs, D, st, 1, g->qstat.p));
        CHECK_RC(launch_l2norm_rows(negatives, D, g->qf.p + (size_t)half * D, D, g->qb.p + (size_t)half * D, D, n_pairs, D, st, 1,
                                    g->qstat.p + 2 * half));
        if (has_target)
            CHECK_RC(launch_l2norm_rows(target, D, g->qf.p + (size_t)(half - 1) * D, D, g->qb.p + (size_t)(half - 1) * D, D, 1, D, st,
                                        1, g->qstat.p + 2 * (half - 1)));
        return 0;
    };
    auto rescore = [&](const uint32_t* cand, long n, int b, unsigned long long* kept, uint64_t* out_keys, float* out_scores) -> int {
        return launch_discover_rescore(cand, n, g->qf.p, D, half, n_pairs, has_target, g->gf.p, D, D, has_thr, thr, b, kept, out_keys,
                                       out_scores, st);
    };
    return search_by_examples(g, "discover", rows, 2 * n_pairs + has_target, pa, k, has_thr, thr, index_offset, scores,
                              (long long*)indices, counts, allow, st, normalise, launch_discover_pass, rescore, ExamplesPlain{});
    API_END
}

// ---- boosted search (include/revo.h revo_search_boosted; boost.hip): the third user of the skeleton
namespace {
// what the boosted search adds: the similarities by row behind the workspace, the strided sample, the domain check of mult and
// bias (the candidate pass counted the allowed rows outside it), the emit that also delivers the similarities
struct ExamplesBoosted {
    float* sim = nullptr;
    float* similarities = nullptr;
    void carve(Layout& l, long N) { sim = l.take<float>(N); }
    void sample(revo::BoostPassArgs& pa, long n_s, long N) const { pa.N = N; pa.n_sample = n_s; }
    int after_pass(const unsigned long long (&h)[4]) const {
        REVO_REQUIRE(h[3] == 0, "search_boosted: " + std::to_string(h[3]) + " allowed rows have a mult that is negative or not "
                                "finite, or a bias that is not finite");
        return 0;
    }
    int emit(const uint64_t* sk, const float* sv, long n, int k, int b, long index_offset, float* scores, long long* indices,
             int* counts, hipStream_t st) const {
        return revo::launch_boost_emit(sk, sv, n, k, b, index_offset, sim, scores, similarities, indices, counts, st);
    }
};
}  // namespace
extern "C" int32_t revo_search_boosted(revo_gallery* g, const float* query, const float* mult, const float* bias, int32_t k,
                                       int32_t has_thr, float thr, int32_t has_min, float min_sim, int64_t index_offset,
                                       float* scores, float* similarities, int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && query && scores && similarities && indices && counts, "search_boosted: null argument");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_boosted: k must be in [1, 1024]");
    CHECK_RC(require_threshold(has_thr, thr, "search_boosted"));
    REVO_REQUIRE(!has_min || !std::isnan(min_sim), "search_boosted: min_similarity is NaN");
    CHECK_RC(require_f32_rows(g, "search_boosted"));
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const int D = g->D;
    BoostPassArgs pa{};
    pa.mult = mult; pa.bias = bias; pa.has_min = has_min ? 1 : 0; pa.min_sim = min_sim;
    ExamplesBoosted ext;
    ext.similarities = similarities;
    // (an empty gallery: the skeleton pads scores, indices and counts; the similarities' padding goes in front of it)
    if (g->size == 0) CHECK_RC(launch_topk_fill_empty(similarities, (long long*)indices, counts, 1, k, st));
    auto normalise = [&]() -> int { return launch_l2norm_rows(query, D, g->qf.p, D, g->qb.p, D, 1, D, st, 1, g->qstat.p); };
    auto rescore = [&](const uint32_t* cand, long n, int b, unsigned long long* kept, uint64_t* out_keys, float* out_scores) -> int {
        BoostRescoreArgs ra{};
        ra.cand = cand; ra.n = n; ra.Qf = g->qf.p; ra.Gf = g->gf.p; ra.ldg = D; ra.D = D; ra.mult = mult; ra.bias = bias;
        ra.has_min = pa.has_min; ra.min_sim = min_sim; ra.has_thr = has_thr ? 1 : 0; ra.thr = thr; ra.b = b;
        ra.kept = kept; ra.out_keys = out_keys; ra.out_scores = out_scores; ra.sim = ext.sim;
        return launch_boost_rescore(ra, st);
    };
    return search_by_examples(g, "boosted", 1, 1, pa, k, has_thr, thr, index_offset, scores, (long long*)indices, counts, allow, st,
                              normalise, launch_boost_pass, rescore, ext);
    API_END
}

// ---- multi-vector search (include/revo.h revo_search_maxsim; maxsim.hip)
// the CSR of the handle's group ids, built for the gallery's current rows (N >= 1)
static int maxsim_build_index(revo_gallery* g, hipStream_t st) {
    using namespace revo;
    const long N = g->size;
    g->maxsim.rows = -1;
    CHECK_RC(carve_buffer(g->maxsim.csr, st, [&](Layout& l) {
        g->maxsim.gid = l.take<int32_t>(N); g->maxsim.off = l.take<uint32_t>(N + 1); g->maxsim.row = l.take<uint32_t>(N);
        g->maxsim.pos = l.take<uint32_t>(N);
    }));
    // (scratch of the build: the candidate pipeline's buffer, carved again by the next search that uses it)
    uint64_t *keys = nullptr, *keys_alt = nullptr; float *vals = nullptr, *vals_alt = nullptr; uint32_t* hist = nullptr;
    unsigned long long *flags = nullptr, *meta = nullptr;
    CHECK_RC(carve_buffer(g->pbuf, st, [&](Layout& l) {
        keys = l.take<uint64_t>(N); keys_alt = l.take<uint64_t>(N); vals = l.take<float>(N); vals_alt = l.take<float>(N);
        hist = l.take<uint32_t>(256l * SORT_MAX_BLOCKS); flags = l.take<unsigned long long>(N); meta = l.take<unsigned long long>(2);
    }));
    ProfScope ps("maxsim_index", st);
    CHECK_RC(launch_maxsim_index(g->groups.p, N, keys, keys_alt, vals, vals_alt, hist, flags, meta, g->maxsim.gid, g->maxsim.off,
                                 g->maxsim.row, g->maxsim.pos, st));
    unsigned long long h[2] = {0, 0};
    REVO_HIP_CHECK(hipMemcpyAsync(h, meta, sizeof(h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    REVO_REQUIRE(h[0] <= h[1] && h[1] <= (unsigned long long)N, "search_maxsim: inconsistent group index");
    g->maxsim.groups = (long)h[0]; g->maxsim.grouped = (long)h[1]; g->maxsim.rows = N;
    return 0;
}
extern "C" int32_t revo_search_maxsim(revo_gallery* g, const float* queries, int32_t n, int32_t k, int32_t has_thr, float thr,
                                      int64_t index_offset, float* scores, int32_t* group_ids, int32_t* counts, float* part_scores,
                                      int64_t* part_rows_out, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "search_maxsim: null handle");
    REVO_REQUIRE(queries, "search_maxsim: null queries");
    REVO_REQUIRE(scores, "search_maxsim: null scores");
    REVO_REQUIRE(group_ids, "search_maxsim: null group_ids");
    REVO_REQUIRE(counts, "search_maxsim: null counts");
    REVO_REQUIRE(n >= 1 && n <= revo::MAXSIM_MAX_VECTORS, "search_maxsim: n_vectors must be in [1, 64]");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_maxsim: k must be in [1, 1024]");
    CHECK_RC(require_threshold(has_thr, thr, "search_maxsim"));
    CHECK_RC(require_f32_rows(g, "search_maxsim"));
    REVO_REQUIRE(g->groups_rows >= 0, "search_maxsim: no group ids (revo_search_set_groups)");
    REVO_REQUIRE(g->groups_rows == g->size,
                 "search_maxsim: the group ids were set for " + std::to_string(g->groups_rows) + " rows but the gallery holds " +
                     std::to_string(g->size) + " (set them again after appending)");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    long long* part_rows = (long long*)part_rows_out;
    const long N = g->size;
    const int D = g->D;
    const int n_pad = (n + 3) / 4 * 4;
    g->drop_two_phase();
    CHECK_RC(begin_counted(g, n, "search_maxsim", st));
    MaxsimGroupArgs ga{};
    ga.n = n; ga.n_pad = n_pad; ga.lanes = maxsim_group_lanes(n_pad); ga.allow = allow; ga.D = D;
    if (N > 0 && g->maxsim.rows != N) CHECK_RC(maxsim_build_index(g, st));
    const long G = N > 0 ? g->maxsim.groups : 0, n_grouped = N > 0 ? g->maxsim.grouped : 0;
    if (G == 0) {
        // an empty gallery, or no row with a group: all padding
        CHECK_RC(launch_maxsim_emit(ga, nullptr, nullptr, 0, k, n, index_offset, scores, group_ids, counts, part_scores, part_rows, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    REVO_REQUIRE(G < (1l << 31), "search_maxsim: too many groups");
    const size_t s_bytes = (size_t)N * n_pad * sizeof(float);
    if (g->maxsim.s.bytes < s_bytes && g->maxsim.s.grow(s_bytes, st) != 0) {
        (void)hipGetLastError();
        revo_set_error("search_maxsim: could not allocate the score workspace of " + std::to_string(s_bytes) + " bytes (rows x " +
                       std::to_string(n_pad) + " x 4)");
        return -3;
    }
    // the candidate pipeline's workspace over GROUPS (kept keys, sort buffers), and behind it the bounds and the candidate lists
    long cap = 0;
    CandidateWs ws{g->pbuf, cap};
    float *tau = nullptr, *lb = nullptr, *ub = nullptr; uint32_t *acnt = nullptr, *cgroups = nullptr, *crows = nullptr;
    CHECK_RC(ws.carve(G, st, [&](Layout& l) {
        tau = l.take<float>(1); lb = l.take<float>(G); ub = l.take<float>(G); acnt = l.take<uint32_t>(G);
        cgroups = l.take<uint32_t>(G); crows = l.take<uint32_t>(n_grouped);
    }));
    { ProfScope ps("search_prep", st);
      CHECK_RC(launch_l2norm_rows(queries, D, g->qf.p, D, g->qb.p, D, n, D, st, 1, g->qstat.p));
      REVO_HIP_CHECK(hipMemsetAsync(ws.cnt, 0, sizeof(ws.h), st)); }
    ga.S = g->maxsim.s.p; ga.gid = g->maxsim.gid; ga.off = g->maxsim.off; ga.rows = g->maxsim.row; ga.G = G;
    ga.qstat = g->qstat.p; ga.gstat = g->gstat.p;
    { ProfScope ps("maxsim_pass", st);
      MaxsimPassArgs pa{};
      pa.Qb = g->qb.p; pa.ldq = D; pa.Gb = g->gb.p; pa.ldg = D; pa.n = n; pa.n_pad = n_pad; pa.N = N; pa.D = D; pa.allow = allow;
      pa.S = g->maxsim.s.p;
      CHECK_RC(launch_maxsim_pass(pa, st)); }
    { ProfScope ps("maxsim_bounds", st);
      CHECK_RC(launch_maxsim_bounds(ga, lb, ub, acnt, ws.cnt, st)); }
    { ProfScope ps("maxsim_level", st);
      CHECK_RC(launch_recommend_level(lb, (int)G, k, has_thr, thr, tau, st));
      CHECK_RC(launch_maxsim_select(ga, n_grouped, g->maxsim.pos, ub, acnt, tau, ws.cnt, crows, cgroups, st)); }
    // counters: [0] candidate rows, [1] kept groups, [2] groups with an allowed row, [3] candidate groups
    REVO_HIP_CHECK(hipMemcpyAsync(ws.h, ws.cnt, sizeof(ws.h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    REVO_REQUIRE(ws.h[0] <= (unsigned long long)n_grouped && ws.h[3] <= (unsigned long long)G, "search_maxsim: more candidates than rows");
    { ProfScope ps("maxsim_rescore", st);
      CHECK_RC(launch_maxsim_rescore(crows, (long)ws.h[0], g->qf.p, D, n, n_pad, g->gf.p, D, D, g->maxsim.s.p, st)); }
    { ProfScope ps("maxsim_reduce", st);
      CHECK_RC(launch_maxsim_reduce(ga, cgroups, (long)ws.h[3], has_thr, thr, ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    ws.n_cand = ws.h[3];
    CHECK_RC(ws.sort_kept("maxsim_sort", 64, st));   // (the score sits above all 32 bits of the group position)
    { ProfScope ps("maxsim_emit", st);
      CHECK_RC(launch_maxsim_emit(ga, ws.sk, ws.sv, (long)ws.n_kept, k, n, index_offset, scores, group_ids, counts, part_scores,
                                  part_rows, st)); }
    return publish_candidate_stats(g->xw.ctr, ws.h[0], ws.h[2] > 0 ? 1 : 0, st);
    API_END
}

// ---- diverse search (include/revo.h revo_search_mmr; mmr.hip)
constexpr size_t MMR_GRAM_BYTES = 256ul << 20;   // the similarity matrices of one chunk of queries
extern "C" int32_t revo_search_mmr(revo_gallery* g, const float* queries, int32_t Q, int32_t k, int32_t C, float diversity,
                                   int32_t has_thr, float thr, int64_t index_offset, float* scores, float* mmr_values,
                                   int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (queries || Q == 0), "search_mmr: null argument");
    REVO_REQUIRE(Q >= 0, "search_mmr: negative query count");
    REVO_REQUIRE(C >= 1 && C <= revo::LARGE_K_MAX, "search_mmr: candidates must be in [1, 1024]");
    REVO_REQUIRE(k >= 1 && k <= C, "search_mmr: k must be in [1, candidates]");
    REVO_REQUIRE(diversity >= 0.f && diversity <= 1.f, "search_mmr: diversity must be in [0, 1] (and not NaN)");
    CHECK_RC(require_threshold(has_thr, thr, "search_mmr"));
    CHECK_RC(require_f32_rows(g, "search_mmr"));
    if (Q == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const size_t per_query = (size_t)C * C * sizeof(float);
    const int QC = (int)std::min<size_t>((size_t)Q, std::max<size_t>(1, MMR_GRAM_BYTES / per_query));
    float *rel = nullptr, *gram = nullptr; long long* cand = nullptr; int* n_cand = nullptr;
    CHECK_RC(carve_buffer(g->pbuf, st, [&](Layout& l) {
        rel = l.take<float>((size_t)Q * C); cand = l.take<long long>((size_t)Q * C); n_cand = l.take<int>(Q);
        gram = l.take<float>((size_t)QC * C * C);
    }));
    // the candidates: the large-k search's own lists (it clears and fills the handle's counters, and drops the two-phase state)
    CHECK_RC(search_topk_large(g, queries, Q, C, has_thr, thr, 0, rel, cand, n_cand, allow, st));
    int tile = 8;
#ifdef REVO_EXPERIMENTS
    if (const char* e = getenv("REVO_MMR_TILE")) tile = atoi(e) == 4 ? 4 : 8;                // tile shape study (scripts/)
#endif
    for (int c0 = 0; c0 < Q; c0 += QC) {
        const int Qc = Q - c0 < QC ? Q - c0 : QC;
        MmrGramArgs ga{};
        ga.Gf = g->gf.p; ga.ldg = g->D; ga.N = g->size; ga.D = g->D; ga.cand = cand + (size_t)c0 * C; ga.counts = n_cand + c0;
        ga.gram = gram; ga.Q = Qc; ga.C = C; ga.tile = tile;
        { ProfScope ps("mmr_gram", st);
          CHECK_RC(launch_mmr_gram(ga, st)); }
        MmrSelectArgs sa{};
        sa.rel = rel + (size_t)c0 * C; sa.cand = ga.cand; sa.counts = ga.counts; sa.gram = gram; sa.C = C; sa.k = k;
        sa.lam = 1.0f - diversity; sa.diversity = diversity; sa.idx_offset = index_offset;
        sa.scores = scores + (size_t)c0 * k; sa.mmr = mmr_values ? mmr_values + (size_t)c0 * k : nullptr;
        sa.idx = (long long*)indices + (size_t)c0 * k; sa.out_counts = counts + c0;
        { ProfScope ps("mmr_select", st);
          CHECK_RC(launch_mmr_select(sa, Qc, st)); }
    }
    return 0;
    API_END
}

// ---- hybrid queries (include/revo.h FUSION; fusion.hip)
namespace {
// the domains both entry points share, and the kernel's arguments they decide (weights and list thresholds travel by value)
int fusion_args(const char* who, int32_t n, int32_t m, int32_t C, int32_t method, float rrf_k, const float* weights,
                const float* list_thresholds, int32_t k, int32_t has_thr, float thr, revo::FusionArgs& a) {
    const std::string w(who);
    REVO_REQUIRE(n >= 0, w + ": negative search count");
    REVO_REQUIRE(m >= 1 && m <= revo::FUSION_MAX_LISTS, w + ": lists must be in [1, 64]");
    REVO_REQUIRE(C >= 1 && C <= revo::LARGE_K_MAX, w + ": limit must be in [1, 1024]");
    REVO_REQUIRE(m * C <= revo::FUSION_MAX_KEYS, w + ": lists * limit must be at most 8192");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, w + ": k must be in [1, 1024]");
    REVO_REQUIRE(method == 0 || method == 1, w + ": method must be 0 (RRF) or 1 (DBSF)");
    REVO_REQUIRE(std::isfinite(rrf_k) && rrf_k >= 0.f, w + ": rrf_k must be finite and >= 0");
    REVO_REQUIRE((long long)n * m <= 0x7fffffffll, w + ": searches * lists must fit 31 bits");
    a.m = m; a.C = C; a.k = k; a.method = method; a.rrf_k = rrf_k; a.has_thr = has_thr ? 1 : 0; a.thr = thr;
    for (int j = 0; j < revo::FUSION_MAX_LISTS; ++j) { a.w[j] = 1.f; a.t[j] = -INFINITY; }
    for (int j = 0; j < m; ++j) {
        if (weights) {
            REVO_REQUIRE(std::isfinite(weights[j]) && weights[j] >= 0.f, w + ": a weight must be finite and >= 0");
            a.w[j] = weights[j];
        }
        if (list_thresholds) {
            REVO_REQUIRE(!std::isnan(list_thresholds[j]), w + ": a list threshold is NaN");
            a.t[j] = list_thresholds[j];
        }
    }
    return require_threshold(has_thr, thr, who);
}
}  // namespace

extern "C" int32_t revo_topk_fuse(const float* scores, const int64_t* indices, const int32_t* counts, int32_t n, int32_t m,
                                  int32_t C, int32_t method, float rrf_k, const float* weights, const float* list_thresholds,
                                  int32_t k, int32_t has_thr, float thr, float* out_scores, int64_t* out_indices,
                                  int32_t* out_counts, int32_t* out_ranks, void* stream) {
    API_BEGIN
    REVO_REQUIRE(out_scores && out_indices && out_counts && ((scores && indices && counts) || n == 0), "topk_fuse: null argument");
    revo::FusionArgs a{};
    CHECK_RC(fusion_args("topk_fuse", n, m, C, method, rrf_k, weights, list_thresholds, k, has_thr, thr, a));
    if (n == 0) return 0;
    a.scores = scores; a.idx = (const long long*)indices; a.counts = counts; a.idx_offset = 0;
    a.out_scores = out_scores; a.out_idx = (long long*)out_indices; a.out_counts = out_counts; a.out_ranks = out_ranks;
    ProfScope ps("fusion_fuse", (hipStream_t)stream);
    return revo::launch_fusion_fuse(a, n, (hipStream_t)stream);
    API_END
}

extern "C" int32_t revo_search_fusion(revo_gallery* g, const float* queries, int32_t n, int32_t m, int32_t C, int32_t method,
                                      float rrf_k, const float* weights, const float* list_thresholds, int32_t k,
                                      int32_t has_thr, float thr, int64_t index_offset, float* scores, int64_t* indices,
                                      int32_t* counts, int32_t* ranks, float* list_scores, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (queries || n == 0), "search_fusion: null argument");
    revo::FusionArgs a{};
    CHECK_RC(fusion_args("search_fusion", n, m, C, method, rrf_k, weights, list_thresholds, k, has_thr, thr, a));
    CHECK_RC(require_f32_rows(g, "search_fusion"));
    if (n == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const int Q = n * m, D = g->D;
    float *ls = nullptr, *qn = nullptr; long long* li = nullptr; int* lc = nullptr;
    CHECK_RC(carve_buffer(g->fbuf, st, [&](Layout& l) {
        ls = l.take<float>((size_t)Q * C); li = l.take<long long>((size_t)Q * C); lc = l.take<int>(Q);
        qn = l.take<float>(list_scores ? (size_t)Q * D : 0);
    }));
    // the lists: the large-k search's own results (it clears and fills the handle's counters, and drops the two-phase state)
    CHECK_RC(search_topk_large(g, queries, Q, C, 0, 0.f, 0, ls, li, lc, allow, st));
    a.scores = ls; a.idx = li; a.counts = lc; a.idx_offset = index_offset;
    a.out_scores = scores; a.out_idx = (long long*)indices; a.out_counts = counts; a.out_ranks = ranks;
    { ProfScope ps("fusion_fuse", st);
      CHECK_RC(launch_fusion_fuse(a, n, st)); }
    if (list_scores) {
        // the inner search normalises its queries a chunk at a time into rows it reuses: the same kernel, every row kept
        ProfScope ps("fusion_list_scores", st);
        CHECK_RC(launch_l2norm_rows(queries, D, qn, D, nullptr, 0, Q, D, st));
        CHECK_RC(launch_fusion_list_scores(qn, D, g->gf.p, D, D, a.out_idx, counts, index_offset, n, m, k, list_scores, st));
    }
    return 0;
    API_END
}
