// C ABI of the gallery handle and the search (include/revo.h): the handle's rows, filter, group ids and workspace, the
// search pipeline with its exactness fallback, grouped search, the row-sharded protocol's entry points and the merges.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "api_internal.h"
#include "kernels.h"

// ------------------------------------------------------------ the gallery --
namespace {
// A device allocation owned by the handle, grown on demand and never shrunk.  Growing a buffer that holds an allocation
// first waits for the stream (an earlier launch may still read it), then frees it.  After a failed allocation the
// buffer is empty.
template <class T = char> struct DeviceBuffer {
    T* p = nullptr; size_t bytes = 0;
    DeviceBuffer() = default; DeviceBuffer(const DeviceBuffer&) = delete; DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    int grow(size_t need, hipStream_t st) {
        if (bytes >= need) return 0;
        if (p) REVO_HIP_CHECK(hipStreamSynchronize(st));
        release();
        REVO_HIP_CHECK(hipMalloc((void**)&p, need));
        bytes = need;
        return 0;
    }
    // grown to at least `need` bytes (at least twice its size) with its first `keep` bytes carried over
    int grow_keep(size_t need, size_t keep, hipStream_t st) {
        if (bytes >= need) return 0;
        const size_t nb = need > 2 * bytes ? need : 2 * bytes;
        T* q = nullptr;
        REVO_HIP_CHECK(hipMalloc((void**)&q, nb));
        hipError_t e = keep > 0 ? hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess && keep > 0) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(q);
            revo_set_error(std::string("DeviceBuffer::grow_keep: ") + hipGetErrorString(e));
            return -1;
        }
        release();
        p = q; bytes = nb;
        return 0;
    }
  private:
    void release() { (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Sub-arrays carved out of one buffer in order, each at the next multiple of 256 bytes (a null base: sizing only).
struct Layout {
    char* base = nullptr;
    size_t size = 0;
    template <class T> T* take(size_t count) {
        size = (size + 255) / 256 * 256;
        T* p = base ? (T*)(base + size) : nullptr;
        size += count * sizeof(T);
        return p;
    }
};
// Runs carve(Layout&) once to size `buf`, grows it, and again to hand out the sub-arrays of the grown buffer.
template <class F> int carve_buffer(DeviceBuffer<>& buf, hipStream_t st, F&& carve) {
    Layout sizing; carve(sizing);
    CHECK_RC(buf.grow(sizing.size, st));
    Layout l{buf.p}; carve(l);
    return 0;
}

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
}  // namespace

struct revo_gallery {
    int D = 0, device = 0, keep_f32 = 1;
    int64_t capacity = 0, size = 0;
    DeviceBuffer<bf16_t> gb;   // [capacity][D] normalised rows, scan copy
    DeviceBuffer<float> gf;    // [capacity][D] normalised rows, fp32 master (re-score + persistence)
    // per-call workspace, grown on demand: the per-query arrays (sized for q_cap queries; qstat, marg and dropflag
    // below), the scan's workspace (part) and the staging rows of an append from the host
    DeviceBuffer<float> qf; DeviceBuffer<bf16_t> qb; DeviceBuffer<uint32_t> tau0; int q_cap = 0;
    DeviceBuffer<> part;
    DeviceBuffer<float> stage;
    // candidates of the last scan (inside `part`), consumed by the finish step
    const uint64_t* cand = nullptr; long cand_stride = 0; int cand_Q = 0, cand_ksel = 0;
    // the last scan ran with an admission margin: its segments can answer uncertified queries (CertArgs, kernels.h)
    revo::SegSrc segs[2] = {}; int nsegs = 0; const uint64_t* prelist = nullptr;
    DeviceBuffer<float> marg; DeviceBuffer<int> dropflag;
    int64_t total_rows = 0;        // revo_search_set_total_rows: this handle is one shard of a gallery of that many rows (0: the whole)
    bool cand_estimated = false;   // the last scan started from estimated admission scores (CertArgs::estimated)
    // exactness certificate (kernels.h): per-query rounding norms of the last search's queries, running maxima over the
    // gallery's rows, the fallback workspace (xbuf, sized with q_cap; its layout is xw) and the handle's mode
    DeviceBuffer<float> qstat; DeviceBuffer<uint32_t> gstat;
    DeviceBuffer<> xbuf; revo::ExactWs xw{};
    int mode = 0;
    const uint32_t* seed_bounds = nullptr;   // experiment build only (revo_debug_seed_bounds): admission bounds from outside
    // revo_search_set_filter: the handle's own copy of the allow-bitmap, zero-padded to whole 256-row tiles; filter_rows =
    // the gallery size it was set for, -1 = no filter
    DeviceBuffer<uint32_t> filter; int64_t filter_rows = -1;
    // revo_search_set_groups: the handle's copy of the rows' group ids, set for groups_rows rows, -1 = none; the grouped
    // search's workspace: top-GROUP_K1 scores | indices | counts | fallback queries | chosen groups
    DeviceBuffer<int32_t> groups; int64_t groups_rows = -1;
    DeviceBuffer<> gbuf;
    // revo_search_topk_large's workspace (revo::LargeWs, carved per search)
    DeviceBuffer<> lbuf;
    // revo_gallery_pairs: its workspace (counters | candidate keys | kept keys and scores | sort buffers), the candidate keys
    // that workspace holds, and the last result ([pairs_n][2] row pairs, [pairs_n] scores), valid until the rows change
    DeviceBuffer<> pbuf; long pairs_cap = 0;
    DeviceBuffer<long long> pair_idx; DeviceBuffer<float> pair_score;
    int64_t pairs_n = 0; bool pairs_valid = false;
    // revo_search_range: the candidate keys its workspace (in pbuf) holds, and the last result ([range_n] indices and scores,
    // [range_q + 1] offsets), valid until the rows change
    long range_cap = 0;
    DeviceBuffer<long long> range_idx; DeviceBuffer<float> range_score; DeviceBuffer<unsigned long long> range_off;
    int64_t range_n = 0, range_q = 0; bool range_valid = false;
    // revo_search_maxsim: the CSR of the group ids (gid | off | rows | pos_group in csr; revo::launch_maxsim_index), built at
    // the first call for csr_rows rows (-1: none; dropped by revo_search_set_groups, an append and a clear), and the score
    // workspace S [N][n_pad]
    DeviceBuffer<> csr; int64_t csr_rows = -1; long csr_groups = 0, csr_grouped = 0;
    int32_t* csr_gid = nullptr; uint32_t *csr_off = nullptr, *csr_row = nullptr, *csr_pos = nullptr;
    DeviceBuffer<float> maxsim_s;
    // revo_gallery_clusters: its workspace (counters | union-find and error word | sizes | member keys and the sort's buffers),
    // and the last result ([clusters_rows] labels, [clusters_n + 1] offsets, [clusters_members] rows), valid until the rows
    // change
    DeviceBuffer<> cbuf;
    DeviceBuffer<long long> cl_labels, cl_off, cl_members;
    int64_t clusters_rows = 0, clusters_n = 0, clusters_members = 0; bool clusters_valid = false;
    // revo_gallery_remove: per-chunk counts | first removed rows | the copy of a host bitmap; revo_gallery_update: the row map
    DeviceBuffer<> edit;
    // the rows change: results held in the handle and the two-phase candidate state go
    void rows_changed() {
        pairs_valid = false; range_valid = false; clusters_valid = false;
        cand = nullptr; cand_Q = 0; cand_ksel = 0; nsegs = 0; prelist = nullptr; cand_estimated = false;
    }
    revo::CertArgs cert_args(float* cert_out) const {
        revo::CertArgs c{};
        c.qstat = qstat.p; c.gstat = gstat.p; c.mode = mode; c.ws = xw; c.Qb = qb.p; c.ldq = D; c.cert_out = cert_out;
        c.nsegs = nsegs; c.segs[0] = segs[0]; c.segs[1] = segs[1]; c.seg_ksel = cand_ksel; c.prelist = prelist;
        c.tau_base = tau0.p; c.marg = marg.p; c.dropflag = dropflag.p; c.estimated = cand_estimated ? 1 : 0;
        return c;
    }
};

extern "C" int32_t revo_gallery_create(int32_t dim, int64_t capacity, int32_t device, int32_t keep_f32,
                                       revo_gallery** out) {
    API_BEGIN
    REVO_REQUIRE(out, "gallery_create: null argument");
    REVO_REQUIRE(dim >= 64 && dim % 64 == 0, "gallery_create: dim must be a positive multiple of 64");
    REVO_REQUIRE(capacity >= 1 && capacity < (1ll << 32), "gallery_create: capacity must be in [1, 2^32)");
    REVO_ON_DEVICE(device);
    std::unique_ptr<revo_gallery> g(new revo_gallery());
    g->D = dim; g->device = device; g->capacity = capacity; g->keep_f32 = keep_f32 != 0;
    CHECK_RC(g->gb.grow((size_t)capacity * dim * 2, nullptr));
    if (g->keep_f32) CHECK_RC(g->gf.grow((size_t)capacity * dim * 4, nullptr));
    CHECK_RC(g->gstat.grow(8, nullptr));
    REVO_HIP_CHECK(hipMemset(g->gstat.p, 0, 8));
    *out = g.release();
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_destroy(revo_gallery* g) {
    API_BEGIN
    if (g) { DeviceGuard dg(g->device); delete g; }
    return 0;
    API_END
}
extern "C" int64_t revo_gallery_size(const revo_gallery* g) { return g ? g->size : -1; }
extern "C" int32_t revo_search_set_total_rows(revo_gallery* g, int64_t total_rows) {
    REVO_REQUIRE(g && total_rows >= 0, "search_set_total_rows: null handle or negative row count");
    g->total_rows = total_rows;
    return 0;
}
// the handle's copy of an allow-bitmap: dst[i] = src[i] for the `nsrc` words that hold rows, bits from row `rows` on cleared,
// zero words up to `total` (whole 256-row tiles: the filtered scans read a wave's 64 bits of any tile they touch).  src may
// be dst (a host bitmap is first copied into place).
__global__ void filter_copy_kernel(uint32_t* dst, const uint32_t* src, long rows, long nsrc, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    uint32_t w = i < nsrc ? src[i] : 0u;
    if (i == rows >> 5 && (rows & 31)) w &= (1u << (rows & 31)) - 1u;
    dst[i] = w;
}
extern "C" int32_t revo_search_set_filter(revo_gallery* g, const uint32_t* allow_bits, int64_t rows, int32_t src_on_device,
                                          void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "search_set_filter: null handle");
    REVO_REQUIRE(rows >= 0, "search_set_filter: negative row count");
    if (!allow_bits) { g->filter_rows = -1; return 0; }
    REVO_REQUIRE(rows == g->size, "search_set_filter: rows must equal revo_gallery_size (the filter covers the whole gallery)");
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    const long nsrc = (long)((rows + 31) / 32);
    const long total = (long)((rows + 255) / 256 * 8) > 8 ? (long)((rows + 255) / 256 * 8) : 8;
    g->filter_rows = -1;                                  // (until the copy below has been enqueued)
    CHECK_RC(g->filter.grow((size_t)total * 4, st));
    const uint32_t* src = allow_bits;
    if (!src_on_device) {
        // the caller may free its host buffer on return: copy now
        if (nsrc > 0) REVO_HIP_CHECK(hipMemcpyAsync(g->filter.p, allow_bits, (size_t)nsrc * 4, hipMemcpyHostToDevice, st));
        src = g->filter.p;
    }
    hipLaunchKernelGGL(filter_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g->filter.p, src, (long)rows,
                       nsrc, total);
    REVO_HIP_CHECK(hipGetLastError());
    if (!src_on_device) REVO_HIP_CHECK(hipStreamSynchronize(st));
    g->filter_rows = rows;
    return 0;
    API_END
}
// the allow-bitmap the next search of this handle runs with (null: none) -- a filter set for another gallery size is an
// error, never a silently unfiltered search
static int search_filter(const revo_gallery* g, const uint32_t** out) {
    *out = nullptr;
    if (g->filter_rows < 0) return 0;
    REVO_REQUIRE(g->filter_rows == g->size,
                 "search: the filter was set for " + std::to_string(g->filter_rows) + " rows but the gallery holds " +
                     std::to_string(g->size) + " (set it again after appending)");
    *out = g->filter.p;
    return 0;
}

extern "C" int32_t revo_search_set_groups(revo_gallery* g, const int32_t* group_of_row, int64_t rows, int32_t src_on_device,
                                          void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "search_set_groups: null handle");
    REVO_REQUIRE(rows >= 0, "search_set_groups: negative row count");
    g->csr_rows = -1;
    if (!group_of_row) { g->groups_rows = -1; return 0; }
    REVO_REQUIRE(rows == g->size, "search_set_groups: rows must equal revo_gallery_size (one group id per gallery row)");
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    g->groups_rows = -1;                                  // (until the copy below has been enqueued)
    CHECK_RC(g->groups.grow((size_t)(rows > 1 ? rows : 1) * 4, st));
    if (rows > 0)
        REVO_HIP_CHECK(hipMemcpyAsync(g->groups.p, group_of_row, (size_t)rows * 4,
                                      src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!src_on_device) REVO_HIP_CHECK(hipStreamSynchronize(st));   // the caller may free its host buffer on return
    g->groups_rows = rows;
    return 0;
    API_END
}

extern "C" int32_t revo_gallery_clear(revo_gallery* g) {
    REVO_REQUIRE(g, "null handle");
    REVO_ON_DEVICE(g->device);
    REVO_HIP_CHECK(hipMemset(g->gstat.p, 0, 8));      // the row maxima of the certificate start over with the rows
    g->size = 0;
    g->pairs_valid = false;
    g->range_valid = false;
    g->clusters_valid = false;
    g->csr_rows = -1;
    return 0;
}

extern "C" int32_t revo_gallery_append(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize,
                                       int32_t src_on_device, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && (vecs || n == 0), "gallery_append: null argument");
    REVO_REQUIRE(n >= 0 && g->size + n <= g->capacity, "gallery_append: exceeds the capacity given at create");
    if (n == 0) return 0;
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    g->pairs_valid = false;
    g->range_valid = false;
    g->clusters_valid = false;
    g->csr_rows = -1;
    const int D = g->D;
    const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / (D * 4));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        const float* src = vecs + done * D;
        if (!src_on_device) {
            const size_t need = (size_t)m * D * 4;
            CHECK_RC(g->stage.grow(need, st));
            REVO_HIP_CHECK(hipMemcpyAsync(g->stage.p, src, need, hipMemcpyHostToDevice, st));
            src = g->stage.p;
        }
        const int64_t row0 = g->size + done;
        bf16_t* db = g->gb.p + row0 * D;
        float* df = g->keep_f32 ? g->gf.p + row0 * D : nullptr;
        ProfScope ps("gallery_append", st);
        // one kernel either way: fp32 master row, bf16 scan row, and the row's share of the certificate's maxima
        // (max ||g||, max ||bf16(g) - g||; with normalize = 0 the rows are stored as given, whatever their length)
        CHECK_RC(revo::launch_l2norm_rows(src, D, df, D, db, D, m, D, st, normalize ? 1 : 0, nullptr, g->gstat.p));
        if (!src_on_device) REVO_HIP_CHECK(hipStreamSynchronize(st));   // staging buffer is reused
    }
    g->size += n;
    return 0;
    API_END
}

extern "C" int32_t revo_gallery_read(revo_gallery* g, int64_t start, int64_t n, float* dst, int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g && dst, "gallery_read: null argument");
    REVO_REQUIRE(g->keep_f32, "gallery_read: gallery was created without the fp32 master copy");
    REVO_REQUIRE(start >= 0 && n >= 0 && start + n <= g->size, "gallery_read: range outside the gallery");
    if (n == 0) return 0;
    REVO_ON_DEVICE(g->device);
    REVO_HIP_CHECK(hipMemcpy(dst, g->gf.p + start * g->D, (size_t)n * g->D * 4,
                             dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return 0;
    API_END
}

// ---- rows leave and change in place (include/revo.h EDIT; gallery_edit.hip)
#ifdef REVO_EXPERIMENTS
static long g_remove_chunk = 0;
extern "C" int32_t revo_debug_set_remove_chunk(int64_t rows) {
    REVO_REQUIRE(rows >= 0, "debug_set_remove_chunk: negative row count");
    g_remove_chunk = rows == 0 ? 0 : std::min<long>(revo::REMOVE_MAX_CHUNK, (long)((rows + 31) / 32 * 32));
    return 0;
}
#endif
extern "C" int32_t revo_gallery_remove(revo_gallery* g, const uint32_t* remove_bits, int64_t rows, int32_t src_on_device,
                                       int64_t* n_removed, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_remove: null handle");
    REVO_REQUIRE(n_removed, "gallery_remove: null n_removed");
    REVO_REQUIRE(rows >= 0, "gallery_remove: negative row count");
    REVO_REQUIRE(remove_bits || rows == 0, "gallery_remove: null remove_bits");
    REVO_REQUIRE(rows == g->size, "gallery_remove: rows must equal revo_gallery_size (the bitmap covers the whole gallery)");
    g->rows_changed();
    if (rows == 0) { *n_removed = 0; return 0; }
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    const int D = g->D;
    const long N = (long)rows;
    // a chunk: the append's 64 MB of fp32 rows, in whole bitmap words
    long chunk = std::min<long>(revo::REMOVE_MAX_CHUNK, std::max<long>(32, (64l << 20) / (D * 4) / 32 * 32));
#ifdef REVO_EXPERIMENTS
    if (g_remove_chunk > 0) chunk = g_remove_chunk;
#endif
    const long nchunks = (N + chunk - 1) / chunk, nwords = (N + 31) / 32;
    uint32_t *cnt = nullptr, *first = nullptr, *own_bits = nullptr;
    CHECK_RC(carve_buffer(g->edit, st, [&](Layout& l) {
        cnt = l.take<uint32_t>(nchunks); first = l.take<uint32_t>(nchunks);
        if (!src_on_device) own_bits = l.take<uint32_t>(nwords);
    }));
    const uint32_t* bits = remove_bits;
    if (!src_on_device) {
        REVO_HIP_CHECK(hipMemcpyAsync(own_bits, remove_bits, (size_t)nwords * 4, hipMemcpyHostToDevice, st));
        bits = own_bits;
    }
    std::vector<uint32_t> h_cnt(nchunks), h_first(nchunks);
    { ProfScope ps("gallery_remove", st);
      CHECK_RC(revo::launch_remove_count(bits, N, chunk, cnt, first, st)); }
    REVO_HIP_CHECK(hipMemcpyAsync(h_cnt.data(), cnt, (size_t)nchunks * 4, hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipMemcpyAsync(h_first.data(), first, (size_t)nchunks * 4, hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    // Chunk after chunk, front to back, everything ordered on the stream.  The kept rows of chunk c go to rows
    // [base, base + cnt) with base <= row0 and base + cnt <= row0 + len: below every later chunk's rows.  Where that range
    // ends at or before row0 the gather writes it directly (source and destination rows are disjoint); otherwise it gathers
    // into staging memory, and a copy ordered behind it brings the run down.  No launch writes a row it also reads.
    long base = 0;
    {
        ProfScope ps("gallery_remove", st);
        for (long c = 0; c < nchunks; ++c) {
            const long row0 = c * chunk, len = std::min(chunk, N - row0), kept = (long)h_cnt[c];
            REVO_REQUIRE(kept <= len && base <= row0, "gallery_remove: internal: inconsistent chunk counts");
            // rows in front of the first removed row of the whole gallery stay where they are
            const long j0 = base == row0 ? std::min<long>((long)h_first[c], kept) : 0;
            if (kept > j0) {
                const bool direct = base + kept <= row0;
                if (!direct) CHECK_RC(g->stage.grow((size_t)chunk * D * 4, st));
                for (int which = g->keep_f32 ? 0 : 1; which < 2; ++which) {
                    const int u4 = which == 0 ? D / 4 : D / 8;       // 16-byte units of a row (D % 64 == 0)
                    uint4* arr = which == 0 ? (uint4*)g->gf.p : (uint4*)g->gb.p;
                    uint4* dst = direct ? arr + base * u4 : (uint4*)g->stage.p;
                    CHECK_RC(revo::launch_remove_gather(bits, N, row0, len, j0, arr, dst, u4, st));
                    if (!direct)
                        REVO_HIP_CHECK(hipMemcpyAsync(arr + (base + j0) * u4, dst + j0 * u4, (size_t)(kept - j0) * u4 * 16,
                                                      hipMemcpyDeviceToDevice, st));
                }
            }
            base += kept;
        }
        // an emptied gallery starts its certificate maxima over, as revo_gallery_clear does; otherwise they stay: maxima over
        // more rows are upper bounds still
        if (base == 0) REVO_HIP_CHECK(hipMemsetAsync(g->gstat.p, 0, 8, st));
    }
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    if (base < N) g->csr_rows = -1;
    g->size = base;
    *n_removed = N - base;
    return 0;
    API_END
}

extern "C" int32_t revo_gallery_update(revo_gallery* g, const int64_t* row_idx, const float* vecs, int64_t n, int32_t normalize,
                                       int32_t src_on_device, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_update: null handle");
    REVO_REQUIRE(n >= 0, "gallery_update: negative count");
    if (n == 0) return 0;
    REVO_REQUIRE(row_idx, "gallery_update: null row_idx");
    REVO_REQUIRE(vecs, "gallery_update: null vecs");
    {
        std::vector<int64_t> sorted(row_idx, row_idx + n);
        for (int64_t r : sorted)
            REVO_REQUIRE(r >= 0 && r < g->size, "gallery_update: row_idx " + std::to_string(r) + " outside the gallery of " +
                                                    std::to_string(g->size) + " rows");
        std::sort(sorted.begin(), sorted.end());
        for (int64_t i = 1; i < n; ++i)
            REVO_REQUIRE(sorted[i] != sorted[i - 1], "gallery_update: row_idx " + std::to_string(sorted[i]) + " is given twice");
    }
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    g->rows_changed();
    const int D = g->D;
    CHECK_RC(g->edit.grow((size_t)n * 8, st));
    long long* map = (long long*)g->edit.p;
    REVO_HIP_CHECK(hipMemcpyAsync(map, row_idx, (size_t)n * 8, hipMemcpyHostToDevice, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));             // the caller may free its host array on return
    const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / (D * 4));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        const float* src = vecs + done * D;
        if (!src_on_device) {
            const size_t need = (size_t)m * D * 4;
            CHECK_RC(g->stage.grow(need, st));
            REVO_HIP_CHECK(hipMemcpyAsync(g->stage.p, src, need, hipMemcpyHostToDevice, st));
            src = g->stage.p;
        }
        ProfScope ps("gallery_update", st);
        // the append's kernel with a destination-row map: the same bits an append of the vector would have written
        CHECK_RC(revo::launch_l2norm_rows(src, D, g->keep_f32 ? g->gf.p : nullptr, D, g->gb.p, D, m, D, st, normalize ? 1 : 0,
                                          nullptr, g->gstat.p, nullptr, 0, nullptr, 0, map + done));
        if (!src_on_device) REVO_HIP_CHECK(hipStreamSynchronize(st));   // staging buffer is reused
    }
    return 0;
    API_END
}

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
constexpr long SEARCH_SMALL_ROWS = 16384;     // below this the 128 x 128 scan with LDS lists takes the gallery
constexpr long SEARCH_WIDE_ROWS = 1l << 22;   // from here on the unsharded search keeps 64 candidates per query for every k

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
static int search_grow_queries(revo_gallery* g, int Q, hipStream_t st) {
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
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
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
                g->cand_estimated = true;
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
              if (margin) g->segs[i] = SegSrc{pt.seg, pt.cnt, pt.splits, pt.q0, pt.nq};
          }
          if (margin) { g->nsegs = nparts; g->prelist = prelist; } }
        { ProfScope ps("topk_reduce", st);
          for (int i = 0; i < nparts; ++i) {
              const Part& pt = parts[i];
              CHECK_RC(launch_topk_reduce_segs(pt.seg, pt.cnt, pt.splits, prelist + (size_t)pt.q0 * ksel,
                                               final_lists + (size_t)pt.q0 * ksel, pt.nq, ksel, st,
                                               bounds ? bounds + (size_t)pt.q0 * top_m : nullptr, top_m));
          } }
        g->cand = final_lists; g->cand_stride = ksel;
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
        g->cand = part; g->cand_stride = (long)splits * ksel;
        if (bounds) { ProfScope ps("topk_bounds", st); CHECK_RC(launch_topk_publish(g->cand, g->cand_stride, Q, top_m, bounds, st)); }
    }
    g->cand_Q = Q; g->cand_ksel = ksel;
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
      CHECK_RC(launch_topk_finish(g->cand, g->cand_stride, ksel, g->qf.p, g->D, g->keep_f32 ? g->gf.p : nullptr, g->D, g->D, Q, k,
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
static long large_sample_rows(int Q, long N, int k) {
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
static int search_topk_large(revo_gallery* g, const float* queries, int Q, int k, int has_thr, float thr, long index_offset,
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
    // (the two-phase protocol's state refers to the handle's query rows, which this search overwrites)
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
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
    REVO_REQUIRE(g->keep_f32, "search_topk_large: the gallery was created without the fp32 master copy (keep_f32 = 0)");
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
    g->cand = nullptr; g->cand_Q = Q; g->cand_ksel = ksel;
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
    REVO_REQUIRE(Q == g->cand_Q && search_ksel(k) == g->cand_ksel,
                 "search_finish: no matching revo_search_candidates call on this handle");
    REVO_REQUIRE(!all_bounds || (parts >= 1 && top_m >= 1 && top_m <= g->cand_ksel), "search_finish: bad bounds layout");
    // A scan that started from an ESTIMATED admission level (revo_search_set_total_rows) has dropped rows on the strength of
    // that estimate: only the certificate (cert -> revo_topk_merge_packed -> revo_search_exact) makes the result exhaustive
    REVO_REQUIRE(cert || !g->cand_estimated,
                 "search_finish: this shard scanned against an estimated admission level (revo_search_set_total_rows): cert must "
                 "be given and checked by revo_topk_merge_packed, with revo_search_exact as the second round");
    if (Q == 0) return 0;
    { const uint32_t* allow; CHECK_RC(search_filter(g, &allow)); }
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    if (g->size == 0 || !g->cand) {
        // an empty shard holds no row that could change a result: its certificate bound is -inf
        if (cert) REVO_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)cert, (int)0xff800000u, (size_t)Q, st));
        return launch_topk_fill_empty(scores, (long long*)indices, counts, Q, k, st);
    }
    ProfScope ps("topk_finish", st);
    const CertArgs ca = g->cert_args(cert);
    return launch_topk_finish(g->cand, g->cand_stride, g->cand_ksel, g->qf.p, g->D, g->keep_f32 ? g->gf.p : nullptr, g->D, g->D,
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
    REVO_REQUIRE(n <= g->cand_Q, "search_exact: more entries than queries in the last revo_search_candidates call");
    if (n == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    if (g->size == 0) return launch_topk_fill_empty(scores, (long long*)indices, counts, n, k, st);
    REVO_REQUIRE(g->keep_f32 && g->xw.ctr, "search_exact: the gallery was created without the fp32 master copy");
    const CertArgs ca = g->cert_args(nullptr);
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    CHECK_RC(launch_topk_exact_prepare(g->xw, q_idx, need, n, ca, g->D, g->cand, g->cand_stride, g->cand_ksel, st));
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
    REVO_REQUIRE(g->keep_f32, "search_groups: the gallery was created without the fp32 master copy (keep_f32 = 0)");
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

// ---- near-duplicate pairs of one gallery (include/revo.h revo_gallery_pairs; pairs.hip)
extern "C" int32_t revo_gallery_pairs(revo_gallery* g, float threshold, int64_t* n_pairs, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_pairs, "gallery_pairs: null argument");
    REVO_REQUIRE(!std::isnan(threshold), "gallery_pairs: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "gallery_pairs: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    REVO_REQUIRE(g->size < (1ll << 31), "gallery_pairs: row indices must fit in 31 bits");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    g->pairs_valid = false;
    const long N = g->size;
    const int D = g->D;
    // the handle's counters (revo_search_stats): this call's alone
    CHECK_RC(search_grow_queries(g, 1, st));
    REVO_REQUIRE(g->xw.ctr, "gallery_pairs: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    CandidateWs ws{g->pbuf, g->pairs_cap};
    CHECK_RC(ws.carve(g->pairs_cap > PAIRS_WS_KEYS ? g->pairs_cap : PAIRS_WS_KEYS, st));
    PairsJoinArgs ja{};
    ja.Gb = g->gb.p; ja.ldg = D; ja.N = N; ja.D = D; ja.gstat = g->gstat.p; ja.thr = threshold; ja.allow = allow;
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        ja.cnt = ws.cnt; ja.keys = ws.cand; ja.cap = ws.cap;
        ProfScope ps("pairs_join", st);
        return launch_pairs_join(ja, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)PAIRS_MAX_CAND,
                     "gallery_pairs: " + std::to_string(n_cand) + " candidate pairs exceed the limit of " +
                         std::to_string(PAIRS_MAX_CAND) + " (raise the threshold)");
        return 0;
    }, "gallery_pairs: the candidate count changed between two joins"));
    // fp32 re-score; the kept entries as (i << b) | j
    const int b = row_index_bits(N);
    { ProfScope ps("pairs_rescore", st);
      CHECK_RC(launch_pairs_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, threshold, b, ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    CHECK_RC(ws.sort_kept("pairs_sort", 2 * b, st));
    const unsigned long long n_kept = ws.n_kept;
    CHECK_RC(g->pair_idx.grow((size_t)(n_kept > 0 ? n_kept : 1) * 16, st));
    CHECK_RC(g->pair_score.grow((size_t)(n_kept > 0 ? n_kept : 1) * 4, st));
    CHECK_RC(launch_pairs_emit(ws.sk, ws.sv, (long)n_kept, b, g->pair_idx.p, g->pair_score.p, st));
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.passes, st));
    g->pairs_n = (int64_t)n_kept;
    g->pairs_valid = true;
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
    REVO_REQUIRE(g->pairs_valid, "gallery_pairs_read: no result (call revo_gallery_pairs again after the rows change)");
    REVO_REQUIRE(start + n <= g->pairs_n, "gallery_pairs_read: range past the result's " + std::to_string(g->pairs_n) + " pairs");
    if (n == 0) return 0;
    REVO_ON_DEVICE(g->device);
    const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    REVO_HIP_CHECK(hipMemcpy(pairs, g->pair_idx.p + start * 2, (size_t)n * 16, kind));
    REVO_HIP_CHECK(hipMemcpy(scores, g->pair_score.p + start, (size_t)n * 4, kind));
    return 0;
    API_END
}

// ---- duplicate clusters of one gallery (include/revo.h revo_gallery_clusters; clusters.hip)
extern "C" int32_t revo_gallery_clusters(revo_gallery* g, float threshold, int64_t* n_clusters, int64_t* n_members, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_clusters && n_members, "gallery_clusters: null argument");
    REVO_REQUIRE(!std::isnan(threshold), "gallery_clusters: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "gallery_clusters: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    REVO_REQUIRE(g->size < (1ll << 31), "gallery_clusters: row indices must fit in 31 bits");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    g->clusters_valid = false;
    const long N = g->size;
    const int D = g->D;
    const int b = row_index_bits(N);
    // the handle's counters (revo_search_stats): this call's alone
    CHECK_RC(search_grow_queries(g, 1, st));
    REVO_REQUIRE(g->xw.ctr, "gallery_clusters: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    // the union-find and the finish step's arrays: a buffer of their own, so the candidate workspace's regrow leaves parent[] be
    const size_t rows = (size_t)(N > 0 ? N : 1);
    uint32_t *parent = nullptr, *sizes = nullptr, *hist = nullptr;
    unsigned long long *ctr4 = nullptr, *rank = nullptr;
    uint64_t *keys = nullptr, *keys_alt = nullptr;
    float *vals = nullptr, *vals_alt = nullptr;
    CHECK_RC(carve_buffer(g->cbuf, st, [&](Layout& l) {
        ctr4 = l.take<unsigned long long>(4);
        parent = l.take<uint32_t>(rows + 1); sizes = l.take<uint32_t>(rows);      // parent[N]: the error word
        keys = l.take<uint64_t>(rows); keys_alt = l.take<uint64_t>(rows);
        vals = l.take<float>(rows); vals_alt = l.take<float>(rows);       // (the sort moves a value with every key: unused here)
        rank = l.take<unsigned long long>(rows);
        hist = l.take<uint32_t>(256l * SORT_MAX_BLOCKS);
    }));
    CHECK_RC(g->cl_labels.grow(rows * 8, st));
    CHECK_RC(launch_clusters_init(parent, sizes, N, ctr4, st));
    CandidateWs ws{g->pbuf, g->pairs_cap};
    CHECK_RC(ws.carve(g->pairs_cap > PAIRS_WS_KEYS ? g->pairs_cap : PAIRS_WS_KEYS, st));
    ClustersJoinArgs ja{};
    ja.j.Gb = g->gb.p; ja.j.ldg = D; ja.j.N = N; ja.j.D = D; ja.j.gstat = g->gstat.p; ja.j.thr = threshold; ja.j.allow = allow;
    ja.parent = parent;
    // (a second join repeats the first one's merges: parent[] is not reset between the passes)
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        ja.j.cnt = ws.cnt; ja.j.keys = ws.cand; ja.j.cap = ws.cap;
        ProfScope ps("clusters_join", st);
        return launch_clusters_join(ja, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)PAIRS_MAX_CAND,
                     "gallery_clusters: " + std::to_string(n_cand) + " pairs inside the rounding bound of the threshold exceed the "
                     "limit of " + std::to_string(PAIRS_MAX_CAND) + " (move the threshold)");
        return 0;
    }, "gallery_clusters: the candidate count changed between two joins"));
    { ProfScope ps("clusters_rescore", st);
      CHECK_RC(launch_clusters_rescore(ws.cand, (long)ws.n_cand, g->gf.p, D, D, threshold, parent, N, st)); }
    unsigned long long h[4] = {0, 0, 0, 0};
    { ProfScope ps("clusters_finish", st);
      CHECK_RC(launch_clusters_labels(parent, allow, N, b, g->cl_labels.p, sizes, keys, ctr4, st)); }
    REVO_HIP_CHECK(hipMemcpyAsync(h, ctr4, sizeof(h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    if (h[2] != 0) {
        revo_set_error("clusters: union-find did not converge");
        return -4;
    }
    const long n_mem = (long)h[0], n_cl = (long)h[1];
    REVO_REQUIRE(n_mem <= N && n_cl <= n_mem / 2, "gallery_clusters: internal: inconsistent counts");
    CHECK_RC(g->cl_off.grow((size_t)(n_cl + 1) * 8, st));
    CHECK_RC(g->cl_members.grow((size_t)(n_mem > 0 ? n_mem : 1) * 8, st));
    {
        ProfScope ps("clusters_finish", st);
        uint64_t* sk = nullptr; float* sv = nullptr;
        CHECK_RC(launch_sort_keys_u64(keys, vals, keys_alt, vals_alt, n_mem, 2 * b, hist, &sk, &sv, st));
        CHECK_RC(launch_clusters_emit(sk, n_mem, n_cl, b, rank, g->cl_members.p, g->cl_off.p, st));
    }
    CHECK_RC(publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.passes, st));
    g->clusters_rows = N; g->clusters_n = n_cl; g->clusters_members = n_mem;
    g->clusters_valid = true;
    *n_clusters = n_cl;
    *n_members = n_mem;
    return 0;
    API_END
}
extern "C" int32_t revo_gallery_clusters_read(revo_gallery* g, int64_t* labels, int64_t* offsets, int64_t* members,
                                              int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "gallery_clusters_read: null handle");
    REVO_REQUIRE(g->clusters_valid, "gallery_clusters_read: no result (call revo_gallery_clusters again after the rows change)");
    if (!labels && !offsets && !members) return 0;
    REVO_ON_DEVICE(g->device);
    const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (labels && g->clusters_rows > 0) REVO_HIP_CHECK(hipMemcpy(labels, g->cl_labels.p, (size_t)g->clusters_rows * 8, kind));
    if (offsets) REVO_HIP_CHECK(hipMemcpy(offsets, g->cl_off.p, (size_t)(g->clusters_n + 1) * 8, kind));
    if (members && g->clusters_members > 0)
        REVO_HIP_CHECK(hipMemcpy(members, g->cl_members.p, (size_t)g->clusters_members * 8, kind));
    return 0;
    API_END
}

// ---- range search (include/revo.h revo_search_range; range.hip)
static int search_range(revo_gallery* g, const float* queries, int Q, float thr, long index_offset, const uint32_t* allow,
                        hipStream_t st, int64_t* n_results) {
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    // sort keys (query << (32 + b)) | (score << b) | row in 64 bits: at most 2^(32 - b) queries per chunk
    const int b = row_index_bits(N);
    int QC = Q < RANGE_CHUNK ? Q : RANGE_CHUNK;
    if ((long)QC > (1l << (32 - b))) QC = (int)(1l << (32 - b));
    int qbits = 0;
    while ((1l << qbits) < QC) ++qbits;
    // (the two-phase protocol's state refers to the handle's query rows, which this search overwrites)
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
    CHECK_RC(search_grow_queries(g, QC > 0 ? QC : 1, st));
    REVO_REQUIRE(g->xw.ctr, "search_range: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    // offsets: off[1 + q] collects query q's count, then the prefix sums make them the CSR offsets (off[0] = 0)
    CHECK_RC(g->range_off.grow((size_t)(Q + 1) * 8, st));
    REVO_HIP_CHECK(hipMemsetAsync(g->range_off.p, 0, (size_t)(Q + 1) * 8, st));
    unsigned long long* off = g->range_off.p;
    CandidateWs ws{g->pbuf, g->range_cap};
    long total = 0;
    unsigned long long cand_total = 0;
    int max_passes = 0;
    if (N > 0 && Q > 0) {
        const long cap0 = (long)QC * RANGE_WS_PER_QUERY;
        CHECK_RC(ws.carve(g->range_cap > cap0 ? g->range_cap : cap0, st));
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
            CHECK_RC(g->range_idx.grow_keep(need * 8, (size_t)total * 8, st));
            CHECK_RC(g->range_score.grow_keep(need * 4, (size_t)total * 4, st));
            CHECK_RC(launch_range_emit(ws.sk, ws.sv, n_kept, b, index_offset, g->range_idx.p + total, g->range_score.p + total, st));
            total += n_kept;
        }
        CHECK_RC(launch_inclusive_sums_u64(off + 1, Q, st));
    }
    CHECK_RC(publish_candidate_stats(g->xw.ctr, cand_total, max_passes, st));
    g->range_n = total;
    g->range_q = Q;
    g->range_valid = true;
    *n_results = total;
    return 0;
}
extern "C" int32_t revo_search_range(revo_gallery* g, const float* queries, int32_t n_queries, float threshold,
                                     int64_t index_offset, int64_t* n_results, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && n_results && (queries || n_queries == 0), "search_range: null argument");
    REVO_REQUIRE(n_queries >= 0, "search_range: negative query count");
    REVO_REQUIRE(!std::isnan(threshold), "search_range: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "search_range: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    g->range_valid = false;
    return search_range(g, queries, n_queries, threshold, index_offset, allow, (hipStream_t)stream, n_results);
    API_END
}
extern "C" int32_t revo_search_range_read(revo_gallery* g, int64_t* offsets, int64_t start, int64_t n, int64_t* indices,
                                          float* scores, int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(g, "search_range_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "search_range_read: negative start or count");
    REVO_REQUIRE((indices && scores) || n == 0, "search_range_read: null argument");
    REVO_REQUIRE(g->range_valid, "search_range_read: no result (call revo_search_range again after the rows change)");
    REVO_REQUIRE(start + n <= g->range_n,
                 "search_range_read: range past the result's " + std::to_string(g->range_n) + " entries");
    REVO_ON_DEVICE(g->device);
    const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (offsets) REVO_HIP_CHECK(hipMemcpy(offsets, g->range_off.p, (size_t)(g->range_q + 1) * 8, kind));
    if (n == 0) return 0;
    REVO_HIP_CHECK(hipMemcpy(indices, g->range_idx.p + start, (size_t)n * 8, kind));
    REVO_HIP_CHECK(hipMemcpy(scores, g->range_score.p + start, (size_t)n * 4, kind));
    return 0;
    API_END
}

// ---- search by examples (include/revo.h revo_search_recommend; recommend.hip)
static int search_recommend(revo_gallery* g, const float* examples, int P, int Nn, int k, int has_thr, float thr, long index_offset,
                            float* scores, long long* indices, int* counts, const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    const int E = P + Nn;
    // (the two-phase protocol's state refers to the handle's query rows, which this search overwrites)
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
    CHECK_RC(search_grow_queries(g, E, st));
    REVO_REQUIRE(g->xw.ctr, "search_recommend: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    if (N == 0) {
        CHECK_RC(launch_topk_fill_empty(scores, indices, counts, 1, k, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    // the sample: the rows revo_search_topk_large's sample pass covers (none in a small gallery: tau = -inf or the threshold)
    const long n_s = large_sample_rows(E, N, k);
    // candidates are rows (32-bit indices in the key array), at most N: sized once; counter [2] = allowed rows the pass met
    long cap = 0;
    CandidateWs ws{g->pbuf, cap};
    float *tau = nullptr, *lb = nullptr;
    CHECK_RC(ws.carve(N, st, [&](Layout& l) { tau = l.take<float>(1); lb = l.take<float>(n_s > 0 ? n_s : 1); }));
    uint32_t* cand = (uint32_t*)ws.cand;
    // (the pairs' and the range search's layouts of this buffer are carved again by their next call)
    { ProfScope ps("search_prep", st);
      CHECK_RC(launch_l2norm_rows(examples, D, g->qf.p, D, g->qb.p, D, E, D, st, 1, g->qstat.p)); }
    RecommendPassArgs pa{};
    pa.Qb = g->qb.p; pa.ldq = D; pa.Gb = g->gb.p; pa.ldg = D; pa.P = P; pa.Nn = Nn; pa.D = D;
    pa.qstat = g->qstat.p; pa.gstat = g->gstat.p; pa.allow = allow;
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        { ProfScope ps("recommend_sample", st);
          if (n_s > 0) { pa.N = n_s; pa.lb_out = lb; CHECK_RC(launch_recommend_pass(pa, 1, st)); }
          CHECK_RC(launch_recommend_level(lb, (int)n_s, k, has_thr, thr, tau, st)); }
        ProfScope ps("recommend_pass", st);
        pa.N = N; pa.lb_out = nullptr; pa.tau = tau; pa.cnt = ws.cnt; pa.rows = cand; pa.cap = N;
        return launch_recommend_pass(pa, 0, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)N, "search_recommend: more candidates than rows");
        return 0;
    }, "search_recommend: the candidate count changed between two passes"));
    const int b = row_index_bits(N);
    { ProfScope ps("recommend_rescore", st);
      CHECK_RC(launch_recommend_rescore(cand, (long)ws.n_cand, g->qf.p, D, P, Nn, g->gf.p, D, D, has_thr, thr, b, ws.cnt + 1,
                                        ws.kept_k, ws.kept_v, st)); }
    CHECK_RC(ws.sort_kept("recommend_sort", 32 + b, st));
    CHECK_RC(launch_recommend_emit(ws.sk, ws.sv, (long)ws.n_kept, k, b, index_offset, scores, indices, counts, st));
    return publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.h[2] > 0 ? 1 : 0, st);   // (no allowed row: no candidate pass counted)
}
extern "C" int32_t revo_search_recommend(revo_gallery* g, const float* examples, int32_t n_positive, int32_t n_negative, int32_t k,
                                         int32_t has_threshold, float threshold, int64_t index_offset, float* scores,
                                         int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && examples && scores && indices && counts, "search_recommend: null argument");
    REVO_REQUIRE(n_positive >= 1, "search_recommend: needs at least one positive example");
    REVO_REQUIRE(n_negative >= 0, "search_recommend: negative count of negative examples");
    REVO_REQUIRE((int64_t)n_positive + n_negative <= revo::RECOMMEND_MAX_EXAMPLES,
                 "search_recommend: at most 128 examples (n_positive + n_negative)");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_recommend: k must be in [1, 1024]");
    REVO_REQUIRE(!has_threshold || !std::isnan(threshold), "search_recommend: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "search_recommend: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_recommend(g, examples, n_positive, n_negative, k, has_threshold, threshold, index_offset, scores,
                            (long long*)indices, counts, allow, (hipStream_t)stream);
    API_END
}

// ---- discovery and context search (include/revo.h revo_search_discover; discover.hip)
static int search_discover(revo_gallery* g, const float* target, const float* positives, const float* negatives, int n_pairs, int k,
                           int has_thr, float thr, long index_offset, float* scores, long long* indices, int* counts,
                           const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    const int has_target = target ? 1 : 0;
    const int rows = discover_tile_rows(n_pairs, has_target), half = rows / 2;
    // (the two-phase protocol's state refers to the handle's query rows, which this search overwrites)
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
    CHECK_RC(search_grow_queries(g, rows, st));
    REVO_REQUIRE(g->xw.ctr, "search_discover: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    if (N == 0) {
        CHECK_RC(launch_topk_fill_empty(scores, indices, counts, 1, k, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    const long n_s = large_sample_rows(2 * n_pairs + has_target, N, k);
    // candidates are rows (32-bit indices in the key array), at most N: sized once; counter [2] = allowed rows the pass met
    long cap = 0;
    CandidateWs ws{g->pbuf, cap};
    float *tau = nullptr, *lb = nullptr;
    CHECK_RC(ws.carve(N, st, [&](Layout& l) { tau = l.take<float>(1); lb = l.take<float>(n_s > 0 ? n_s : 1); }));
    uint32_t* cand = (uint32_t*)ws.cand;
    // (the pairs' and the range search's layouts of this buffer are carved again by their next call)
    { ProfScope ps("search_prep", st);
      // the example tile: zero rows, then positive i -> row i, negative i -> row half + i, the target -> row half - 1
      REVO_HIP_CHECK(hipMemsetAsync(g->qb.p, 0, (size_t)rows * D * sizeof(bf16_t), st));
      CHECK_RC(launch_l2norm_rows(positives, D, g->qf.p, D, g->qb.p, D, n_pairs, D, st, 1, g->qstat.p));
      CHECK_RC(launch_l2norm_rows(negatives, D, g->qf.p + (size_t)half * D, D, g->qb.p + (size_t)half * D, D, n_pairs, D, st, 1,
                                  g->qstat.p + 2 * half));
      if (has_target)
          CHECK_RC(launch_l2norm_rows(target, D, g->qf.p + (size_t)(half - 1) * D, D, g->qb.p + (size_t)(half - 1) * D, D, 1, D, st,
                                      1, g->qstat.p + 2 * (half - 1))); }
    DiscoverPassArgs pa{};
    pa.Qb = g->qb.p; pa.ldq = D; pa.Gb = g->gb.p; pa.ldg = D; pa.n_pairs = n_pairs; pa.has_target = has_target; pa.D = D;
    pa.qstat = g->qstat.p; pa.gstat = g->gstat.p; pa.allow = allow;
    CHECK_RC(ws.join_until_it_fits(st, [&]() -> int {
        { ProfScope ps("discover_sample", st);
          if (n_s > 0) { pa.N = n_s; pa.lb_out = lb; CHECK_RC(launch_discover_pass(pa, 1, st)); }
          CHECK_RC(launch_recommend_level(lb, (int)n_s, k, has_thr, thr, tau, st)); }
        ProfScope ps("discover_pass", st);
        pa.N = N; pa.lb_out = nullptr; pa.tau = tau; pa.cnt = ws.cnt; pa.rows = cand; pa.cap = N;
        return launch_discover_pass(pa, 0, st);
    }, [&](unsigned long long n_cand) -> int {
        REVO_REQUIRE(n_cand <= (unsigned long long)N, "search_discover: more candidates than rows");
        return 0;
    }, "search_discover: the candidate count changed between two passes"));
    const int b = row_index_bits(N);
    { ProfScope ps("discover_rescore", st);
      CHECK_RC(launch_discover_rescore(cand, (long)ws.n_cand, g->qf.p, D, half, n_pairs, has_target, g->gf.p, D, D, has_thr, thr, b,
                                       ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    CHECK_RC(ws.sort_kept("discover_sort", 32 + b, st));
    CHECK_RC(launch_recommend_emit(ws.sk, ws.sv, (long)ws.n_kept, k, b, index_offset, scores, indices, counts, st));
    return publish_candidate_stats(g->xw.ctr, ws.n_cand, ws.h[2] > 0 ? 1 : 0, st);   // (no allowed row: no candidate pass counted)
}
extern "C" int32_t revo_search_discover(revo_gallery* g, const float* target, const float* positives, const float* negatives,
                                        int32_t n_pairs, int32_t k, int32_t has_threshold, float threshold, int64_t index_offset,
                                        float* scores, int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts, "search_discover: null argument");
    if (target) REVO_REQUIRE(n_pairs >= 0 && n_pairs <= revo::DISCOVER_MAX_PAIRS - 1,
                             "search_discover: n_pairs must be in [0, 63] with a target");
    else REVO_REQUIRE(n_pairs >= 1 && n_pairs <= revo::DISCOVER_MAX_PAIRS,
                      "search_discover: n_pairs must be in [1, 64] without a target (context search)");
    REVO_REQUIRE(n_pairs == 0 || (positives && negatives), "search_discover: null positives or negatives");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_discover: k must be in [1, 1024]");
    REVO_REQUIRE(!has_threshold || !std::isnan(threshold), "search_discover: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "search_discover: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_discover(g, target, positives, negatives, n_pairs, k, has_threshold, threshold, index_offset, scores,
                           (long long*)indices, counts, allow, (hipStream_t)stream);
    API_END
}

// ---- multi-vector search (include/revo.h revo_search_maxsim; maxsim.hip)
// the CSR of the handle's group ids, built for the gallery's current rows (N >= 1)
static int maxsim_build_index(revo_gallery* g, hipStream_t st) {
    using namespace revo;
    const long N = g->size;
    g->csr_rows = -1;
    CHECK_RC(carve_buffer(g->csr, st, [&](Layout& l) {
        g->csr_gid = l.take<int32_t>(N); g->csr_off = l.take<uint32_t>(N + 1); g->csr_row = l.take<uint32_t>(N);
        g->csr_pos = l.take<uint32_t>(N);
    }));
    // (scratch of the build: the candidate pipeline's buffer, carved again by the next search that uses it)
    uint64_t *keys = nullptr, *keys_alt = nullptr; float *vals = nullptr, *vals_alt = nullptr; uint32_t* hist = nullptr;
    unsigned long long *flags = nullptr, *meta = nullptr;
    CHECK_RC(carve_buffer(g->pbuf, st, [&](Layout& l) {
        keys = l.take<uint64_t>(N); keys_alt = l.take<uint64_t>(N); vals = l.take<float>(N); vals_alt = l.take<float>(N);
        hist = l.take<uint32_t>(256l * SORT_MAX_BLOCKS); flags = l.take<unsigned long long>(N); meta = l.take<unsigned long long>(2);
    }));
    ProfScope ps("maxsim_index", st);
    CHECK_RC(launch_maxsim_index(g->groups.p, N, keys, keys_alt, vals, vals_alt, hist, flags, meta, g->csr_gid, g->csr_off,
                                 g->csr_row, g->csr_pos, st));
    unsigned long long h[2] = {0, 0};
    REVO_HIP_CHECK(hipMemcpyAsync(h, meta, sizeof(h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    REVO_REQUIRE(h[0] <= h[1] && h[1] <= (unsigned long long)N, "search_maxsim: inconsistent group index");
    g->csr_groups = (long)h[0]; g->csr_grouped = (long)h[1]; g->csr_rows = N;
    return 0;
}
static int search_maxsim(revo_gallery* g, const float* queries, int n, int k, int has_thr, float thr, long index_offset,
                         float* scores, int32_t* group_ids, int32_t* counts, float* part_scores, long long* part_rows,
                         const uint32_t* allow, hipStream_t st) {
    using namespace revo;
    const long N = g->size;
    const int D = g->D;
    const int n_pad = (n + 3) / 4 * 4;
    // (the two-phase protocol's state refers to the handle's query rows, which this search overwrites)
    g->cand = nullptr; g->cand_Q = 0; g->nsegs = 0; g->prelist = nullptr; g->cand_estimated = false;
    CHECK_RC(search_grow_queries(g, n, st));
    REVO_REQUIRE(g->xw.ctr, "search_maxsim: no counter workspace");
    REVO_HIP_CHECK(hipMemsetAsync(g->xw.ctr, 0, CTR_SLOTS * sizeof(int), st));
    MaxsimGroupArgs ga{};
    ga.n = n; ga.n_pad = n_pad; ga.lanes = maxsim_group_lanes(n_pad); ga.allow = allow; ga.D = D;
    if (N > 0 && g->csr_rows != N) CHECK_RC(maxsim_build_index(g, st));
    const long G = N > 0 ? g->csr_groups : 0, n_grouped = N > 0 ? g->csr_grouped : 0;
    if (G == 0) {
        // an empty gallery, or no row with a group: all padding
        CHECK_RC(launch_maxsim_emit(ga, nullptr, nullptr, 0, k, n, index_offset, scores, group_ids, counts, part_scores, part_rows, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    REVO_REQUIRE(G < (1l << 31), "search_maxsim: too many groups");
    const size_t s_bytes = (size_t)N * n_pad * sizeof(float);
    if (g->maxsim_s.bytes < s_bytes && g->maxsim_s.grow(s_bytes, st) != 0) {
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
    ga.S = g->maxsim_s.p; ga.gid = g->csr_gid; ga.off = g->csr_off; ga.rows = g->csr_row; ga.G = G;
    ga.qstat = g->qstat.p; ga.gstat = g->gstat.p;
    { ProfScope ps("maxsim_pass", st);
      MaxsimPassArgs pa{};
      pa.Qb = g->qb.p; pa.ldq = D; pa.Gb = g->gb.p; pa.ldg = D; pa.n = n; pa.n_pad = n_pad; pa.N = N; pa.D = D; pa.allow = allow;
      pa.S = g->maxsim_s.p;
      CHECK_RC(launch_maxsim_pass(pa, st)); }
    { ProfScope ps("maxsim_bounds", st);
      CHECK_RC(launch_maxsim_bounds(ga, lb, ub, acnt, ws.cnt, st)); }
    { ProfScope ps("maxsim_level", st);
      CHECK_RC(launch_recommend_level(lb, (int)G, k, has_thr, thr, tau, st));
      CHECK_RC(launch_maxsim_select(ga, n_grouped, g->csr_pos, ub, acnt, tau, ws.cnt, crows, cgroups, st)); }
    // counters: [0] candidate rows, [1] kept groups, [2] groups with an allowed row, [3] candidate groups
    REVO_HIP_CHECK(hipMemcpyAsync(ws.h, ws.cnt, sizeof(ws.h), hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    REVO_REQUIRE(ws.h[0] <= (unsigned long long)n_grouped && ws.h[3] <= (unsigned long long)G, "search_maxsim: more candidates than rows");
    { ProfScope ps("maxsim_rescore", st);
      CHECK_RC(launch_maxsim_rescore(crows, (long)ws.h[0], g->qf.p, D, n, n_pad, g->gf.p, D, D, g->maxsim_s.p, st)); }
    { ProfScope ps("maxsim_reduce", st);
      CHECK_RC(launch_maxsim_reduce(ga, cgroups, (long)ws.h[3], has_thr, thr, ws.cnt + 1, ws.kept_k, ws.kept_v, st)); }
    ws.n_cand = ws.h[3];
    CHECK_RC(ws.sort_kept("maxsim_sort", 64, st));   // (the score sits above all 32 bits of the group position)
    { ProfScope ps("maxsim_emit", st);
      CHECK_RC(launch_maxsim_emit(ga, ws.sk, ws.sv, (long)ws.n_kept, k, n, index_offset, scores, group_ids, counts, part_scores,
                                  part_rows, st)); }
    return publish_candidate_stats(g->xw.ctr, ws.h[0], ws.h[2] > 0 ? 1 : 0, st);
}
extern "C" int32_t revo_search_maxsim(revo_gallery* g, const float* queries, int32_t n_vectors, int32_t k, int32_t has_threshold,
                                      float threshold, int64_t index_offset, float* scores, int32_t* group_ids, int32_t* counts,
                                      float* part_scores, int64_t* part_rows, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g, "search_maxsim: null handle");
    REVO_REQUIRE(queries, "search_maxsim: null queries");
    REVO_REQUIRE(scores, "search_maxsim: null scores");
    REVO_REQUIRE(group_ids, "search_maxsim: null group_ids");
    REVO_REQUIRE(counts, "search_maxsim: null counts");
    REVO_REQUIRE(n_vectors >= 1 && n_vectors <= revo::MAXSIM_MAX_VECTORS, "search_maxsim: n_vectors must be in [1, 64]");
    REVO_REQUIRE(k >= 1 && k <= revo::LARGE_K_MAX, "search_maxsim: k must be in [1, 1024]");
    REVO_REQUIRE(!has_threshold || !std::isnan(threshold), "search_maxsim: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "search_maxsim: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    REVO_REQUIRE(g->groups_rows >= 0, "search_maxsim: no group ids (revo_search_set_groups)");
    REVO_REQUIRE(g->groups_rows == g->size,
                 "search_maxsim: the group ids were set for " + std::to_string(g->groups_rows) + " rows but the gallery holds " +
                     std::to_string(g->size) + " (set them again after appending)");
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_maxsim(g, queries, n_vectors, k, has_threshold, threshold, index_offset, scores, group_ids, counts, part_scores,
                         (long long*)part_rows, allow, (hipStream_t)stream);
    API_END
}

// ---- diverse search (include/revo.h revo_search_mmr; mmr.hip)
constexpr size_t MMR_GRAM_BYTES = 256ul << 20;   // the similarity matrices of one chunk of queries
static int search_mmr(revo_gallery* g, const float* queries, int Q, int k, int C, float diversity, int has_thr, float thr,
                      long index_offset, float* scores, float* mmr_values, long long* indices, int* counts, const uint32_t* allow,
                      hipStream_t st) {
    using namespace revo;
    const size_t per_query = (size_t)C * C * sizeof(float);
    const int QC = (int)std::min<size_t>((size_t)Q, std::max<size_t>(1, MMR_GRAM_BYTES / per_query));
    float *rel = nullptr, *gram = nullptr; long long* cand = nullptr; int* n_cand = nullptr;
    // (the pairs', the range search's and the recommend search's layouts of this buffer are carved again by their next call)
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
        sa.idx = indices + (size_t)c0 * k; sa.out_counts = counts + c0;
        { ProfScope ps("mmr_select", st);
          CHECK_RC(launch_mmr_select(sa, Qc, st)); }
    }
    return 0;
}
extern "C" int32_t revo_search_mmr(revo_gallery* g, const float* queries, int32_t n_queries, int32_t k, int32_t candidates,
                                   float diversity, int32_t has_threshold, float threshold, int64_t index_offset, float* scores,
                                   float* mmr_values, int64_t* indices, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && scores && indices && counts && (queries || n_queries == 0), "search_mmr: null argument");
    REVO_REQUIRE(n_queries >= 0, "search_mmr: negative query count");
    REVO_REQUIRE(candidates >= 1 && candidates <= revo::LARGE_K_MAX, "search_mmr: candidates must be in [1, 1024]");
    REVO_REQUIRE(k >= 1 && k <= candidates, "search_mmr: k must be in [1, candidates]");
    REVO_REQUIRE(diversity >= 0.f && diversity <= 1.f, "search_mmr: diversity must be in [0, 1] (and not NaN)");
    REVO_REQUIRE(!has_threshold || !std::isnan(threshold), "search_mmr: threshold is NaN");
    REVO_REQUIRE(g->keep_f32, "search_mmr: the gallery was created without the fp32 master copy (keep_f32 = 0)");
    if (n_queries == 0) return 0;
    const uint32_t* allow; CHECK_RC(search_filter(g, &allow));
    REVO_ON_DEVICE(g->device);
    return search_mmr(g, queries, n_queries, k, candidates, diversity, has_threshold, threshold, index_offset, scores, mmr_values,
                      (long long*)indices, counts, allow, (hipStream_t)stream);
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
    REVO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    REVO_HIP_CHECK(hipMemcpy(c, g->xw.ctr, sizeof(c), hipMemcpyDeviceToHost));
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
