// The gallery handle and the host helpers shared by gallery.hip (the handle and its rows), search.hip (the certified top-k
// pipeline) and candidate_search.hip (the candidate-pipeline searches).  Not part of the C ABI.
#pragma once
#include <cmath>
#include <string>

#include "../../include/revo.h"
#include "api_internal.h"
#include "kernels.h"
#pragma GCC visibility push(hidden)   // nothing declared here is exported by librevo.so
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

// ---- what a feature keeps in the handle between calls (buffers: grown on demand, never shrunk, freed with the handle)
// The two-phase search (revo_search_candidates / _finish / _exact): the candidates of the last scan (inside `part`), consumed
// by the finish step.  After a scan with an admission margin its segments can answer uncertified queries (CertArgs,
// kernels.h); `estimated`: the scan started from estimated admission scores (CertArgs::estimated).
struct TwoPhaseState {
    const uint64_t* cand = nullptr; long stride = 0; int Q = 0, ksel = 0;
    revo::SegSrc segs[2] = {}; int nsegs = 0; const uint64_t* prelist = nullptr;
    bool estimated = false;
};
// revo_gallery_pairs: the candidate keys its workspace (in pbuf) holds, and the last result ([n][2] row pairs, [n] scores),
// valid until the rows change
struct PairsResult {
    long cap = 0;
    DeviceBuffer<long long> idx; DeviceBuffer<float> score;
    int64_t n = 0; bool valid = false;
};
// revo_search_range: the candidate keys its workspace (in pbuf) holds, and the last result ([n] indices and scores, [q + 1]
// offsets), valid until the rows change
struct RangeResult {
    long cap = 0;
    DeviceBuffer<long long> idx; DeviceBuffer<float> score; DeviceBuffer<unsigned long long> off;
    int64_t n = 0, q = 0; bool valid = false;
};
// revo_gallery_clusters: its workspace (counters | union-find and error word | sizes | member keys and the sort's buffers), and
// the last result ([rows] labels, [n + 1] offsets, [n_members] rows), valid until the rows change
struct ClustersResult {
    DeviceBuffer<> ws;
    DeviceBuffer<long long> labels, off, members;
    int64_t rows = 0, n = 0, n_members = 0; bool valid = false;
};
// revo_gallery_knn: the last result ([n][k] scores and indices, [n] counts), valid until the rows change, and the score buffer of
// its exhaustive fallback (allocated when a row first needs it)
struct KnnResult {
    DeviceBuffer<long long> idx; DeviceBuffer<float> score; DeviceBuffer<int> counts;
    DeviceBuffer<float> fb;
    int64_t n = 0; int k = 0; bool valid = false;
};
// revo_gallery_kmeans: the last result ([n] labels and scores, [C] sizes, the centroids' fp32 rows in cf[cur]), valid until the
// rows change; the centroids' two generations (fp32 rows and bf16 copies of ceil(C / 256) * 256 rows, an update writes the other
// one) and the call's workspace (ws: what must survive a regrow of the candidate workspace in pbuf)
struct KmeansResult {
    DeviceBuffer<int> labels; DeviceBuffer<float> score; DeviceBuffer<unsigned long long> sizes;
    DeviceBuffer<float> cf[2]; DeviceBuffer<bf16_t> cb[2]; int cur = 0;
    DeviceBuffer<> ws;
    long cap = 0;
    int64_t n = 0, C = 0; bool valid = false;
};
// revo_search_maxsim: the CSR of the group ids (gid | off | row | pos in csr; revo::launch_maxsim_index), built at the first
// call for `rows` rows (-1: none; dropped by revo_search_set_groups, an append, a clear and a remove that moves rows), and the
// score workspace S [N][n_pad]
struct MaxsimIndex {
    DeviceBuffer<> csr; int64_t rows = -1; long groups = 0, grouped = 0;
    int32_t* gid = nullptr; uint32_t *off = nullptr, *row = nullptr, *pos = nullptr;
    DeviceBuffer<float> s;
};

struct __attribute__((visibility("default"))) revo_gallery {   // (the C ABI names the type: exported as it always was)
    int D = 0, device = 0, keep_f32 = 1;
    int64_t capacity = 0, size = 0;
    DeviceBuffer<bf16_t> gb;   // [capacity][D] normalised rows, scan copy
    DeviceBuffer<float> gf;    // [capacity][D] normalised rows, fp32 master (re-score + persistence)
    // per-call workspace, grown on demand: the per-query arrays (sized for q_cap queries; qstat, marg and dropflag
    // below), the scan's workspace (part) and the staging rows of an append from the host
    DeviceBuffer<float> qf; DeviceBuffer<bf16_t> qb; DeviceBuffer<uint32_t> tau0; int q_cap = 0;
    DeviceBuffer<> part;
    DeviceBuffer<float> stage;
    DeviceBuffer<float> marg; DeviceBuffer<int> dropflag;
    int64_t total_rows = 0;        // revo_search_set_total_rows: this handle is one shard of a gallery of that many rows (0: the whole)
    // exactness certificate (kernels.h): per-query rounding norms of the last search's queries, running maxima over the
    // gallery's rows, the fallback workspace (xbuf, sized with q_cap; its layout is xw) and the handle's mode
    DeviceBuffer<float> qstat; DeviceBuffer<uint32_t> gstat;
    bool gstat_reset = false;      // revo_gallery_clear: the next gallery_write_rows zeroes gstat on its stream, ahead of its kernel
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
    // the candidate pipeline's workspace (CandidateWs, candidate_search.hip): every search that uses it carves its own layout
    DeviceBuffer<> pbuf;
    // revo_search_fusion's workspace: the lists' scores | rows | counts | the normalised query rows (for list_scores)
    DeviceBuffer<> fbuf;
    // revo_gallery_remove: per-chunk counts | first removed rows | the copy of a host bitmap; revo_gallery_update: the row map
    DeviceBuffer<> edit;
    // revo_gallery_append_unique: edges (first_old | bit matrix) | representatives | rows | scores | kept count | the
    // remove-bitmap of the dropped rows and its chunk words; allocated at the first call, grown with the batch size
    DeviceBuffer<> dedup;
    TwoPhaseState two;
    PairsResult pairs;
    RangeResult range;
    ClustersResult clusters;
    KnnResult knn;
    KmeansResult kmeans;
    MaxsimIndex maxsim;
    // a search overwrites the handle's query rows: the two-phase candidates that refer to them go
    void drop_two_phase() { two.cand = nullptr; two.Q = 0; two.nsegs = 0; two.prelist = nullptr; two.estimated = false; }
    // rows were added or all removed: the results held in the handle go (and, the caller's part, the group index)
    void drop_results() { pairs.valid = false; range.valid = false; clusters.valid = false; knn.valid = false; kmeans.valid = false; }
    // rows left or changed in place: the results and the two-phase candidate state go
    void rows_changed() { drop_results(); two.ksel = 0; drop_two_phase(); }
    revo::CertArgs cert_args(float* cert_out) const {
        revo::CertArgs c{};
        c.qstat = qstat.p; c.gstat = gstat.p; c.mode = mode; c.ws = xw; c.Qb = qb.p; c.ldq = D; c.cert_out = cert_out;
        c.nsegs = two.nsegs; c.segs[0] = two.segs[0]; c.segs[1] = two.segs[1]; c.seg_ksel = two.ksel; c.prelist = two.prelist;
        c.tau_base = tau0.p; c.marg = marg.p; c.dropflag = dropflag.p; c.estimated = two.estimated ? 1 : 0;
        return c;
    }
};
constexpr long SEARCH_SMALL_ROWS = 16384;     // below this the 128 x 128 scan with LDS lists takes the gallery
constexpr long SEARCH_WIDE_ROWS = 1l << 22;   // from here on the unsharded search keeps 64 candidates per query for every k

// ---- argument checks and the copy-out that the entry points share (`who`: the entry point's name in the message)
inline int require_f32_rows(const revo_gallery* g, const char* who) {
    REVO_REQUIRE(g->keep_f32, std::string(who) + ": the gallery was created without the fp32 master copy (keep_f32 = 0)");
    return 0;
}
inline int require_threshold(int has_thr, float thr, const char* who) {
    REVO_REQUIRE(!has_thr || !std::isnan(thr), std::string(who) + ": threshold is NaN");
    return 0;
}
// `count` elements of a result held in the handle, to the caller's host or device array (a _read entry point; synchronous: a
// device-to-device hipMemcpy may return before the default stream has run it, and the caller's stream is not ordered behind
// that one, so the copy is waited for here)
template <class T> int copy_out(void* dst, const T* src, size_t count, int dst_on_device) {
    REVO_HIP_CHECK(hipMemcpy(dst, src, count * sizeof(T), dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (dst_on_device) REVO_HIP_CHECK(hipStreamSynchronize(nullptr));
    return 0;
}

// ---- host helpers that cross the files (`allow`: what search_filter gave; the device of the handle is current)
// gallery.hip: the allow-bitmap the next search of this handle runs with (null: none)
int search_filter(const revo_gallery* g, const uint32_t** out);
// gallery.hip: the row writer of append and update (row i of vecs -> row row0 + i, or map[i]), and the in-place compaction of
// the rows [R0, R0 + N) behind revo_gallery_remove
int gallery_write_rows(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize, int32_t src_on_device, int64_t row0,
                       const long long* map, const char* prof, hipStream_t st);
int gallery_compact_rows(revo_gallery* g, const uint32_t* bits, long R0, long N, long chunk, uint32_t* cnt, uint32_t* first,
                         const char* prof, hipStream_t st, long* kept_out);
// search.hip: the handle's per-query arrays, grown to hold Q queries; the rows of the large-k sample; revo_search_topk_large
// behind its argument checks (search_prepass_rows and search_topk stay inside search.hip: nothing else calls them)
int search_grow_queries(revo_gallery* g, int Q, hipStream_t st);
long large_sample_rows(int Q, long N, int k);
int search_topk_large(revo_gallery* g, const float* queries, int Q, int k, int has_thr, float thr, long index_offset,
                      float* scores, long long* indices, int* counts, const uint32_t* allow, hipStream_t st);
#pragma GCC visibility pop
