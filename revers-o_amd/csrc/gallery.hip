// C ABI of the gallery handle (include/revo.h): its rows (create, append, read, clear, remove, update), its filter, its group
// ids and the shard's total row count.  The handle itself is gallery_internal.h; the searches are search.hip and
// candidate_search.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "gallery_internal.h"

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
int search_filter(const revo_gallery* g, const uint32_t** out) {
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
    g->maxsim.rows = -1;
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
    // The row maxima of the certificate start over with the rows -- on the stream of the next write, ahead of its kernel
    // (gallery_write_rows): a reset issued from here would run on no stream of the caller's and could overtake an append that
    // is still pending, or land behind the next one.  No device memory is touched.
    g->gstat_reset = true;
    g->size = 0;
    g->drop_results(); g->maxsim.rows = -1;
    return 0;
}

// Rows come in from `vecs` (host rows: staged in chunks of 64 MB) through one kernel: fp32 master row, bf16 scan row, and the
// row's share of the certificate's maxima (max ||g||, max ||bf16(g) - g||; with normalize = 0 the rows are stored as given,
// whatever their length).  Row i goes to row row0 + i or, with a map (device [n]), to row map[i]: the same bits either way.
int gallery_write_rows(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize, int32_t src_on_device, int64_t row0,
                       const long long* map, const char* prof, hipStream_t st) {
    const int D = g->D;
    const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / (D * 4));
    if (g->gstat_reset && n > 0) {                        // the first rows after revo_gallery_clear
        REVO_HIP_CHECK(hipMemsetAsync(g->gstat.p, 0, 8, st));
        g->gstat_reset = false;
    }
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        const float* src = vecs + done * D;
        if (!src_on_device) {
            const size_t need = (size_t)m * D * 4;
            CHECK_RC(g->stage.grow(need, st));
            REVO_HIP_CHECK(hipMemcpyAsync(g->stage.p, src, need, hipMemcpyHostToDevice, st));
            src = g->stage.p;
        }
        const int64_t first = map ? 0 : row0 + done;
        ProfScope ps(prof, st);
        CHECK_RC(revo::launch_l2norm_rows(src, D, g->keep_f32 ? g->gf.p + first * D : nullptr, D, g->gb.p + first * D, D, m, D, st,
                                          normalize ? 1 : 0, nullptr, g->gstat.p, nullptr, 0, nullptr, 0, map ? map + done : nullptr));
        if (!src_on_device) REVO_HIP_CHECK(hipStreamSynchronize(st));   // staging buffer is reused
    }
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
    g->drop_results(); g->maxsim.rows = -1;
    CHECK_RC(gallery_write_rows(g, vecs, n, normalize, src_on_device, g->size, nullptr, "gallery_append", st));
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
    return copy_out(dst, g->gf.p + start * g->D, (size_t)n * g->D, dst_on_device);
    API_END
}

// the certificate's maxima as the handle holds them (gstat: max ||g||, max ||bf16(g) - g|| over every row written since the
// gallery was last empty), after the work enqueued on `stream`
extern "C" int32_t revo_op_gallery_cert_stats(revo_gallery* g, float* out, void* stream) {
    API_BEGIN
    REVO_REQUIRE(g && out, "op_gallery_cert_stats: null argument");
    REVO_ON_DEVICE(g->device);
    if (g->gstat_reset) out[0] = out[1] = 0.f;            // cleared, nothing written since: the reset is still to be enqueued
    else REVO_HIP_CHECK(hipMemcpyAsync(out, g->gstat.p, 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    REVO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
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
// The rows [R0, R0 + N) of the gallery (R0 a multiple of 32) compacted by a device bitmap over them -- bit p: row R0 + p leaves
// -- in chunks of `chunk` rows; cnt / first: [chunks] device words.  *kept_out = the rows that stay (rows R0 .. R0 + kept - 1
// afterwards).  Enqueued on `st` behind one synchronisation (the host reads the chunks' counts).
int gallery_compact_rows(revo_gallery* g, const uint32_t* bits, long R0, long N, long chunk, uint32_t* cnt, uint32_t* first,
                         const char* prof, hipStream_t st, long* kept_out) {
    const int D = g->D;
    const long nchunks = (N + chunk - 1) / chunk;
    std::vector<uint32_t> h_cnt(nchunks), h_first(nchunks);
    { ProfScope ps(prof, st);
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
        ProfScope ps(prof, st);
        for (long c = 0; c < nchunks; ++c) {
            const long row0 = c * chunk, len = std::min(chunk, N - row0), kept = (long)h_cnt[c];
            REVO_REQUIRE(kept <= len && base <= row0, std::string(prof) + ": internal: inconsistent chunk counts");
            // rows in front of the first removed row of the whole range stay where they are
            const long j0 = base == row0 ? std::min<long>((long)h_first[c], kept) : 0;
            if (kept > j0) {
                const bool direct = base + kept <= row0;
                if (!direct) CHECK_RC(g->stage.grow((size_t)chunk * D * 4, st));
                for (int which = g->keep_f32 ? 0 : 1; which < 2; ++which) {
                    const int u4 = which == 0 ? D / 4 : D / 8;       // 16-byte units of a row (D % 64 == 0)
                    uint4* arr = (which == 0 ? (uint4*)g->gf.p : (uint4*)g->gb.p) + R0 * u4;
                    uint4* dst = direct ? arr + base * u4 : (uint4*)g->stage.p;
                    CHECK_RC(revo::launch_remove_gather(bits, N, row0, len, j0, arr, dst, u4, st));
                    if (!direct)
                        REVO_HIP_CHECK(hipMemcpyAsync(arr + (base + j0) * u4, dst + j0 * u4, (size_t)(kept - j0) * u4 * 16,
                                                      hipMemcpyDeviceToDevice, st));
                }
            }
            base += kept;
        }
    }
    *kept_out = base;
    return 0;
}

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
    long base = 0;
    CHECK_RC(gallery_compact_rows(g, bits, 0, N, chunk, cnt, first, "gallery_remove", st, &base));
    // an emptied gallery starts its certificate maxima over, as revo_gallery_clear does; otherwise they stay: maxima over
    // more rows are upper bounds still
    if (base == 0) REVO_HIP_CHECK(hipMemsetAsync(g->gstat.p, 0, 8, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    if (base < N) g->maxsim.rows = -1;
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
    CHECK_RC(g->edit.grow((size_t)n * 8, st));
    long long* map = (long long*)g->edit.p;
    REVO_HIP_CHECK(hipMemcpyAsync(map, row_idx, (size_t)n * 8, hipMemcpyHostToDevice, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));             // the caller may free its host array on return
    return gallery_write_rows(g, vecs, n, normalize, src_on_device, 0, map, "gallery_update", st);
    API_END
}
