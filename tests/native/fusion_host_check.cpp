// The fusion entry points of the C ABI (include/revo.h, FUSION: revo_search_fusion, revo_topk_fuse) under AddressSanitizer +
// UBSan with no GPU: every refusal they make before the device is touched, with its message; the host arrays they are given
// (weights, list thresholds) are exactly as long as the call says, so a read past the end is a sanitizer report.  The handle is
// a zero-filled stand-in (no fp32 master rows: a call whose arguments are all valid stops at the keep_f32 check).  Built by
// `make -C revers-o_amd/csrc fusion_check` (the translation units of the C ABI compiled with -fsanitize=address,undefined on the
// host side, as for abi_host_check) and run by tests/test_fusion_host.py in the CPU tier.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/revo.h"

static int failures = 0;
static void section(const char* name) { std::printf("case: %s\n", name); }
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d  %s   [last error: %s]\n", __FILE__, __LINE__, #cond, revo_last_error()); ++failures; } \
    } while (0)
static bool err_has(const char* needle) { return std::strstr(revo_last_error(), needle) != nullptr; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<uint64_t> handle_words(8192, 0);
    revo_gallery* g = reinterpret_cast<revo_gallery*>(handle_words.data());
    std::vector<float> q(64, 0.f), s(16, -7.f);
    std::vector<int64_t> ix(16, -7);
    std::vector<int32_t> ct(4, -7), rk(64, -7);
    auto untouched = [&] {
        for (float v : s) if (v != -7.f) return false;
        for (int64_t v : ix) if (v != -7) return false;
        for (int32_t v : ct) if (v != -7) return false;
        for (int32_t v : rk) if (v != -7) return false;
        return true;
    };
    auto search = [&](int n, int m, int C, int method, float rrf_k, const float* w, const float* t, int k, int has, float thr) {
        return revo_search_fusion(g, q.data(), n, m, C, method, rrf_k, w, t, k, has, thr, 0, s.data(), ix.data(), ct.data(),
                                  rk.data(), nullptr, nullptr);
    };
    auto fuse = [&](int n, int m, int C, int method, float rrf_k, const float* w, const float* t, int k, int has, float thr) {
        return revo_topk_fuse(q.data(), ix.data(), ct.data(), n, m, C, method, rrf_k, w, t, k, has, thr, s.data(), ix.data(),
                              ct.data(), rk.data(), nullptr);
    };

    section("search_fusion: null arguments");
    EXPECT(revo_search_fusion(nullptr, q.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, 0, s.data(), ix.data(), ct.data(),
                              nullptr, nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_fusion(g, nullptr, 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, 0, s.data(), ix.data(), ct.data(), nullptr,
                              nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_fusion(g, q.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, 0, nullptr, ix.data(), ct.data(), nullptr,
                              nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_fusion(g, q.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, 0, s.data(), nullptr, ct.data(), nullptr,
                              nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_fusion(g, q.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, 0, s.data(), ix.data(), nullptr, nullptr,
                              nullptr, nullptr) == -2 && err_has("null"));

    for (int which = 0; which < 2; ++which) {
        section(which ? "topk_fuse: domains" : "search_fusion: domains");
        auto call = [&](int n, int m, int C, int method, float rrf_k, const float* w, const float* t, int k, int has, float thr) {
            return which ? fuse(n, m, C, method, rrf_k, w, t, k, has, thr) : search(n, m, C, method, rrf_k, w, t, k, has, thr);
        };
        EXPECT(call(-1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("negative"));
        EXPECT(call(1, 0, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("lists"));
        EXPECT(call(1, 65, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("lists"));
        EXPECT(call(1, 2, 0, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("limit"));
        EXPECT(call(1, 2, 1025, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("limit"));
        EXPECT(call(1, 9, 1024, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("8192"));
        EXPECT(call(1, 64, 129, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("8192"));
        EXPECT(call(1, 2, 4, 0, 60.f, nullptr, nullptr, 0, 0, 0.f) == -2 && err_has("k must"));
        EXPECT(call(1, 2, 4, 0, 60.f, nullptr, nullptr, 1025, 0, 0.f) == -2 && err_has("k must"));
        EXPECT(call(1, 2, 4, 2, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("method"));
        EXPECT(call(1, 2, 4, -1, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("method"));
        EXPECT(call(1, 2, 4, 0, -1.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("rrf_k"));
        EXPECT(call(1, 2, 4, 0, inf, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("rrf_k"));
        EXPECT(call(1, 2, 4, 0, nan, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("rrf_k"));
        EXPECT(call(33554432, 64, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f) == -2 && err_has("31 bits"));
        // arrays of exactly m entries, the bad one last
        for (int m : {1, 3, 64}) {
            std::vector<float> w(m, 1.f), t(m, -inf);
            const int C = 8192 / m > 1024 ? 1024 : 8192 / m;
            w[m - 1] = -0.5f;
            EXPECT(call(1, m, C, 0, 60.f, w.data(), t.data(), 2, 0, 0.f) == -2 && err_has("weight"));
            w[m - 1] = inf;
            EXPECT(call(1, m, C, 0, 60.f, w.data(), t.data(), 2, 0, 0.f) == -2 && err_has("weight"));
            w[m - 1] = nan;
            EXPECT(call(1, m, C, 0, 60.f, w.data(), t.data(), 2, 0, 0.f) == -2 && err_has("weight"));
            w[m - 1] = 0.f;
            t[m - 1] = nan;
            EXPECT(call(1, m, C, 1, 60.f, w.data(), t.data(), 2, 0, 0.f) == -2 && err_has("list threshold"));
            t[m - 1] = inf;
            EXPECT(call(1, m, C, 1, 60.f, w.data(), t.data(), 2, 1, nan) == -2 && err_has("NaN"));
            if (!which) {        // every argument valid, the boundary values included: the handle has no fp32 master rows
                EXPECT(call(1, m, C, 1, 0.f, w.data(), t.data(), 1024, 1, -inf) == -2 && err_has("keep_f32"));
                EXPECT(call(0, m, C, 0, 60.f, w.data(), nullptr, 1, 0, nan) == -2 && err_has("keep_f32"));
            }
        }
        EXPECT(untouched());
    }

    section("topk_fuse: null arguments and the empty call");
    EXPECT(revo_topk_fuse(nullptr, ix.data(), ct.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), ix.data(), ct.data(),
                          nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_topk_fuse(q.data(), nullptr, ct.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), ix.data(), ct.data(),
                          nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_topk_fuse(q.data(), ix.data(), nullptr, 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), ix.data(), ct.data(),
                          nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_topk_fuse(q.data(), ix.data(), ct.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, nullptr, ix.data(), ct.data(),
                          nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_topk_fuse(q.data(), ix.data(), ct.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), nullptr, ct.data(),
                          nullptr, nullptr) == -2 && err_has("null"));
    EXPECT(revo_topk_fuse(q.data(), ix.data(), ct.data(), 1, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), ix.data(), nullptr,
                          nullptr, nullptr) == -2 && err_has("null"));
    // no fused search: nothing to do, the inputs may be null
    EXPECT(revo_topk_fuse(nullptr, nullptr, nullptr, 0, 2, 4, 0, 60.f, nullptr, nullptr, 2, 0, 0.f, s.data(), ix.data(), ct.data(),
                          nullptr, nullptr) == 0);
    EXPECT(untouched());

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
