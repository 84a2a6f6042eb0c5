// The boosted search's entry point of the C ABI (include/revo.h, BOOSTED: revo_search_boosted) under AddressSanitizer + UBSan
// with no GPU: every refusal it makes before the device is touched, with its message, and the outputs untouched.  The handle is
// a zero-filled stand-in (no fp32 master rows: a call whose arguments are all valid stops at the keep_f32 check).  Built by
// `make -C revers-o_amd/csrc boost_check` (the translation units of the C ABI compiled with -fsanitize=address,undefined on the
// host side, as for abi_host_check) and run by tests/test_boost_host.py in the CPU tier.
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
    std::vector<float> q(64, 0.f), m(4, 1.f), b(4, 0.f), s(8, -7.f), sim(8, -7.f);
    std::vector<int64_t> ix(8, -7);
    std::vector<int32_t> ct(1, -7);
    auto untouched = [&] {
        for (float v : s) if (v != -7.f) return false;
        for (float v : sim) if (v != -7.f) return false;
        for (int64_t v : ix) if (v != -7) return false;
        return ct[0] == -7;
    };
    auto call = [&](int k, int has, float thr, int has_min, float min_sim) {
        return revo_search_boosted(g, q.data(), m.data(), b.data(), k, has, thr, has_min, min_sim, 0, s.data(), sim.data(), ix.data(),
                                   ct.data(), nullptr);
    };

    section("search_boosted: null arguments");
    EXPECT(revo_search_boosted(nullptr, q.data(), nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), sim.data(), ix.data(), ct.data(),
                               nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_boosted(g, nullptr, nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), sim.data(), ix.data(), ct.data(),
                               nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_boosted(g, q.data(), nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, nullptr, sim.data(), ix.data(), ct.data(),
                               nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_boosted(g, q.data(), nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), nullptr, ix.data(), ct.data(),
                               nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_boosted(g, q.data(), nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), sim.data(), nullptr, ct.data(),
                               nullptr) == -2 && err_has("null"));
    EXPECT(revo_search_boosted(g, q.data(), nullptr, nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), sim.data(), ix.data(), nullptr,
                               nullptr) == -2 && err_has("null"));
    EXPECT(untouched());

    section("search_boosted: domains");
    EXPECT(call(0, 0, 0.f, 0, 0.f) == -2 && err_has("k must"));
    EXPECT(call(1025, 0, 0.f, 0, 0.f) == -2 && err_has("k must"));
    EXPECT(call(-3, 0, 0.f, 0, 0.f) == -2 && err_has("k must"));
    EXPECT(call(5, 1, nan, 0, 0.f) == -2 && err_has("threshold is NaN"));
    EXPECT(call(5, 0, 0.f, 1, nan) == -2 && err_has("min_similarity is NaN"));
    EXPECT(untouched());

    section("search_boosted: valid arguments stop at the master rows");
    // (a NaN that is not in use, infinite cuts, the largest k; null mult and bias)
    EXPECT(call(1024, 0, nan, 0, nan) == -2 && err_has("keep_f32"));
    EXPECT(call(1, 1, -inf, 1, inf) == -2 && err_has("keep_f32"));
    EXPECT(revo_search_boosted(g, q.data(), nullptr, b.data(), 5, 0, 0.f, 0, 0.f, 1ll << 40, s.data(), sim.data(), ix.data(), ct.data(),
                               nullptr) == -2 && err_has("keep_f32"));
    EXPECT(revo_search_boosted(g, q.data(), m.data(), nullptr, 5, 0, 0.f, 0, 0.f, 0, s.data(), sim.data(), ix.data(), ct.data(),
                               nullptr) == -2 && err_has("keep_f32"));
    EXPECT(untouched());

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
