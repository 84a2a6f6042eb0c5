// The detect entry points of the C ABI (include/revo.h, TOKENS and DETECT: revo_vit_forward_tokens, revo_vit_detect and its reads,
// revo_op_detect_scores, revo_op_detect_regions) under AddressSanitizer + UBSan with no GPU: every refusal they make before the
// device is touched, with its message; the host arrays they are given are exactly as long as the call says (a read past the end
// is a sanitizer report).  Built by `make -C revers-o_amd/csrc detect_check` (the translation units of the C ABI compiled with
// -fsanitize=address,undefined on the host side, as for abi_host_check) and run by tests/test_detect_host.py in the CPU tier.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    std::vector<float> buf(64, 0.f), thr(3, 0.f);
    std::vector<int32_t> cnt(2, -7);
    int64_t n = -7;

    section("tower entry points: null handle");
    EXPECT(revo_vit_detect(nullptr, buf.data(), 1, 1, buf.data(), 3, thr.data(), 0, 1, 1, nullptr, 0, 1, &n, nullptr) == -2);
    EXPECT(err_has("null handle") && n == -7);
    EXPECT(revo_vit_forward_tokens(nullptr, buf.data(), 1, 1, nullptr, buf.data(), 1, nullptr) == -2);
    EXPECT(err_has("null handle"));
    EXPECT(revo_vit_detect_read(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == -2);
    EXPECT(err_has("null handle"));
    EXPECT(revo_vit_detect_maps(nullptr, nullptr, nullptr, 0) == -2);
    EXPECT(err_has("null handle"));

    section("op scores: sizes and null arguments");
    EXPECT(revo_op_detect_scores(buf.data(), 4, buf.data(), 0, 16, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(err_has("n_prompts"));
    EXPECT(revo_op_detect_scores(buf.data(), 4, buf.data(), 65, 16, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(revo_op_detect_scores(buf.data(), 4, buf.data(), 2, 6, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(err_has("dim"));
    EXPECT(revo_op_detect_scores(buf.data(), -1, buf.data(), 2, 16, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(err_has("rows"));
    EXPECT(revo_op_detect_scores(nullptr, 4, buf.data(), 2, 16, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(err_has("null"));
    EXPECT(revo_op_detect_scores(buf.data(), 4, nullptr, 2, 16, buf.data(), buf.data(), nullptr) == -2);
    EXPECT(revo_op_detect_scores(buf.data(), 4, buf.data(), 2, 16, nullptr, buf.data(), nullptr) == -2);
    EXPECT(revo_op_detect_scores(buf.data(), 4, buf.data(), 2, 16, buf.data(), nullptr, nullptr) == -2);

    section("op regions: limits");
    auto regions = [&](int batch, int P, int g, int cls, int nbg, int mc, int mr, const float* s, const float* t, int32_t* c) {
        return revo_op_detect_regions(s, batch, P, g, cls, t, nbg, mc, mr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, c, nullptr);
    };
    EXPECT(regions(1, 0, 4, 1, 0, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("n_prompts"));
    EXPECT(regions(1, 65, 4, 1, 0, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("n_prompts"));
    EXPECT(regions(1, 3, 4, 1, 3, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("n_background"));
    EXPECT(regions(1, 3, 4, 1, -1, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("n_background"));
    EXPECT(regions(1, 3, 4, 1, 0, 0, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("min_cells"));
    EXPECT(regions(1, 3, 4, 1, 0, 1, 0, buf.data(), thr.data(), cnt.data()) == -2 && err_has("max_regions"));
    EXPECT(regions(1, 3, 4, 1, 0, 1, 17, buf.data(), thr.data(), cnt.data()) == -2 && err_has("max_regions"));
    EXPECT(regions(1, 3, 0, 1, 0, 1, 1, buf.data(), thr.data(), cnt.data()) == -2 && err_has("g * g"));
    EXPECT(regions(1, 3, 33, 1, 0, 1, 1, buf.data(), thr.data(), cnt.data()) == -2 && err_has("g * g"));
    EXPECT(regions(1, 3, 46341, 1, 0, 1, 1, buf.data(), thr.data(), cnt.data()) == -2 && err_has("g * g"));   // g * g past 2^31
    EXPECT(regions(1, 3, 4, 2, 0, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("use_cls"));
    EXPECT(regions(-1, 3, 4, 1, 0, 1, 4, buf.data(), thr.data(), cnt.data()) == -2 && err_has("batch"));

    section("op regions: null arguments");
    EXPECT(regions(1, 3, 4, 1, 0, 1, 4, nullptr, thr.data(), cnt.data()) == -2 && err_has("null"));
    EXPECT(regions(1, 3, 4, 1, 0, 1, 4, buf.data(), nullptr, cnt.data()) == -2 && err_has("null"));
    EXPECT(regions(1, 3, 4, 1, 0, 1, 4, buf.data(), thr.data(), nullptr) == -2 && err_has("null"));
    // no images: nothing to do
    EXPECT(regions(0, 3, 4, 1, 0, 1, 4, nullptr, thr.data(), cnt.data()) == 0);
    EXPECT(cnt[0] == -7 && cnt[1] == -7);

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
