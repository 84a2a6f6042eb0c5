// The region entry points of the C ABI (include/revo.h, REGIONS: revo_vit_forward_regions, revo_op_pool_rows_masked) under
// AddressSanitizer + UBSan with no GPU: every refusal they make before the device is touched, with its message; the host
// arrays they are given are exactly as long as the call says (a read past the end is a sanitizer report).  Built by
// `make -C revers-o_amd/csrc regions_check` (the translation units of the C ABI compiled with -fsanitize=address,undefined on
// the host side, as for abi_host_check) and run by tests/test_region_masks.py in the CPU tier.
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
    const int words = 19;                                   // S = 577
    std::vector<int32_t> img = {0, 1, 1, 0, 1};
    std::vector<uint32_t> bits((size_t)img.size() * words, 0xFFFFFFFFu);
    std::vector<float> out(img.size() * 8), images(16);
    const int n = (int)img.size();

    section("null handle");
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 0, n, out.data(), out.data(), 1, nullptr) == -2);
    EXPECT(err_has("null handle"));
    EXPECT(revo_vit_forward_regions(nullptr, nullptr, 0, 2, img.data(), bits.data(), 0, n, nullptr, out.data(), 0, nullptr) == -2);
    EXPECT(err_has("null handle or images"));

    section("negative counts");
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 0, -1, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("negative"));
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, -1, img.data(), bits.data(), 0, 0, out.data(), nullptr, 1, nullptr) == -2);
    EXPECT(err_has("negative"));

    section("null region arrays");
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, nullptr, bits.data(), 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("null region_image"));
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), nullptr, 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("region_bits"));
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 1, n, out.data(), nullptr, 1, nullptr) == -2);
    EXPECT(err_has("out_regions"));

    section("image index out of range");
    // every entry is looked at, none past the end: the last one is the bad one
    img[4] = 2;
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("region 4 names image 2, outside [0, batch = 2)"));
    img[4] = 1; img[0] = -7;
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("region 0 names image -7"));
    img[0] = 0;
    // batch 0: no index can be valid
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 0, img.data(), bits.data(), 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("outside [0, batch = 0)"));
    // all valid: the next refusal is the handle
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, img.data(), bits.data(), 0, n, nullptr, out.data(), 1, nullptr) == -2);
    EXPECT(err_has("null handle"));

    section("no regions, no output");
    EXPECT(revo_vit_forward_regions(nullptr, images.data(), 1, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, 1, nullptr) == -2);

    section("op: null arguments");
    EXPECT(revo_op_pool_rows_masked(nullptr, 128, images.data(), img.data(), bits.data(), 1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(err_has("null argument"));
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, nullptr, img.data(), bits.data(), 1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), nullptr, bits.data(), 1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), nullptr, 1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), 1, 2, 17, 128, 2, nullptr, nullptr) == -2);

    section("op: bad sizes");
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), -1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(err_has("sizes"));
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), 1, 0, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), 1, 2, 0, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 64, images.data(), img.data(), bits.data(), 1, 2, 17, 128, 2, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), 1, 2, 17, 128, 0, out.data(), nullptr) == -2);
    // more heads than a thread carries, a width that is no multiple of 4: refused by the launcher, before any launch
    EXPECT(revo_op_pool_rows_masked(images.data(), 128, images.data(), img.data(), bits.data(), 1, 2, 17, 128, 17, out.data(), nullptr) == -2);
    EXPECT(revo_op_pool_rows_masked(images.data(), 130, images.data(), img.data(), bits.data(), 1, 2, 17, 130, 2, out.data(), nullptr) == -2);
    // no regions: nothing to do, whatever the pointers
    EXPECT(revo_op_pool_rows_masked(nullptr, 128, nullptr, nullptr, nullptr, 0, 2, 17, 128, 2, nullptr, nullptr) == 0);

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
