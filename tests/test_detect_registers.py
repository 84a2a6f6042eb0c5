"""CPU: the resource report of the detect kernels (detect.hip), from hipcc's own remarks (hipcc cross-compiles for gfx950
without a GPU): no scratch and no spills in the score, region and compaction kernels, and the region kernel's static LDS --
an image's 1 024 cells with their attributes -- under the 64 KiB a launch gets without opting in."""
from _hipcc_report import assert_no_spill, usage


def test_detect_kernels_use_no_scratch():
    assert_no_spill("detect.hip", "detect_", 3)
    d = usage("detect.hip")
    (regions,) = [k for k in d if "detect_regions_kernel" in k]
    (scores,) = [k for k in d if "detect_scores_kernel" in k]
    print(d[regions], d[scores])
    assert d[scores]["LDS Size"] == 0
    assert 0 < d[regions]["LDS Size"] <= 64 * 1024
    assert d[regions]["VGPRs"] <= 128 and d[scores]["VGPRs"] <= 128
