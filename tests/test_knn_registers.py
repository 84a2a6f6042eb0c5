"""CPU: the register allocation of the kNN graph's kernels (knn.hip), from hipcc's own resource report (hipcc cross-compiles
for gfx950 without a GPU).  The join and the level pass run the 256 x 256 main loop with 128 accumulator registers per lane
under __launch_bounds__(512, 2): two waves per SIMD, which 256 VGPRs allow and 257 would not; a spill inside the tile loop
would wait for the next tile's operand DMA."""
import functools

from _hipcc_report import assert_no_spill, usage


@functools.lru_cache(maxsize=None)
def _report():
    return usage("knn.hip")


def test_knn_join_does_not_spill_and_keeps_its_occupancy():
    assert_no_spill("knn.hip", "knn_join_kernel", 1)
    d = _report()
    (name,) = [k for k in d if "knn_join_kernel" in k]
    print("knn_join_kernel:", d[name])
    assert d[name]["VGPRs"] <= 256, d[name]


def test_knn_level_pass_does_not_spill_and_keeps_its_occupancy():
    assert_no_spill("knn.hip", "knn_level_kernel", 1)
    d = _report()
    (name,) = [k for k in d if "knn_level_kernel" in k]
    print("knn_level_kernel:", d[name])
    assert d[name]["VGPRs"] <= 256, d[name]


def test_no_knn_kernel_spills():
    d = _report()
    names = [k for k in d if "knn_" in k]
    assert len(names) == 7, names                        # sample, level pass, levels, dense rows, join, rescore, select
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
