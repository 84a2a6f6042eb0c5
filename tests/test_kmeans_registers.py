"""CPU: the register allocation of the k-means kernels (kmeans.hip), from hipcc's own resource report (hipcc cross-compiles for
gfx950 without a GPU).  The two assignment passes run the 256 x 256 main loop with 128 accumulator registers per lane under
__launch_bounds__(512, 2): two waves per SIMD, which 256 VGPRs allow and 257 would not; a spill inside the tile loop would
wait for the next tile's operand DMA."""
import functools

from _hipcc_report import assert_no_spill, usage


@functools.lru_cache(maxsize=None)
def _report():
    return usage("kmeans.hip")


def test_the_two_main_loop_kernels_do_not_spill_and_keep_their_occupancy():
    d = _report()
    for kernel in ("kmeans_best_kernel", "kmeans_decide_kernel"):
        assert_no_spill("kmeans.hip", kernel, 1)
        (name,) = [k for k in d if kernel in k]
        print(kernel, d[name])
        assert d[name]["VGPRs"] <= 256, d[name]


def test_no_kmeans_kernel_spills():
    d = _report()
    names = [k for k in d if "kmeans_" in k]
    # rows, best, bound, decide, rescore, finish, keys, counts, partial, sum, keep
    assert len(names) == 11, names
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
