"""CPU: the register allocation of the boosted search's kernels (boost.hip), from hipcc's own resource report (hipcc
cross-compiles for gfx950 without a GPU).  The pass runs the 256 x 256 main loop with 128 accumulator registers per lane and
holds a row multiplier and a row bias per lane across it (requested before the main loop starts): a
spill inside the tile loop would wait for the next tile's operand DMA.  (Occupancy is not at stake: the kernel's 129 KiB of
LDS leave room for one workgroup per CU, as with the recommend pass, and __launch_bounds__(512, 2) caps the registers by
itself -- no spill and no scratch is the whole check.)"""
import functools

from _hipcc_report import assert_no_spill, usage


@functools.lru_cache(maxsize=None)
def _report():
    return usage("boost.hip")


def test_boost_pass_does_not_spill():
    assert_no_spill("boost.hip", "boost_pass_kernel", 2)                 # the sample form and the candidate form
    d = _report()
    for name in [k for k in d if "boost_pass_kernel" in k]:
        print(name, d[name])


def test_no_boost_kernel_spills():
    d = _report()
    names = [k for k in d if "boost_" in k]
    assert len(names) == 4, names                                        # sample pass, candidate pass, rescore, emit
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
