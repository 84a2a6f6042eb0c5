"""CPU: region -> token bitmap (reverso_amd/regions.py token_masks) on known answers, the facade's region modes, and the
refusals of the region entry points of the C ABI before the device is touched (through ctypes and, under AddressSanitizer +
UBSan, through the stand-alone tests/native/regions_host_check.cpp: `make regions_check`)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reverso_amd
from reverso_amd import _lib, regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")

L14 = reverso_amd.get_config("PE-Core-L14-336")          # g = 24, class token, S = 577
G14 = reverso_amd.get_config("PE-Core-G14-448")          # g = 32, no class token, S = 1024
N14 = reverso_amd.get_config("PE-Tiny-N14-56")           # g = 4, no class token, S = 16
T14 = reverso_amd.get_config("PE-Tiny-T14-56")           # g = 4, class token, S = 17


def _tokens(bits_row, S=None):
    """set bits of one bitmap row, ascending"""
    out = [w * 32 + b for w, v in enumerate(bits_row) for b in range(32) if (int(v) >> b) & 1]
    assert S is None or all(t < S for t in out)
    return out


def test_full_image_box_gives_every_patch_and_the_class_token_only_on_request():
    bits = regions.token_masks(L14, [(0, 0, 640, 480)], 640, 480)
    assert bits.dtype == np.uint32 and bits.shape == (1, 19)
    assert _tokens(bits[0], 577) == list(range(1, 577))
    bits = regions.token_masks(L14, [(0, 0, 640, 480)], 640, 480, include_cls=True)
    assert _tokens(bits[0], 577) == list(range(577))
    assert np.array_equal(bits[0], regions.full_mask(L14, include_cls=True))
    assert _tokens(regions.full_mask(L14, include_cls=False)) == list(range(1, 577))
    # a mask of every pixel is that box
    assert np.array_equal(regions.token_masks(L14, [np.ones((480, 640), bool)], 640, 480), regions.token_masks(L14, [(0, 0, 640, 480)], 640, 480))


def test_word_layout_at_577_and_1024_tokens():
    # S = 577: 19 words, word 18 holds one bit (token 576, the last patch)
    bits = regions.token_masks(L14, [(0, 0, 640, 480)], 640, 480)
    assert bits.shape[1] == 19 and int(bits[0, 18]) == 1 and all(int(v) == 0xFFFFFFFF for v in bits[0, 1:18])
    assert int(bits[0, 0]) == 0xFFFFFFFE
    # S = 1024: 32 words exactly, no padding word
    bits = regions.token_masks(G14, [(0, 0, 100, 100)], 100, 100, include_cls=True)     # (no class token to include)
    assert bits.shape == (1, 32) and all(int(v) == 0xFFFFFFFF for v in bits[0])
    assert regions.words_per_region(G14) == 32 and regions.words_per_region(L14) == 19 and regions.words_per_region(T14) == 1


@pytest.mark.parametrize("px,py", [(0, 0), (639, 479), (333, 250), (26, 19), (27, 20)])
def test_one_pixel_mask_gives_the_token_of_its_cell(px, py):
    m = np.zeros((480, 640), dtype=bool)
    m[py, px] = True
    bits = regions.token_masks(L14, [m], 640, 480)
    gx, gy = px * 24 // 640, py * 24 // 480
    assert _tokens(bits[0], 577) == [1 + gy * 24 + gx]


def test_towers_without_a_class_token_start_at_cell_0_0():
    m = np.zeros((56, 56), dtype=bool)
    m[0, 0] = True
    assert _tokens(regions.token_masks(N14, [m], 56, 56)[0], 16) == [0]
    assert _tokens(regions.token_masks(T14, [m], 56, 56)[0], 17) == [1]
    assert _tokens(regions.token_masks(N14, [m], 56, 56, include_cls=True)[0], 16) == [0]
    m[:] = False
    m[55, 55] = True
    assert _tokens(regions.token_masks(N14, [m], 56, 56)[0], 16) == [15]
    assert _tokens(regions.token_masks(T14, [m], 56, 56, include_cls=True)[0], 17) == [0, 16]


def test_cover_threshold_and_fallback_and_ties():
    # 56 x 56 source, g = 4: cells of 14 x 14 = 196 pixels.  98 pixels = exactly half: allowed; 97: not
    m = np.zeros((56, 56), dtype=bool)
    m[14:21, 14:28] = True                                  # 7 rows x 14 = 98 pixels of cell (1, 1)
    assert _tokens(regions.token_masks(T14, [m], 56, 56)[0]) == [1 + 1 * 4 + 1]
    m[20, 27] = False                                       # 97: below half -- and nothing else: the fallback gives the cell
    assert _tokens(regions.token_masks(T14, [m], 56, 56)[0]) == [1 + 1 * 4 + 1]
    # 49 % of one cell and a little of another: the fallback picks the fuller one only
    m = np.zeros((56, 56), dtype=bool)
    cell = np.zeros((14, 14), dtype=bool)
    cell.reshape(-1)[:96] = True                            # 96 / 196 = 49 %
    m[28:42, 42:56] = cell                                  # cell (gy 2, gx 3)
    m[0, 0:5] = True                                        # 5 pixels of cell (0, 0)
    assert _tokens(regions.token_masks(T14, [m], 56, 56)[0]) == [1 + 2 * 4 + 3]
    assert _tokens(regions.token_masks(T14, [m], 56, 56, min_cover=0.02)[0]) == [1, 1 + 2 * 4 + 3]
    # a tie goes to the lowest token
    m = np.zeros((56, 56), dtype=bool)
    m[50, 50] = True                                        # cell (3, 3)
    m[20, 30] = True                                        # cell (1, 2)
    m[30, 1] = True                                         # cell (2, 0)
    assert _tokens(regions.token_masks(T14, [m], 56, 56)[0]) == [1 + 1 * 4 + 2]
    # cells of unequal size (57 pixels over 4 cells: 15, 14, 14, 14): the ratio decides, not the count
    m = np.zeros((57, 57), dtype=bool)
    m[0:7, 0:15] = True                                     # 105 of 225 in cell (0, 0): 46.7 %
    m[15:22, 15:29] = True                                  # 98 of 196 in cell (1, 1): 50 %
    assert _tokens(regions.token_masks(T14, [m], 57, 57)[0]) == [1 + 1 * 4 + 1]


def test_boxes_are_their_rectangles_and_empty_regions_raise():
    m = np.zeros((48, 64), dtype=bool)
    m[10:30, 8:40] = True
    a = regions.token_masks(T14, [m, (8, 10, 40, 30)], 64, 48)
    assert np.array_equal(a[0], a[1]) and a.shape == (2, 1)
    # clipped to the image; fractional corners go by pixel centres
    assert np.array_equal(regions.token_masks(T14, [(-5, -5, 700, 500)], 64, 48), regions.token_masks(T14, [(0, 0, 64, 48)], 64, 48))
    assert np.array_equal(regions.token_masks(T14, [(7.6, 9.6, 39.6, 29.6)], 64, 48)[0], a[0])
    with pytest.raises(ValueError):
        regions.token_masks(T14, [np.zeros((48, 64), bool)], 64, 48)
    with pytest.raises(ValueError):
        regions.token_masks(T14, [(70, 10, 80, 20)], 64, 48)
    with pytest.raises(ValueError):
        regions.token_masks(T14, [np.ones((10, 10), bool)], 64, 48)
    assert regions.token_masks(T14, [], 64, 48).shape == (0, 1)


def test_region_mode_names():
    """`pool` joins `global` and `crop`; anything else is still refused before a device is asked for."""
    import inspect
    from reverso_amd.core_system import SimpleReverso
    with pytest.raises(ValueError, match="region_mode"):
        SimpleReverso(model_name="PE-Tiny-T14-56", region_mode="nonsense")
    src = inspect.getsource(SimpleReverso.__init__)
    assert '("global", "crop", "pool")' in src
    assert inspect.signature(SimpleReverso.__init__).parameters["region_mode"].default == "global"


def test_region_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    img = (C.c_int32 * 2)(0, 1)
    bits = (C.c_uint32 * 2)(1, 1)
    out = (C.c_float * 8)()
    p = lambda a: C.cast(a, C.c_void_p)
    # null handle
    assert lib.revo_vit_forward_regions(None, p(out), 1, 2, p(img), p(bits), 0, 2, None, p(out), 1, None) == -2
    assert b"null handle" in lib.revo_last_error()
    # null region arrays / output with regions
    assert lib.revo_vit_forward_regions(None, p(out), 1, 2, None, p(bits), 0, 2, None, p(out), 1, None) == -2
    assert b"null region_image" in lib.revo_last_error()
    assert lib.revo_vit_forward_regions(None, p(out), 1, 2, p(img), p(bits), 0, 2, None, None, 1, None) == -2
    assert b"out_regions" in lib.revo_last_error()
    # negative counts
    assert lib.revo_vit_forward_regions(None, p(out), 1, 2, p(img), p(bits), 0, -1, None, p(out), 1, None) == -2
    assert b"negative" in lib.revo_last_error()
    assert lib.revo_vit_forward_regions(None, p(out), 1, -2, p(img), p(bits), 0, 0, None, p(out), 1, None) == -2
    assert b"negative" in lib.revo_last_error()
    # an image index outside [0, batch)
    assert lib.revo_vit_forward_regions(None, p(out), 1, 1, p(img), p(bits), 0, 2, None, p(out), 1, None) == -2
    assert b"region 1 names image 1, outside [0, batch = 1)" in lib.revo_last_error()
    img[0] = -1
    assert lib.revo_vit_forward_regions(None, p(out), 1, 2, p(img), p(bits), 0, 2, None, p(out), 1, None) == -2
    assert b"region 0 names image -1" in lib.revo_last_error()
    # the single kernel
    assert lib.revo_op_pool_rows_masked(None, 128, p(out), p(img), p(bits), 1, 1, 17, 128, 2, p(out), None) == -2
    assert b"null" in lib.revo_last_error()
    assert lib.revo_op_pool_rows_masked(p(out), 128, p(out), p(img), p(bits), -1, 1, 17, 128, 2, p(out), None) == -2
    assert lib.revo_op_pool_rows_masked(p(out), 64, p(out), p(img), p(bits), 1, 1, 17, 128, 2, p(out), None) == -2
    assert lib.revo_op_pool_rows_masked(p(out), 128, p(out), p(img), p(bits), 1, 0, 17, 128, 2, p(out), None) == -2


def test_region_entry_points_under_address_and_ub_sanitizers():
    """tests/native/regions_host_check.cpp: the same refusals from a stand-alone program whose host code (api.hip and the
    other translation units of the C ABI) is compiled with -fsanitize=address,undefined; no device is touched."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "all", "regions_check"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "regions_host_check")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("null handle", "negative counts", "image index out of range", "null region arrays", "op: null arguments",
                 "op: bad sizes", "no regions, no output"):
        assert case in r.stdout
