"""Native-aspect embedding, the parts that need no GPU: the menu of grids and the choice for an image,
the region bitmaps of a rectangular grid, the host resize to a rectangle, the refusals the new entry points make before the
device is touched, and the fp64 reference of the GPU tests held to the oracle at the native grid."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import reverso_amd
from reverso_amd import _lib, config, preprocess, regions, weights
from oracle import pe_vit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grid_reference as gr  # noqa: E402

SIX = [(1080, 1920), (1920, 1080), (768, 1024), (1000, 1500), (500, 500), (300, 2000)]


# ---- menus and choices -----------------------------------------------------------------------------------------------------------
def test_menu_sizes_and_members():
    tiny, b16, l14, g14 = (reverso_amd.get_config(n) for n in ("PE-Tiny-T14-56", "PE-Core-B16-224", "PE-Core-L14-336",
                                                               "PE-Core-G14-448"))
    assert config.aspect_grids(tiny) == [(2, 8), (3, 5), (4, 4), (5, 3), (8, 2)]
    assert len(config.aspect_grids(b16)) == 15 and len(config.aspect_grids(l14)) == 25 and len(config.aspect_grids(g14)) == 33
    half = [(12, 48), (13, 44), (14, 41), (15, 38), (16, 36), (17, 33), (18, 32), (19, 30), (20, 28), (21, 27), (22, 26),
            (23, 25), (24, 24)]
    assert config.aspect_grids(l14) == half + [(w, h) for h, w in reversed(half[:-1])]
    menu = config.aspect_grids(b16)
    assert menu[0] == (7, 28) and menu[-1] == (28, 7) and (14, 14) in menu
    for cfg in (tiny, b16, l14, g14):
        G2 = cfg.grid ** 2
        for ratio in (1.0, 2.0, 4.0, 7.5):
            m = config.aspect_grids(cfg, ratio)
            assert (cfg.grid, cfg.grid) in m and m == sorted(m)
            for gh, gw in m:
                assert gh >= 1 and gw >= 1 and gw == G2 // gh and gh == G2 // gw and max(gh, gw) <= ratio * min(gh, gw)
            assert sorted((w, h) for h, w in m) == m                     # closed under transposition
        assert config.aspect_grids(cfg, 1.0) == [(cfg.grid, cfg.grid)]
    with pytest.raises(ValueError):
        config.aspect_grids(tiny, 0.5)


def test_known_choices_and_the_tie_rule():
    l14, b16 = reverso_amd.get_config("PE-Core-L14-336"), reverso_amd.get_config("PE-Core-B16-224")
    assert [config.aspect_grid(l14, h, w) for h, w in SIX] == [(18, 32), (32, 18), (21, 27), (19, 30), (24, 24), (12, 48)]
    assert [config.aspect_grid(b16, h, w) for h, w in SIX] == [(10, 19), (19, 10), (12, 16), (11, 17), (14, 14), (7, 28)]
    rng = np.random.default_rng(0)
    for cfg in (l14, b16, reverso_amd.get_config("PE-Tiny-N14-56")):
        for h, w in rng.integers(1, 5000, (200, 2)).tolist():
            gh, gw = config.aspect_grid(cfg, h, w)
            assert (gh, gw) in config.aspect_grids(cfg)
            if h != w:            # (a square image is a tie of every pair of transposes: the rule, below, decides)
                assert config.aspect_grid(cfg, w, h) == (gw, gh), (h, w)
            # brute force over the menu: nothing is closer in log aspect
            d = lambda g: abs(np.log(g[1] / g[0]) - np.log(w / h))
            assert d((gh, gw)) <= min(d(g) for g in config.aspect_grids(cfg)) + 1e-12
    # ties: a square image is exactly as far from (3, 5) as from (5, 3) -- the same cells, so the smaller gh wins -- and
    # more cells win before that
    tiny = reverso_amd.get_config("PE-Tiny-T14-56")
    assert config.aspect_grid(tiny, 100, 100, grids=[(5, 3), (3, 5)]) == (3, 5)
    assert config.aspect_grid(tiny, 100, 100, grids=[(3, 5), (5, 3)]) == (3, 5)
    assert config.aspect_grid(tiny, 100, 100, grids=[(1, 2), (4, 2), (2, 4), (2, 1)]) == (2, 4)
    assert config.aspect_grid(tiny, 100, 100, grids=[(1, 2), (2, 1), (6, 3)]) == (6, 3)
    assert config.aspect_grid(tiny, 10, 1000) == (2, 8) and config.aspect_grid(tiny, 10, 1000, max_ratio=1.7) == (3, 5)
    with pytest.raises(ValueError):
        config.aspect_grid(tiny, 0, 5)


# ---- regions ---------------------------------------------------------------------------------------------------------------------
def _unpack(bits, S):
    b = np.asarray(bits, dtype=np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], -1)[:, :S]


@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
@pytest.mark.parametrize("grid", [(2, 8), (5, 3)])
def test_token_masks_of_a_grid_against_a_brute_force_cover_count(cname, grid):
    cfg = reverso_amd.get_config(cname)
    gh, gw = grid
    first, S = (1 if cfg.use_cls else 0), gh * gw + (1 if cfg.use_cls else 0)
    assert regions.words_per_region(cfg, grid) == (S + 31) // 32
    rng = np.random.default_rng(gh * 100 + gw)
    for width, height in ((97, 41), (33, 64), (7, 4), (200, 50)):
        masks = [rng.random((height, width)) < p for p in (0.1, 0.5, 0.9)]
        boxes = [(3.2, 1.0, width - 2.5, height - 0.4), (0, 0, width, height), (width / 3, height / 4, width / 2, height / 2)]
        for min_cover in (0.0, 0.5, 1.0):
            got = _unpack(regions.token_masks(cfg, masks + boxes, width, height, min_cover=min_cover, grid=grid), S)
            for r, region in enumerate(masks + boxes):
                if r >= len(masks):
                    x0, y0, x1, y1 = region
                    m = np.zeros((height, width), bool)
                    for py in range(height):
                        for px in range(width):
                            m[py, px] = x0 <= px + 0.5 < x1 and y0 <= py + 0.5 < y1
                else:
                    m = region
                count, cell = np.zeros((gh, gw), np.int64), np.zeros((gh, gw), np.int64)
                for py in range(height):
                    for px in range(width):
                        cell[py * gh // height, px * gw // width] += 1
                        count[py * gh // height, px * gw // width] += m[py, px]
                ok = (count > 0) & (count >= min_cover * cell)
                if not ok.any():
                    ratio = np.where(cell > 0, count / np.maximum(cell, 1), 0.0)
                    ok.reshape(-1)[int(np.argmax(ratio.reshape(-1)))] = True
                want = np.zeros(S, bool)
                want[first:] = ok.reshape(-1)
                assert np.array_equal(got[r], want), (width, height, min_cover, r)


@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_cell_masks_round_trip_and_full_mask_under_a_grid(cname):
    cfg = reverso_amd.get_config(cname)
    rng = np.random.default_rng(3)
    for grid in ((2, 8), (5, 3), None):
        gh, gw, S = regions._grid(cfg, grid)
        first = 1 if cfg.use_cls else 0
        allow = np.zeros((6, S), bool)
        allow[:, first:] = rng.random((6, gh * gw)) < 0.4
        allow[0, first] = True
        bits = regions._pack(allow)
        for width, height in ((gw, gh), (97, 41), (64, 64)):
            px = regions.cell_masks(cfg, bits, width, height, grid=grid)
            assert px.shape == (6, height, width)
            keep = allow.any(axis=1)
            back = regions.token_masks(cfg, list(px[keep]), width, height, grid=grid)
            assert np.array_equal(back, bits[keep]), (grid, width, height)
        full = _unpack(regions.full_mask(cfg, grid=grid)[None], S)[0]
        assert full.all() and regions.full_mask(cfg, grid=grid).shape == ((S + 31) // 32,)
        nocls = _unpack(regions.full_mask(cfg, include_cls=False, grid=grid)[None], S)[0]
        assert nocls[first:].all() and (not cfg.use_cls or not nocls[0])
        boxes = regions.cell_boxes(cfg, [[0, 0, gw - 1, gh - 1], [gw - 1, 0, gw - 1, 0]], 97, 41, grid=grid)
        assert boxes[0].tolist() == [0, 0, 97, 41] and boxes[1].tolist() == [-((-(gw - 1) * 97) // gw), 0, 97, -((-41) // gh)]
        with pytest.raises(ValueError):
            regions.cell_boxes(cfg, [[0, 0, gw, 0]], 97, 41, grid=grid)
    with pytest.raises(ValueError):
        regions.token_masks(cfg, [(0, 0, 4, 4)], 10, 10, grid=(0, 4))


def test_grid_none_is_the_native_grid():
    for cname in ("PE-Tiny-T14-56", "PE-Tiny-N14-56", "PE-Core-B16-224"):
        cfg = reverso_amd.get_config(cname)
        g = cfg.grid
        rng = np.random.default_rng(5)
        regs = [rng.random((77, 120)) < 0.5, (5, 6, 60.5, 70), (0, 0, 120, 77)]
        a = regions.token_masks(cfg, regs, 120, 77)
        assert np.array_equal(a, regions.token_masks(cfg, regs, 120, 77, grid=(g, g))) and a.shape == (3, (cfg.seq + 31) // 32)
        assert regions.words_per_region(cfg) == regions.words_per_region(cfg, (g, g)) == (cfg.seq + 31) // 32
        assert np.array_equal(regions.full_mask(cfg), regions.full_mask(cfg, grid=(g, g)))
        assert np.array_equal(regions.cell_masks(cfg, a, 120, 77), regions.cell_masks(cfg, a, 120, 77, grid=(g, g)))
        bx = [[0, 1, g - 1, g - 1], [2, 2, 2, 3]]
        assert np.array_equal(regions.cell_boxes(cfg, bx, 120, 77), regions.cell_boxes(cfg, bx, 120, 77, grid=(g, g)))
        # the native rule, restated: cell (px * g // width, py * g // height)
        cells = regions._unpack_cells(cfg, a)
        m = regs[0]
        count = np.zeros((g, g), np.int64)
        cell = np.zeros((g, g), np.int64)
        for py in range(77):
            for px in range(120):
                cell[py * g // 77, px * g // 120] += 1
                count[py * g // 77, px * g // 120] += m[py, px]
        ok = (count > 0) & (count >= 0.5 * cell)
        if not ok.any():
            ok.reshape(-1)[int(np.argmax((count / cell).reshape(-1)))] = True
        assert np.array_equal(cells[0], ok)


# ---- the host resize -------------------------------------------------------------------------------------------------------------
def test_resize_u8_to_a_rectangle_is_pils_resize():
    rng = np.random.default_rng(9)
    for (h, w) in ((37, 211), (640, 480), (1, 1), (56, 56)):
        im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        for oh, ow in ((28, 112), (112, 28), (70, 42), (56, 56)):
            got = preprocess.resize_u8(im, (oh, ow))
            want = np.asarray(im.resize((ow, oh), Image.BILINEAR), dtype=np.uint8).transpose(2, 0, 1)
            assert got.shape == (3, oh, ow) and np.array_equal(got.numpy(), want)
        assert torch.equal(preprocess.resize_u8(im, 56), preprocess.resize_u8(im, (56, 56)))
        assert np.array_equal(preprocess.resize_u8(im, 56).numpy(),
                              np.asarray(im.resize((56, 56), Image.BILINEAR), dtype=np.uint8).transpose(2, 0, 1))
    ims = [Image.fromarray(rng.integers(0, 256, (30 + i, 50, 3), dtype=np.uint8)) for i in range(3)]
    b = preprocess.batch_u8(ims, (28, 112))
    assert b.shape == (3, 3, 28, 112) and all(torch.equal(b[i], preprocess.resize_u8(ims[i], (28, 112))) for i in range(3))
    assert torch.equal(preprocess.batch_u8(ims, 56), preprocess.batch_u8(ims, (56, 56)))


# ---- refusals before the device is touched ---------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    lib = _lib.load()
    for name in ("revo_vit_set_grid", "revo_preprocess_crop_resize_hw"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "revo_vit_read_grid_tables" in _lib.EXPERIMENT_SIGNATURES and hasattr(_lib.load_exp(), "revo_vit_read_grid_tables")
    assert not hasattr(lib, "revo_vit_read_grid_tables")                     # the experiments library only
    for gh, gw in ((2, 8), (0, 0), (-1, 4), (1 << 20, 1 << 20)):
        assert lib.revo_vit_set_grid(None, gh, gw, None) == -2
        assert b"null handle" in lib.revo_last_error()
    job = (_lib.CropJob * 1)()
    out = np.zeros(16, np.uint8)
    for oh, ow in ((0, 56), (56, 0), (-3, 56), (56, 4097), (4097, 4097)):
        assert lib.revo_preprocess_crop_resize_hw(job, 1, oh, ow, out.ctypes.data, None) == -2, (oh, ow)
        assert b"out_size" in lib.revo_last_error() and b"1..4096" in lib.revo_last_error()
    assert lib.revo_preprocess_crop_resize_hw(None, 1, 28, 112, out.ctypes.data, None) == -2
    assert b"null argument" in lib.revo_last_error()
    assert lib.revo_preprocess_crop_resize_hw(job, 1, 28, 112, None, None) == -2 and b"null argument" in lib.revo_last_error()
    assert lib.revo_preprocess_crop_resize_hw(job, -1, 28, 112, out.ctypes.data, None) == -2
    assert b"negative" in lib.revo_last_error()
    assert lib.revo_preprocess_crop_resize_hw(None, 0, 28, 112, None, None) == 0                 # no jobs: nothing to do
    # the square entry is the same call with out_h = out_w
    assert lib.revo_preprocess_crop_resize(job, 1, 0, out.ctypes.data, None) == -2 and b"out_size" in lib.revo_last_error()
    assert lib.revo_preprocess_crop_resize(None, 0, 56, None, None) == 0


# ---- the reference of the GPU tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-T14-56-LS", "PE-Tiny-N14-56"])
def test_the_grid_reference_is_the_oracle_at_the_native_grid(cname):
    cfg = reverso_amd.get_config(cname)
    sd = weights.synth_weights(cfg, seed=5, randomize_affine=True)
    g = torch.Generator().manual_seed(6)
    images = torch.rand(3, 3, cfg.image_size, cfg.image_size, generator=g) * 2 - 1
    want = pe_vit.embed(sd, cfg, images, torch.float64)
    assert torch.equal(gr.embed(sd, cfg, images), want)
    assert torch.equal(gr.embed(sd, cfg, images, grid=(cfg.grid, cfg.grid)), want)
    assert torch.equal(gr.rope_angles(cfg), pe_vit.rope_angles(cfg, torch.float64))
    # and it is a different function elsewhere: the swapped table and the nearest positions are distinguishable in the tables
    grid = (2, 8)
    assert not torch.equal(gr.rope_angles(cfg, grid), gr.rope_angles(cfg, grid, swap_axes=True))
    pos = sd["visual.positional_embedding"]
    assert not torch.equal(gr.resample_positions(cfg, pos, grid)[0], gr.resample_positions(cfg, pos, grid, nearest=True)[0])


def test_resampled_positions_are_torchs_bilinear_interpolation():
    """the formula of include/revo.h (half-pixel centres, clamps) against F.interpolate in fp64"""
    for cname in ("PE-Tiny-T14-56", "PE-Tiny-N14-56", "PE-Core-B16-224"):
        cfg = reverso_amd.get_config(cname)
        G, first = cfg.grid, 1 if cfg.use_cls else 0
        pos = torch.randn(cfg.seq, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        for grid in gr.non_native_menu(cfg) + [(1, G * G), (G * G, 1), (3, 4), (1, 1)]:
            got, corner = gr.resample_positions(cfg, pos, grid)
            want = torch.nn.functional.interpolate(pos[first:].reshape(1, G, G, 8).permute(0, 3, 1, 2), size=grid, mode="bilinear",
                                                   align_corners=False).permute(0, 2, 3, 1).reshape(grid[0] * grid[1], 8)
            assert (got[first:] - want).abs().max().item() <= 1e-14, (cname, grid)
            assert torch.equal(got[:first], pos[:first]) and (got.abs() <= corner + 1e-15).all()
