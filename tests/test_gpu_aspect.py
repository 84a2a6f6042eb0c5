"""Native-aspect embedding on the device (include/revo.h GRIDS): the tables of every grid shape held to
the fp64 formulas within the two derived bounds, the native path bit for bit what it was, the forward on rectangular grids
against the fp64 reference of tests/_grid_reference.py at the project's existing bars (tests/test_gpu_embed.py), one test on
sharpened attention that can tell a transposed rotary table, regions and tokens under a grid, the refusal of detect, and the
rectangular device resize against Pillow.

Why the tables are checked directly: with the seeded N(0, 0.02^2) towers the final embedding barely reacts to the rotary table
(RoPE axes swapped: 1 - cos 2e-8 ... 9e-7 on the tiny towers, 2e-5 on B16-224; nearest instead of bilinear positions: 3e-4), so
the end-to-end bar of cosine >= 0.9999 cannot see a transposed table on those weights."""
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import reverso_amd
from reverso_amd import _lib, engine, preprocess, regions, weights
from oracle import pe_vit

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _grid_reference as gr  # noqa: E402
import make_golden  # noqa: E402

TINY = ("PE-Tiny-T14-56", "PE-Tiny-T14-56-LS", "PE-Tiny-N14-56")
B16_GRIDS = [(7, 28), (12, 16), (13, 15), (9, 21)]


@functools.lru_cache(maxsize=None)
def _tiny(cname):
    cfg, sd, _ = make_golden.tiny_case(cname)
    return cfg, sd


@functools.lru_cache(maxsize=None)
def _seeded(cname):
    """the seeded N(0, 0.02^2) tower of smoke(): the weights on which the suite holds scores against a gallery to 1e-3 (the
    scaled towers of the goldens, _tiny, are held to the taps and the cosine only: their 64-dimensional embeddings sit at
    cosine 0.99999 of the reference, which is a score error of 1e-3 ... 2e-3 against 256 random unit vectors)"""
    cfg = reverso_amd.get_config(cname)
    return cfg, weights.synth_weights(cfg, seed=3, randomize_affine=True)


def _engines(cfg, sd, dev, max_batch, product=True, hooks=True):
    """(the product library's engine, the experiment library's with the tap hooks), each only when asked for"""
    dsd = {k: v.to(dev) for k, v in sd.items()}
    return (engine.VitEngine(cfg, dsd, device=0, max_batch=max_batch) if product else None,
            engine.VitEngine(cfg, dsd, device=0, max_batch=max_batch, experiments=True) if hooks else None)


def _read_tables(engx, grid):
    """(pos [S', W], rope [S', head_dim / 2, 2]) of the shape `grid` as the handle holds them"""
    cfg = engx.cfg
    S = engx._grid(grid)[2]
    pos = torch.full((S, cfg.width), float("nan"), device=engx.device)
    rope = torch.full((S, cfg.head_dim // 2, 2), float("nan"), device=engx.device)
    with engx._grid_frame(grid) as st:
        assert engx._lib.revo_vit_seq_len(engx._h) == S
        engx._call("revo_vit_read_grid_tables", _lib.ptr(pos), _lib.ptr(rope), st)
    torch.cuda.synchronize()
    return pos.cpu(), rope.cpu()


def _check_embedding(emb, ref, gallery, what):
    """the bars of tests/test_gpu_embed.py: cosine >= 0.9999, unit norm within 1e-5, scores against a gallery within 1e-3"""
    emb, ref = emb.cpu().double(), ref.cpu().double()
    cos = (emb * ref).sum(-1)
    nrm = (emb.norm(dim=-1) - 1).abs().max().item()
    sc = (emb @ gallery.T - ref @ gallery.T).abs().max().item()
    print(f"{what}: cosine min {cos.min().item():.7f}, |norm - 1| {nrm:.2e}, score error {sc:.2e}")
    assert (cos >= 0.9999).all(), (what, cos.min().item())
    assert nrm <= 1e-5, (what, nrm)
    assert sc <= 1e-3, (what, sc)


def _check_tap(got, ref, what):
    got, ref = got.cpu().double(), ref.cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, top = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max|d| {err:.3e} of max|x| {top:.3e} ({err / top:.2e})")
    assert err <= 3e-2 * top, (what, err, top)


def _gallery(dim, seed=99, n=256):
    g = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return g / g.norm(dim=-1, keepdim=True)


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_tables_of_every_shape_against_the_fp64_formulas(dev, cname):
    """Positions within 6 * 2^-24 * max|corner| of the bilinear formula in fp64 (four weights rounded once each and one fma
    chain: five roundings of the result and its weights), every cos and sin within 2^-24 + 1e-12 of the fp64 table; at (G, G)
    the native tables themselves, bit for bit.  T14: class token, head_dim 64; N14: no class token, head_dim 96."""
    cfg, sd = _tiny(cname)
    _, engx = _engines(cfg, sd, dev, 2, product=False)
    G = cfg.grid
    pos0 = sd["visual.positional_embedding"]
    for grid in gr.non_native_menu(cfg) + [(1, 16), (16, 1), (3, 4), (1, 1)]:
        pos, rope = _read_tables(engx, grid)
        want, corner = gr.resample_positions(cfg, pos0, grid)
        err = (pos.double() - want).abs()
        assert torch.isfinite(pos).all() and (err <= gr.POS_BOUND * corner).all(), (grid, (err / corner.clamp_min(1e-30)).max().item())
        if cfg.use_cls:
            assert torch.equal(pos[0], pos0[0])
        rerr = (rope.double() - gr.rope_cos_sin(cfg, grid)).abs().max().item()
        assert torch.isfinite(rope).all() and rerr <= gr.ROPE_BOUND, (grid, rerr)
        # teeth: the same checks refuse the tables of the transposed grid's walk and nearest positions
        if grid[0] != grid[1]:
            swapped = gr.rope_angles(cfg, grid, swap_axes=True)[:, 0::2]
            assert (rope.double()[..., 0] - swapped.cos()).abs().max().item() > 1e-3, grid
        if grid[0] * grid[1] > 1:
            near = gr.resample_positions(cfg, pos0, grid, nearest=True)[0]
            assert ((pos.double() - near).abs() > gr.POS_BOUND * corner).any(), grid
    for grid in ((G, G), None):
        pos, rope = _read_tables(engx, grid)
        assert torch.equal(pos, pos0)
        assert (rope.double() - gr.rope_cos_sin(cfg, None)).abs().max().item() <= gr.ROPE_BOUND
        assert torch.equal(rope, _read_tables(engx, None)[1])
    engx.close()


def test_set_grid_refusals_and_the_64_shape_limit(dev):
    cfg, sd = _tiny("PE-Tiny-T14-56")
    eng = _engines(cfg, sd, dev, 2, hooks=False)[0]
    lib, st = eng._lib, _lib.current_stream()
    for gh, gw, word in ((3, 6, "more than the native"), (17, 1, "more than the native"), (-1, 4, "positive sides"),
                         (0, 4, "positive sides"), (4, 0, "positive sides")):
        assert lib.revo_vit_set_grid(eng._h, gh, gw, st) == -2, (gh, gw)
        msg = lib.revo_last_error().decode()
        assert word in msg and f"({gh}, {gw})" in msg, msg
        assert lib.revo_vit_seq_len(eng._h) == cfg.seq                    # a refused call changes nothing
    with pytest.raises(ValueError):
        eng.embed(torch.zeros((1, 3, 56, 56), dtype=torch.uint8, device=dev), grid=(2, 9))
    with pytest.raises(ValueError):                                       # the image must have the grid's shape
        eng.embed(torch.zeros((1, 3, 56, 56), dtype=torch.uint8, device=dev), grid=(2, 8))
    # 16 cells allow 50 shapes (gh * gw <= 16): all of them fit beside the native one, and come back from the cache
    shapes = [(gh, gw) for gh in range(1, 17) for gw in range(1, 17) if gh * gw <= 16 and (gh, gw) != (4, 4)]
    assert len(shapes) == 49
    for gh, gw in shapes + shapes[:5]:
        assert lib.revo_vit_set_grid(eng._h, gh, gw, st) == 0
        assert lib.revo_vit_seq_len(eng._h) == gh * gw + 1
    assert lib.revo_vit_set_grid(eng._h, 0, 0, st) == 0 and lib.revo_vit_seq_len(eng._h) == cfg.seq
    eng.close()
    # a tower with 196 cells has more than 64 shapes: the 65th is refused with a message, the handle keeps working
    b16 = dataclasses.replace(reverso_amd.get_config("PE-Core-B16-224"), layers=1)
    e2 = engine.VitEngine.synthetic(b16, seed=0, device=0, max_batch=1)
    n = 1
    for gw in range(1, 80):
        rc = e2._lib.revo_vit_set_grid(e2._h, 1, gw, st)
        if n < 64:
            assert rc == 0, (gw, e2._lib.revo_last_error())
            n += 1
        else:
            assert rc == -2 and "64 grid shapes" in e2._lib.revo_last_error().decode() and f"(1, {gw})" in e2._lib.revo_last_error().decode()
            break
    assert n == 64
    assert e2._lib.revo_vit_set_grid(e2._h, 1, 5, st) == 0 and e2._lib.revo_vit_seq_len(e2._h) == 6     # (a cached shape)
    assert e2._lib.revo_vit_set_grid(e2._h, 14, 14, st) == 0 and e2._lib.revo_vit_seq_len(e2._h) == 197
    e2.close()


# ---- 2. the native path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_the_native_path_is_untouched(dev, cname):
    cfg, sd = _tiny(cname)
    eng = _engines(cfg, sd, dev, 8, hooks=False)[0]
    G = cfg.grid
    u8 = gr.random_u8(5, cfg, None, 1).to(dev)
    ri = np.array([0, 4, 2, 2])
    bits = regions.token_masks(cfg, [(0, 0, 20, 56), (10, 10, 50, 30), (0, 0, 56, 56), (30, 0, 56, 56)], 56, 56)
    want = (eng.embed(u8), eng.embed_tokens(u8), eng.embed_regions(u8, ri, bits))

    def same():
        got = (eng.embed(u8, grid=(G, G)), eng.embed_tokens(u8, grid=(G, G)), eng.embed_regions(u8, ri, bits, grid=(G, G)))
        again = (eng.embed(u8), eng.embed_tokens(u8), eng.embed_regions(u8, ri, bits))
        for a, b, c in ((want[0], got[0], again[0]), (want[1][0], got[1][0], again[1][0]), (want[1][1], got[1][1], again[1][1]),
                        (want[2][0], got[2][0], again[2][0]), (want[2][1], got[2][1], again[2][1])):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert eng._lib.revo_vit_seq_len(eng._h) == cfg.seq
    same()
    wide = gr.random_u8(3, cfg, (2, 8), 2).to(dev)
    e = eng.embed(wide, grid=(2, 8))
    assert e.shape == (3, cfg.out_dim) and torch.isfinite(e).all()
    assert eng._lib.revo_vit_seq_len(eng._h) == cfg.seq                       # restored on the way out
    same()
    # whatever ends the frame restores the grid
    with pytest.raises(RuntimeError):
        with eng._grid_frame((5, 3)):
            assert eng._lib.revo_vit_seq_len(eng._h) == 15 + (1 if cfg.use_cls else 0)
            raise RuntimeError("inside the frame")
    assert eng._lib.revo_vit_seq_len(eng._h) == cfg.seq
    same()
    eng.close()


# ---- 3. the tiny towers end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(2, 8), (3, 5), (5, 3), (8, 2)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("cname", TINY)
def test_tiny_towers_on_every_menu_grid(dev, cname, grid):
    """f32 and u8 images, batch 3 and batch 32 (at 32, (2, 8) meets the band patchify's B * gh >= 64 with a width that is a
    multiple of 16; (8, 2), (3, 5) and (5, 3) take the gather forms): the embedded tokens, the residual stream after ln_pre
    and after every block, and the embedding against the fp64 reference."""
    cfg, sd = _seeded(cname)
    assert grid in gr.non_native_menu(cfg)
    eng, engx = _engines(cfg, sd, dev, 32)
    gal = _gallery(cfg.out_dim)
    for B in (3, 32):
        u8 = gr.random_u8(B, cfg, grid, B + grid[0])
        f32 = pe_vit.preprocess_u8(u8)
        taps = {}
        ref = pe_vit.l2_normalize(gr.encode_image(sd, cfg, f32, grid, taps=taps))
        embs = {}
        for kind, img in (("u8", u8.to(dev)), ("f32", f32.to(dev))):
            what = f"{cname} {grid} B={B} {kind}"
            _check_tap(engx.residual_after(img, -2, grid=grid), taps["embed"], what + " embed")
            _check_tap(engx.residual_after(img, 0, grid=grid), taps["ln_pre"], what + " ln_pre")
            for n in range(1, cfg.layers + 1):
                _check_tap(engx.residual_after(img, n, grid=grid), taps[f"block{n - 1}"], what + f" block{n - 1}")
            t = engx.taps(img, grid=grid)
            _check_tap(t["ln_post"], taps["ln_post"], what + " ln_post")
            _check_tap(t["pooled"], taps["pooled"], what + " pooled")
            embs[kind] = eng.embed(img, grid=grid)
            assert torch.equal(embs[kind], t["embedding"])                    # the product library: the same bits
            _check_embedding(embs[kind], ref, gal, what)
            if cfg.use_cls:      # the class row is exactly cls + pos[0]
                ref0 = (sd["visual.class_embedding"] + sd["visual.positional_embedding"][0]).to(dev)
                assert torch.equal(t["embed"][:, 0], ref0[None].expand(B, -1))
        d = (embs["u8"] - embs["f32"]).abs().max().item()
        assert d <= 1e-3 and ((embs["u8"] * embs["f32"]).sum(-1) >= 0.99999).all(), (cname, grid, B, d)
        if B == 32:          # rows of a batch do not depend on the batch: the first three alone give the same bits
            assert torch.equal(eng.embed(u8[:3].to(dev), grid=grid), embs["u8"][:3])
    eng.close()
    engx.close()


# ---- 4. B16-224, full depth -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def b16(dev):
    cfg = reverso_amd.get_config("PE-Core-B16-224")
    sd = weights.synth_weights(cfg, seed=0, randomize_affine=True, device=dev)
    engx = engine.VitEngine(cfg, sd, device=0, max_batch=64, experiments=True)
    yield cfg, sd, engx
    engx.close()


@pytest.mark.parametrize("grid", B16_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_b16_full_depth_on_the_attention_kernels_tile_edges(dev, b16, grid):
    """(7, 28): S' = 197, the native length with other tables; (12, 16): S' = 193 = 3 * 64 + 1, the class-key split; (13, 15):
    196; (9, 21): 190.  Batch 3, and batch 64 (up to 12 608 rows: the large-tile GEMM forms, the folded LayerNorm and the plane
    layout of the stream at a row count the native path never produces).  The fp64 reference runs on the device."""
    cfg, sd, engx = b16
    gal = _gallery(cfg.out_dim).to(dev)
    for B in (3, 64):
        u8 = gr.random_u8(B, cfg, grid, 7 * B + grid[0]).to(dev)
        taps = {}
        ref = pe_vit.l2_normalize(gr.encode_image(sd, cfg, pe_vit.preprocess_u8(u8), grid, taps=taps))
        what = f"B16 {grid} B={B}"
        _check_tap(engx.residual_after(u8, -2, grid=grid), taps["embed"], what + " embed")
        for n in (1, 6, 12):
            _check_tap(engx.residual_after(u8, n, grid=grid), taps[f"block{n - 1}"], what + f" block{n - 1}")
        emb = engx.embed(u8, grid=grid)
        emb, ref = emb.cpu().double(), ref.cpu()
        _check_embedding(emb, ref, gal.cpu(), what)
        del taps
    assert engx._lib.revo_vit_seq_len(engx._h) == cfg.seq


# ---- 5. the tables are wired in --------------------------------------------------------------------------------------------------
SHARPEN = 4.0


@pytest.mark.parametrize("grid", [(7, 28), (12, 16)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_sharpened_attention_tells_a_transposed_rotary_table(dev, grid):
    """B16-224 with the q and k rows of every in_proj_weight multiplied by SHARPEN: attention that depends on the rotary
    phases.  sep = min over images of 1 - cos(reference, reference with the RoPE axes swapped) must be at least 1e-2 (computed
    from the references alone), and the device embedding within sep / 10 of the right reference.
    Measured on an MI355X, (7, 28) / (12, 16): at SHARPEN = 8 sep 2.33e-2 / 1.93e-2 and the device at 1.94e-3 / 2.02e-3 of the
    right reference -- the bf16 body on attention that sharp, above sep / 10 on (12, 16); at 4, the scale used, sep 1.16e-2 /
    1.07e-2 and the device at 8.7e-6 / 7.9e-6 (1.16e-2 / 1.07e-2 from the swapped reference); at 2 sep 4.8e-4 / 2.2e-4, too
    small to tell the tables apart."""
    cfg = reverso_amd.get_config("PE-Core-B16-224")
    sd = weights.synth_weights(cfg, seed=0, randomize_affine=True, device=dev)
    W = cfg.width
    for k in list(sd):
        if k.endswith("attn.in_proj_weight") and "resblocks" in k:
            sd[k] = torch.cat([sd[k][:2 * W] * SHARPEN, sd[k][2 * W:]]).contiguous()
    u8 = gr.random_u8(3, cfg, grid, 31 + grid[0]).to(dev)
    f32 = pe_vit.preprocess_u8(u8)
    ref = gr.embed(sd, cfg, f32, grid)
    bad = gr.embed(sd, cfg, f32, grid, swap_axes=True)
    sep = (1 - (ref * bad).sum(-1)).min().item()
    eng = engine.VitEngine(cfg, sd, device=0, max_batch=4)
    emb = eng.embed(u8, grid=grid).double()
    err = (1 - (emb * ref).sum(-1)).max().item()
    wrong = (1 - (emb * bad).sum(-1)).min().item()
    print(f"sharpened x{SHARPEN} {grid}: sep {sep:.4e}, device 1 - cos to the right reference {err:.4e}, to the swapped one {wrong:.4e}")
    eng.close()
    assert sep >= 1e-2, sep
    assert err <= sep / 10, (err, sep)


# ---- 6. regions and tokens under a grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(2, 8), (5, 3)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_regions_and_tokens_under_a_grid(dev, cname, grid):
    import test_gpu_region_pool as rp
    cfg, sd = _tiny(cname)
    eng, engx = _engines(cfg, sd, dev, 4)
    gh, gw = grid
    first, S = (1 if cfg.use_cls else 0), gh * gw + (1 if cfg.use_cls else 0)
    B = 3
    u8 = gr.random_u8(B, cfg, grid, 17).to(dev)
    emb = eng.embed(u8, grid=grid)
    glob_t, tok = eng.embed_tokens(u8, grid=grid)
    assert tok.shape == (B, S, cfg.out_dim) and torch.equal(glob_t, emb)
    # per image: the full mask, one token, the top two rows as a box in source pixels, nothing
    width, height = 97, 41
    box = regions.token_masks(cfg, [(0, 0, width, height * 2 / gh)], width, height, grid=grid)[0]
    allow_box = np.zeros(S, bool)
    allow_box[first:first + 2 * gw] = True
    assert np.array_equal(box, rp._pack(allow_box[None])[0])                 # two rows of the grid, gw tokens each
    ri, allow, kind = [], [], []
    for b in range(B):
        one = np.zeros(S, bool)
        one[(5 * b + 3) % S] = True
        for name, a in (("full", np.ones(S, bool)), ("one", one), ("box", allow_box), ("empty", np.zeros(S, bool))):
            ri.append(b); allow.append(a); kind.append(name)
    ri, allow = np.asarray(ri), np.stack(allow)
    bits = rp._pack(allow)
    assert bits.shape[1] == regions.words_per_region(cfg, grid)
    assert np.array_equal(bits[0], regions.full_mask(cfg, grid=grid))
    glob, reg = eng.embed_regions(u8, ri, bits, grid=grid)
    assert torch.equal(glob, emb)
    tap = engx.taps(u8, grid=grid)["ln_post"].cpu()
    assert torch.equal(engx.embed(u8, grid=grid), emb)
    keep = [r for r, k in enumerate(kind) if k != "empty"]
    ref_r = pe_vit.l2_normalize(rp.masked_head(sd, cfg, tap[ri[keep]], allow[keep]))
    ref_g = pe_vit.l2_normalize(rp.masked_head(sd, cfg, tap, np.ones((B, S), bool)))
    e_g = (emb.cpu().double() - ref_g).abs().max().item()
    for j, r in enumerate(keep):
        if kind[r] == "full":
            assert torch.equal(reg[r], emb[ri[r]]), r
        elif kind[r] == "one":
            assert torch.equal(reg[r], tok[ri[r], int(np.flatnonzero(allow[r])[0])]), r
        else:        # the bar of test_region_head_against_the_fp64_head_of_the_same_rows: 4 x the global vectors' error
            e = (reg[r].cpu().double() - ref_r[j]).abs().max().item()
            print(f"{cname} {grid} box region of image {ri[r]}: {e:.3e} (global vectors {e_g:.3e})")
            assert e <= 4 * e_g, (r, e, e_g)
            # (on (2, 8) without a class token two rows are the whole grid: the full mask again)
            assert torch.equal(reg[r], emb[ri[r]]) == bool(allow_box.all())
    for r, k in enumerate(kind):
        if k == "empty":
            assert torch.equal(reg[r], torch.zeros_like(reg[r]))
    # end to end: the un-normalised box features against the fp64 reference's ln_post rows through the fp64 masked head, at the
    # bound test_region_features_end_to_end_against_the_cpu_oracle holds them to
    taps = {}
    gr.encode_image(sd, cfg, pe_vit.preprocess_u8(u8.cpu()), grid, taps=taps)
    boxes = [r for r, k in enumerate(kind) if k == "box"]
    want = rp.masked_head(sd, cfg, taps["ln_post"][ri[boxes]], allow[boxes])
    _, un = eng.embed_regions(u8, ri[boxes], bits[boxes], normalize=False, with_global=False, grid=grid)
    err, bound = (un.cpu().double() - want).abs().max().item(), 3e-2 * want.abs().max().item()
    print(f"{cname} {grid}: max |box feature - fp64 reference| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    eng.close()
    engx.close()


# ---- 7. detect -------------------------------------------------------------------------------------------------------------------
def test_detect_is_refused_under_a_grid_and_works_again_after(dev):
    cfg, sd = _tiny("PE-Tiny-T14-56")
    eng = _engines(cfg, sd, dev, 4, hooks=False)[0]
    u8 = gr.random_u8(2, cfg, None, 41).to(dev)
    prompts = torch.randn((3, cfg.out_dim), generator=torch.Generator().manual_seed(42)).to(dev)
    before = eng.detect(u8, prompts, n_background=1, max_regions=16, with_maps=True, with_global=True)
    assert len(before) > 0
    st = _lib.current_stream()
    assert eng._lib.revo_vit_set_grid(eng._h, 2, 8, st) == 0
    try:
        with pytest.raises(_lib.RevoError) as e:
            eng.detect(u8, prompts, n_background=1, max_regions=16)
        assert "(2, 8)" in str(e.value) and "native grid" in str(e.value)
        assert eng._lib.revo_vit_detect_read(eng._h, 0, 1, None, None, None, None, None, None, None, 0) == -2   # no result either
    finally:
        assert eng._lib.revo_vit_set_grid(eng._h, 0, 0, st) == 0
    after = eng.detect(u8, prompts, n_background=1, max_regions=16, with_maps=True, with_global=True)
    for f in dataclasses.fields(engine.Detections):
        assert torch.equal(getattr(before, f.name), getattr(after, f.name)), f.name
    eng.close()


# ---- 8. the resize ---------------------------------------------------------------------------------------------------------------
def _pil(img, oh, ow, box):
    p = Image.fromarray(img)
    if box is not None:
        p = p.crop(box)
    return np.asarray(p.resize((ow, oh), Image.BILINEAR)).transpose(2, 0, 1)


@pytest.mark.parametrize("oh,ow", [(28, 112), (112, 28), (70, 42), (56, 56)])
def test_crop_resize_to_a_rectangle_matches_pillow(dev, oh, ow):
    rng = np.random.default_rng(oh)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((37, 211), (640, 480), (1, 1))]
    frames = [torch.from_numpy(i).to(dev) for i in imgs]
    out = preprocess.crop_resize_device(frames, None, (oh, ow))
    assert out.shape == (3, 3, oh, ow)
    for i in range(3):
        assert np.array_equal(out[i].cpu().numpy(), _pil(imgs[i], oh, ow, None)), i
    # boxes: wide slivers, tall slivers, single pixels -- up- and downscaling on each axis
    boxes = [(0, 3, 1, 200, 30), (0, 100, 0, 104, 37), (0, 0, 0, 211, 37), (0, 210, 36, 211, 37), (1, 0, 0, 480, 20),
             (1, 7, 9, 30, 600), (1, 100, 100, 400, 500), (1, 479, 0, 480, 640), (2, 0, 0, 1, 1), (1, 13, 17, 14, 630)]
    for _ in range(20):
        fi = int(rng.integers(0, 2))
        H, W = imgs[fi].shape[:2]
        x0, y0 = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
        boxes.append((fi, x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))))
    out = preprocess.crop_resize_device(frames, boxes, (oh, ow)).cpu().numpy()
    for i, (fi, x0, y0, x1, y1) in enumerate(boxes):
        assert np.array_equal(out[i], _pil(imgs[fi], oh, ow, (x0, y0, x1, y1))), (i, boxes[i])
    if oh == ow:      # the square call: the same bytes through the int, the pair and the rectangular entry point itself
        sq = preprocess.crop_resize_device(frames, boxes, oh)
        assert np.array_equal(sq.cpu().numpy(), out)
        jobs = (_lib.CropJob * len(boxes))()
        for i, (fi, x0, y0, x1, y1) in enumerate(boxes):
            f = frames[fi]
            jobs[i].src, jobs[i].height, jobs[i].width, jobs[i].row_stride = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
            jobs[i].x0, jobs[i].y0, jobs[i].x1, jobs[i].y1 = x0, y0, x1, y1
        hw = torch.zeros_like(sq)
        _lib.check(_lib.load().revo_preprocess_crop_resize_hw(jobs, len(boxes), oh, ow, _lib.ptr(hw), _lib.current_stream()), "hw")
        torch.cuda.synchronize()
        assert torch.equal(hw, sq)
