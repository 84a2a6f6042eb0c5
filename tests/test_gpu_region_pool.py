"""Region embeddings from one forward: the masked pooling kernel against fp64 and bit for bit against
the unmasked kernel; the region head of revo_vit_forward_regions against the fp64 head of the same ln_post rows, held to
the error of the existing global vectors; end to end against the CPU oracle's head restricted to the region's tokens;
3 200 regions in one call; the facade's `pool` mode."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_bounds as hb
import reverso_amd
from reverso_amd import _lib, engine, regions, weights
from oracle import pe_vit

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden  # noqa: E402


# ------------------------------------------------------------------ helpers ----
def _pack(allow):
    """bool [R, S] -> int32 device-ready bitmap rows (bit s & 31 of word s >> 5)"""
    a = np.asarray(allow, dtype=bool)
    R, S = a.shape
    words = (S + 31) // 32
    pad = np.zeros((R, words * 32), dtype=np.uint64)
    pad[:, :S] = a
    return (pad.reshape(R, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _bits_t(bits_u32, dev):
    return torch.from_numpy(np.ascontiguousarray(bits_u32).view(np.int32)).to(dev)


def _pool_masked(lib, x, logits, ri, bits, B, S, W, H):
    R = ri.shape[0]
    u = torch.full((R, H, W), float("nan"), device=x.device)
    _lib.check(lib.revo_op_pool_rows_masked(_lib.ptr(x), W, _lib.ptr(logits), _lib.ptr(ri), _lib.ptr(bits), R, B, S, W, H,
                                            _lib.ptr(u), _lib.current_stream()), "revo_op_pool_rows_masked")
    torch.cuda.synchronize()
    return u


def masked_head(sd, cfg, x, allow, dtype=torch.float64):
    """oracle.pe_vit.attn_pool with -inf on the disallowed logits, then visual.proj: x [n, S, W] ln_post rows, allow bool
    [n, S].  Returns the un-normalised features [n, D]."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if k.startswith("visual.attn_pool.") or k == "visual.proj"}
    x = x.detach().cpu().to(dtype)
    n, S, W = x.shape
    H = cfg.pool_heads
    hd = W // H
    pre = "visual.attn_pool."
    wi, bi = p[pre + "attn.in_proj_weight"], p[pre + "attn.in_proj_bias"]
    probe = p[pre + "probe"].reshape(1, 1, W).expand(n, 1, W)
    q = F.linear(probe, wi[:W], bi[:W]).reshape(n, 1, H, hd).transpose(1, 2)
    k = F.linear(x, wi[W:2 * W], bi[W:2 * W]).reshape(n, S, H, hd).transpose(1, 2)
    v = F.linear(x, wi[2 * W:], bi[2 * W:]).reshape(n, S, H, hd).transpose(1, 2)
    lg = (q @ k.transpose(-1, -2)) * (hd ** -0.5)                                    # [n, H, 1, S]
    lg = lg.masked_fill(~torch.as_tensor(allow, dtype=torch.bool)[:, None, None, :], float("-inf"))
    att = torch.softmax(lg, dim=-1)
    o = (att @ v).transpose(1, 2).reshape(n, 1, W)
    o = F.linear(o, p[pre + "attn.out_proj.weight"], p[pre + "attn.out_proj.bias"])
    h = pe_vit.layer_norm(o, p[pre + "layernorm.weight"], p[pre + "layernorm.bias"], cfg.ln_eps)
    o = o + pe_vit.mlp(h, p, pre + "mlp.")
    return o[:, 0] @ p["visual.proj"]


def _tower_regions(cfg, B, seed):
    """the regions of the whole-forward tests, per image: full, patches only, one token, a 2 x 2 block, a random half, the
    class token alone (where there is one).  Returns (region_image [R], allow bool [R, S], kind [R])."""
    g, S, first = cfg.grid, cfg.seq, 1 if cfg.use_cls else 0
    rng = np.random.default_rng(seed)
    ri, allow, kind = [], [], []
    for b in range(B):
        def add(name, a):
            ri.append(b); allow.append(a); kind.append(name)
        a = np.ones(S, bool); add("full", a)
        a = np.ones(S, bool); a[:first] = False; add("patches", a)
        a = np.zeros(S, bool); a[first + int(rng.integers(0, g * g))] = True; add("one", a)
        a = np.zeros(S, bool)
        gy, gx = int(rng.integers(0, g - 1)), int(rng.integers(0, g - 1))
        for dy in (0, 1):
            for dx in (0, 1):
                a[first + (gy + dy) * g + gx + dx] = True
        add("block", a)
        a = np.zeros(S, bool); a[first + rng.permutation(g * g)[: g * g // 2]] = True; add("half", a)
        if cfg.use_cls:
            a = np.zeros(S, bool); a[0] = True; add("cls", a)
    return np.asarray(ri, dtype=np.int64), np.stack(allow), kind


# ------------------------------------------------------------------ the kernel ----
@pytest.mark.parametrize("B,S,W,H,R", [(3, 577, 1024, 8, 40), (2, 17, 128, 2, 9), (2, 1024, 1536, 8, 12), (4, 197, 768, 8, 200)])
def test_masked_pool_rows_against_fp64_and_bit_for_bit_against_the_unmasked_kernel(dev, B, S, W, H, R):
    """revo_op_pool_rows_masked (region_pool.hip) with the inputs of test_pool_rows_equal_the_softmax_weighted_sum...: within
    that test's 2e-5 of the fp64 masked-softmax sums (a masked sum is a convex combination of the same rows), and exactly:
    a full mask = revo_op_pool_rows; a one-token region = that token's row for every head; bits past S, NaN in every
    disallowed row and logit, the other regions of the call, their order and their number change no byte; an empty
    region is zeros.  (4, 197, 768, 8, 200) takes the four-column form, single regions of it the one-column form.)"""
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S)
    x = torch.randn(B * S, W, generator=g).to(dev)
    logits = (torch.randn(B, H, S, generator=g) * 2).to(dev)
    rng = np.random.default_rng(S + R)
    words = (S + 31) // 32
    allow = np.zeros((R, S), dtype=bool)
    ri = rng.integers(0, B, R)                               # non-monotone image indices
    for r in range(R):
        allow[r] = rng.random(S) < rng.choice([0.03, 0.2, 0.5, 0.9])
    FULL, TOK0, LAST, EMPTY, FULL_PAD = 0, 1, 2, 3, 4
    ri[FULL], ri[TOK0], ri[LAST], ri[EMPTY], ri[FULL_PAD] = B - 1, 0, B - 1, 0, B - 1
    allow[FULL] = True
    allow[TOK0] = False; allow[TOK0, 0] = True
    allow[LAST] = False; allow[LAST, S - 1] = True          # S = 577: the lone bit of the last word
    allow[EMPTY] = False
    allow[FULL_PAD] = True
    bits = _pack(allow)
    if S % 32:
        bits[FULL_PAD, words - 1] = 0xFFFFFFFF               # bits at and past S
        bits[EMPTY, words - 1] = np.uint32(0xFFFFFFFF) << np.uint32(S % 32)     # ... and only those: still empty
    ri_t = torch.from_numpy(ri.astype(np.int32)).to(dev)
    u = _pool_masked(lib, x, logits, ri_t, _bits_t(bits, dev), B, S, W, H)

    # fp64 masked-softmax sums
    al = torch.from_numpy(allow).to(dev)
    lg = logits.double()[ri_t.long()].masked_fill(~al[:, None, :], float("-inf"))
    p = torch.nan_to_num(torch.softmax(lg, dim=-1), nan=0.0)                        # (the empty region: no term)
    ref = torch.einsum("rhs,rsw->rhw", p, x.double().view(B, S, W)[ri_t.long()])
    err = (u.double() - ref).abs().max().item()
    print(f"masked pool rows B={B} S={S} W={W} H={H} R={R}: max |u - fp64| = {err:.3e}")
    assert err <= 2e-5
    xs, masked = x.view(B, S, W), (ri_t.long(), al)
    assert hb.ratio(u, hb.PoolRows.reference(xs, logits, masked), hb.PoolRows.bound(xs, logits, masked)) <= 1.0

    # exact
    u_all = torch.zeros(B, H, W, device=dev)
    _lib.check(lib.revo_op_pool_rows(_lib.ptr(x), W, _lib.ptr(logits), B, S, W, H, _lib.ptr(u_all), _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(u[FULL], u_all[B - 1])
    assert torch.equal(u[FULL_PAD], u_all[B - 1])
    for h in range(H):
        assert torch.equal(u[TOK0, h], x[0 * S + 0]), h
        assert torch.equal(u[LAST, h], x[(B - 1) * S + S - 1]), h
    assert torch.equal(u[EMPTY], torch.zeros(H, W, device=dev)) and not torch.isnan(u).any()

    # permuted and duplicated in another call
    perm = np.concatenate([rng.permutation(R), rng.integers(0, R, 7)])
    u2 = _pool_masked(lib, x, logits, ri_t[perm], _bits_t(bits[perm], dev), B, S, W, H)
    assert torch.equal(u2, u[perm])

    # alone in a call, NaN in every row and logit the region does not allow (its image's and the other images')
    for r in [TOK0, LAST, FULL_PAD] + [int(v) for v in rng.choice(np.arange(5, R), 3, replace=False)]:
        b = int(ri[r])
        keep = torch.zeros(B, S, dtype=torch.bool, device=dev)
        keep[b] = al[r]
        xn = torch.where(keep.view(B * S, 1), x, torch.full_like(x, float("nan")))
        ln = torch.where(keep[:, None, :], logits, torch.full_like(logits, float("nan")))
        u1 = _pool_masked(lib, xn, ln, ri_t[r:r + 1], _bits_t(bits[r:r + 1], dev), B, S, W, H)
        assert torch.equal(u1[0], u[r]), r


# ------------------------------------------------------- the head, on the product's own ln_post rows ----
def _towers():
    out = []
    for cname in ("PE-Tiny-T14-56", "PE-Tiny-N14-56"):
        cfg, sd, images = make_golden.tiny_case(cname)
        out.append((cname, cfg, sd, images))
    cfg = reverso_amd.get_config("PE-Core-B16-224")
    sd = weights.synth_weights(cfg, seed=0, randomize_affine=True)
    g = torch.Generator().manual_seed(224)
    out.append(("PE-Core-B16-224", cfg, sd, torch.randint(0, 256, (3, 3, 224, 224), generator=g, dtype=torch.uint8)))
    return out


@pytest.mark.parametrize("which", [0, 1, 2], ids=["PE-Tiny-T14-56", "PE-Tiny-N14-56", "PE-Core-B16-224"])
def test_region_head_against_the_fp64_head_of_the_same_rows(dev, which):
    """The head, isolated from the body's bf16 error: the fp32 ln_post rows of the forward (the experiment library's tap;
    the product engine gives the same bits) go through the fp64 head with the softmax restricted to the region's tokens;
    every region vector of embed_regions must be within 4 x the error the existing global vectors have against the same
    fp64 head (a small region's softmax averages over fewer terms; the five GEMMs behind it are the same arithmetic).
    Measured on an MI355X (max |d| of unit vectors): T14 e_g 1.24e-7, worst region 1.24e-7; N14 8.43e-8 /
    8.43e-8; B16 at batch 3 4.34e-8 / 4.48e-8."""
    cname, cfg, sd, images = _towers()[which]
    dsd = {k: v.to(dev) for k, v in sd.items()}
    eng = engine.VitEngine(cfg, dsd, device=0, max_batch=4)
    engx = engine.VitEngine(cfg, dsd, device=0, max_batch=4, experiments=True)
    img = images.to(dev)
    B = img.shape[0]
    emb = eng.embed(img)
    assert torch.equal(engx.embed(img), emb)
    tap = engx.taps(img)["ln_post"].cpu()                                             # [B, S, W]
    ri, allow, kind = _tower_regions(cfg, B, seed=which)
    bits = _pack(allow)
    glob, reg = eng.embed_regions(img, ri, bits)
    assert torch.equal(glob, emb)                                                     # out_global = embed, bit for bit
    for r, name in enumerate(kind):
        if name == "full":
            assert torch.equal(reg[r], emb[ri[r]]), r                                 # the full mask = the global vector
    # device bitmaps, no global output, a permuted order: the same bytes
    perm = np.random.default_rng(which).permutation(len(ri))
    none, reg2 = eng.embed_regions(img, ri[perm], _bits_t(bits[perm], dev), with_global=False)
    assert none is None and torch.equal(reg2, reg[perm])

    ref_g = pe_vit.l2_normalize(masked_head(sd, cfg, tap, np.ones((B, cfg.seq), bool)))
    e_g = (emb.cpu().double() - ref_g).abs().max().item()
    ref_r = pe_vit.l2_normalize(masked_head(sd, cfg, tap[ri], allow))
    e_r = (reg.cpu().double() - ref_r).abs().amax(dim=1)
    worst = int(e_r.argmax())
    print(f"{cname}: e_g = {e_g:.3e}, worst region error = {e_r.max().item():.3e} ({kind[worst]}), "
          f"ratio {e_r.max().item() / e_g:.2f}")
    assert e_r.max().item() <= 4 * e_g, (cname, e_g, e_r.max().item(), kind[worst])
    # un-normalised output and zeros for an empty region (not normalised: no NaN)
    empty = np.zeros((1, cfg.seq), bool)
    _, z = eng.embed_regions(img, [B - 1], _pack(empty), with_global=False)
    assert torch.equal(z, torch.zeros_like(z))
    _, un = eng.embed_regions(img, ri, bits, normalize=False, with_global=False)
    assert (F.normalize(un.double(), dim=-1) - reg.double()).abs().max().item() <= 1e-6      # (fp32 roundings of the division)
    eng.close()
    engx.close()


@pytest.mark.parametrize("cname", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_region_features_end_to_end_against_the_cpu_oracle(dev, cname):
    """Whole forward against the fp32 CPU oracle restated for a region (its ln_post rows through attn_pool with the softmax
    restricted to the region's tokens, then visual.proj): un-normalised region features within 3e-2 x max |ref|, the bound
    test_tiny_vit_layer_by_layer holds the `proj` tap to -- and every region but the full one further than that from its
    image's global vector (a forward that ignored the mask would not pass)."""
    cfg, sd, images = make_golden.tiny_case(cname)
    eng = engine.VitEngine(cfg, {k: v.to(dev) for k, v in sd.items()}, device=0, max_batch=4)
    B, g, S, first = images.shape[0], cfg.grid, cfg.seq, 1 if cfg.use_cls else 0
    rng = np.random.default_rng(7)
    ri, allow, full = [], [], []
    for b in range(B):
        a = np.ones(S, bool); ri.append(b); allow.append(a); full.append(True)
        a = np.zeros(S, bool)                                                          # a 2 x 2 block
        gy, gx = int(rng.integers(0, g - 1)), int(rng.integers(0, g - 1))
        for dy in (0, 1):
            for dx in (0, 1):
                a[first + (gy + dy) * g + gx + dx] = True
        ri.append(b); allow.append(a); full.append(False)
        a = np.zeros(S, bool); a[first + rng.permutation(g * g)[:5]] = True            # five scattered tokens
        ri.append(b); allow.append(a); full.append(False)
        a = np.zeros(S, bool); a[first + b % g * g: first + b % g * g + g] = True       # one row of the grid
        ri.append(b); allow.append(a); full.append(False)
    ri, allow = np.asarray(ri), np.stack(allow)
    with torch.no_grad():
        taps = {}
        pe_vit.encode_image(sd, cfg, images, taps)
        ref = masked_head(sd, cfg, taps["ln_post"][ri], allow, dtype=torch.float32)
    bound = 3e-2 * ref.abs().max().item()
    glob, got = eng.embed_regions(images.to(dev), ri, _pack(allow), normalize=False)
    err = (got.cpu() - ref).abs().max().item()
    print(f"{cname}: max |region feature - oracle| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    for r in range(len(ri)):
        d = (got[r] - glob[ri[r]]).abs().max().item()
        if full[r]:
            assert d == 0.0
        else:
            assert d > bound, (r, d, bound)
    eng.close()


# ------------------------------------------------------------------ scale ----
def test_3200_regions_in_one_call_chunks_and_memory(dev):
    """PE-Core-L14-336 (synthetic), 64 images, 50 regions each in one call (seven passes of the region head), with host and
    with device bitmaps: the same bytes twice; full-mask rows = embed; a region's bytes do not depend on the other regions
    of the call; device memory does not grow across calls."""
    cfg = reverso_amd.get_config("PE-Core-L14-336")
    eng = engine.VitEngine.synthetic(cfg, seed=0, device=0, max_batch=64)
    g = torch.Generator().manual_seed(64)
    u8 = torch.randint(0, 256, (64, 3, 336, 336), generator=g, dtype=torch.uint8).to(dev)
    rng = np.random.default_rng(50)
    B, per, S = 64, 50, cfg.seq
    ri = np.tile(np.arange(B), per)                          # region r belongs to image r % 64: every chunk mixes images
    allow = rng.random((B * per, S)) < rng.choice([0.02, 0.1, 0.5, 0.95], size=(B * per, 1))
    allow[:B] = True                                         # the first region of every image: the full mask
    allow[B:2 * B] = False
    allow[np.arange(B, 2 * B), rng.integers(0, S, B)] = True  # the second: one token
    bits = _pack(allow)
    emb = eng.embed(u8)
    glob, a = eng.embed_regions(u8, ri, bits)
    _, b = eng.embed_regions(u8, ri, bits, with_global=False)
    _, c = eng.embed_regions(u8, ri, _bits_t(bits, dev), with_global=False)
    assert torch.equal(glob, emb) and torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a[:B], emb)
    assert torch.isfinite(a).all() and ((a.norm(dim=-1) - 1).abs() <= 1e-5).all()
    # the regions of one image alone (one pass instead of seven, other neighbours), the same 64 images in the batch
    mine = np.nonzero(ri == 17)[0]
    _, d = eng.embed_regions(u8, ri[mine], bits[mine], with_global=False)
    assert torch.equal(d, a[mine])
    # the handle's region workspace is allocated once (test_gpu_embed.py test_handles_release_device_memory's method)
    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free
    torch.cuda.synchronize()
    base = used()
    alloc0 = torch.cuda.memory_allocated()
    for _ in range(5):
        _, e = eng.embed_regions(u8, ri, bits, with_global=False)
        del e
    torch.cuda.synchronize()
    assert used() - base <= 8 << 20 and torch.cuda.memory_allocated() - alloc0 <= 0, (used() - base, torch.cuda.memory_allocated() - alloc0)
    eng.close()


# ------------------------------------------------------------------ facade ----
def _make_jpegs(folder, n, seed):
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i in range(n):
        w, h = int(rng.integers(90, 160)), int(rng.integers(80, 140))
        arr = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        im = Image.fromarray(arr)
        d = ImageDraw.Draw(im)
        for _ in range(3):
            x0, y0 = int(rng.integers(0, w - 20)), int(rng.integers(0, h - 20))
            d.ellipse([x0, y0, x0 + int(rng.integers(10, 60)), y0 + int(rng.integers(10, 60))],
                      fill=tuple(int(v) for v in rng.integers(0, 256, 3)))
        p = os.path.join(folder, f"img_{i:03d}.jpg")
        im.save(p, quality=92)
        paths.append(p)
    return paths


def _three_masks(w, h):
    masks = np.zeros((3, h, w), dtype=bool)
    masks[0, : h // 2, : w // 2] = True                                       # a quadrant
    yy, xx = np.mgrid[0:h, 0:w]
    masks[1] = (xx - 0.7 * w) ** 2 + (yy - 0.6 * h) ** 2 <= (0.25 * min(w, h)) ** 2      # a disc
    masks[2] = (xx + yy) > 0.8 * (w + h) / 1.0 * 0.9                          # a corner triangle
    return masks


def test_facade_pool_mode(tmp_path, dev):
    from PIL import Image
    from reverso_amd import preprocess as pp
    from reverso_amd.core_system import Regions, SimpleReverso
    folder = str(tmp_path / "images")
    paths = _make_jpegs(folder, n=8, seed=3)

    def detector(pil, prompt):
        w, h = pil.size
        return Regions([[0, 0, w // 2, h // 2], [w // 3, h // 3, w - 1, h - 1], [w // 2, h // 2, w - 1, h - 1]],
                       mask=_three_masks(w, h), confidence=[0.9, 0.8, 0.7], class_id=[0, 1, 0], class_names=["person", "car"])

    def detector_no_masks(pil, prompt):
        w, h = pil.size
        return Regions([[0, 0, w // 2, h // 2], [w // 3, h // 3, w - 1, h - 1]], mask=None, confidence=[0.9, 0.8])

    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8, detector=detector,
                      region_mode="pool")
    cfg = r.pe_model.cfg
    assert r.detect_regions(paths[0], "person . car") == 3
    embs, metas = r.extract_embeddings(paths[0])
    pil = Image.open(paths[0]).convert("RGB")
    w, h = pil.size
    u8 = pp.resize_u8(pil, cfg.image_size)[None].to(dev)
    bits = regions.token_masks(cfg, list(_three_masks(w, h)), w, h)
    glob, want = r.pe_model.embed_regions(u8, [0, 0, 0], bits)
    assert len(embs) == 3 and torch.equal(torch.stack(embs), want.cpu())
    assert torch.unique(want, dim=0).shape[0] == 3 and not any(torch.equal(want[i], glob[0]) for i in range(3))
    # metadata is _region_metadata's
    r.detect_regions(paths[0], "person . car")
    _, metas_ref = r._region_metadata(pil, r.detected_regions)
    strip = lambda ms: [{k: v for k, v in m.items() if k != "region_id"} for m in ms]
    assert strip(metas) == strip(metas_ref) and metas[0]["mask_status"] == "processed"

    msg = r.create_database(folder, "pooled", text_prompt="person . car")
    assert "✅" in msg and len(r.vector_db.payloads) == 24 and len(r.vector_db) == 24
    assert r.vector_db.build_info["region_mode"] == "pool"            # the manifest records the mode
    stored = r.vector_db.gallery.read().cpu()
    assert torch.unique(stored, dim=0).shape[0] == 24
    # a region's own vector finds that region first
    for q, which in ((paths[0], 0), (paths[5], 0)):
        r.detect_regions(q, "person . car")
        embs, metas = r.extract_embeddings(q)
        _, items = r.search_similar(0.0, 1)
        assert items[0]["filename"] == os.path.basename(q) and items[0]["bbox"] == metas[which]["bbox"]
        assert abs(items[0]["score"] - 1.0) <= 1e-6, items[0]["score"]

    # a region without a mask: every token, class token included = the image's global vector, bit for bit
    r.detector = detector_no_masks
    assert r.detect_regions(paths[1]) == 2
    embs, metas = r.extract_embeddings(paths[1])
    pil1 = Image.open(paths[1]).convert("RGB")
    want = r.pe_model.embed(pp.resize_u8(pil1, cfg.image_size)[None].to(dev))[0].cpu()
    assert len(embs) == 2 and torch.equal(embs[0], want) and torch.equal(embs[1], want)
    assert metas[0]["mask_status"] == "missing_or_unavailable"

    # the global mode is what it was: every region stores embed() of its frame
    rg_ = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db_global"), max_batch=8, detector=detector)
    assert rg_.region_mode == "global"
    msg = rg_.create_database(folder, "glob", text_prompt="person . car")
    assert "✅" in msg and len(rg_.vector_db) == 24
    frames = torch.stack([pp.resize_u8(Image.open(p).convert("RGB"), cfg.image_size) for p in sorted(paths)]).to(dev)
    e = rg_.pe_model.embed(frames)
    gal = engine.Gallery(cfg.out_dim, 64, device=0)
    gal.add(e.repeat_interleave(3, dim=0))
    assert torch.equal(rg_.vector_db.gallery.read(), gal.read())
    gal.close()
