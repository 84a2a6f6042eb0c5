"""The patch embedding -- patchify (both forms), the (hi | lo | hi) weight split, the split-precision patch GEMM with the
EPI_PATCH epilogue, the position add and the class-token rows -- against fp64, element by element (tests/_kernel_bounds.py
PatchEmbed), in every launch form the patch GEMM can take: kb.PATCH_FORM_CASES.

Each case is one front-end-only forward on librevo_exp.so (VitEngine.residual_after(images, -2) returns before ln_pre) of a
one-layer tower with the real front-end shape.  It asserts the exact launch form of the patch GEMM (revo_debug_gemm_forms),
holds EVERY element of the [B, S, W] tokens to its bound (the reference is fp64 on the GPU, in row chunks), the class rows
to the fp32 sum bit for bit, and a second identical call to the same bits.  uint8 and fp32 images, random and coherent
weights (kb.patch_weights: with the coherent ones a dropped low part is 13 to 29 times the bound), an fp32 image with special
values.  The largest |got - ref| / bound of each case is printed."""
import dataclasses
import os
import time

import pytest
import torch

import _kernel_bounds as kb
import reverso_amd
from reverso_amd import _lib, engine, weights

pytestmark = pytest.mark.gpu

CONFIGS = {"T14-56": "PE-Tiny-T14-56", "N14-56": "PE-Tiny-N14-56", "B16": "PE-Core-B16-224", "L14": "PE-Core-L14-336",
           "G14": "PE-Core-G14-448"}
CHUNK_ELEMS = 1 << 24                  # rows per fp64 chunk: CHUNK_ELEMS / max(W, parts Kp)


@pytest.fixture(scope="module")
def engines(dev):
    """one handle per (tower, weights), created on first use with the largest batch of its cases: every smaller case is a
    batch below the handle's max_batch"""
    made = {}

    def get(tower, fixture):
        wfix = "coherent" if fixture == "coherent" else "random"
        if (tower, wfix) not in made:
            cfg = dataclasses.replace(reverso_amd.get_config(CONFIGS[tower]), layers=1)
            t = kb.PATCH_TOWERS[tower]
            assert (cfg.image_size, cfg.patch_size, cfg.width, cfg.use_cls) == (t["image"], t["P"], t["W"], t["cls"])
            sd = weights.synth_weights(cfg, seed=11, device=dev, randomize_affine=True)
            w, pos, cls = kb.patch_weights(tower, wfix, seed=len(tower) + t["W"], device=dev)
            sd["visual.conv1.weight"], sd["visual.positional_embedding"] = w, pos
            if cls is not None:
                sd["visual.class_embedding"] = cls
            mb = max(c[3] for c in kb.PATCH_FORM_CASES if c[0] == tower and (c[1] == "coherent") == (wfix == "coherent"))
            made[(tower, wfix)] = (engine.VitEngine(cfg, sd, device=0, max_batch=mb, experiments=True), w, pos, cls)
        return made[(tower, wfix)]

    yield get
    for eng, *_ in made.values():
        eng.close()


@pytest.mark.parametrize("case", kb.PATCH_FORM_CASES, ids=[kb.patch_case_id(c) for c in kb.PATCH_FORM_CASES])
def test_patch_embed_within_bound(engines, dev, case):
    tower, fixture, u8, B, gather, want = case
    t0 = time.time()
    eng, w, pos, cls = engines(tower, fixture)
    assert B <= eng.max_batch
    images = kb.patch_images(tower, fixture, u8, B, seed=B, device=dev)
    xlib = _lib.load_exp()
    if gather:
        os.environ["REVO_PATCHIFY_GATHER"] = "1"
    try:
        torch.cuda.synchronize()
        xlib.revo_debug_gemm_forms(1)
        got = eng.residual_after(images, -2)
        torch.cuda.synchronize()
        forms = kb.form_names(xlib.revo_debug_gemm_forms(1))
        again = eng.residual_after(images, -2)
        torch.cuda.synchronize()
    finally:
        if gather:
            del os.environ["REVO_PATCHIFY_GATHER"]
    t_run = time.time() - t0
    c = kb.PatchCase(w, pos, cls, images)
    assert got.shape == (B, c.S, c.W)
    assert forms == [want], f"launch forms {forms}, expected {[want]}"
    assert want == kb.patch_gemm_form(c.M, c.W, (2 if u8 else 3) * c.Kp)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "a second run changed the tokens"
    if cls is not None:
        assert torch.equal(got[:, 0, :], kb.PatchEmbed.class_rows(c)[None].expand(B, c.W)), "class rows != fp32(cls + pos[0])"
    t1 = time.time()
    tok = c.tokens(got)
    P = kb.PatchEmbed
    step = max(64, CHUNK_ELEMS // max(c.W, (2 if u8 else 3) * c.Kp))
    worst, err2, ref2 = 0.0, 0.0, 0.0
    for r0 in range(0, c.M, step):
        r1 = min(c.M, r0 + step)
        ref = P.reference(c, r0, r1)
        worst = max(worst, kb.ratio(tok[r0:r1], ref, P.bound(c, r0, r1)))
        err2 += float(((tok[r0:r1].double() - ref) ** 2).sum())
        ref2 += float((ref ** 2).sum())
    rel = (err2 / ref2) ** 0.5
    band = "band" if kb.patch_band(tower, u8, B, gather) else "gather"
    print(f"[patch embed {kb.patch_case_id(case)}] {band} patchify, form {want}: max |got - ref| / bound = {worst:.3f}; "
          f"relative L2 error {rel:.3g} = 2^{torch.log2(torch.tensor(rel)).item():.1f} (patchify_kernel's comment: ~2^-16); "
          f"run {t_run:.2f} s, fp64 check {time.time() - t1:.2f} s")
    assert worst <= 1.0, (kb.patch_case_id(case), worst)
