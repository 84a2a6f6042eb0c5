"""GPU: the Python model of tower.h body_blocks (kb.body_gemm_launches), from which tests/test_gemm_form_coverage.py
enumerates the GEMM launches the towers make, against the forward itself.

Each tower at its real widths, cut to two blocks (block 0, a fc2 with a LayerNorm behind it, the last fc2: the model passes
through every state in two blocks, test_gemm_form_coverage.py), runs one forward on librevo_exp.so; the launch forms the
launcher recorded (revo_debug_gemm_forms) must be the union of the form bits the model plans for that tower and row count
-- for the image tower with the patch embedding's GEMM, which goes through the same launcher."""
import dataclasses

import numpy as np
import pytest
import torch

import _kernel_bounds as kb
import reverso_amd
from reverso_amd import _lib, engine
from test_gemm_form_coverage import image_launches, image_towers, text_launches, text_towers
from test_gemm_plan import knobs, plan

pytestmark = pytest.mark.gpu

IMAGE_BATCHES = [1, 8]
TEXT_SHAPES = [(1, 13), (5, 13), (64, None)]                  # (prompts, positions; None: the context length)


def _forms_of(lib, forward):
    torch.cuda.synchronize()
    lib.revo_debug_gemm_forms(1)
    forward()
    torch.cuda.synchronize()
    return lib.revo_debug_gemm_forms(1)


def _union(launches):
    bits = 0
    for *_, b, _steps in launches:
        bits |= b
    return bits


@pytest.mark.parametrize("name", sorted(image_towers()))
def test_image_forward_issues_the_forms_the_model_plans(dev, name):
    cfg = dataclasses.replace(reverso_amd.get_config(name), layers=2)
    eng = engine.VitEngine.synthetic(cfg, seed=5, device=0, max_batch=max(IMAGE_BATCHES), experiments=True)
    lib = _lib.load_exp()
    try:
        for B in IMAGE_BATCHES:
            g = torch.Generator().manual_seed(B)
            u8 = torch.randint(0, 256, (B, 3, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8).to(dev)
            got = _forms_of(lib, lambda: eng.embed(u8))
            with knobs():
                # vit.hip vit_forward: uint8 patches hold their values twice (K = 2 Kp) against weight rows of 3 Kp
                Kp = (cfg.patch_k + 63) // 64 * 64
                patch, _ = plan(4, B * cfg.grid * cfg.grid, cfg.width, 2 * Kp, lda=2 * Kp, ldb=3 * Kp)
                body = image_launches(cfg, B, 2)
            assert patch >= 0
            want = patch | _union(body)
            print(f"[forward forms] image {name} batch {B}: {'+'.join(kb.form_names(got))}")
            assert kb.form_names(got) == kb.form_names(want), (name, B, [(l[0], l[1], kb.form_names(l[6])) for l in body])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(text_towers()))
def test_text_forward_issues_the_forms_the_model_plans(dev, name):
    cfg = dataclasses.replace(reverso_amd.get_text_config(name), layers=2, vocab_size=512)
    eng = engine.TextEngine.synthetic(cfg, seed=5, device=0, max_batch=max(b for b, _ in TEXT_SHAPES), experiments=True)
    lib = _lib.load_exp()
    try:
        for B, S in TEXT_SHAPES:
            S = S or cfg.context_length
            tokens = np.random.default_rng(B + S).integers(0, cfg.vocab_size, size=(B, S)).astype(np.int32)
            got = _forms_of(lib, lambda: eng.embed_tokens(tokens))
            with knobs():
                body = text_launches(cfg, B * S, 2)
            print(f"[forward forms] text {name} {B} x {S}: {'+'.join(kb.form_names(got))}")
            assert kb.form_names(got) == kb.form_names(_union(body)), (name, B, S, [(l[0], l[1], kb.form_names(l[6])) for l in body])
    finally:
        eng.close()
