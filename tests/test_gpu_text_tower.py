"""GPU: the text tower's forward (revo_text_forward through engine.TextEngine) against the CPU restatement
(tests/_text_reference.py, pinned to an independent implementation by tests/test_text_reference_pin.py), layer by layer on the
miniatures and end to end at the real shapes, with the image tower's criteria (tests/test_gpu_embed.py): embedded rows equal
bit for bit, residual stream max |d| <= 3e-2 max |x| after each block, final cosine >= 0.9999, norms within 1e-5, cosine
scores against a fixed gallery within 1e-3."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd
from reverso_amd import _lib, engine, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _text_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu


def _reference(sd, cfg, tokens):
    with torch.no_grad():
        return tr.forward(sd, cfg, tokens, dtype=torch.float32)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


@pytest.fixture(scope="module")
def miniatures(dev):
    out = {}
    for name in ("PE-Tiny-Text-16", "PE-Tiny-Text-40"):
        cfg = reverso_amd.get_text_config(name)
        sd = weights.synth_text_weights(cfg, seed=7, randomize_affine=True)
        on = {k: v.to(dev) for k, v in sd.items()}
        out[name] = (cfg, sd, engine.TextEngine(cfg, on, device=0, max_batch=64),
                     engine.TextEngine(cfg, on, device=0, max_batch=64, experiments=True))
    yield out
    for _, _, a, b in out.values():
        a.close()
        b.close()


@pytest.mark.parametrize("name,seq", [("PE-Tiny-Text-16", 16), ("PE-Tiny-Text-40", 40), ("PE-Tiny-Text-40", 33)])
@pytest.mark.parametrize("batch", [1, 5, 64])
def test_miniature_layer_by_layer(miniatures, name, seq, batch):
    cfg, sd, eng, engx = miniatures[name]
    lengths = [(3 + 5 * i) % (seq - 2) + 1 for i in range(batch)]
    lengths[-1] = seq - 2                                     # the end token in the last column
    tokens = tr.prompts(cfg, lengths, seed=batch)[:, :seq]
    ref = _reference(sd, cfg, tokens)
    assert torch.equal(engx.residual_after(tokens, -2).cpu(), ref["embed"])
    for n in range(cfg.layers + 1):
        x = engx.residual_after(tokens, n).cpu()
        want = ref["embed"] if n == 0 else ref["blocks"][n - 1]
        err = float((x - want).abs().max())
        assert err <= 3e-2 * float(want.abs().max()), (n, err, float(want.abs().max()))
    emb = eng.embed_tokens(tokens).cpu()
    assert torch.equal(engx.embed_tokens(tokens).cpu(), emb)
    cos = _cos(emb, ref["normalized"])
    assert float(cos.min()) >= 0.9999, float(cos.min())
    assert float((emb.norm(dim=-1) - 1).abs().max()) <= 1e-5
    un = eng.embed_tokens(tokens, normalize=False).cpu()
    assert float((un - ref["out"]).abs().max()) <= 3e-2 * float(ref["out"].abs().max())
    # the whole context and the batch's longest prompt: the same rows (a causal row never sees what follows it)
    full = tr.prompts(cfg, lengths, seed=batch)
    a, b = eng.embed_tokens(full).cpu(), eng.embed_tokens(full, trim=True).cpu()
    assert float(_cos(a, emb).min()) >= 0.99999 and float(_cos(b, emb).min()) >= 0.99999


@pytest.fixture(scope="module")
def l14(dev):
    cfg = reverso_amd.get_text_config("PE-Core-L14-336")
    sd = weights.synth_text_weights(cfg, seed=0, randomize_affine=True)
    eng = engine.TextEngine(cfg, {k: v.to(dev) for k, v in sd.items()}, device=0, max_batch=64)
    yield cfg, sd, eng
    eng.close()


def _gallery_scores_agree(emb, ref, D):
    g = torch.Generator().manual_seed(4096)
    gal = torch.nn.functional.normalize(torch.randn(4096, D, generator=g), dim=-1)
    return float(((emb @ gal.T) - (ref @ gal.T)).abs().max())


def test_l14_text_tower_against_the_restatement(l14):
    cfg, sd, eng = l14
    tokens = tr.prompts(cfg, [1, 2, 5, 9, 14, 20, 27, 30], seed=1)
    ref = _reference(sd, cfg, tokens)["normalized"]
    emb = eng.embed_tokens(tokens).cpu()
    cos = _cos(emb, ref)
    d = _gallery_scores_agree(emb, ref, cfg.out_dim)
    print(f"[L14 text] cosine min {float(cos.min()):.6f}, gallery scores max |d| {d:.2e}")
    assert float(cos.min()) >= 0.9999 and float((emb.norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert d <= 1e-3, d
    assert torch.equal(eng.embed_tokens(tokens).cpu(), emb)


def test_l14_batch_composition(l14):
    """A prompt alone and the same prompt as row 37 of 64: other launch forms of the GEMMs (M = 32 and M = 2048), the same
    vector up to bf16 noise -- the tolerance of the image tower's uint8-against-float test."""
    cfg, sd, eng = l14
    tokens = tr.prompts(cfg, [(7 * i) % 30 + 1 for i in range(64)], seed=2)
    full = eng.embed_tokens(tokens)
    alone = eng.embed_tokens(tokens[37:38])
    assert float((alone[0] - full[37]).abs().max()) <= 1e-3 and float(_cos(alone[0], full[37])) >= 0.99999
    assert torch.equal(eng.embed_tokens(tokens), full) and torch.equal(eng.embed_tokens(tokens[37:38]), alone)
    ref = _reference(sd, cfg, tokens[[0, 37, 63]])["normalized"]
    assert float(_cos(full[[0, 37, 63]].cpu(), ref).min()) >= 0.9999


def test_g14_shaped_block_pair(dev):
    """The G14 text tower's shapes (width 1280 = five 256-column slices of the folded LayerNorm, 20 heads, context 72) cut to
    two blocks; 64 prompts (4608 rows: the batch-sized launch forms), eight of them against the restatement."""
    cfg = dataclasses.replace(reverso_amd.get_text_config("PE-Core-G14-448"), layers=2, vocab_size=512)
    sd = weights.synth_text_weights(cfg, seed=3, randomize_affine=True)
    eng = engine.TextEngine(cfg, {k: v.to(dev) for k, v in sd.items()}, device=0, max_batch=64)
    tokens = tr.prompts(cfg, [(11 * i) % 70 + 1 for i in range(64)], seed=3)
    tokens[5] = tr.prompts(cfg, [70], seed=9)[0]
    pick = [0, 5, 9, 17, 30, 41, 52, 63]
    ref = _reference(sd, cfg, tokens[pick])["normalized"]
    emb = eng.embed_tokens(tokens).cpu()
    assert float(_cos(emb[pick], ref).min()) >= 0.9999 and float((emb.norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert _gallery_scores_agree(emb[pick], ref, cfg.out_dim) <= 1e-3
    few = eng.embed_tokens(tokens[pick]).cpu()
    assert float(_cos(few, ref).min()) >= 0.9999
    eng.close()


def test_refusals_on_a_live_handle(miniatures):
    cfg, sd, eng, _ = miniatures["PE-Tiny-Text-40"]
    tokens = tr.prompts(cfg, [4, 9, 6, 12], seed=4)
    before = eng.embed_tokens(tokens)
    for bad in (-1, cfg.vocab_size):
        t = tokens.copy()
        t[2, 3] = bad
        with pytest.raises(_lib.RevoError, match=rf"status -2.*prompt 2 position 3 holds token id {bad}"):
            eng.embed_tokens(t)
    lib, p = eng._lib, C.c_void_p(tokens.ctypes.data)
    out = torch.empty(65, cfg.out_dim, device=eng.device)
    assert lib.revo_text_forward(eng._h, p, 65, 1, _lib.ptr(out), 1, None) == -2 and b"max_batch" in lib.revo_last_error()
    assert lib.revo_text_forward(eng._h, p, 1, 41, _lib.ptr(out), 1, None) == -2 and b"context_length" in lib.revo_last_error()
    assert lib.revo_text_forward(eng._h, p, 0, 40, _lib.ptr(out), 1, None) == -2
    assert lib.revo_text_forward(eng._h, p, 4, 0, _lib.ptr(out), 1, None) == -2
    assert torch.equal(eng.embed_tokens(tokens), before)
    with pytest.raises(_lib.RevoError, match="tokenizer"):
        os.environ.pop("REVERSO_BPE_VOCAB", None)
        eng.embed(["a red pickup truck at night"])
    with pytest.raises(_lib.RevoError, match="hook"):
        eng.residual_after(tokens, 1)
    bad_sd = {k: v for k, v in sd.items() if k != "ln_final.bias"}
    with pytest.raises(KeyError, match="ln_final.bias"):
        engine.TextEngine(cfg, bad_sd, device=0)


def test_strings_through_a_synthetic_vocabulary(dev):
    """embed(texts) = embed_tokens(tokenizer(texts)); a tower whose vocabulary is the synthetic BPE's."""
    from reverso_amd.tokenizer import ClipTokenizer
    vocab, merges = tr.synthetic_bpe()
    cfg = dataclasses.replace(reverso_amd.get_text_config("PE-Tiny-Text-16"), vocab_size=len(vocab))
    tok = ClipTokenizer(merges, context_length=cfg.context_length, vocab_size=cfg.vocab_size)
    eng = engine.TextEngine.synthetic(cfg, seed=1, device=0, max_batch=8, tokenizer=tok, randomize_affine=True)
    texts = ["the red car on the road", "it's 42 cars", "", "café  ñandú", "the " * 40]
    a = eng.embed(texts)
    b = eng.embed_tokens(tok(texts), trim=True)
    assert torch.equal(a, b) and a.shape == (5, cfg.out_dim)
    assert float(_cos(a[0], eng.embed("The  RED car on the\troad")[0])) >= 0.99999        # case and spacing do not count
    eng.close()
