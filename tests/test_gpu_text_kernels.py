"""GPU: the text tower's kernels one at a time (text.hip) -- the token embedding bit for bit against torch, the causal
attention against the fp64 reference within the per-element bound of tests/_text_reference.py (whose teeth
tests/test_text_attention_teeth.py shows on the same inputs), its prefix independence and its determinism."""
import os
import sys

import pytest
import torch

from reverso_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_bounds as kb  # noqa: E402
import _text_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu


def _embed(lib, tokens, table, pos, ldx):
    B, S = tokens.shape
    W = table.shape[1]
    x = torch.full((B * S, ldx), -7.0, dtype=torch.float32, device=tokens.device)
    _lib.check(lib.revo_op_embed_tokens(_lib.ptr(tokens), _lib.ptr(table), _lib.ptr(pos), B, S, table.shape[0], W, _lib.ptr(x), ldx,
                                        _lib.current_stream()), "revo_op_embed_tokens")
    return x


@pytest.mark.parametrize("vocab,W,B,S,pad", [(49408, 64, 3, 5, 0), (49408, 64, 3, 5, 12), (300, 1280, 2, 72, 0), (64, 128, 1, 1, 4)])
def test_embed_tokens_is_bit_exact(dev, lib, vocab, W, B, S, pad):
    g = torch.Generator().manual_seed(vocab + W + pad)
    table = torch.randn(vocab, W, generator=g).to(dev)
    pos = torch.randn(S, W, generator=g).to(dev)
    tok = torch.randint(0, vocab, (B, S), generator=g, dtype=torch.int32)
    tok[0, 0], tok[-1, -1] = 0, vocab - 1                   # the table's first and last row
    tok = tok.to(dev)
    x = _embed(lib, tok, table, pos, W + pad)
    want = (table[tok.long()] + pos[None]).reshape(B * S, W)
    assert torch.equal(x[:, :W], want)
    assert (x[:, W:] == -7.0).all()                         # nothing written between the rows


def _attention(lib, qkv, B, S, H, ldo):
    out = torch.full((B * S, ldo), float("nan"), dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.revo_op_attention_causal(_lib.ptr(qkv), qkv.shape[1], _lib.ptr(out), ldo, B, S, H, 64, _lib.current_stream()),
               "revo_op_attention_causal")
    return out


@pytest.mark.parametrize("pad", [(0, 0), (64, 32)], ids=["dense", "padded"])
@pytest.mark.parametrize("B,H", tr.ATT_BH)
@pytest.mark.parametrize("S", tr.ATT_SEQS)
def test_causal_attention_within_the_fp64_bound(dev, lib, S, B, H, pad):
    W = H * 64
    ld, ldo = 3 * W + pad[0], W + pad[1]
    qkv = tr.attention_qkv(B, S, H, ld).to(dev)
    out = _attention(lib, qkv, B, S, H, ldo)
    q, k, v = tr.attention_split(qkv, B, S, H)
    A = tr.CausalAttention
    ref, bound = A.reference(q, k, v), A.bound(q, k, v)
    r = kb.ratio(tr.attention_unsplit(out, B, S, H), ref, bound)
    print(f"[causal S{S} B{B} H{H} ld{ld} ldo{ldo}] kernel / bound max {r:.3f}")
    assert r <= 1.0, r
    if ldo > W:
        assert torch.isnan(out[:, W:].float()).all()        # nothing written between the rows


@pytest.mark.parametrize("cut", [1, 31, 32, 33, 64])
def test_row_i_depends_on_rows_up_to_i_only(dev, lib, cut):
    B, S, H = 2, 77, 2
    qkv = tr.attention_qkv(B, S, H).to(dev)
    base = _attention(lib, qkv, B, S, H, H * 64).reshape(B, S, -1)
    big = qkv.clone().reshape(B, S, -1)
    big[:, cut + 1:] = (big[:, cut + 1:].float() * 1024.0).bfloat16()       # q, k and v rows past the cut (a power of two: exact)
    out = _attention(lib, big.reshape(B * S, -1), B, S, H, H * 64).reshape(B, S, -1)
    assert torch.equal(out[:, :cut + 1], base[:, :cut + 1])
    assert torch.isfinite(out.float()).all()


def test_causal_attention_is_deterministic(dev, lib):
    B, S, H = 3, 128, 5
    qkv = tr.attention_qkv(B, S, H).to(dev)
    a = _attention(lib, qkv, B, S, H, H * 64)
    b = _attention(lib, qkv, B, S, H, H * 64)
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
