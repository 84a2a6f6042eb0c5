"""GPU: the text tower's kernels one at a time (text.hip) -- the token embedding and the end-of-text pooling bit for bit
against torch, the causal attention against the fp64 reference within the per-element bound of tests/_text_reference.py (whose teeth
tests/test_text_attention_teeth.py shows on the same inputs), its prefix independence and its determinism."""
import os
import sys

import numpy as np
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


INT32_MIN = -2 ** 31


def _pool_prompts(S, seed):
    """int32 [B][S]: one prompt per way the first position of the largest id can be found (or missed)"""
    rng = np.random.default_rng(seed)
    rows = {}
    base = lambda: rng.integers(-1000, 40000, size=S, dtype=np.int64)
    t = base(); t[0] = 49407; rows["maximum in column 0"] = t
    t = base(); t[S - 1] = 49407; rows["maximum in the last column"] = t
    t = base(); t[S // 2:] = 49407; rows["maximum repeated from the middle on: the first wins"] = t
    t = base(); t[S // 3] = 49407; t[S - 1] = 49407; rows["maximum twice"] = t
    if S > 64:                                               # positions s and s + 64 are the same lane's
        t = base(); t[0] = 49407; t[64] = 49407; rows["twice in lane 0"] = t
        t = base(); t[S - 65] = 49407; t[S - 1] = 49407; rows["twice in the last position's lane"] = t
        t = base(); t[64] = 49407; t[63] = 49407; rows["lane 0's second position against lane 63's first"] = t
    rows["every id equal"] = np.full(S, 7, dtype=np.int64)
    rows["every id the smallest int32"] = np.full(S, INT32_MIN, dtype=np.int64)
    t = np.full(S, INT32_MIN, dtype=np.int64); t[S - 1] = INT32_MIN + 1; rows["one above the smallest int32, last"] = t
    t = -base() - 5; rows["negative ids"] = t
    t = base(); t[S // 2] = 2 ** 31 - 1; rows["the largest int32"] = t
    return list(rows), np.stack(list(rows.values())).astype(np.int32)


@pytest.mark.parametrize("W,pad", [(1280, 0), (1280, 12), (256, 4), (4, 4)])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 128])
def test_pool_eot_is_the_row_at_the_first_largest_id(dev, lib, S, W, pad):
    names, tok = _pool_prompts(S, S + W)
    B, ldx = tok.shape[0], W + pad
    g = torch.Generator().manual_seed(S * 7 + W)
    # one spare row behind the last prompt: a position S (no lane found an id above its start value) reads it, not past x
    x = torch.randn(B * S + 1, ldx, generator=g).to(dev)
    x[B * S] = -7.0
    buf = torch.full((B + 2, W), 3.0, dtype=torch.float32, device=dev)          # a guard row on either side of out
    out = buf[1:B + 1]
    _lib.check(lib.revo_op_pool_eot(_lib.ptr(torch.from_numpy(tok).to(dev)), _lib.ptr(x), ldx, B, S, W, _lib.ptr(out),
                                    _lib.current_stream()), "revo_op_pool_eot")
    at = np.argmax(tok, axis=1)                              # numpy: the first occurrence of the maximum
    want = x[torch.from_numpy(np.arange(B) * S + at).to(dev), :W]
    for b, name in enumerate(names):
        assert torch.equal(out[b], want[b]), f"{name} (S {S}): not the row of position {at[b]}"
    assert (buf[0] == 3.0).all() and (buf[B + 1] == 3.0).all()                  # nothing written outside out


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
