"""The text tower restated for the tests: the forward in fp64 / fp32 torch (pinned against an independent implementation by
tests/test_text_reference_pin.py), the causal attention's fp64 reference with its per-element bound, the fp32 emulation of
the kernel's rounding steps, three wrong references, and the fixtures the CPU and GPU tests share.

    x   = token_embedding[tokens] + positional_embedding[:S]
    for each block:  x += ls_1 . out_proj(causal_attention(qkv(ln_1(x))));  x += ls_2 . c_proj(gelu_erf(c_fc(ln_2(x))))
    p   = ln_final(x[b, argmax_s tokens[b, s]])          (the first position of the largest id: the end-of-text token)
    out = p @ text_projection;  optionally out / ||out||

The causal bound is the derivation of _kernel_bounds.Attention.bound (its header has the terms) with row i's sums taken
over the keys 0..i it may see and the key count S replaced by i + 1."""
import math

import numpy as np
import torch

import _kernel_bounds as kb
from _kernel_bounds import LN2, LOG2E, U_BF16, U_F32


# ------------------------------------------------------------------ the forward ----
def forward(sd, cfg, tokens, dtype=torch.float64):
    """sd: names without a prefix; tokens: integer [B, S], S <= context.  Returns a dict: ``embed`` [B, S, W], ``blocks``
    (the residual stream after each block), ``last_hidden`` (ln_final of every row), ``pooled`` [B, W] (ln_final of the
    end-of-text row), ``out`` [B, D], ``normalized``."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long)
    B, S = tok.shape
    W, H = cfg.width, cfg.heads
    hd = W // H
    ln = lambda x, n: torch.nn.functional.layer_norm(x, (W,), p[n + ".weight"], p[n + ".bias"], cfg.ln_eps)
    x = p["token_embedding.weight"][tok] + p["positional_embedding"][:S]
    res = {"embed": x.clone(), "blocks": []}
    allowed = torch.ones(S, S, dtype=torch.bool).tril()
    for i in range(cfg.layers):
        pre = f"transformer.resblocks.{i}."
        qkv = ln(x, pre + "ln_1") @ p[pre + "attn.in_proj_weight"].T + p[pre + "attn.in_proj_bias"]
        q, k, v = (t.reshape(B, S, H, hd).transpose(1, 2) for t in qkv.split(W, dim=-1))
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        a = torch.softmax(s.masked_fill(~allowed, -math.inf), dim=-1) @ v
        a = a.transpose(1, 2).reshape(B, S, W) @ p[pre + "attn.out_proj.weight"].T + p[pre + "attn.out_proj.bias"]
        x = x + (a * p[pre + "ls_1.gamma"] if cfg.use_ls else a)
        h = ln(x, pre + "ln_2") @ p[pre + "mlp.c_fc.weight"].T + p[pre + "mlp.c_fc.bias"]
        h = torch.nn.functional.gelu(h) @ p[pre + "mlp.c_proj.weight"].T + p[pre + "mlp.c_proj.bias"]
        x = x + (h * p[pre + "ls_2.gamma"] if cfg.use_ls else h)
        res["blocks"].append(x.clone())
    eot = tok.argmax(dim=-1)                      # torch: the first occurrence of the maximum
    res["last_hidden"] = ln(x, "ln_final")
    res["pooled"] = res["last_hidden"][torch.arange(B), eot]
    res["out"] = res["pooled"] @ p["text_projection"]
    res["normalized"] = res["out"] / res["out"].norm(dim=-1, keepdim=True)
    return res


def prompts(cfg, lengths, seed=0):
    """Token rows [len(lengths), context]: start token, `n` word ids in [1, vocab - 2), end token, pad 0."""
    g = np.random.default_rng(seed)
    out = np.zeros((len(lengths), cfg.context_length), dtype=np.int32)
    for r, n in enumerate(lengths):
        assert 0 <= n <= cfg.context_length - 2
        out[r, 0] = cfg.vocab_size - 2
        out[r, 1:1 + n] = g.integers(1, cfg.vocab_size - 2, n)
        out[r, 1 + n] = cfg.vocab_size - 1
    return out


def hf_model(sd, cfg):
    """transformers.CLIPTextModelWithProjection holding the same weights (eager attention, exact-erf GELU, the end token =
    the highest id): the independently written implementation the restatement is pinned to."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    c = CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.width, intermediate_size=cfg.mlp_dim, projection_dim=cfg.out_dim,
                       num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, max_position_embeddings=cfg.context_length,
                       hidden_act="gelu", layer_norm_eps=cfg.ln_eps, pad_token_id=0, bos_token_id=cfg.vocab_size - 2,
                       eos_token_id=cfg.vocab_size - 1, attn_implementation="eager")
    m = CLIPTextModelWithProjection(c).double().eval()      # fp64 weights and matmuls; its eager softmax stays fp32
    W = cfg.width
    new = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].T}
    for i in range(cfg.layers):
        a, b = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):       # q / k / v are the thirds of in_proj
            new[b + f"self_attn.{n}.weight"] = sd[a + "attn.in_proj_weight"][j * W:(j + 1) * W]
            new[b + f"self_attn.{n}.bias"] = sd[a + "attn.in_proj_bias"][j * W:(j + 1) * W]
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                         ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            new[b + dst + ".weight"] = sd[a + src + ".weight"]
            new[b + dst + ".bias"] = sd[a + src + ".bias"]
    own = m.state_dict()
    missing = [k for k in own if k not in new and not k.endswith("position_ids")]
    assert not missing, missing
    m.load_state_dict({k: v.detach().clone().double().contiguous() for k, v in new.items()}, strict=False)
    return m


# -------------------------------------------------------------- causal attention ----
def causal_mask(S, device="cpu", shift=0):
    """allowed[i, j] = j <= i + shift"""
    i = torch.arange(S, device=device)
    return i[None, :] <= i[:, None] + shift


class CausalAttention:
    """q, k, v: fp64 [pairs, S, hd] (the exact bf16 values the kernel receives)."""

    @staticmethod
    def reference(q, k, v):
        S, hd = q.shape[-2], q.shape[-1]
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        return torch.softmax(s.masked_fill(~causal_mask(S, q.device), -math.inf), dim=-1) @ v

    @staticmethod
    def bound(q, k, v):
        S, hd = q.shape[-2], q.shape[-1]
        ok = causal_mask(S, q.device)
        s = q @ k.transpose(-1, -2)
        c = hd ** -0.5 * LOG2E
        p = torch.softmax((s * hd ** -0.5).masked_fill(~ok, -math.inf), dim=-1)
        ref = p @ v
        pv = p @ v.abs()
        qk = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~ok, 0.0)
        sc = (s.abs() * c).masked_fill(~ok, 0.0)
        eps = LN2 * (c * (hd + 1) * U_F32 * qk.amax(-1) + 2.0 ** -22 * sc.amax(-1)) + 2.0 ** -22
        n = torch.arange(1, S + 1, device=q.device, dtype=torch.float64)          # keys row i sums over
        d32 = (2 * n * U_F32 + 2.0 ** -21 + 2 * eps)[..., None] * pv
        return U_BF16 * (ref.abs() + pv) + (1 + U_BF16) * d32

    @staticmethod
    def emulate(q, k, v):
        """The kernel's rounding steps in fp32: e = fp32(s) c, the row's real maximum over the allowed keys, p = exp2(e - m),
        l = sum p, O = bf16(p) . v, out = bf16(O (1 / l))."""
        S, hd = q.shape[-2], q.shape[-1]
        c = float(np.float32(np.float32(1.0) / np.sqrt(np.float32(hd))) * np.float32(LOG2E))
        e = ((q.float() @ k.float().transpose(-1, -2)) * c).masked_fill(~causal_mask(S, q.device), -math.inf)
        p = torch.exp2(e - e.amax(-1, keepdim=True))
        l = p.sum(-1, keepdim=True)
        o = p.bfloat16().float() @ v.float()
        return (o * (1.0 / l)).bfloat16().double()

    @staticmethod
    def _softmax_v(q, k, v, allowed):
        hd = q.shape[-1]
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        return torch.softmax(s.masked_fill(~allowed, -math.inf), dim=-1) @ v

    @staticmethod
    def wrong_no_mask(q, k, v):
        return CausalAttention._softmax_v(q, k, v, torch.ones(q.shape[-2], q.shape[-2], dtype=torch.bool, device=q.device))

    @staticmethod
    def wrong_mask_plus_one(q, k, v):
        return CausalAttention._softmax_v(q, k, v, causal_mask(q.shape[-2], q.device, +1))

    @staticmethod
    def wrong_mask_minus_one(q, k, v):
        S = q.shape[-2]
        ok = causal_mask(S, q.device, -1)
        ok[0, 0] = True                           # (row 0 would have no key at all)
        return CausalAttention._softmax_v(q, k, v, ok)

    @staticmethod
    def wrong_mask_after_max(q, k, v):
        """The row maximum taken over ALL keys, the mask applied afterwards, in the kernel's fp32 arithmetic (in exact
        arithmetic the maximum cancels; in fp32 a masked key with a large score pushes the allowed ones out of range)."""
        S, hd = q.shape[-2], q.shape[-1]
        c = float(np.float32(np.float32(1.0) / np.sqrt(np.float32(hd))) * np.float32(LOG2E))
        e = (q.float() @ k.float().transpose(-1, -2)) * c
        p = torch.exp2(e - e.amax(-1, keepdim=True)).masked_fill(~causal_mask(S, q.device), 0.0)
        l = p.sum(-1, keepdim=True)
        o = p.bfloat16().float() @ v.float()
        return (o * (1.0 / l)).bfloat16().double()

    MUTATIONS = (("no mask", "wrong_no_mask"), ("mask shifted by +1", "wrong_mask_plus_one"),
                 ("mask shifted by -1", "wrong_mask_minus_one"), ("mask after the row maximum", "wrong_mask_after_max"))


ATT_SEQS = (1, 2, 31, 32, 33, 63, 64, 65, 72, 77, 96, 127, 128)
ATT_BH = ((1, 1), (3, 2), (2, 5))


def attention_qkv(B, S, H, ld=None, seed=None):
    """The GPU test's seeded input: [B S, ld] bf16 rows of q | k | v (CPU), N(0, 1) -- except in the LAST sequence of the
    batch, where every fourth key row is scaled by 64: there a key the row may not see can hold the row's largest score by
    more than fp32's exponent range (2^-126) absorbs, which is what separates a maximum taken before the mask from one
    taken after it (in exact arithmetic the two are the same function)."""
    W = H * 64
    ld = ld or 3 * W
    g = torch.Generator(device="cpu").manual_seed(seed if seed is not None else 1000 * S + 10 * H + B + (ld - 3 * W))
    x = torch.randn(B * S, ld, generator=g)
    x[(B - 1) * S:][3::4, W:2 * W] *= 64.0
    return x.bfloat16()


def attention_split(qkv, B, S, H):
    return kb.attention_split(qkv, B, S, H, 64)


def attention_unsplit(out, B, S, H):
    return kb.attention_unsplit(out, B, S, H, 64)


# ------------------------------------------------------------------- tokenizer ----
def synthetic_bpe():
    """A CLIP-format vocabulary small enough to write down: the 256 byte symbols, the same with </w>, a handful of merges,
    the two specials.  Returns (vocab dict, merges as tuples)."""
    from reverso_amd.tokenizer import bytes_to_unicode
    base = list(bytes_to_unicode().values())
    merges = [("t", "h"), ("th", "e</w>"), ("c", "a"), ("ca", "r"), ("car", "s</w>"), ("r", "e"), ("re", "d</w>"), ("o", "n</w>"),
              ("'", "s</w>"), ("r", "o"), ("ro", "a"), ("roa", "d</w>"), ("4", "2</w>"), ("i", "t</w>"), ("Ã", "©</w>"),
              ("a", "n"), ("an", "d"), ("!", "!"), ("!!", "!</w>")]
    vocab = base + [b + "</w>" for b in base] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
    return {t: i for i, t in enumerate(vocab)}, merges
