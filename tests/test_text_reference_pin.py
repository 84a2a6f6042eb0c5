"""CPU: the text tower's restatement (tests/_text_reference.py) pinned to an independently written implementation,
transformers.CLIPTextModelWithProjection, on both miniatures with randomised affine terms and prompts of every length from
1 to context - 2.

Tolerance: 1e-6 of the largest element.  Both sides run in fp64 except the other side's eager softmax, which is taken in
fp32 whatever the model's dtype: its rounding is what is left (the test prints the figure; a few 1e-8).

The other implementation has no LayerScale.  For the miniature that has it the gains are folded into the projections that
feed the residual stream -- gamma . (W a + b) = (gamma W) a + gamma b, the same function -- and the restatement WITH
LayerScale is held to the restatement on the folded weights as well."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd
from reverso_amd import weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _text_reference as tr  # noqa: E402

MINIATURES = ("PE-Tiny-Text-16", "PE-Tiny-Text-40")


def _case(name):
    cfg = reverso_amd.get_text_config(name)
    sd = weights.synth_text_weights(cfg, seed=11, randomize_affine=True)
    tokens = tr.prompts(cfg, list(range(1, cfg.context_length - 1)), seed=5)
    return cfg, sd, tokens


def _fold_layerscale(cfg, sd):
    out = dict(sd)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        for g, lin in (("ls_1.gamma", "attn.out_proj"), ("ls_2.gamma", "mlp.c_proj")):
            gam = out.pop(p + g).double()
            out[p + lin + ".weight"] = gam[:, None] * sd[p + lin + ".weight"].double()
            out[p + lin + ".bias"] = gam * sd[p + lin + ".bias"].double()
    return dataclasses.replace(cfg, use_ls=False), out


@pytest.mark.parametrize("name", MINIATURES)
def test_restatement_equals_the_independent_implementation(name):
    cfg, sd, tokens = _case(name)
    if cfg.use_ls:
        with_ls = tr.forward(sd, cfg, tokens)["out"]
        cfg, sd = _fold_layerscale(cfg, sd)
        folded = tr.forward(sd, cfg, tokens)["out"]
        assert float((with_ls - folded).abs().max() / folded.abs().max()) <= 1e-12      # fp64 on both sides
    ours = tr.forward(sd, cfg, tokens)
    model = tr.hf_model(sd, cfg)
    with torch.no_grad():
        r = model(input_ids=torch.as_tensor(tokens, dtype=torch.long))
    for what, a, b in (("pooled output", ours["out"], r.text_embeds.double()),
                       ("last hidden state", ours["last_hidden"], r.last_hidden_state.double())):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"[{name}] {what}: max |d| / max |x| = {err:.3g}")
        assert err <= 1e-6, (what, err)


@pytest.mark.parametrize("name", MINIATURES)
def test_tokens_behind_the_end_token_change_nothing(name):
    cfg, sd, tokens = _case(name)
    a = tr.forward(sd, cfg, tokens)["out"]
    g = np.random.default_rng(3)
    other = tokens.copy()
    for r in range(other.shape[0]):
        e = int(other[r].argmax())
        other[r, e + 1:] = g.integers(0, cfg.vocab_size - 1, other.shape[1] - e - 1)      # anything below the end token's id
    b = tr.forward(sd, cfg, other)["out"]
    assert torch.equal(a, b)
    # ... and so does cutting them off: seq_len = the longest prompt computes the same rows (other matrix shapes: the fp64
    # sums may be taken in another order)
    L = int(tokens.argmax(axis=1).max()) + 1
    c = tr.forward(sd, cfg, tokens[:, :L])["out"]
    assert float((a - c).abs().max()) <= 1e-12 * float(a.abs().max())
