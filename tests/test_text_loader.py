"""CPU: the text tower's side of the checkpoint loader (reverso_amd/weights.py): both key prefixes, the config from the
shapes, and errors that name the missing, unknown or mis-shaped tensor."""
import pytest
import torch

import reverso_amd
from reverso_amd import weights


def _clip_state_dict(name, prefix):
    cfg = reverso_amd.get_text_config(name)
    text = weights.synth_text_weights(cfg, seed=2)
    vcfg = reverso_amd.get_config("PE-Tiny-T14-56")
    sd = dict(weights.synth_weights(vcfg, seed=3))
    sd.update({prefix + k: v for k, v in text.items()})
    sd["logit_scale"] = torch.tensor(4.6)
    sd[prefix + "attn_mask"] = torch.zeros(cfg.context_length, cfg.context_length)
    return cfg, text, sd


@pytest.mark.parametrize("prefix", ["", "text."])
@pytest.mark.parametrize("name", ["PE-Tiny-Text-16", "PE-Tiny-Text-40"])
def test_both_prefixes_and_the_config_from_the_shapes(tmp_path, name, prefix):
    cfg, text, sd = _clip_state_dict(name, prefix)
    path = str(tmp_path / "clip.pt")
    torch.save(sd, path)
    got = weights.load_text_state_dict(path)
    assert sorted(got) == sorted(text) and all(torch.equal(got[k], text[k]) for k in text)
    rc = weights.resolve_text_config(got, name=cfg.name)
    assert rc == cfg, (rc, cfg)
    weights.check_text_state_dict(rc, got)
    assert {k: tuple(v.shape) for k, v in got.items()} == weights.expected_text_shapes(cfg)
    # the image tower's loader is as it was: the visual.* tensors only
    vis = weights.load_state_dict(path)
    assert vis and all(k.startswith("visual.") for k in vis)


def test_a_checkpoint_without_a_text_tower_says_so(tmp_path):
    path = str(tmp_path / "visual_only.pt")
    torch.save(dict(weights.synth_weights(reverso_amd.get_config("PE-Tiny-T14-56"), seed=3)), path)
    with pytest.raises(KeyError, match="token_embedding.weight"):
        weights.load_text_state_dict(path)


def test_missing_unknown_and_misshaped_tensors_are_named():
    cfg = reverso_amd.get_text_config("PE-Tiny-Text-40")
    sd = weights.synth_text_weights(cfg, seed=2)
    bad = dict(sd)
    bad.pop("transformer.resblocks.1.mlp.c_proj.bias")
    with pytest.raises(KeyError, match=r"resblocks\.1\.mlp\.c_proj\.bias"):
        weights.check_text_state_dict(cfg, bad)
    bad = dict(sd, **{"transformer.resblocks.0.attn.rel_bias": torch.zeros(3)})
    with pytest.raises(KeyError, match=r"rel_bias"):
        weights.check_text_state_dict(cfg, bad)
    bad = dict(sd, text_projection=torch.zeros(cfg.out_dim, cfg.width))
    with pytest.raises(ValueError, match=r"text_projection: expected \(256, 96\), got \(96, 256\)"):
        weights.check_text_state_dict(cfg, bad)
    # LayerScale follows the checkpoint, all blocks or none
    bad = dict(sd)
    bad.pop("transformer.resblocks.1.ls_2.gamma")
    with pytest.raises(KeyError, match=r"ls_2\.gamma of block 1"):
        weights.resolve_text_config(bad)
    no_ls = {k: v for k, v in sd.items() if ".ls_" not in k}
    assert not weights.resolve_text_config(no_ls).use_ls
    with pytest.raises(KeyError, match="positional_embedding"):
        weights.resolve_text_config({k: v for k, v in sd.items() if k != "positional_embedding"})


def test_variant_table_and_synthetic_weights():
    for name in ("PE-Core-B16-224", "PE-Core-L14-336", "PE-Core-G14-448"):
        t = reverso_amd.get_text_config(name)
        assert t.head_dim == 64 and t.vocab_size == 49408 and t.out_dim == reverso_amd.get_config(name).out_dim
    t = reverso_amd.get_text_config("PE-Tiny-Text-40")
    sd = weights.synth_text_weights(t, seed=0, randomize_affine=True)
    assert {k: tuple(v.shape) for k, v in sd.items()} == weights.expected_text_shapes(t)
    again = weights.synth_text_weights(t, seed=0, randomize_affine=True)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    with pytest.raises(KeyError):
        reverso_amd.get_text_config("nope")
