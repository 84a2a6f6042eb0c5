"""The text tower (revo_text_forward, engine.TextEngine) of PE-Core-L14-336 on seeded random-init weights at 1, 64 and 1 024
prompts: the full 32-token context, and 8-token prompts with trim=True (seq_len 8).  Warm, median of runs alternated with
the same tower in torch on the same box -- fp32, and bf16 with a causal scaled_dot_product_attention -- each timed with
device events around `inner` back-to-back forwards.  One profiled forward per shape gives the per-class breakdown
(revo_prof_report).  Writes one JSON file.
    python scripts/text_embed_bench.py [out.json] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import reverso_amd
from reverso_amd import engine, weights

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/text_embed_bench.json"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
cfg = reverso_amd.get_text_config("PE-Core-L14-336")
sd = {k: v.to(dev) for k, v in weights.synth_text_weights(cfg, seed=0, randomize_affine=True).items()}
eng = engine.TextEngine(cfg, sd, device=0, max_batch=1024)


def prompts(n, words, seed):
    g = np.random.default_rng(seed)
    t = np.zeros((n, cfg.context_length), dtype=np.int32)
    t[:, 0] = cfg.vocab_size - 2
    t[:, 1:1 + words] = g.integers(1, cfg.vocab_size - 2, (n, words))
    t[:, 1 + words] = cfg.vocab_size - 1
    return t


def torch_tower(dtype):
    p = {k: v.to(dtype) for k, v in sd.items()}
    W, H = cfg.width, cfg.heads

    def fwd(tok):
        B, S = tok.shape
        x = p["token_embedding.weight"][tok] + p["positional_embedding"][:S]
        for i in range(cfg.layers):
            a = f"transformer.resblocks.{i}."
            h = F.layer_norm(x, (W,), p[a + "ln_1.weight"], p[a + "ln_1.bias"], cfg.ln_eps)
            q, k, v = (t.reshape(B, S, H, W // H).transpose(1, 2) for t in F.linear(h, p[a + "attn.in_proj_weight"], p[a + "attn.in_proj_bias"]).split(W, dim=-1))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, S, W)
            x = x + F.linear(o, p[a + "attn.out_proj.weight"], p[a + "attn.out_proj.bias"])
            h = F.layer_norm(x, (W,), p[a + "ln_2.weight"], p[a + "ln_2.bias"], cfg.ln_eps)
            x = x + F.linear(F.gelu(F.linear(h, p[a + "mlp.c_fc.weight"], p[a + "mlp.c_fc.bias"])), p[a + "mlp.c_proj.weight"], p[a + "mlp.c_proj.bias"])
        e = x[torch.arange(B, device=dev), tok.argmax(-1)]
        return F.normalize(F.layer_norm(e, (W,), p["ln_final.weight"], p["ln_final.bias"], cfg.ln_eps) @ p["text_projection"], dim=-1)
    return fwd


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


res = {"model": cfg.name, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "cases": []}
t32, t16 = torch_tower(torch.float32), torch_tower(torch.bfloat16)
with torch.no_grad():
    for n in (1, 64, 1024):
        for label, words, trim in (("full context", 30, False), ("8-token prompts, trim", 6, True)):
            tok = prompts(n, words, seed=n + words)
            L = cfg.context_length if not trim else int(tok.argmax(1).max()) + 1
            tok_dev = torch.as_tensor(tok[:, :L].astype(np.int64), device=dev)
            inner = 20 if n <= 64 else 3
            routes = {"librevo": lambda: eng.embed_tokens(tok, trim=trim), "torch_fp32": lambda: t32(tok_dev),
                      "torch_bf16_sdpa": lambda: t16(tok_dev)}
            for f in routes.values():               # warm-up: workspaces, first launches, library heuristics
                f()
                f()
            ms = {k: [] for k in routes}
            for _ in range(ROUNDS):                 # alternated
                for k, f in routes.items():
                    ms[k].append(timed_ms(f, inner))
            cos = float((eng.embed_tokens(tok, trim=trim) * t32(tok_dev)).sum(-1).min())
            engine.prof_reset()
            engine.prof_enable(True)
            eng.embed_tokens(tok, trim=trim)
            stages = engine.prof_report()
            engine.prof_enable(False)
            row = {"prompts": n, "case": label, "seq_len": L, "rows": n * L, "inner": inner,
                   "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                   "min_ms": {k: round(min(v), 4) for k, v in ms.items()}, "max_ms": {k: round(max(v), 4) for k, v in ms.items()},
                   "min_cosine_against_torch_fp32": round(cos, 6), "stages": stages}
            res["cases"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "stages"}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
