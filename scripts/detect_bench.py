"""Text-prompted regions (revo_vit_detect) on PE-Core-L14-336, seeded random-init weights, batch 1 and
batch 64, 3 prompts + 1 background prompt.  Routes, alternated, best of `rounds` (default three), each timed with device events
around `inner` back-to-back calls: `embed` (revo_vit_forward: the baseline), `embed_tokens` (revo_vit_forward_tokens),
`detect` with and without the regions' vectors.  One profiled detect per batch splits the time into token head / scores /
regions / region head (revo_prof_report classes; the region head is also given as detect minus detect-without-vectors).
Random-init weights give many small regions: the region counts are in the file.  Writes one JSON file.
    python scripts/detect_bench.py [out.json] [rounds]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/detect_bench.json"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
cfg = reverso_amd.get_config("PE-Core-L14-336")
eng = engine.VitEngine.synthetic(cfg, seed=0, device=0, max_batch=64, randomize_affine=True)
gen = torch.Generator().manual_seed(1)
prompts = torch.randn((4, cfg.out_dim), generator=gen).to(dev)


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


res = {"model": cfg.name, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "prompts": 3, "background": 1,
       "max_regions": 50, "cases": []}
for B in (1, 64):
    u8 = torch.randint(0, 256, (B, 3, cfg.image_size, cfg.image_size), generator=gen, dtype=torch.uint8).to(dev)
    # the planted prompts: token vectors of the batch itself, so that regions of more than one cell exist
    _, tok = eng.embed_tokens(u8[:1], with_global=False)
    pr = torch.cat([tok[0, 1 + 100:1 + 103], prompts[:1]]).contiguous()
    inner = 10 if B == 1 else 3
    det = lambda vec: eng.detect(u8, pr, n_background=1, max_regions=50, with_vectors=vec, with_global=True)
    routes = {"embed": lambda: eng.embed(u8), "embed_tokens": lambda: eng.embed_tokens(u8),
              "detect": lambda: det(True), "detect_no_vectors": lambda: det(False)}
    for f in routes.values():                   # warm-up: workspaces, first launches
        f()
        f()
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):                     # alternated
        for k, f in routes.items():
            ms[k].append(timed_ms(f, inner))
    d = det(True)
    engine.prof_reset()
    engine.prof_enable(True)
    det(True)
    stages = engine.prof_report()
    engine.prof_enable(False)
    best = {k: round(min(v), 4) for k, v in ms.items()}
    pick = lambda name: round(stages.get(name, {}).get("ms", 0.0), 4)
    rows = B * cfg.seq
    row = {"batch": B, "inner": inner, "token_rows": rows, "regions": len(d), "cells_in_regions": int(d.cells.sum()),
           "best_ms": best, "all_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "split_ms": {"token_head": pick("token_head"), "scores": pick("detect_scores"), "regions": pick("detect_regions"),
                        "region_pool": pick("pool_regions"),
                        "region_head_by_difference": round(best["detect"] - best["detect_no_vectors"], 4)},
           "token_head_us_per_row": round(1e3 * pick("token_head") / rows, 4),
           "token_head_us_per_row_by_difference": round(1e3 * (best["embed_tokens"] - best["embed"]) / rows, 4),
           "stages": stages}
    res["cases"].append(row)
    print(json.dumps({k: v for k, v in row.items() if k != "stages"}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
