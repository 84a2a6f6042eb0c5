"""Native-aspect embedding (revo_vit_set_grid, VitEngine.embed(grid=...)) on PE-Core-L14-336 with seeded
random-init weights:
  1. batch 64 of u8 images at the grids (24, 24), (18, 32), (32, 18), (12, 48) and (21, 27) against the native forward of the
     same run, alternated: a grid of 576 cells should cost what the native forward costs;
  2. a 64-image batch split over 1, 3, 5 and 25 grids of the menu (as equal groups as 64 allows; one forward per group, as
     SimpleReverso(aspect="keep") runs a batch) against one native batch of 64 and against the sum of native forwards at the
     groups' sizes: a split batch should cost what its sub-batches cost at their sizes.
Warm, medians over rounds, each timed with device events around `inner` back-to-back runs.  Writes one JSON file.
    python scripts/aspect_embed_bench.py [out.json] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd
from reverso_amd import config, engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/aspect_embed_bench.json"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
INNER = 3
B = 64
cfg = reverso_amd.get_config("PE-Core-L14-336")
eng = engine.VitEngine.synthetic(cfg, seed=0, device=0, max_batch=B)
G, P = cfg.grid, cfg.patch_size
gen = torch.Generator().manual_seed(0)


def images(n, grid):
    return torch.randint(0, 256, (n, 3, grid[0] * P, grid[1] * P), generator=gen, dtype=torch.uint8).to(dev)


def timed_ms(fn, inner=INNER):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(routes):
    for f in routes.values():                   # warm-up: a shape's tables, workspaces, first launches
        f()
        f()
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, f in routes.items():
            ms[k].append(timed_ms(f))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


res = {"model": cfg.name, "device": torch.cuda.get_device_name(0), "batch": B, "rounds": ROUNDS, "inner": INNER, "grids": [],
       "splits": []}
native = images(B, (G, G))
out = torch.empty((B, cfg.out_dim), dtype=torch.float32, device=dev)

# 1. one grid per batch
for grid in ((24, 24), (18, 32), (32, 18), (12, 48), (21, 27)):
    u8 = images(B, grid)
    r = alternate({"native": lambda: eng.embed(native, out=out), "on_grid": lambda: eng.embed(u8, out=out, grid=grid)})
    row = {"grid": list(grid), "cells": grid[0] * grid[1], "seq_len": grid[0] * grid[1] + int(cfg.use_cls), **r,
           "grid_over_native": round(r["on_grid"]["median_ms"] / r["native"]["median_ms"], 4)}
    res["grids"].append(row)
    print(json.dumps(row), flush=True)

# 2. one batch over several grids
menu = config.aspect_grids(cfg)
mid = menu.index((G, G))
for n_grids in (1, 3, 5, 25):
    # the grids nearest the square first (1: the native grid itself, through the grouped route)
    order = sorted(range(len(menu)), key=lambda i: (abs(i - mid), i))[:n_grids]
    sizes = [B // n_grids + (1 if j < B % n_grids else 0) for j in range(n_grids)]
    groups = [(menu[i], images(n, menu[i])) for i, n in zip(order, sizes)]
    subs = [native[:n] for n in sizes]

    def split():
        at = 0
        for grid, u8 in groups:
            eng.embed(u8, out=out[at:at + u8.shape[0]], grid=grid)
            at += u8.shape[0]

    def native_subs():
        at = 0
        for u8 in subs:
            eng.embed(u8, out=out[at:at + u8.shape[0]])
            at += u8.shape[0]

    r = alternate({"native_one_batch": lambda: eng.embed(native, out=out), "split": split, "native_sub_batches": native_subs})
    row = {"grids": n_grids, "group_sizes": sizes, "shapes": [list(menu[i]) for i in order], **r,
           "split_over_one_batch": round(r["split"]["median_ms"] / r["native_one_batch"]["median_ms"], 4),
           "split_over_sub_batches": round(r["split"]["median_ms"] / r["native_sub_batches"]["median_ms"], 4)}
    res["splits"].append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
