"""Deduplicating append (revo_gallery_append_unique, Gallery.add_unique) into a 1 M x 1024 gallery:
video-like batches of n = 1 024 / 4 096 / 16 384 rows -- shots of perturbed copies of one frame, 10 % and 90 % of the rows
first of their shot -- and one batch of 16 384 identical rows, threshold 0.9.  Per case, alternated in rounds behind one
warm-up round, every round on the same N gallery rows (the rows a round added are removed again, untimed):
  (a) add           Gallery.add of the batch: what an insert costs without the dedup
  (b) add_unique    the call under test (wall clock, it is synchronous), its stages from the library's profiler (one
                    profiled call), the ambiguous pairs re-scored and the join passes
  (c) parent route  what the library offered before: search_range(batch, t) against the gallery, a torch fp32 batch x batch
                    product, the greedy on the host, add of the kept rows
Every sample is reported, with median, minimum and maximum.  The join's expectation is recorded next to the result: its tile
pairs at the pairs join's rate per tile pair, from a revo_gallery_pairs call timed in the same run.  Writes one JSON file.
    python scripts/dedup_append_bench.py [out.json] [N] [D] [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/dedup_append_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
T = 0.9
NMAX = 16384
G = engine.Gallery(D, N + NMAX, device=0)
gen = torch.Generator(device=dev).manual_seed(42)
for s in range(0, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=gen, device=dev))
torch.cuda.synchronize()


def batch(n, kept_fraction):
    """shots in order: round(kept_fraction n) centres, each followed by its perturbed copies (scores about 0.997)"""
    shots = max(1, round(kept_fraction * n))
    centre = torch.nn.functional.normalize(torch.randn(shots, D, generator=gen, device=dev), dim=1)
    owner = torch.sort(torch.cat([torch.arange(shots, device=dev),
                                  torch.randint(0, shots, (n - shots,), generator=gen, device=dev)])).values
    return centre[owner] + 0.05 * torch.randn(n, D, generator=gen, device=dev) / D ** 0.5


def reset():
    if len(G) > N:
        G.remove(torch.arange(N, len(G), device=dev))
    torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def parent_route(v):
    off, idx, _ = G.search_range(v, T)
    in_gallery = (off[1:] > off[:-1]).cpu().numpy()
    x = torch.nn.functional.normalize(v, dim=1)
    near = ((x @ x.T) >= T).cpu().numpy()
    kept = np.zeros(v.shape[0], dtype=bool)
    for j in range(v.shape[0]):
        kept[j] = not in_gallery[j] and not (near[j, :j] & kept[:j]).any()
    G.add(v[torch.from_numpy(kept).to(dev)])
    return int(kept.sum())


def spread(xs):
    return {"samples_ms": [round(x * 1e3, 3) for x in xs], "median_ms": round(statistics.median(xs) * 1e3, 3),
            "min_ms": round(min(xs) * 1e3, 3), "max_ms": round(max(xs) * 1e3, 3)}


res = {"N": N, "D": D, "threshold": T, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "cases": []}
# the pairs join's rate per tile pair in this run
G.pairs(0.99)
pw = [timed(lambda: G.pairs(0.99))[0] for _ in range(2)]
tiles = (N + 255) // 256
rate = min(pw) / (tiles * (tiles + 1) / 2)
res["pairs_join"] = {"call_s": [round(w, 4) for w in pw], "tile_pairs": tiles * (tiles + 1) // 2, "s_per_tile_pair": rate}
print(json.dumps(res["pairs_join"]), flush=True)

cases = [(n, f, "video") for n in (1024, 4096, 16384) for f in (0.1, 0.9)] + [(16384, 0.0, "identical")]
for n, f, kind in cases:
    v = batch(n, f) if kind == "video" else torch.randn(1, D, generator=gen, device=dev).repeat(n, 1)
    t_add, t_uni, t_par = [], [], []
    kept_u = kept_p = None
    for r in range(ROUNDS + 1):                             # round 0: warm-up (workspaces, first launches), not recorded
        reset()
        a = timed(lambda: G.add(v))[0]
        reset()
        u, out = timed(lambda: G.add_unique(v, T))
        kept_u = int(out[2].sum())
        st = G.search_stats()
        reset()
        p, kept_p = timed(lambda: parent_route(v))
        if r:
            t_add.append(a), t_uni.append(u), t_par.append(p)
    reset()
    engine.prof_reset()
    engine.prof_enable(True)
    G.add_unique(v, T)
    stages = engine.prof_report()
    engine.prof_enable(False)
    reset()
    t0, t1 = N // 256, (N + n + 255) // 256
    tile_pairs = t1 * (t1 + 1) // 2 - t0 * (t0 + 1) // 2
    row = {"n": n, "kind": kind, "kept_fraction_asked": f, "kept": kept_u, "parent_route_kept": kept_p,
           "ambiguous_rescored": st["collected_rows"], "join_passes": st["join_passes"],
           "add": spread(t_add), "add_unique": spread(t_uni), "parent_route": spread(t_par), "stages": stages,
           "join_tile_pairs": tile_pairs, "join_expected_ms": round(tile_pairs * rate * 1e3, 3),
           "add_unique_under_parent_route": bool(max(t_uni) < min(t_par))}
    res["cases"].append(row)
    print(json.dumps({k: row[k] for k in row if k != "stages"}), flush=True)
    print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f_:
    json.dump(res, f_, indent=1)
print("wrote", OUT)
