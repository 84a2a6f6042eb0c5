"""Boosted search (revo_search_boosted, Gallery.search_boosted) over the 1 M x 1024 gallery of recommend_bench.py (planted
clusters of perturbed copies), one query (a perturbed cluster row), k = 10 / 1024, multiplier 1 and three shapes of bias:
    random      uniform in [0, 0.2], in no relation to the row index
    rising      0.2 * row / N: grows with the row index, as a timestamp does
    date_decay  a Gaussian decay around row 0.8 N whose value exceeds 0.01 on about 1 % of the rows (0.2 at the centre)
Per point: the whole call (wall clock, it is synchronous) next to (a) revo_search_topk at k = 10 of the same vector -- one
pass over the gallery, the floor --, (b) revo_search_recommend with that vector as the one positive -- the same pass without
the two arrays: DESIGN.md section 4z expects the candidate pass within 10 % of it -- and (c) what the caller had before: torch
fp32 rows @ q, the fma (torch.addcmul: one rounding where the device fuses it), torch.topk.  Alternated rounds, medians; the
stage split (the library's profiler, one profiled call each of boosted and recommend) and the candidate rows.  Writes one
JSON file.
    python scripts/boosted_search_bench.py [out.json] [N] [D] [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/boosted_search_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
x = torch.randn(N, D, generator=g, device=dev)
sizes = torch.randint(2, 7, (20_000,), generator=g, device=dev)
rows = torch.randperm(N, generator=g, device=dev)[: int(sizes.sum())]
centre = torch.nn.functional.normalize(torch.randn(sizes.shape[0], D, generator=g, device=dev), dim=1)
owner = torch.repeat_interleave(torch.arange(sizes.shape[0], device=dev), sizes)
sigma = 0.1 + 0.3 * torch.rand(rows.shape[0], 1, generator=g, device=dev)
x[rows] = centre[owner] + sigma * torch.randn(rows.shape[0], D, generator=g, device=dev) / D ** 0.5
for s in range(0, N, 131072):
    G.add(x[s:s + 131072])
del x
torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_route(allrows, qn, m, b, k):
    return torch.topk(torch.addcmul(b, m, allrows @ qn), k)


def stages_of(fn):
    engine.prof_reset()
    engine.prof_enable(True)
    fn()
    rep = engine.prof_report()
    engine.prof_enable(False)
    return rep


pos = torch.arange(N, device=dev, dtype=torch.float32)
# exp(ln(0.5) d^2 / scale^2) > 0.05 (0.01 after the factor 0.2) on 1 % of the rows: |d| < 0.005 N = scale * sqrt(log2(20))
scale = 0.005 * N / (torch.log2(torch.tensor(20.0)).item() ** 0.5)
biases = {"random": 0.2 * torch.rand(N, generator=g, device=dev), "rising": 0.2 * pos / N,
          "date_decay": 0.2 * torch.exp(torch.log(torch.tensor(0.5)).item() * ((pos - 0.8 * N) / scale) ** 2)}
mult = torch.ones(N, device=dev)
res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "points": []}
allrows = G.read(0, N)
pick = rows[torch.randint(0, rows.shape[0], (1,), generator=g, device=dev)]
q = (allrows[pick] + 0.05 * torch.randn(1, D, generator=g, device=dev) / D ** 0.5)[0]
qn = torch.nn.functional.normalize(q, dim=0)
for name, bias in biases.items():
    for k in (10, 1024):
        runs = {"boosted": lambda: G.search_boosted(q, mult, bias, k=k), "topk_k10": lambda: G.search(q[None], k=10),
                "recommend_one_positive": lambda: G.recommend(q[None], None, k=k),
                "torch_fp32": lambda: torch_route(allrows, qn, mult, bias, k)}
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {n: [] for n in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for n, fn in runs.items():
                times[n].append(wall(fn))
        G.recommend(q[None], None, k=k)
        rec_candidates = G.search_stats()["collected_rows"]
        G.search_boosted(q, mult, bias, k=k)
        st = G.search_stats()
        stages = stages_of(runs["boosted"])
        rec_stages = stages_of(runs["recommend_one_positive"])
        row = {"bias": name, "k": k, "candidates": st["collected_rows"], "recommend_candidates": rec_candidates,
               "median_ms": {n: round(statistics.median(v), 4) for n, v in times.items()},
               "runs_ms": {n: [round(t, 4) for t in v] for n, v in times.items()}, "stages": stages,
               "recommend_stages": rec_stages}
        res["points"].append(row)
        print(json.dumps({key: row[key] for key in ("bias", "k", "candidates", "recommend_candidates", "median_ms")}), flush=True)
        print(json.dumps(stages), flush=True)
        print(json.dumps(rec_stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
