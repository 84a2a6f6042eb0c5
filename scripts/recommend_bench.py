"""Search by examples (revo_search_recommend, Gallery.recommend) over the 1 M x 1024 gallery of range_search_bench.py (planted
clusters of perturbed copies), at (positives, negatives) = (1, 0), (4, 2), (32, 32), (100, 28) and k = 10 / 1024 (examples:
perturbed cluster rows).  Per point: the whole call (wall clock, it is synchronous) next to (a) revo_search_topk at k = 10 of
the same vectors as plain queries -- one pass over the gallery, the floor -- and (b) what the caller had before: torch fp32
examples @ rows.T, the max / compare, torch.topk.  Alternated rounds, medians; the stage split (the library's profiler, one
profiled call) and the candidate rows.  Writes one JSON file.
    python scripts/recommend_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/recommend_bench.json"
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


def torch_route(allrows, ex, P, k):
    s = ex @ allrows.T
    sp = s[:P].max(0).values
    if ex.shape[0] > P:
        sn = s[P:].max(0).values
        sp = torch.where(sp > sn, sp, -(sn * sn))
    return torch.topk(sp, k)


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "points": []}
allrows = G.read(0, N)
for P, Nn in ((1, 0), (4, 2), (32, 32), (100, 28)):
    pick = rows[torch.randint(0, rows.shape[0], (P + Nn,), generator=g, device=dev)]
    ex = allrows[pick] + 0.05 * torch.randn(P + Nn, D, generator=g, device=dev) / D ** 0.5
    pos, neg = ex[:P], (ex[P:] if Nn else None)
    exn = torch.nn.functional.normalize(ex, dim=1)
    for k in (10, 1024):
        runs = {"recommend": lambda: G.recommend(pos, neg, k=k), "topk_k10_same_vectors": lambda: G.search(ex, k=10),
                "torch_fp32": lambda: torch_route(allrows, exn, P, k)}
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {name: [] for name in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for name, fn in runs.items():
                times[name].append(wall(fn))
        G.recommend(pos, neg, k=k)
        st = G.search_stats()
        engine.prof_reset()
        engine.prof_enable(True)
        G.recommend(pos, neg, k=k)
        stages = engine.prof_report()
        engine.prof_enable(False)
        row = {"positives": P, "negatives": Nn, "k": k, "candidates": st["collected_rows"],
               "median_ms": {name: round(statistics.median(v), 4) for name, v in times.items()},
               "runs_ms": {name: [round(t, 4) for t in v] for name, v in times.items()}, "stages": stages}
        res["points"].append(row)
        print(json.dumps({key: row[key] for key in ("positives", "negatives", "k", "candidates", "median_ms")}), flush=True)
        print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
