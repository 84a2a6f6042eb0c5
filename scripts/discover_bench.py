"""Discovery and context search (revo_search_discover, Gallery.discover) over the 1 M x 1024 gallery of range_search_bench.py
(planted clusters of perturbed copies), at (target + 2, 8, 63 pairs) and (4, 64 pairs, no target), k = 10 / 1024 (examples:
perturbed cluster rows).  Per point: the whole call (wall clock, it is synchronous) next to (a) revo_search_recommend at the
same number of example rows -- the same plan with another epilogue -- and (b) what the caller had before: torch fp32
examples @ rows.T, the formula, torch.topk.  Alternated rounds, medians; the stage split of both (the library's profiler, one
profiled call each) and the candidate rows.  Writes one JSON file.
    python scripts/discover_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/discover_bench.json"
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
EPS = 1.1920928955078125e-07


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fs(v):
    return v / (1 + v.abs())


def torch_route(allrows, tgt, pos, neg, k):
    sp, sn = pos @ allrows.T, neg @ allrows.T
    if tgt is not None:
        score = torch.where(sp > sn, 1.0, -1.0).sum(0) + 0.5 * (fs(allrows @ tgt) + 1)
    else:
        score = fs(torch.clamp(sp - sn - EPS, max=0.0)).sum(0)
    return torch.topk(score, k)


def staged(fn):
    engine.prof_reset()
    engine.prof_enable(True)
    fn()
    stages = engine.prof_report()
    engine.prof_enable(False)
    return stages


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "points": []}
allrows = G.read(0, N)
for n, has_target in ((2, True), (8, True), (63, True), (4, False), (64, False)):
    E = 2 * n + int(has_target)
    pick = rows[torch.randint(0, rows.shape[0], (E,), generator=g, device=dev)]
    ex = allrows[pick] + 0.05 * torch.randn(E, D, generator=g, device=dev) / D ** 0.5
    tgt = ex[2 * n] if has_target else None
    pos, neg = ex[:n], ex[n:2 * n]
    exn = torch.nn.functional.normalize(ex, dim=1)
    P = (E + 1) // 2                            # (a): the same example rows, split into positives and negatives
    for k in (10, 1024):
        runs = {"discover": lambda: G.discover(tgt, pos, neg, k=k),
                "recommend_same_rows": lambda: G.recommend(ex[:P], ex[P:] if E > P else None, k=k),
                "torch_fp32": lambda: torch_route(allrows, exn[2 * n] if has_target else None, exn[:n], exn[n:2 * n], k)}
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {name: [] for name in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for name, fn in runs.items():
                times[name].append(wall(fn))
        runs["discover"]()
        cand = G.search_stats()["collected_rows"]
        runs["recommend_same_rows"]()
        cand_rec = G.search_stats()["collected_rows"]
        row = {"pairs": n, "target": has_target, "example_rows": E, "k": k, "candidates": cand, "recommend_candidates": cand_rec,
               "median_ms": {name: round(statistics.median(v), 4) for name, v in times.items()},
               "runs_ms": {name: [round(t, 4) for t in v] for name, v in times.items()},
               "stages": staged(runs["discover"]), "recommend_stages": staged(runs["recommend_same_rows"])}
        res["points"].append(row)
        print(json.dumps({key: row[key] for key in ("pairs", "target", "k", "candidates", "recommend_candidates", "median_ms")}),
              flush=True)
        print(json.dumps(row["stages"]), flush=True)
        print(json.dumps(row["recommend_stages"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
