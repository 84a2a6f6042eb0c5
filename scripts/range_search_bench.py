"""Range search (revo_search_range, Gallery.search_range) over a 1 M x 1024 gallery with planted clusters of perturbed copies,
at thresholds 0.8 and 0.9, for 1, 64, 1 000 and 10 000 queries (perturbed cluster rows: every query has hits).  Per point:
the whole call (wall clock, it is synchronous), next to the top-k searches it replaces -- revo_search_topk at k = 10 and
revo_search_topk_large at k = 1024 (each the wall clock of one call between two synchronizes) -- timed in alternated
rounds, medians; the stage split (the library's profiler, one profiled call); results and candidates
per query and the candidate passes.  Writes one JSON file.
    python scripts/range_search_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/range_search_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
# planted clusters: 20 000 groups of 2..6 perturbed copies of one direction (scores about 0.85 .. 0.99 within a group)
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


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "points": []}
allrows = G.read(0, N)
for Q in (1, 64, 1000, 10000):
    # queries: planted rows with a little more noise (near their cluster, not on it)
    pick = rows[torch.randint(0, rows.shape[0], (Q,), generator=g, device=dev)]
    q = allrows[pick] + 0.05 * torch.randn(Q, D, generator=g, device=dev) / D ** 0.5
    for t in (0.8, 0.9):
        runs = {"range": lambda: G.search_range(q, t), "topk_k10": lambda: G.search(q, k=10, score_threshold=t)}
        if Q <= 1000:
            runs["topk_large_k1024"] = lambda: G.search(q, k=1024, score_threshold=t)
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {k: [] for k in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for k, fn in runs.items():
                times[k].append(wall(fn))
        off, idx, sc = G.search_range(q, t)
        st = G.search_stats()
        cnt = (off[1:] - off[:-1]).float()
        engine.prof_reset()
        engine.prof_enable(True)
        G.search_range(q, t)
        stages = engine.prof_report()
        engine.prof_enable(False)
        row = {"Q": Q, "threshold": t, "results": int(idx.shape[0]), "results_per_query_mean": round(float(cnt.mean()), 1),
               "results_per_query_max": int(cnt.max()), "candidates": st["collected_rows"],
               "candidates_per_query": round(st["collected_rows"] / Q, 1), "candidate_passes": st["join_passes"],
               "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
               "runs_ms": {k: [round(x, 4) for x in v] for k, v in times.items()}, "stages": stages}
        res["points"].append(row)
        print(json.dumps({k: row[k] for k in ("Q", "threshold", "results", "candidates", "candidate_passes", "median_ms")}),
              flush=True)
        print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
