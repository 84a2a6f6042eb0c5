"""Cost of the grouped search (revo_search_groups) at 1 M x 1024, 3 rows per image (group = row // 3), against the
ungrouped Gallery.search(k=50) it runs internally, alternated: group_size 1, limit 5 / 10 / 50, 1 / 64 / 1000 queries.
Then the grouped fallback (the fp32 passes over the gallery) at 1 and 64 uncertified queries, group_size 1 (pass A) and
3 (passes A and B): its queries sit at rows of the first 64 images, which hold 60 identical rows each (a "global"
region-mode image), so that their top 50 is one image.  Device events on the launch stream; one JSON line.
    python scripts/grouped_search_bench.py [N] [D] > profiles/grouped_search_bench.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
BIG, BIG_ROWS = 64, 60                      # images of identical rows at the front (the fallback's queries)
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
front = torch.randn(BIG, D, generator=g, device=dev).repeat_interleave(BIG_ROWS, 0)
G.add(front)
for s in range(BIG * BIG_ROWS, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=g, device=dev))
r = torch.arange(N, device=dev)
groups = torch.where(r < BIG * BIG_ROWS, r // BIG_ROWS, BIG + (r - BIG * BIG_ROWS) // 3).to(torch.int32)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"N": N, "D": D, "rows_per_image": 3, "certified": [], "fallback": []}
for Q in (1, 64, 1000):
    q = torch.randn(Q, D, generator=g, device=dev)
    for L in (5, 10, 50):
        row = {"Q": Q, "limit": L, "group_size": 1, "search_k50_ms": [], "grouped_ms": []}
        for _ in range(3):
            row["search_k50_ms"].append(round(timed(lambda: G.search(q, 50)), 4))
            row["grouped_ms"].append(round(timed(lambda: G.search_groups(q, groups, limit=L)), 4))
        row["uncertified"] = G.search_stats()["grouped_fallback"]
        row["ratio_best"] = round(min(row["grouped_ms"]) / min(row["search_k50_ms"]), 4)
        out["certified"].append(row)
        print(json.dumps(row), file=sys.stderr)
for Q in (1, 64):
    qi = torch.arange(Q, device=dev) * BIG_ROWS                 # one query per front image
    q = G.read(0, BIG * BIG_ROWS)[qi] * 4 + 0.05 * torch.randn(Q, D, generator=g, device=dev)
    for S in (1, 3):
        row = {"Q": Q, "limit": 5, "group_size": S, "search_k50_ms": [], "grouped_ms": []}
        for _ in range(2):
            row["search_k50_ms"].append(round(timed(lambda: G.search(q, 50), reps=5), 4))
            row["grouped_ms"].append(round(timed(lambda: G.search_groups(q, groups, limit=5, group_size=S), reps=5), 4))
        row["uncertified"] = G.search_stats()["grouped_fallback"]
        row["fallback_ms"] = round(min(row["grouped_ms"]) - min(row["search_k50_ms"]), 4)
        out["fallback"].append(row)
        print(json.dumps(row), file=sys.stderr)
print(json.dumps(out))
