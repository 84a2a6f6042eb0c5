"""Near-duplicate pairs (revo_gallery_pairs, Gallery.pairs) over a 1 M x 1024 gallery with planted clusters of perturbed
copies, at thresholds 0.9 and 0.95: the whole call (wall clock, it is synchronous), the join's time and TFLOP/s against the
2.5 PFLOP/s bf16 peak (N^2 D / 2 multiply-adds), the re-score and sort share (the library's profiler, one profiled call),
the candidate count and the join passes.  For comparison the same answer built from Gallery.search with every row as a
query (k = 50), timed in the same run, and whether the two answers agree.  Writes one JSON file.
    python scripts/pairs_bench.py [out.json] [N] [D]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/gallery_pairs_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
PEAK = 2.5e15
QCHUNK = 10_000
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
# planted clusters: 20 000 groups of 2..6 perturbed copies of one direction (pair scores about 0.85 .. 0.99)
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


def search_route(t):
    """every row as a query (k = 50, threshold t): pairs i < j, each once"""
    out = []
    for q0 in range(0, N, QCHUNK):
        q = G.read(q0, min(QCHUNK, N - q0))
        s, i, c = G.search(q, k=50, score_threshold=t)
        src = torch.arange(q0, q0 + q.shape[0], device=dev)[:, None].expand_as(i)
        keep = (i > src) & (i >= 0)
        out.append(torch.stack([src[keep], i[keep]], 1))
    p = torch.cat(out)
    return p[torch.argsort(p[:, 0] * N + p[:, 1])]


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "planted_rows": int(rows.shape[0]), "thresholds": []}
G.pairs(0.99)                       # warm-up (workspace, first launches)
search_route(0.99)
flop = 2.0 * N * N * D / 2
for t in (0.9, 0.95):
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pairs, scores = G.pairs(t)
        walls.append(time.perf_counter() - t0)
    st = G.search_stats()
    engine.prof_reset()
    engine.prof_enable(True)
    G.pairs(t)
    stages = engine.prof_report()
    engine.prof_enable(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sp = search_route(t)
    torch.cuda.synchronize()
    search_s = time.perf_counter() - t0
    row = {"threshold": t, "pairs": int(pairs.shape[0]), "candidates": st["collected_rows"], "join_passes": st["join_passes"],
           "pairs_call_s": [round(w, 4) for w in walls], "stages": stages,
           "search_route_s": round(search_s, 4), "search_route_pairs": int(sp.shape[0]),
           "search_route_equal": bool(sp.shape == pairs.shape and torch.equal(sp, pairs))}
    best = min(walls)
    row["pairs_call_tflops"] = round(flop / best / 1e12, 1)
    row["pairs_call_fraction_of_peak"] = round(flop / best / PEAK, 3)
    res["thresholds"].append(row)
    print(json.dumps({k: row[k] for k in ("threshold", "pairs", "candidates", "join_passes", "pairs_call_s", "pairs_call_tflops",
                                          "search_route_s", "search_route_pairs", "search_route_equal")}), flush=True)
    print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
