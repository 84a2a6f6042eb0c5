"""The large-k search (revo_search_topk_large) over 1 M x 1024: whole-search ms (device events on the launch stream) for
1, 64, 256 and 1 000 queries at k = 50 (the k <= 50 path, for reference), 100, 256 and 1024, the configurations alternated
over several rounds (median reported); per-stage ms from the library's profiler (one profiled search per configuration);
band rows per query (revo_search_stats slot 3 / Q) and exhaustive-fallback queries (slot 6).  Writes one JSON file.
    python scripts/large_k_search_bench.py [out.json] [N] [D]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/large_k_search_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = 5
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
for s in range(0, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=g, device=dev))
configs = [(Q, k) for Q in (1, 64, 256, 1000) for k in (50, 100, 256, 1024)]
queries = {Q: torch.randn(Q, D, generator=g, device=dev) for Q in (1, 64, 256, 1000)}
for Q, k in configs:                      # warm-up (workspace growth, first launches)
    G.search(queries[Q], k)
torch.cuda.synchronize()
times = {c: [] for c in configs}
for _ in range(ROUNDS):                   # alternated: every configuration once per round
    for Q, k in configs:
        reps = 10 if Q <= 256 else 4
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            G.search(queries[Q], k)
        e1.record()
        torch.cuda.synchronize()
        times[(Q, k)].append(e0.elapsed_time(e1) / reps)
rows = []
for Q, k in configs:
    G.search(queries[Q], k)
    st = G.search_stats()
    engine.prof_reset()
    engine.prof_enable(True)
    G.search(queries[Q], k)
    torch.cuda.synchronize()
    stages = engine.prof_report()
    engine.prof_enable(False)
    rows.append({"Q": Q, "k": k, "path": "topk" if k <= 50 else "topk_large",
                 "search_ms": round(statistics.median(times[(Q, k)]), 4),
                 "search_ms_rounds": [round(t, 4) for t in times[(Q, k)]],
                 "band_rows_per_query": None if k <= 50 else round(st["collected_rows"] / Q, 1),
                 "large_k_fallback": st["large_k_fallback"], "stages": stages})
    print(json.dumps({key: rows[-1][key] for key in ("Q", "k", "search_ms", "band_rows_per_query", "large_k_fallback")}),
          flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"N": N, "D": D, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
print("wrote", OUT)
