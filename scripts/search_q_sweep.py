"""Whole-search time (every kernel of Gallery.search, device events on the launch stream) of the unfiltered search over
1 M x 1024 for 1, 64, 1 000 and 10 000 queries, k = 10 and 50: one JSON line.  Run it alternately against two builds of
the library (REVO_LIBRARY_PATH=<other librevo.so>) to A/B a change of the scan.
    python scripts/search_q_sweep.py [N] [D]"""
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
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
for s in range(0, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=g, device=dev))
out = {"N": N, "D": D, "rows": []}
for Q in (1, 64, 1000, 10000):
    q = torch.randn(Q, D, generator=g, device=dev)
    for k in (10, 50):
        for _ in range(3):
            G.search(q, k)
        torch.cuda.synchronize()
        reps = 20 if Q <= 1000 else 5
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            G.search(q, k)
        e1.record()
        torch.cuda.synchronize()
        out["rows"].append({"Q": Q, "k": k, "search_ms": round(e0.elapsed_time(e1) / reps, 4)})
print(json.dumps(out))
