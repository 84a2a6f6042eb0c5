"""Filtered against unfiltered search, 1 000 queries, k = 50 and 10, 1 M x 1024 (50 % random mask): the target of a kernel
trace, plus the certificate counters of each kind of search (one JSON line).
    rocprofv3 --kernel-trace --stats -d <dir> -o k50 -- python scripts/filtered_k50_trace.py"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, reverso_amd  # noqa
from reverso_amd import engine
dev = torch.device("cuda", 0)
N, D = 1_000_000, 1024
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
for s in range(0, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=g, device=dev))
q = torch.randn(1000, D, generator=g, device=dev)
m = torch.rand(N, device=dev, generator=g) < 0.5
bits = G.allow_bits(m)
out = {}
for tag, k, allow in (("unf_k50", 50, None), ("flt_k50", 50, bits), ("unf_k10", 10, None), ("flt_k10", 10, bits)):
    for _ in range(5):
        G.search(q, k, allow=allow)
    torch.cuda.synchronize()
    out[tag] = G.search_stats()
print(json.dumps(out))
