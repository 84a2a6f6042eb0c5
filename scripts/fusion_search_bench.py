"""Hybrid queries (revo_search_fusion, Gallery.search_fusion) over the 1 M x 1024 gallery of mmr_search_bench.py (planted
clusters of perturbed copies), at (searches n, lists m, limit C, k) = (1, 2, 100, 10), (1, 8, 1024, 50), (64, 2, 100, 10),
(64, 8, 1024, 50), both methods.  The m queries of a fused search are perturbed copies of one cluster row, each further away
than the last, so the lists overlap as those of two views of one thing do.  Per point: (a) the whole call next to (b)
Gallery.search of the same n * m queries at k = C alone -- the inner search, the floor -- and (c) the route that existed
before: (b) plus a fusion of its outputs in torch ops on the same device (sort by row, segment sums, top-k).  Alternated
rounds in one process, medians (wall clock around a device synchronise); also the fuse launch alone (engine.fuse_topk on the
lists of (b)) and the stage split of one profiled call.  Writes one JSON file.
    python scripts/fusion_search_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/fusion_search_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
RRF_K = 60.0
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


def torch_fuse(s, i, c, k, method):
    """the fusion in torch ops: contributions, rows sorted per search, segment sums, top-k (fp32, torch's own summation order)"""
    n, m, C = s.shape
    live = torch.arange(C, device=dev)[None, None] < c[:, :, None]
    if method == "rrf":
        contrib = (1.0 / (RRF_K + torch.arange(1, C + 1, device=dev, dtype=torch.float32))).expand(n, m, C)
    else:
        cnt = c.clamp(min=1)[:, :, None].to(torch.float64)
        s64 = torch.where(live, s, 0.0).to(torch.float64)
        mu = s64.sum(-1, keepdim=True) / cnt
        sd = (torch.where(live, (s64 - mu) ** 2, 0.0).sum(-1, keepdim=True) / cnt).sqrt()
        contrib = torch.where(sd > 0, (s64 - (mu - 3 * sd)) / (6 * sd), 0.5).to(torch.float32)
    big = torch.iinfo(torch.int64).max
    flat_i = torch.where(live, i, big).reshape(n, m * C)
    flat_c = torch.where(live, contrib, 0.0).reshape(n, m * C)
    si, order = flat_i.sort(dim=1)
    sc = flat_c.gather(1, order)
    new = torch.ones_like(si, dtype=torch.bool)
    new[:, 1:] = si[:, 1:] != si[:, :-1]
    seg = new.cumsum(1) - 1
    F = torch.zeros_like(sc).scatter_add_(1, seg, sc)
    row_of = torch.full_like(si, big).scatter_(1, seg, si)
    F = torch.where(row_of != big, F, float("-inf"))
    top = F.topk(min(k, m * C), dim=1)
    return top.values, row_of.gather(1, top.indices)


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "rrf_k": RRF_K, "points": []}
allrows = G.read(0, N)
for n, m, C, k in ((1, 2, 100, 10), (1, 8, 1024, 50), (64, 2, 100, 10), (64, 8, 1024, 50)):
    pick = rows[torch.randint(0, rows.shape[0], (n,), generator=g, device=dev)]
    spread = 0.05 + 0.1 * torch.arange(m, device=dev, dtype=torch.float32)[None, :, None]
    q = allrows[pick][:, None] + spread * torch.randn(n, m, D, generator=g, device=dev) / D ** 0.5
    flat = q.reshape(n * m, D)
    for method in ("rrf", "dbsf"):
        def route_before():
            s, i, c = G.search(flat, k=C)
            return torch_fuse(s.reshape(n, m, C), i.reshape(n, m, C), c.reshape(n, m), k, method)

        ls, li, lc = G.search(flat, k=C)
        ls, li, lc = ls.reshape(n, m, C).clone(), li.reshape(n, m, C).clone(), lc.reshape(n, m).clone()
        runs = {"search_fusion": lambda: G.search_fusion(q, k=k, limit=C, method=method, rrf_k=RRF_K),
                "search_k_is_limit": lambda: G.search(flat, k=C),
                "search_plus_torch_fusion": route_before,
                "fuse_launch_alone": lambda: engine.fuse_topk(ls, li, lc, k=k, method=method, rrf_k=RRF_K)}
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {name: [] for name in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for name, fn in runs.items():
                times[name].append(wall(fn))
        # the same rows as the torch route wherever its summation rounds to the same order (reported, not required)
        same = float((G.search_fusion(q, k=k, limit=C, method=method, rrf_k=RRF_K)[1] == route_before()[1]).float().mean())
        engine.prof_reset()
        engine.prof_enable(True)
        G.search_fusion(q, k=k, limit=C, method=method, rrf_k=RRF_K, with_list_scores=True)
        stages = engine.prof_report()
        engine.prof_enable(False)
        med = {name: round(statistics.median(v), 4) for name, v in times.items()}
        row = {"searches": n, "lists": m, "limit": C, "k": k, "method": method, "median_ms": med,
               "over_inner_search_ms": round(med["search_fusion"] - med["search_k_is_limit"], 4),
               "ratio_to_route_before": round(med["search_fusion"] / med["search_plus_torch_fusion"], 4),
               "rows_equal_to_torch_route": round(same, 4),
               "runs_ms": {name: [round(t, 4) for t in v] for name, v in times.items()}, "stages_with_list_scores": stages}
        res["points"].append(row)
        print(json.dumps({key: row[key] for key in ("searches", "lists", "limit", "k", "method", "median_ms", "over_inner_search_ms",
                                                    "ratio_to_route_before", "rows_equal_to_torch_route")}), flush=True)
        print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
