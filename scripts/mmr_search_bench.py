"""Diverse search (revo_search_mmr, Gallery.search_mmr) over the 1 M x 1024 gallery of range_search_bench.py (planted clusters of
perturbed copies; queries: perturbed cluster rows), diversity 0.5, at (queries, k, candidates) = (1, 10, 100), (1, 50, 1024),
(64, 10, 100), (64, 50, 1024), (1, 1024, 1024).  Per point: the whole call next to (a) revo_search_topk_large at k =
candidates alone -- the inner search, the floor -- and (b) the torch route on the same device: the same candidates gathered,
cand @ cand.T in fp32, the k-step greedy loop in torch ops.  Alternated rounds in one process, medians (wall clock around a
device synchronise); the stage split (the library's profiler, one profiled call) and the similarity kernel's pair rate.
With the experiment library (REVO_EXPERIMENTS=1) REVO_MMR_TILE=4 selects the 4 x 4 form of the similarity kernel.
Writes one JSON file.
    python scripts/mmr_search_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/mmr_search_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
DIVERSITY = 0.5
G = engine.Gallery(D, N, device=0, experiments=bool(os.environ.get("REVO_EXPERIMENTS")))
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


def torch_route(allrows, q, k, C):
    """what a caller had: the candidates of the plain search, their fp32 Gram matrix, the greedy loop in torch ops"""
    s, i, _ = G.search(q, k=C)
    cand = allrows[i]                                        # [Q, C, D]
    sim = cand @ cand.transpose(1, 2)                        # [Q, C, C]
    lr = (1.0 - DIVERSITY) * s
    m = torch.full_like(s, float("-inf"))
    dead = torch.zeros_like(s, dtype=torch.bool)
    ar = torch.arange(q.shape[0], device=dev)
    picks = []
    for step in range(k):
        v = lr if step == 0 else lr - DIVERSITY * m
        p = torch.where(dead, float("-inf"), v).argmax(dim=1)
        picks.append(p)
        dead[ar, p] = True
        m = torch.maximum(m, sim[ar, p])
    return i.gather(1, torch.stack(picks, 1))


res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "diversity": DIVERSITY,
       "tile": os.environ.get("REVO_MMR_TILE", "8"), "points": []}
allrows = G.read(0, N)
for Q, k, C in ((1, 10, 100), (1, 50, 1024), (64, 10, 100), (64, 50, 1024), (1, 1024, 1024)):
    pick = rows[torch.randint(0, rows.shape[0], (Q,), generator=g, device=dev)]
    q = allrows[pick] + 0.05 * torch.randn(Q, D, generator=g, device=dev) / D ** 0.5
    runs = {"search_mmr": lambda: G.search_mmr(q, k=k, candidates=C, diversity=DIVERSITY),
            "topk_large_k_is_candidates": lambda: G.search(q, k=max(C, 51)),
            "torch_fp32": lambda: torch_route(allrows, q, k, C)}
    for fn in runs.values():                # warm-up (workspaces, first launches)
        fn()
        fn()
    times = {name: [] for name in runs}
    for _ in range(ROUNDS):                 # alternated rounds
        for name, fn in runs.items():
            times[name].append(wall(fn))
    # the same picks as the torch route wherever its fp32 matmul rounds to the same order (reported, not required)
    same = float((G.search_mmr(q, k=k, candidates=C, diversity=DIVERSITY)[2] == torch_route(allrows, q, k, C)).float().mean())
    n_cand = G.search(q, k=max(C, 51))[2].clamp(max=C).to(torch.int64)
    pairs = int((n_cand * (n_cand - 1) // 2).sum())
    engine.prof_reset()
    engine.prof_enable(True)
    G.search_mmr(q, k=k, candidates=C, diversity=DIVERSITY)
    stages = engine.prof_report()
    engine.prof_enable(False)
    med = {name: round(statistics.median(v), 4) for name, v in times.items()}
    row = {"queries": Q, "k": k, "candidates": C, "median_ms": med,
           "over_inner_search_ms": round(med["search_mmr"] - med["topk_large_k_is_candidates"], 4),
           "candidate_pairs": pairs, "picks_equal_to_torch_route": round(same, 4),
           "runs_ms": {name: [round(t, 4) for t in v] for name, v in times.items()}, "stages": stages}
    res["points"].append(row)
    print(json.dumps({key: row[key] for key in ("queries", "k", "candidates", "median_ms", "over_inner_search_ms",
                                                "candidate_pairs", "picks_equal_to_torch_route")}), flush=True)
    print(json.dumps(stages), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
