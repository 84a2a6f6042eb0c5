"""Multi-vector search (revo_search_maxsim, Gallery.search_maxsim) over the 1 M x 1024 gallery of range_search_bench.py
(planted clusters of perturbed copies) with three consecutive rows per group, at 1, 4, 16 and 64 query vectors (perturbed
cluster rows), k = 10 / 1024.  Per point: the whole call (wall clock, it is synchronous) next to (a) a torch fp32 route:
queries @ rows.T, scatter_reduce(amax) by group, the sum, torch.topk; (b) n calls of search_groups at limit 10 -- another
answer, but what an application pays today; and revo_search_recommend at the same number of example rows, whose pass is the
same main loop with a reducing epilogue.  Alternated rounds, medians; the stage split (the library's profiler, one profiled
call each) and the candidate rows.  Writes one JSON file.
    python scripts/maxsim_bench.py [out.json] [N] [D] [rounds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/maxsim_bench.json"
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
groups = (torch.arange(N, device=dev) // 3).to(torch.int32)
groups64 = groups.to(torch.int64)
NG = int(groups[-1]) + 1


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_route(allrows, q, k):
    s = q @ allrows.T
    m = torch.full((q.shape[0], NG), -float("inf"), device=dev).scatter_reduce(1, groups64[None].expand(q.shape[0], -1), s, "amax")
    return torch.topk(m.sum(0), k)


def groups_route(q):
    for i in range(q.shape[0]):
        G.search_groups(q[i:i + 1], groups, limit=10, group_size=1)


def staged(fn):
    engine.prof_reset()
    engine.prof_enable(True)
    fn()
    stages = engine.prof_report()
    engine.prof_enable(False)
    return stages


res = {"N": N, "D": D, "groups": NG, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "points": []}
allrows = G.read(0, N)
G.search_maxsim(allrows[:1], groups, k=1)          # the group index is built by the first call
for n in (1, 4, 16, 64):
    pick = rows[torch.randint(0, rows.shape[0], (n,), generator=g, device=dev)]
    q = allrows[pick] + 0.05 * torch.randn(n, D, generator=g, device=dev) / D ** 0.5
    qn = torch.nn.functional.normalize(q, dim=1)
    for k in (10, 1024):
        runs = {"maxsim": lambda: G.search_maxsim(q, groups, k=k),
                "recommend_same_rows": lambda: G.recommend(q, None, k=k),
                "torch_fp32": lambda: torch_route(allrows, qn, k)}
        if k == 10:
            runs["search_groups_x_n"] = lambda: groups_route(q)
        for fn in runs.values():                # warm-up (workspaces, first launches)
            fn()
            fn()
        times = {name: [] for name in runs}
        for _ in range(ROUNDS):                 # alternated rounds
            for name, fn in runs.items():
                times[name].append(wall(fn))
        runs["maxsim"]()
        cand = G.search_stats()["collected_rows"]
        row = {"n_vectors": n, "k": k, "candidate_rows": cand,
               "median_ms": {name: round(statistics.median(v), 4) for name, v in times.items()},
               "runs_ms": {name: [round(t, 4) for t in v] for name, v in times.items()},
               "stages": staged(runs["maxsim"]), "recommend_stages": staged(runs["recommend_same_rows"])}
        res["points"].append(row)
        print(json.dumps({key: row[key] for key in ("n_vectors", "k", "candidate_rows", "median_ms")}), flush=True)
        print(json.dumps(row["stages"]), flush=True)
        print(json.dumps(row["recommend_stages"]), flush=True)
# the cost of the group index (once per set of group ids): a call that rebuilds it against one that does not
t_build = []
for _ in range(3):
    other = groups + 1
    t_build.append(wall(lambda: G.search_maxsim(allrows[:1], other, k=1)))       # (the context manager sets the ids anew each call)
res["note_index"] = "every Gallery.search_maxsim call sets the group ids anew, so each call above includes the index build"
res["call_with_index_build_ms"] = [round(t, 4) for t in t_build]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
