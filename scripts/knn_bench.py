"""Exact kNN graph (revo_gallery_knn, Gallery.knn) at k = 10 over the 1 M x 1024 planted gallery of scripts/pairs_bench.py and
scripts/clusters_bench.py, alternated with the route it replaces -- 100 x Gallery.search of 10 000 master rows at k = 11, the
self-hit dropped on the host: whole-call wall clock of both, the stages of one profiled call (level, join, rescore,
sort/select, fallback; the library's profiler), candidates per row, rows that fell back, and the pairs join's time on the same
box next to the kNN join's.  Then the clusters bench's variant: the first 30 000 rows overwritten by one vector (every one of
them has 29 999 equal partners: the candidate workspace overflows and those rows take the exhaustive fallback), one call.
Writes one JSON file.  One process, no retries: the first error ends it, and an alarm ends a run that takes too long.
    python scripts/knn_bench.py [out.json] [N] [D] [block] [limit seconds]"""
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/knn_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
BLOCK = int(sys.argv[4]) if len(sys.argv) > 4 else 30_000
signal.alarm(int(sys.argv[5]) if len(sys.argv) > 5 else 900)            # SIGALRM's default action ends the process
K = 10
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
# planted clusters: 20 000 groups of 2..6 perturbed copies of one direction (pair scores about 0.85 .. 0.99)
x = torch.randn(N, D, generator=g, device=dev)
sizes = torch.randint(2, 7, (min(20_000, N // 50),), generator=g, device=dev)
rows = torch.randperm(N, generator=g, device=dev)[: int(sizes.sum())]
centre = torch.nn.functional.normalize(torch.randn(sizes.shape[0], D, generator=g, device=dev), dim=1)
owner = torch.repeat_interleave(torch.arange(sizes.shape[0], device=dev), sizes)
sigma = 0.1 + 0.3 * torch.rand(rows.shape[0], 1, generator=g, device=dev)
x[rows] = centre[owner] + sigma * torch.randn(rows.shape[0], D, generator=g, device=dev) / D ** 0.5
for s in range(0, N, 131072):
    G.add(x[s:s + 131072])
shot = x[:1].clone()
del x
torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def profiled(fn):
    engine.prof_reset()
    engine.prof_enable(True)
    out, s = timed(fn)
    stages = engine.prof_report()
    engine.prof_enable(False)
    return out, s, stages


def stage_seconds(stages, *names):
    """seconds of the named kernel classes in a profiler report ({class: {"launches", "ms"}}), None when none of them ran"""
    hit = [stages[n]["ms"] for n in names if n in stages]
    return round(sum(hit) / 1e3, 5) if hit else None


def knn_stages(stages):
    return {"level_s": stage_seconds(stages, "knn_level"), "join_s": stage_seconds(stages, "knn_join"),
            "rescore_s": stage_seconds(stages, "knn_rescore"), "sort_select_s": stage_seconds(stages, "knn_sort", "knn_select"),
            "fallback_s": stage_seconds(stages, "knn_fallback")}


def search_route():
    """the route a user has today: blocks of 10 000 master rows as queries at k + 1, the self-hit dropped on the host side"""
    out = []
    for a in range(0, N, 10_000):
        q = G.read(a, min(10_000, N - a))
        s, i, c = G.search(q, k=K + 1)
        out.append((s, i, c))
    return out


res = {"N": N, "D": D, "k": K, "device": torch.cuda.get_device_name(0), "planted_rows": int(rows.shape[0])}
G.knn(K)                            # warm-up (workspaces, first launches)
G.pairs(0.99)
G.search(G.read(0, 10_000), k=K + 1)
kw, sw = [], []
for _ in range(3):                  # alternated
    out, s = timed(lambda: G.knn(K))
    kw.append(s)
    st = G.search_stats()
    _, s = timed(search_route)
    sw.append(s)
(scores, idx, cnt), _, stages = profiled(lambda: G.knn(K))
_, _, p_stages = profiled(lambda: G.pairs(0.9))
join_s, pairs_join_s = stage_seconds(stages, "knn_join"), stage_seconds(p_stages, "pairs_join")
res["planted"] = {"knn_call_s": [round(w, 4) for w in kw], "search_route_s": [round(w, 4) for w in sw],
                  "knn_over_search_route": round(min(kw) / min(sw), 4), "candidates_per_row": round(st["collected_rows"] / N, 2),
                  "candidates": st["collected_rows"], "rows_fell_back": st["large_k_fallback"], "join_passes": st["join_passes"],
                  "rows_with_k_neighbours": int((cnt == K).sum()), "stages": knn_stages(stages), "knn_stages_raw": stages,
                  "pairs_join_s_at_0.9": pairs_join_s,
                  "knn_join_over_pairs_join": round(join_s / pairs_join_s, 4) if join_s and pairs_join_s else None}
print(json.dumps({k: v for k, v in res["planted"].items() if not k.endswith("_raw")}), flush=True)

# one static shot: rows [0, BLOCK) identical
block = min(BLOCK, N)
for s in range(0, block, 8192):
    n = min(8192, block - s)
    G.update(torch.arange(s, s + n), shot.expand(n, D).contiguous())
torch.cuda.synchronize()
(scores, idx, cnt), wall, stages = profiled(lambda: G.knn(K))
st = G.search_stats()
want = torch.arange(K + 1, device=dev)
ok = all(idx[i].tolist() == [j for j in want.tolist() if j != i][:K] for i in (0, 1, K, K + 1, block - 1))
res["dense_block"] = {"rows": block, "knn_call_s": round(wall, 4), "candidates": st["collected_rows"],
                      "rows_fell_back": st["large_k_fallback"], "join_passes": st["join_passes"],
                      "block_rows_list_the_lowest_other_block_rows": ok, "stages": knn_stages(stages), "knn_stages_raw": stages}
print(json.dumps({k: v for k, v in res["dense_block"].items() if not k.endswith("_raw")}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
