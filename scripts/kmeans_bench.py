"""Exact spherical k-means (revo_gallery_kmeans, Gallery.kmeans) over a 1 M x 1024 gallery of planted blobs at C = 256, 1 024 and
4 096 centroids, 10 updates, started from seeded rows: whole-call wall clock, the stages of one profiled call (the library's
profiler: best pass, decide pass, re-score, finish, update), candidates per row and the share of rows decided without a
re-score, alternated with the same partition by the torch route on the same box -- fp32 matmul + argmax + index_add_ per
step, in row blocks -- whose labels are compared with the exact ones.  Writes one JSON file.  One process, no retries: the
first error ends it, and an alarm ends a run that takes too long.
    python scripts/kmeans_bench.py [out.json] [N] [D] [iterations] [limit seconds]"""
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
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/kmeans_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 10
signal.alarm(int(sys.argv[5]) if len(sys.argv) > 5 else 900)            # SIGALRM's default action ends the process
BLOCK = 131072
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
# planted blobs: 2 000 directions, every row one of them plus noise of 0.5 .. 1.5 times its length (scores to its own
# direction from about 0.55 to 0.9)
centre = torch.nn.functional.normalize(torch.randn(min(2000, max(1, N // 100)), D, generator=g, device=dev), dim=1)
for s in range(0, N, BLOCK):
    n = min(BLOCK, N - s)
    owner = torch.randint(0, centre.shape[0], (n,), generator=g, device=dev)
    sigma = 0.5 + torch.rand(n, 1, generator=g, device=dev)
    G.add(centre[owner] + sigma * torch.randn(n, D, generator=g, device=dev) / D ** 0.5)
torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stage_seconds(stages, *names):
    hit = [stages[n]["ms"] for n in names if n in stages]
    return round(sum(hit) / 1e3, 5) if hit else None


def torch_route(init):
    """the same iteration by torch: ITERS x (assign against the centroids, update), then the final assignment"""
    c = torch.nn.functional.normalize(init, dim=1)
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    for it in range(ITERS + 1):
        sums = torch.zeros_like(c)
        for s in range(0, N, BLOCK):
            rows = G.read(s, min(BLOCK, N - s))
            labels[s:s + rows.shape[0]] = (rows @ c.T).argmax(1)
            if it < ITERS:
                sums.index_add_(0, labels[s:s + rows.shape[0]], rows)
        if it < ITERS:
            norm = sums.norm(dim=1, keepdim=True)
            c = torch.where(norm > 0, sums / norm, c)
    return c, labels


res = {"N": N, "D": D, "iterations": ITERS, "device": torch.cuda.get_device_name(0), "configs": {}}
for n_c in (256, 1024, 4096):
    init = torch.cat([G.read(int(r), 1) for r in torch.randperm(N, generator=g, device=dev)[:n_c].tolist()])   # seeded rows
    G.kmeans(init, max_iter=1)                                           # warm-up (workspaces, first launches)
    kw, tw = [], []
    for _ in range(2):                                                   # alternated
        out, s = timed(lambda: G.kmeans(init, max_iter=ITERS))
        kw.append(s)
        st = G.search_stats()
        (tc, tl), s = timed(lambda: torch_route(init))
        tw.append(s)
    engine.prof_reset()
    engine.prof_enable(True)
    out, wall = timed(lambda: G.kmeans(init, max_iter=ITERS))
    stages = engine.prof_report()
    engine.prof_enable(False)
    cents, labels, scores, sizes, n_iter, converged = out
    steps = n_iter + 1                                                   # assignments run
    res["configs"][str(n_c)] = {
        "kmeans_call_s": [round(w, 4) for w in kw], "torch_route_s": [round(w, 4) for w in tw],
        "kmeans_over_torch_route": round(min(kw) / min(tw), 4), "n_iter": n_iter, "converged": converged,
        "assignment_passes": st["join_passes"], "candidates_beyond_one_per_row_and_step": round(st["collected_rows"] / N / steps, 4),
        "share_of_rows_decided_without_a_rescore": round(1.0 - st["large_k_fallback"] / N / steps, 4),
        "non_empty_clusters": int((sizes > 0).sum()), "largest_cluster": int(sizes.max()),
        "labels_equal_to_the_torch_route": round(float((labels.to(torch.int64) == tl).float().mean()), 6),
        "profiled_call_s": round(wall, 4),
        "stages": {"init_s": stage_seconds(stages, "kmeans_init"), "best_s": stage_seconds(stages, "kmeans_best"),
                   "decide_s": stage_seconds(stages, "kmeans_decide"), "rescore_s": stage_seconds(stages, "kmeans_rescore"),
                   "finish_s": stage_seconds(stages, "kmeans_finish"), "update_s": stage_seconds(stages, "kmeans_update")},
        "per_step": {"assign_pass_pflops": None, "update_gb_per_s": None}, "stages_raw": stages}
    cfg = res["configs"][str(n_c)]
    passes = 2 * steps                                                   # a best and a decide walk per step
    mfma_s = (cfg["stages"]["best_s"] or 0) + (cfg["stages"]["decide_s"] or 0)
    if mfma_s > 0:
        cfg["per_step"]["assign_pass_pflops"] = round(2.0 * N * ((n_c + 255) // 256 * 256) * D * passes / mfma_s / 1e15, 4)
    if cfg["stages"]["update_s"] and n_iter:
        cfg["per_step"]["update_gb_per_s"] = round(N * D * 4.0 * n_iter / cfg["stages"]["update_s"] / 1e9, 1)
    print(json.dumps({k: v for k, v in cfg.items() if not k.endswith("_raw")}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
