"""Duplicate clusters (revo_gallery_clusters, Gallery.clusters) over the 1 M x 1024 planted gallery of scripts/pairs_bench.py
at thresholds 0.9 and 0.95, alternated with the route it replaces (Gallery.pairs, the pairs copied to the host,
store.connected_groups): whole-call wall clock of both (both are synchronous), the join alone and the other stages (the
library's profiler, one profiled call each), the ambiguous pairs re-scored, whether the two routes give the same groups.
Then the same gallery with its first 30 000 rows overwritten by one vector -- a static shot, 4.5e8 pairs, which the pairs
route refuses: the clusters call's time and join time next to the planted gallery's, and the block's share of the join's
tile pairs (what the added time should be in proportion to, if the dense epilogue is cheap).  Writes one JSON file.
    python scripts/clusters_bench.py [out.json] [N] [D] [block]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, store

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/clusters_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
BLOCK = int(sys.argv[4]) if len(sys.argv) > 4 else 30_000
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
    fn()
    stages = engine.prof_report()
    engine.prof_enable(False)
    return stages


def clusters_route(t):
    labels, offsets, members = G.clusters(t)
    return store.split_clusters(offsets.cpu().numpy(), members.cpu().numpy())


def pairs_route(t):
    pairs, _ = G.pairs(t)
    return store.connected_groups(pairs.cpu().numpy(), N)


def stage_seconds(stages, name):
    """seconds of one kernel class in a profiler report ({class: {"launches", "ms"}}), None when it did not run"""
    return round(stages[name]["ms"] / 1e3, 5) if name in stages else None


T = (N + 255) // 256
res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "planted_rows": int(rows.shape[0]), "tile_pairs": T * (T + 1) // 2,
       "thresholds": []}
G.clusters(0.99)                    # warm-up (workspaces, first launches)
G.pairs(0.99)
join_planted = {}
for t in (0.9, 0.95):
    cw, pw = [], []
    for _ in range(3):              # alternated
        cg, s = timed(lambda: clusters_route(t))
        cw.append(s)
        pg, s = timed(lambda: pairs_route(t))
        pw.append(s)
    kernel_only = [timed(lambda: G.clusters(t))[1] for _ in range(2)]
    st = G.search_stats()
    c_stages = profiled(lambda: G.clusters(t))
    p_stages = profiled(lambda: G.pairs(t))
    join_planted[t] = stage_seconds(c_stages, "clusters_join")
    row = {"threshold": t, "clusters": len(cg), "members": sum(len(c) for c in cg), "rescored_pairs": st["collected_rows"],
           "join_passes": st["join_passes"], "clusters_route_s": [round(w, 4) for w in cw],
           "pairs_route_s": [round(w, 4) for w in pw], "clusters_call_s": [round(w, 4) for w in kernel_only],
           "routes_equal": cg == pg, "clusters_stages": c_stages, "pairs_stages": p_stages,
           "clusters_join_s": join_planted[t], "pairs_join_s": stage_seconds(p_stages, "pairs_join")}
    res["thresholds"].append(row)
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_stages")}), flush=True)

# one static shot: rows [0, BLOCK) identical
block = min(BLOCK, N)
for s in range(0, block, 8192):
    n = min(8192, block - s)
    G.update(torch.arange(s, s + n), shot.expand(n, D).contiguous())
torch.cuda.synchronize()
TB = (block + 255) // 256
res["dense_block"] = {"rows": block, "edges": block * (block - 1) // 2, "tile_pairs": TB * (TB + 1) // 2,
                      "tile_pair_share": TB * (TB + 1) / (T * (T + 1)), "thresholds": []}
for t in (0.9, 0.95):
    walls = []
    for _ in range(3):
        out, s = timed(lambda: G.clusters(t))
        walls.append(s)
    st = G.search_stats()
    stages = profiled(lambda: G.clusters(t))
    labels, offsets, members = out
    sizes_c = (offsets[1:] - offsets[:-1])
    join_s = stage_seconds(stages, "clusters_join")
    try:
        G.pairs(t)
        refused = None
    except _lib.RevoError as e:
        refused = str(e)[:200]
    row = {"threshold": t, "clusters": int(offsets.shape[0] - 1), "largest_cluster": int(sizes_c.max()),
           "block_is_one_cluster": bool((labels[:block] == 0).all()), "rescored_pairs": st["collected_rows"],
           "join_passes": st["join_passes"], "clusters_call_s": [round(w, 4) for w in walls], "clusters_stages": stages,
           "clusters_join_s": join_s, "pairs_route": "refused: " + refused if refused else "not refused"}
    if join_s is not None and join_planted.get(t):
        row["join_time_added_by_the_block_share"] = round((join_s - join_planted[t]) / join_s, 5)
    res["dense_block"]["thresholds"].append(row)
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_stages")}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
