"""Removing and overwriting rows of a 1 M x 1024 gallery in place (revo_gallery_remove / revo_gallery_update; Gallery.remove /
update): remove row 0 only, 1 % of the rows scattered, 50 % scattered; update 1 000 rows.  Per case: the
wall clock of the call (medians of alternated rounds, each on a freshly filled gallery), the bytes the scheme moves (read plus
write: a survivor that moves costs its row twice when its chunk goes directly, four times when it goes through staging), that
traffic over the copy rate of revo_probe_copy measured on the same device, and the only route there was before: read the
surviving rows, make a new Gallery, add them.  Writes one JSON file.
    python scripts/gallery_mutate_bench.py [out.json] [N] [D] [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine

dev = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/gallery_mutate_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
g = torch.Generator(device=dev).manual_seed(42)
x = torch.nn.functional.normalize(torch.randn(N, D, generator=g, device=dev), dim=1)
G = engine.Gallery(D, N, device=0)


def fill():
    G.clear()
    for s in range(0, N, 131072):
        G.add(x[s:s + 131072], normalize=False)
    torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def copy_rate():
    """bytes per second of revo_probe_copy (read plus write) on 1 GiB"""
    lib, nbytes = _lib.load(), 1 << 30
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 256, generator=g)
    b = torch.empty_like(a)
    st = _lib.current_stream()
    ms = []
    for _ in range(7):
        ms.append(wall(lambda: _lib.check(lib.revo_probe_copy(_lib.ptr(b), _lib.ptr(a), nbytes, st)))[0])
    return 2.0 * nbytes / (statistics.median(ms[2:]) * 1e-3)


def remove_traffic(mask):
    """bytes revo_gallery_remove reads plus writes for this mask: the plan of gallery.hip's chunk loop, on the host"""
    chunk = min(65536, max(32, (64 << 20) // (D * 4) // 32 * 32))
    m = mask.cpu()
    row_bytes = D * 4 + D * 2
    base = total = 0
    staged_chunks = direct_chunks = 0
    for row0 in range(0, N, chunk):
        part = m[row0:row0 + chunk]
        kept = int((~part).sum())
        gone = torch.nonzero(part)
        j0 = min(int(gone[0]) if gone.numel() else part.shape[0], kept) if base == row0 else 0
        if kept > j0:
            direct = base + kept <= row0
            total += (kept - j0) * row_bytes * (2 if direct else 4)
            direct_chunks += direct
            staged_chunks += not direct
        base += kept
    return total, direct_chunks, staged_chunks


def rebuild(keep_rows=None, new_rows=None, new_vecs=None):
    """the route without the edit calls: the surviving (or changed) rows read, a new gallery filled with them"""
    rows = G.read()
    if keep_rows is not None:
        rows = rows[keep_rows]
    if new_rows is not None:
        rows[new_rows] = torch.nn.functional.normalize(new_vecs, dim=1)
    G2 = engine.Gallery(D, N, device=0)
    for s in range(0, rows.shape[0], 131072):
        G2.add(rows[s:s + 131072], normalize=False)
    torch.cuda.synchronize()
    n = len(G2)
    G2.close()
    return n


rate = copy_rate()
res = {"N": N, "D": D, "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "probe_copy_tbs": round(rate / 1e12, 3),
       "cases": []}
print(json.dumps({"probe_copy_tbs": res["probe_copy_tbs"]}), flush=True)

masks = {"remove_row0": torch.zeros(N, dtype=torch.bool, device=dev),
         "remove_1pct_scattered": torch.rand(N, generator=g, device=dev) < 0.01,
         "remove_50pct_scattered": torch.rand(N, generator=g, device=dev) < 0.5}
masks["remove_row0"][0] = True
for name, mask in masks.items():
    bits = G.allow_bits(mask)                     # packed once: the call is timed, not the packing of a bool mask
    keep = torch.nonzero(~mask).reshape(-1)
    t_new, t_old = [], []
    for r in range(ROUNDS + 1):                   # (round 0: warm-up -- staging buffer, first launches)
        fill()
        ms, removed = wall(lambda: G.remove(bits))
        assert removed == int(mask.sum()) and len(G) == N - removed
        fill()
        ms_old, n_old = wall(lambda: rebuild(keep_rows=keep))
        assert n_old == N - removed
        if r:
            t_new.append(ms)
            t_old.append(ms_old)
    engine.prof_reset()
    engine.prof_enable(True)
    fill()
    G.remove(bits)
    stages = engine.prof_report()
    engine.prof_enable(False)
    traffic, direct_chunks, staged_chunks = remove_traffic(mask)
    row = {"case": name, "rows_removed": int(mask.sum()), "median_ms": round(statistics.median(t_new), 3),
           "runs_ms": [round(v, 3) for v in t_new], "rebuild_median_ms": round(statistics.median(t_old), 3),
           "rebuild_runs_ms": [round(v, 3) for v in t_old], "bytes_moved": traffic, "chunks_direct": direct_chunks,
           "chunks_staged": staged_chunks, "expected_ms_at_probe_rate": round(traffic / rate * 1e3, 3),
           "device_ms": stages.get("gallery_remove", {}).get("ms")}
    res["cases"].append(row)
    print(json.dumps(row), flush=True)

idx = torch.randperm(N, generator=g, device=dev)[:1000].cpu()
vecs = torch.randn(1000, D, generator=g, device=dev)
t_new, t_old = [], []
fill()
for r in range(ROUNDS + 1):
    ms, _ = wall(lambda: G.update(idx, vecs))
    ms_old, _ = wall(lambda: rebuild(new_rows=idx.to(dev), new_vecs=vecs))
    if r:
        t_new.append(ms)
        t_old.append(ms_old)
traffic = 1000 * (D * 4 + D * 4 + D * 2)          # the vectors read, the fp32 and bf16 rows written
row = {"case": "update_1000_rows", "median_ms": round(statistics.median(t_new), 3), "runs_ms": [round(v, 3) for v in t_new],
       "rebuild_median_ms": round(statistics.median(t_old), 3), "rebuild_runs_ms": [round(v, 3) for v in t_old],
       "bytes_moved": traffic, "expected_ms_at_probe_rate": round(traffic / rate * 1e3, 4)}
res["cases"].append(row)
print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", OUT)
