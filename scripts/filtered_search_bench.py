"""Cost of a filtered search (revo_search_set_filter): whole-search time at 1 M x 1024 for 1 / 64 / 1000 queries and
allowed fractions 100 / 50 / 10 / 1 / 0.01 % (random masks) against the unfiltered search, the cost of setting the filter
(pack + upload + copy into the handle), and the GalleryStore's evaluation of a payload filter over 1 M payloads.
Device events on the launch stream; one JSON line.
    python scripts/filtered_search_bench.py [N] [D] > profiles/<name>.json"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine, filters

dev = torch.device("cuda", 0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
G = engine.Gallery(D, N, device=0)
g = torch.Generator(device=dev).manual_seed(42)
for s in range(0, N, 131072):
    G.add(torch.randn(min(131072, N - s), D, generator=g, device=dev))


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"N": N, "D": D, "rows": [], "set_filter_ms": {}, "store_filter_eval_ms": {}}
fracs = (1.0, 0.5, 0.1, 0.01, 0.0001)
masks = {f: (torch.rand(N, device=dev, generator=g) < f) if f < 1.0 else torch.ones(N, dtype=torch.bool, device=dev)
         for f in fracs}
# set_filter: packing a device bool mask, and revo_search_set_filter's copy of a packed one into the handle (+ the clear)
from reverso_amd import _lib  # noqa: E402
for f in (1.0, 0.01):
    bits = G.allow_bits(masks[f])
    def setf():
        _lib.check(G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), N, 1, _lib.current_stream()), "set_filter")
        G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    out["set_filter_ms"][str(f)] = {"pack_bool_mask": round(timed(lambda: G.allow_bits(masks[f])), 4),
                                    "set_filter_device_bitmap": round(timed(setf), 4)}
hb = G.allow_bits(masks[0.5]).cpu().numpy()
t0 = time.perf_counter()
for _ in range(5):
    _lib.check(G._lib.revo_search_set_filter(G._h, hb.ctypes.data_as(_lib.C.c_void_p), N, 0, _lib.current_stream()), "set_filter")
out["set_filter_ms"]["host_bitmap_upload"] = round((time.perf_counter() - t0) * 1e3 / 5, 4)
G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
for Q in (1, 64, 1000):
    q = torch.randn(Q, D, generator=g, device=dev)
    for k in (10, 50):
        # alternated: unfiltered, then each fraction (packed bitmaps: set_filter + search + clear per call)
        row = {"Q": Q, "k": k, "unfiltered_ms": [], "filtered_ms": {str(f): [] for f in fracs}}
        packed = {f: G.allow_bits(masks[f]) for f in fracs}
        for _ in range(2):
            row["unfiltered_ms"].append(round(timed(lambda: G.search(q, k)), 4))
            for f in fracs:
                row["filtered_ms"][str(f)].append(round(timed(lambda: G.search(q, k, allow=packed[f])), 4))
        row["ratio_best"] = {f: round(min(v) / min(row["unfiltered_ms"]), 4) for f, v in row["filtered_ms"].items()}
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr)

# store: payload filter evaluation over 1 M payloads (columnar index, first build and then per query)
rng = np.random.default_rng(0)
n_p = 1_000_000
payloads = [{"image_source": f"video{r % 1000}.mp4", "detected_class": ("car", "person", "dog", "bike")[r % 4],
             "confidence": float(c)} for r, c in zip(range(n_p), rng.random(n_p))]
idx = filters.PayloadIndex()
t0 = time.perf_counter()
idx.sync(list(range(n_p)), payloads)
flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car")),
                           filters.FieldCondition("confidence", range=filters.Range(gte=0.5))],
                     must_not=[filters.FieldCondition("image_source", match=filters.MatchValue("video7.mp4"))])
m = idx.evaluate(flt)
out["store_filter_eval_ms"]["first_incl_index_build"] = round((time.perf_counter() - t0) * 1e3, 2)
t0 = time.perf_counter()
for _ in range(5):
    m = idx.evaluate(flt)
    b = filters.pack_bits(m)
out["store_filter_eval_ms"]["per_query_eval_and_pack"] = round((time.perf_counter() - t0) * 1e3 / 5, 2)
out["store_filter_eval_ms"]["allowed_fraction"] = round(float(m.mean()), 4)
print(json.dumps(out))
