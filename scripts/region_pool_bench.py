"""Cost of region embeddings from one forward (revo_vit_forward_regions) on PE-Core-L14-336 at batch 64,
alternated with what it replaces:
  * embed_regions with 0, 3 and 50 regions per image (host bitmaps, no global output for 3 / 50) against embed() of the same
    64 images -- what the region head adds to a forward;
  * 3 regions per image against the crop mode's three forwards of 64 crops (the device side of it: the crops are ready);
  * ingest images/s through SimpleReverso.create_database in the three region modes, on scripts/ingest_bench.py's inputs
    (640 x 480 JPEGs, three fixed boxes per image -- here with their rectangular masks, so that the pool mode has a mask to
    pool over and the crop mode the same mask-derived boxes).
Device events on the launch stream; writes profiles/region_pool_bench.json and prints the same JSON line.
    python scripts/region_pool_bench.py [n_ingest_images]"""
import contextlib
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import reverso_amd
from reverso_amd import engine, regions
from reverso_amd.core_system import Regions, SimpleReverso

dev = torch.device("cuda", 0)
n_ingest = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
cfg = reverso_amd.get_config("PE-Core-L14-336")
B = 64
eng = engine.VitEngine.synthetic(cfg, seed=0, device=0, max_batch=B)
g = torch.Generator().manual_seed(1)
u8 = torch.randint(0, 256, (B, 3, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8).to(dev)
crops = torch.randint(0, 256, (3 * B, 3, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8).to(dev)
rng = np.random.default_rng(2)


def region_set(per):
    """`per` boxes per image of a 640 x 480 source, sides between a tenth and the whole of the frame"""
    ri, bits = [], []
    for b in range(B):
        boxes = []
        for _ in range(per):
            w, h = rng.integers(64, 641), rng.integers(48, 481)
            x0, y0 = rng.integers(0, 640 - w + 1), rng.integers(0, 480 - h + 1)
            boxes.append((x0, y0, x0 + w, y0 + h))
        if per:
            bits.append(regions.token_masks(cfg, boxes, 640, 480))
        ri += [b] * per
    return np.asarray(ri, dtype=np.int64), (np.concatenate(bits) if bits else np.zeros((0, regions.words_per_region(cfg)), np.uint32))


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


sets = {per: region_set(per) for per in (0, 3, 50)}
out = {"what": "scripts/region_pool_bench.py: PE-Core-L14-336 (synthetic weights), batch 64, one MI355X; ms per call, device events, "
               "runs alternated", "batch": B, "forward": {"embed_ms": [], "regions_0_ms": [], "regions_3_ms": [], "regions_50_ms": [],
                                                          "crop_3_forwards_ms": []},
       "tokens_per_region_mean": {per: (round(float(np.mean([bin(int(v)).count("1") for v in s[1].reshape(-1)]) * s[1].shape[1]), 1)
                                        if per else 0) for per, s in sets.items()}}
f = out["forward"]
for _ in range(3):
    f["embed_ms"].append(round(timed(lambda: eng.embed(u8)), 4))
    f["regions_0_ms"].append(round(timed(lambda: eng.embed_regions(u8, *sets[0])), 4))
    f["regions_3_ms"].append(round(timed(lambda: eng.embed_regions(u8, *sets[3], with_global=False)), 4))
    f["regions_50_ms"].append(round(timed(lambda: eng.embed_regions(u8, *sets[50], with_global=False)), 4))
    f["crop_3_forwards_ms"].append(round(timed(lambda: eng.embed(crops)), 4))
best = {k: min(v) for k, v in f.items()}
out["summary"] = {"region_head_3_per_image_ms": round(best["regions_3_ms"] - best["embed_ms"], 4),
                  "region_head_50_per_image_ms": round(best["regions_50_ms"] - best["embed_ms"], 4),
                  "regions_50_over_forward": round(best["regions_50_ms"] / best["embed_ms"], 4),
                  "pool_3_over_crop_3": round(best["regions_3_ms"] / best["crop_3_forwards_ms"], 4),
                  "images_per_s_pool_3_device_only": round(B / best["regions_3_ms"] * 1e3, 1),
                  "images_per_s_crop_3_device_only": round(B / best["crop_3_forwards_ms"] * 1e3, 1)}
print(json.dumps(out["summary"]), file=sys.stderr, flush=True)
eng.close()

# ---- ingest through the facade, the inputs of scripts/ingest_bench.py
if n_ingest > 0:
    root = tempfile.mkdtemp(prefix="region_ingest_")
    folder = os.path.join(root, "images")
    os.makedirs(folder)
    yy, xx = np.mgrid[0:480, 0:640]
    for i in range(n_ingest):
        base = np.stack([(xx * (i % 7 + 1) + yy) % 256, (yy * 2 + i) % 256, (xx + yy * (i % 5)) % 256], -1).astype(np.float32)
        img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, f"img_{i:05d}.jpg"), quality=90)

    def detector(pil, prompt):
        w, h = pil.size
        boxes = [[0, 0, w // 2, h // 2], [w // 4, h // 4, w - 1, h - 1], [w // 3, 0, w - 1, h // 2]]
        masks = np.zeros((3, h, w), dtype=bool)
        for m, (x0, y0, x1, y1) in zip(masks, boxes):
            m[y0:y1, x0:x1] = True
        return Regions(boxes, mask=masks, confidence=[0.9, 0.8, 0.7], class_id=[0, 1, 0], class_names=["person", "car"])

    out["ingest"] = {"images": n_ingest, "regions_per_image": 3, "modes": []}
    for mode in ("global", "crop", "pool"):
        with contextlib.redirect_stdout(sys.stderr):
            r = SimpleReverso(model_name="PE-Core-L14-336", db_root=os.path.join(root, "db_" + mode), max_batch=B,
                              detector=detector, region_mode=mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            r.create_database(folder, "bench")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        row = {"mode": mode, "images_per_s": round(n_ingest / dt, 1), "vectors": len(r.vector_db), "seconds": round(dt, 3),
               "stage_s": {k: round(v, 3) for k, v in r.last_ingest_stats.items() if k.endswith("_s")}}
        out["ingest"]["modes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        r.vector_db.close()
        r.pe_model.close()
    shutil.rmtree(root, ignore_errors=True)

line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "region_pool_bench.json"), "w") as fh:
    fh.write(line + "\n")
print(line)
