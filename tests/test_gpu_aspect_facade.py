"""SimpleReverso(aspect="keep"): a folder of 40 small JPEGs in five aspect ratios, built into a
database in each of the three region modes -- every batch of the build holds frames of several grids, so the rows must come
back in file and region order from the groups they were embedded in -- and queried; aspect="squash" stays what it was."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import reverso_amd  # noqa: F401
from reverso_amd import config, preprocess as pp, regions
from reverso_amd.core_system import Regions, SimpleReverso

pytestmark = pytest.mark.gpu

SHAPES = [(40, 160), (60, 100), (80, 80), (100, 60), (160, 40)]           # h x w: the grids (2,8) (3,5) (4,4) (5,3) (8,2)
GRIDS = [(2, 8), (3, 5), (4, 4), (5, 3), (8, 2)]
BAR = 0.99995                                                             # the project's batch-invariance bar


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("aspect_images")
    rng = np.random.default_rng(12)
    paths = []
    for i in range(40):                                                   # the shapes alternate: every batch mixes grids
        h, w = SHAPES[i % 5]
        arr = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        p = str(root / f"img_{i:03d}.jpg")
        Image.fromarray(arr).save(p, quality=92)
        paths.append(p)
    return str(root), paths


def _masks(w, h):
    m = np.zeros((3, h, w), dtype=bool)
    m[0, : h // 2, : w // 2] = True                                       # a quadrant: the image's own aspect
    m[1, h // 4:, w // 2: w // 2 + max(2, w // 8)] = True                 # a tall sliver
    m[2, h // 3: h // 3 + max(2, h // 8), :] = True                       # a wide band
    return m


def _detector(pil, prompt):
    w, h = pil.size
    m = _masks(w, h)
    boxes = []
    for k in range(3):
        ys, xs = np.where(m[k])
        boxes.append([int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())])
    return Regions(boxes, mask=m, confidence=[0.9, 0.8, 0.7], class_id=[0, 1, 0], class_names=["person", "car"])


def _system(tmp_path, name, **kw):
    return SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / name), max_batch=16, device_resize=True, **kw)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)


def _embed_at(r, pil, grid):
    P = r.pe_model.cfg.patch_size
    u8 = pp.resize_u8(pil, (grid[0] * P, grid[1] * P))[None].to(r.device)
    return r.pe_model.embed(u8, grid=grid)[0]


def test_direct_pe_build_and_query(tmp_path, folder, dev):
    root, paths = folder
    r = _system(tmp_path, "direct", aspect="keep")
    cfg = r.pe_model.cfg
    msg = r.create_database(root, "d", use_direct_pe=True)
    assert "✅" in msg and len(r.vector_db) == 40
    assert [p["filename"] for p in r.vector_db.payloads] == [os.path.basename(p) for p in paths]
    assert r.vector_db.build_info["aspect"] == "keep" and r.vector_db.build_info["aspect_max_ratio"] == 4.0
    stored = r.vector_db.gallery.read()
    want = []
    for i, p in enumerate(paths):
        pil = Image.open(p).convert("RGB")
        grid = config.aspect_grid(cfg, pil.height, pil.width)
        assert grid == GRIDS[i % 5]
        want.append(_embed_at(r, pil, grid))
    cos = _cos(stored, torch.stack(want))
    print("direct PE, keep: min cosine to the per-file embedding", cos.min().item())
    assert (cos >= BAR).all(), cos.min().item()
    # a shuffled assignment would not pass: files of different shapes are different vectors
    assert _cos(stored[:-1], torch.stack(want)[1:]).max().item() < BAR
    # the query of a 1:4 image is its (2, 8) embedding, and finds its own row
    embs, metas = r.process_image_direct_pe(paths[0])
    assert torch.equal(embs[0], want[0].cpu()) and metas[0]["bbox"] == [0, 0, 160, 40]
    _, items = r.search_similar(0.0, 1)
    assert items[0]["filename"] == os.path.basename(paths[0]) and items[0]["score"] > 0.9999
    # the squashed embedding of the same file is another vector
    sq = r.pe_model.embed(pp.resize_u8(Image.open(paths[0]).convert("RGB"), 56)[None].to(dev))[0]
    assert _cos(sq, want[0]).item() < BAR
    # a system in the other mode says so when it loads the database; one in the same mode does not
    other = _system(tmp_path, "direct")
    assert other.aspect == "squash"
    status = other.load_database("d")
    assert "✅ Loaded database: d" in status and "aspect='keep'" in status and "aspect='squash'" in status
    assert r.load_database("d") == "✅ Loaded database: d"


def test_crop_mode_takes_each_crops_grid_from_its_box(tmp_path, folder, dev):
    root, paths = folder
    r = _system(tmp_path, "crop", aspect="keep", detector=_detector, region_mode="crop")
    cfg = r.pe_model.cfg
    msg = r.create_database(root, "c", text_prompt="person . car")
    assert "✅" in msg and len(r.vector_db) == 120
    assert r.vector_db.build_info["aspect"] == "keep" and r.vector_db.build_info["region_mode"] == "crop"
    stored, payloads = r.vector_db.gallery.read(), r.vector_db.payloads
    want, seen = [], set()
    for i, p in enumerate(paths):
        pil = Image.open(p).convert("RGB")
        for k in range(3):
            pay = payloads[3 * i + k]
            assert pay["filename"] == os.path.basename(p) and pay["detection_index"] == k
            x0, y0, x1, y1 = pay["bbox"]                                  # inclusive, mask derived
            grid = config.aspect_grid(cfg, y1 + 1 - y0, x1 + 1 - x0)
            seen.add(grid)
            want.append(_embed_at(r, pil.crop((x0, y0, x1 + 1, y1 + 1)), grid))
    assert len(seen) >= 4, seen                                           # slivers, bands and quadrants of five shapes
    cos = _cos(stored, torch.stack(want))
    print("crop, keep: min cosine", cos.min().item(), "grids", sorted(seen))
    assert (cos >= BAR).all(), cos.min().item()
    r.detect_regions(paths[3], "person . car")
    embs, metas = r.extract_embeddings(paths[3])
    assert len(embs) == 3 and (_cos(torch.stack(embs), torch.stack(want[9:12])) >= BAR).all()


def test_pool_mode_pools_the_masks_tokens_on_the_images_grid(tmp_path, folder, dev):
    root, paths = folder
    r = _system(tmp_path, "pool", aspect="keep", detector=_detector, region_mode="pool")
    cfg = r.pe_model.cfg
    msg = r.create_database(root, "p", text_prompt="person . car")
    assert "✅" in msg and len(r.vector_db) == 120
    assert r.vector_db.build_info["aspect"] == "keep" and r.vector_db.build_info["region_mode"] == "pool"
    stored = r.vector_db.gallery.read()
    want = []
    for i, p in enumerate(paths):
        pil = Image.open(p).convert("RGB")
        grid = GRIDS[i % 5]
        u8 = pp.resize_u8(pil, (grid[0] * cfg.patch_size, grid[1] * cfg.patch_size))[None].to(dev)
        bits = regions.token_masks(cfg, list(_masks(pil.width, pil.height)), pil.width, pil.height, grid=grid)
        want.append(r.pe_model.embed_regions(u8, [0, 0, 0], bits, with_global=False, grid=grid)[1])
    want = torch.cat(want)
    cos = _cos(stored, want)
    print("pool, keep: min cosine", cos.min().item())
    assert (cos >= BAR).all(), cos.min().item()
    assert torch.unique(stored, dim=0).shape[0] == 120
    r.detect_regions(paths[4], "person . car")
    embs, _ = r.extract_embeddings(paths[4])
    assert len(embs) == 3 and (_cos(torch.stack(embs), want[12:15]) >= BAR).all()


def test_squash_is_what_it_was_and_keep_needs_the_device_resize(tmp_path, folder, dev):
    root, paths = folder
    r = _system(tmp_path, "squash")
    msg = r.create_database(root, "s", use_direct_pe=True)
    assert "✅" in msg and len(r.vector_db) == 40
    assert "aspect" not in r.vector_db.build_info                         # the manifest of a squash build is the parent's
    frames = torch.stack([pp.resize_u8(Image.open(p).convert("RGB"), 56) for p in paths]).to(dev)
    cos = _cos(r.vector_db.gallery.read(), r.pe_model.embed(frames))
    assert (cos >= BAR).all(), cos.min().item()
    embs, _ = r.process_image_direct_pe(paths[0])
    assert torch.equal(embs[0], r.pe_model.embed(frames[:1])[0].cpu())
    host = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "host"), max_batch=16, aspect="keep")
    msg = host.create_database(root, "h", use_direct_pe=True)
    assert msg.startswith("❌") and "device_resize=True" in msg and host.vector_db is None
    embs, _ = host.process_image_direct_pe(paths[0])                       # queries do not depend on the build route
    pil = Image.open(paths[0]).convert("RGB")
    assert torch.equal(embs[0], _embed_at(host, pil, (2, 8)).cpu())
    with pytest.raises(ValueError):
        SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "bad"), aspect="pad")
