"""CPU: the host-side pieces of a gallery build (revers-o_amd/ingest.py): the image listing, the status log, the
ingest mode and the frame slab (without pinning: no device)."""
import os
import threading

import numpy as np
import torch

import reverso_amd  # noqa: F401
from reverso_amd import ingest


def test_list_images_subfolders_extension_case_and_order(tmp_path):
    for rel in ("b.JPG", "a.png", "c.Jpeg", "notes.txt", "d.webp.bak", "sub/z.bmp", "sub/deep/A.TIFF", "sub/readme.md"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"x")
    root = str(tmp_path)
    flat = ingest.list_images(root)
    assert flat == [os.path.join(root, n) for n in ("a.png", "b.JPG", "c.Jpeg")] and flat == ingest.list_images(root, False)
    deep = ingest.list_images(root, include_subfolders=True)
    assert deep == sorted(os.path.join(root, *rel.split("/")) for rel in ("a.png", "b.JPG", "c.Jpeg", "sub/z.bmp", "sub/deep/A.TIFF"))
    assert ingest.list_images(str(tmp_path / "sub" / "deep")) == [os.path.join(root, "sub", "deep", "A.TIFF")]
    (tmp_path / "empty").mkdir()
    assert ingest.list_images(str(tmp_path / "empty"), True) == []


def test_status_log_forwards_every_message_and_joins_lazily():
    seen = []
    log = ingest.StatusLog(lambda m, v: seen.append((m, v)))
    assert str(log) == ""
    first = log("one")
    second = log("two", 0.5)
    assert seen == [("one", None), ("two", 0.5)]
    assert str(second) == "one\ntwo" and str(first) == "one\ntwo"          # the log so far, whenever it is looked at
    log("three", 1.0)
    assert str(second) == "one\ntwo\nthree" and seen[-1] == ("three", 1.0)
    quiet = ingest.StatusLog()                                            # no callback
    assert str(quiet("only")) == "only"


def test_ingest_mode_names_the_five_routes_once():
    of = ingest.IngestMode.of
    cpus = os.cpu_count() or 8
    m = of("global", True, False)
    assert (m.crop, m.pool, m.per_region, m.host_resize, m.pipelined, m.decode_threads) == (False, False, False, True, True, min(cpus, 16))
    assert of("global", False, False) == m and of("crop", True, False) == m and of("pool", True, False) == m     # direct PE: no regions
    m = of("global", False, True)
    assert (m.per_region, m.host_resize, m.pipelined, m.decode_threads) == (False, False, False, min(cpus, 8))
    for resize in (False, True):
        m = of("crop", False, resize)
        assert (m.crop, m.pool, m.per_region, m.host_resize, m.pipelined, m.decode_threads) == (True, False, True, False, False, min(cpus, 6))
    m = of("pool", False, False)
    assert (m.crop, m.pool, m.per_region, m.host_resize, m.pipelined, m.decode_threads) == (False, True, True, True, False, min(cpus, 16))
    m = of("pool", False, True)
    assert (m.pool, m.per_region, m.host_resize, m.pipelined, m.decode_threads) == (True, True, False, False, min(cpus, 8))
    assert of("pool", False, True, 3).decode_threads == 3 and of("global", True, False, 40).decode_threads == 40


def test_frame_slab_without_pinning():
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (int(rng.integers(3, 40)), int(rng.integers(3, 40)), 3), dtype=np.uint8) for _ in range(64)]
    padded = sum((f.size + 255) & ~255 for f in frames)
    slab = ingest.FrameSlab(pin=False)
    results = [None] * len(frames)

    def fill(t):
        for i in range(t, len(frames), 8):
            results[i] = slab.put(frames[i])

    def eight_threads():
        threads = [threading.Thread(target=fill, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()

    # first round: no memory yet, every frame comes back as a pageable tensor and still counts into `wanted`
    eight_threads()
    assert all(off is None and torch.equal(x, torch.from_numpy(f)) for (off, x), f in zip(results, frames))
    assert slab.wanted == padded and slab.used == 0
    slab.reset()
    assert slab.buf.numel() == int(padded * 1.25) and not slab.buf.is_pinned() and (slab.used, slab.wanted) == (0, 0)
    # second round: every frame fits; ranges are 256-byte aligned, disjoint, and hold the frames
    eight_threads()
    assert slab.used == slab.wanted == padded
    spans = sorted((off, off + ((f.size + 255) & ~255)) for (off, _), f in zip(results, frames))
    assert all(off % 256 == 0 for off, _ in spans) and spans[0][0] == 0 and spans[-1][1] == padded
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for (off, shape), f in zip(results, frames):
        assert shape == f.shape and np.array_equal(slab.buf[off:off + f.size].view(shape).numpy(), f)
    # a frame that does not fit in what is left: the pageable fallback, counted
    big = rng.integers(0, 256, (slab.buf.numel() - padded + 1,), dtype=np.uint8)
    off, x = slab.put(big)
    assert off is None and torch.equal(x, torch.from_numpy(big)) and slab.used == padded
    wanted = padded + ((big.size + 255) & ~255)
    assert slab.wanted == wanted
    slab.reset()
    assert slab.buf.numel() == int(wanted * 1.25) and (slab.used, slab.wanted) == (0, 0)
    slab.reset()                                                          # nothing wanted: the buffer stays
    assert slab.buf.numel() == int(wanted * 1.25)
