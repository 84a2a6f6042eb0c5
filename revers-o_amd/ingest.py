"""A gallery build from "folder" to "swapped-in collection": what ``SimpleReverso.create_database`` runs.
Three things overlap: the decode pool works on batches i+1 .. i+DEPTH, the device embeds batch i (its vectors stay
there), and the ingest thread does the per-image bookkeeping of batch i-1."""
import contextlib
import json
import os
import random
import shutil
import threading
import time
import uuid
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime
from typing import NamedTuple

import numpy as np
import torch
from PIL import Image

from . import preprocess as pp
from . import store as st

IMAGE_EXTENSIONS = ['.jpg', '.jpeg', '.png', '.bmp', '.tiff', '.webp']
BUILDING = ".building"      # suffix of the directory a collection is built in (renamed over the old one when complete)
DEPTH = 2                   # batches the decode pool works ahead of the one being embedded
NSLOT = DEPTH + 2           # host buffers (staging rows or frame slabs): batch n uses number n % NSLOT -- decoding / waiting / being uploaded

_uuid_rng = random.Random()   # ids only have to be unique (uuid4 format as upstream), not unpredictable


def uuid4():
    """uuid.uuid4() without the os.urandom system call (35 us each, three per stored region)"""
    return str(uuid.UUID(int=_uuid_rng.getrandbits(128), version=4))


def list_images(folder_path, include_subfolders=False):
    """The files of a build, sorted: by extension (any case), from the folder or from its whole tree"""
    if include_subfolders:
        files = [os.path.join(root, f) for root, _, names in os.walk(folder_path) for f in names]
    else:
        files = [os.path.join(folder_path, f) for f in os.listdir(folder_path)]
    return sorted(f for f in files if f.lower().endswith(tuple(IMAGE_EXTENSIONS)))


class StatusLog:
    """The log of a build.  Calling it appends a message, forwards ``(message, progress)`` to the callback and returns
    the log itself, whose ``str()`` is every message so far: joined only if somebody looks at it (the reference joins on
    every call, which is quadratic in the number of images)."""

    def __init__(self, callback=None):
        self.messages, self.callback = [], callback

    def __call__(self, message, progress_value=None):
        self.messages.append(message)
        if self.callback:
            self.callback(message, progress_value)
        return self

    def __str__(self):
        return "\n".join(self.messages)


class FrameSlab:
    """Pinned host memory for the decoded frames of ONE batch: the decode threads reserve ranges (a bump counter
    under a lock) and copy their frames in; the ingest thread uploads the used prefix with one asynchronous
    copy.  A frame that does not fit goes up from pageable memory and the slab is enlarged for the next round."""

    def __init__(self, pin=True):
        # no memory yet: the first batch of a slab goes up from pageable memory and tells how much the slab needs; it is
        # pinned (tens of ms) when the slab comes round again, by which time the device has batches queued
        self.buf = torch.empty(0, dtype=torch.uint8)
        self.pin, self.lock = pin, threading.Lock()
        self.used = self.wanted = 0                    # bytes handed out / bytes asked for, this round

    def reset(self):
        if self.wanted > self.buf.numel():
            buf = torch.empty(int(self.wanted * 1.25), dtype=torch.uint8)
            self.buf = buf.pin_memory() if self.pin else buf
        self.used = self.wanted = 0

    def put(self, arr):
        """-> (offset, shape) of the frame's copy in the slab, or (None, a pageable tensor) if it did not fit"""
        size = (arr.size + 255) & ~255
        with self.lock:
            off = self.used
            self.wanted += size
            if off + size > self.buf.numel():
                return None, torch.from_numpy(np.array(arr, dtype=np.uint8))
            self.used = off + size
        np.copyto(self.buf[off:off + arr.size].view(arr.shape).numpy(), arr)
        return off, arr.shape


class IngestMode(NamedTuple):
    """How a batch reaches the device, decided once per build: staged (pipelined), device resize, crop, pool with host
    resize, pool with device resize (DESIGN.md 4v lists them with their host buffers)."""
    crop: bool            # one forward per region, from its crop on the device (frames go up through slabs)
    pool: bool            # one forward per image, every region attention-pooled over its mask's tokens
    per_region: bool      # crop or pool: one vector per region, queued with its batch
    host_resize: bool     # PIL resize in the decode pool; else the frames go up as decoded, through slabs
    pipelined: bool       # host resize into pinned staging rows, one embedded row per file
    decode_threads: int

    @classmethod
    def of(cls, region_mode, use_direct_pe, device_resize, decode_workers=None):
        crop = region_mode == "crop" and not use_direct_pe
        pool = region_mode == "pool" and not use_direct_pe
        host_resize = not device_resize and not crop
        # enough decode threads to feed the device in this mode and no more (SimpleReverso.__init__)
        threads = decode_workers or min(os.cpu_count() or 8, 16 if host_resize else (6 if crop else 8))
        return cls(crop, pool, crop or pool, host_resize, host_resize and not (crop or pool), threads)


class Batch(NamedTuple):
    """A batch in flight: queued on the device, its bookkeeping still to do"""
    start: int            # index of its first file in the run's list
    paths: list
    pils: list            # per file: the decoded image, or the exception that opening it raised
    dev_emb: object       # its vectors on the device, or None: a row per file (pipelined), per decoded file, or per region
    last: bool
    det: object           # per-region modes: per file (n_regions, metas, pool bitmaps), None for a failed file


class IngestRun:
    """One build for the ``SimpleReverso`` ``sr``: its files, store, stats, mode, host buffers and counters."""

    def __init__(self, sr, folder_path, database_name, text_prompt, use_direct_pe, resume, include_subfolders, log, skip):
        self.sr, self.log, self.skip = sr, log, skip   # (skip: the files a resumed build already holds)
        self.folder_path, self.database_name, self.text_prompt = folder_path, database_name, text_prompt
        self.use_direct_pe, self.resume, self.include_subfolders = use_direct_pe, resume, include_subfolders
        self.db_path = os.path.join(sr.db_root, database_name)
        self.build_path = self.db_path + BUILDING
        self.ckpt_base = os.path.join(sr.db_root, "checkpoints", f"{database_name}_checkpoint")
        self.collection = f"simple_reverso_{database_name}"
        self.mode = IngestMode.of(sr.region_mode, use_direct_pe, sr.device_resize, sr.decode_workers)
        self.B, self.model_size = sr.max_batch, sr.pe_model.cfg.image_size
        self.files, self.store_db, self.stats, self.stage, self.slabs = [], None, None, None, None
        self.h2d_done = [None] * NSLOT                 # event behind the upload that read a staging buffer
        self.frames_done = [None] * NSLOT              # event behind the upload that read a slab
        self.pending = []                              # futures of the batches being decoded, oldest first
        self.done_files = []                           # files finished (stored, failed or empty) since the last upsert
        self.processed = self.failed = self.submitted = 0
        self.last_ckpt = self.t_start = 0.0

    def run(self):
        sr, log = self.sr, self.log
        early = self.prepare()
        if early is not None:
            return early
        stats = self.stats
        inflight = None
        for it in range(0, (len(self.files) + self.B - 1) // self.B):
            if sr._stop_requested:
                if inflight is not None:
                    self.finalize(inflight)
                return self.stopped("🛑 Stop requested. Saving progress...")
            self.top_up(it)
            futures = self.pending.pop(0)
            t_w = time.perf_counter()
            results = [f.result() for f in futures]
            stats["wait_decode_s"] += time.perf_counter() - t_w
            t_l = time.perf_counter()
            cur = self.launch(it, results)
            stats["launch_s"] += time.perf_counter() - t_l
            self.settle(inflight)
            inflight = cur
        self.settle(inflight)
        store_db = self.store_db
        if len(store_db) == 0:
            store_db.close()                                    # nothing to keep: no empty build directory or note stays behind
            sr._build_store = None
            shutil.rmtree(self.build_path, ignore_errors=True)
            st.remove_checkpoint(self.ckpt_base)
            return str(log("❌ No embeddings extracted from any images"))
        log(f"📦 Recreated collection: {self.collection}", 0.8)
        if sr._stop_requested:
            # a stop between the last embed batch and the completion of the collection: everything is in the shards
            return self.stopped("🛑 Stop requested during database storage. Progress saved.")
        with sr._lock:
            t_f = time.perf_counter()
            store_db.save()                                     # the last delta shard + the "complete" line
            stats["flush_s"] += time.perf_counter() - t_f
            log(f"💾 Stored {len(store_db)} points in {store_db._shards} shards", 0.9)
            if sr.vector_db is not None:
                sr.vector_db.close()
            st.swap_in(self.build_path, self.db_path)           # recreate_collection: the new one replaces the old one only now
            store_db.path = self.db_path
            sr.vector_db = store_db
            sr._build_store = None
            sr.current_database = self.collection
        if os.path.exists(self.ckpt_base + ".json"):
            st.remove_checkpoint(self.ckpt_base)
            log("🧹 Cleaned up checkpoint file")
        stats["total_s"] = time.perf_counter() - self.t_start
        stats["vectors"] = len(sr.vector_db)
        log("\n📊 Final Summary:", 0.9)
        log(f"✅ Successfully processed: {self.processed} images")
        if self.failed > 0:
            log(f"⚠️ Failed to process: {self.failed} images")
        log(f"🔍 Total embeddings stored: {len(sr.vector_db)}")
        log(f"🎯 Database '{self.database_name}' ready for searching!", 1.0)
        return str(log)

    def prepare(self):
        """The file list, the collection being built, the stats and the host buffers; a message if there is nothing to do"""
        sr, log, mode = self.sr, self.log, self.mode
        log(f"📁 Creating database '{self.database_name}' from {self.folder_path}")
        files = list_images(self.folder_path, self.include_subfolders)
        if not files:
            return str(log(f"❌ No images found in {self.folder_path}"))
        if self.resume:
            files = [f for f in files if f not in self.skip]
            if not files and sr._build_store is None:
                return str(log("✅ All files already processed. Database is complete."))
            if not files:
                # every file was embedded before the stop / crash, but the collection was never completed: finish it
                log(f"📋 All files already embedded: storing {len(sr._build_store)} vectors from the checkpoint")
        if files:
            log(f"📊 Found {len(files)} images to process", 0.1)
        if self.include_subfolders:
            log("📂 Including images from subfolders")
        log(f"🔧 Processing mode: {'Direct PE' if self.use_direct_pe else 'Detector + PE'}")
        log(f"📂 Database will be stored at: {self.db_path}")
        self.files = files
        if sr._build_store is None:
            if os.path.isdir(self.build_path):
                shutil.rmtree(self.build_path)
            info = sr._build_info(self.folder_path, self.use_direct_pe, self.include_subfolders)
            sr._build_store = st.GalleryStore(sr.pe_model.cfg.out_dim, device=sr.device.index or 0, capacity=max(len(files), 1024),
                                              collection=self.collection, path=self.build_path, build_info=info)
        self.store_db = sr._build_store
        self.stats = {"images": len(files), "decode_thread_s": 0.0, "wait_decode_s": 0.0, "wait_device_s": 0.0,
                      "launch_s": 0.0, "bookkeeping_s": 0.0, "flush_s": 0.0, "duplicates_skipped": 0}
        sr.last_ingest_stats = self.stats
        self.t_start = time.perf_counter()
        if mode.decode_threads != sr._decode_pool._max_workers:
            sr._decode_pool.shutdown(wait=True)
            sr._decode_pool = ThreadPoolExecutor(max_workers=mode.decode_threads)
        if mode.pipelined:
            shape = (self.B, 3, self.model_size, self.model_size)
            self.stage = [torch.zeros(shape, dtype=torch.uint8).pin_memory() for _ in range(NSLOT)]
        elif not mode.host_resize:
            self.slabs = [FrameSlab() for _ in range(NSLOT)]
        self.last_ckpt = time.monotonic()

    def stopped(self, note):
        """A stop: what is stored so far becomes the checkpoint"""
        self.log(note)
        self.checkpoint()
        return str(self.log) + "\n\n⏸️ Processing stopped. You can resume later."

    def checkpoint(self):
        """the rows and finished files since the last one, as a delta shard of the collection being built; the small
        JSON next to the reference's checkpoint path only says where the build lives"""
        store_db, base = self.store_db, self.ckpt_base
        try:
            t_f = time.perf_counter()
            rows = store_db.flush()
            self.stats["flush_s"] += time.perf_counter() - t_f
            os.makedirs(os.path.dirname(base), exist_ok=True)
            with open(base + ".json.tmp", "w") as f:
                json.dump({"database_name": self.database_name, "folder_path": self.folder_path, "build_path": self.build_path,
                           "timestamp": datetime.now().isoformat(), "processed_files": len(store_db.files_done),
                           "n_embeddings": len(store_db)}, f, indent=2)
            os.replace(base + ".json.tmp", base + ".json")
            if rows:
                self.log(f"💾 Checkpoint: shard {store_db._shards - 1} ({rows} vectors, {len(store_db)} in all)")
        except Exception as e:
            self.log(f"⚠️ Error saving checkpoint: {str(e)}")

    def decode(self, path, slot=None):
        """pool task: decode (and, on the host-resize path, squash-resize) one file -> (image, what the upload needs) or
        (the exception, None).  `slot`: the staging row the resized image is written to, or the slab of the batch, where
        a frame that goes to the device as it is (resized / cropped there) waits for one asynchronous copy"""
        t_dec = time.perf_counter()
        try:
            im = Image.open(path).convert("RGB")
            if not self.mode.host_resize:
                return im, slot.put(np.asarray(im))
            u8 = pp.resize_u8(im, self.model_size)
            if slot is None:
                return im, u8
            slot.copy_(u8)
            return im, True
        except Exception as e:           # per-image failure: logged and skipped (core_system.py:585-591)
            return e, None
        finally:
            self.stats["decode_thread_s"] += time.perf_counter() - t_dec      # (summed over the pool's threads; a float += under the GIL)

    def submit(self, bn):
        """batch `bn` to the pool, into host buffer bn % NSLOT"""
        pool, paths = self.sr._decode_pool, self.files[bn * self.B:(bn + 1) * self.B]
        if self.stage is not None:                     # one staging row per file
            buf = self.stage[bn % NSLOT]
            return [pool.submit(self.decode, p, buf[j]) for j, p in enumerate(paths)]
        if self.slabs is not None:
            slab = self.slabs[bn % NSLOT]
            slab.reset()
            return [pool.submit(self.decode, p, slab) for p in paths]
        return [pool.submit(self.decode, p) for p in paths]

    def top_up(self, it):
        """keep the pool DEPTH batches ahead of batch `it`; a buffer is handed out again only after the upload that
        read it (NSLOT batches ago) has left the host"""
        while self.submitted <= it + DEPTH and self.submitted * self.B < len(self.files):
            bn = self.submitted
            t_ev = time.perf_counter()
            for ev in (self.h2d_done[bn % NSLOT], self.frames_done[bn % NSLOT]):
                if ev is not None:
                    ev.synchronize()
            self.stats["wait_device_s"] += time.perf_counter() - t_ev        # the device is the bottleneck while this grows
            self.pending.append(self.submit(bn))
            self.submitted += 1

    @contextlib.contextmanager
    def slot_frames(self, it, handles):
        """Upload slab it % NSLOT with one asynchronous copy of its used prefix and yield the device frames of `handles`
        (what FrameSlab.put returned; views into the copy), in order; when the block ends, record the event behind it"""
        slab, device = self.slabs[it % NSLOT], self.sr.device
        dev_slab = slab.buf[:slab.used].to(device, non_blocking=True) if slab.used else None
        # (off None: the frame did not fit and goes up from its pageable tensor)
        yield [x.to(device, non_blocking=True) if off is None else dev_slab[off:off + x[0] * x[1] * x[2]].view(x)
               for off, x in handles]
        self.frames_done[it % NSLOT] = torch.cuda.Event()
        self.frames_done[it % NSLOT].record()

    def detect_batch(self, pils):
        """per-region modes, as soon as a batch is decoded: detector boxes and region metadata per image (None for a file
        that failed to decode), so that its regions can be queued on the device before the bookkeeping of the batch in front"""
        sr, det = self.sr, []
        for im in pils:
            if isinstance(im, Exception):
                det.append(None)
                continue
            n_reg = sr.detect_regions(im, self.text_prompt)
            kept, metas = sr._region_metadata(im, sr.detected_regions) if n_reg else ([], [])
            # (aspect="keep": the frame is embedded on the grid of its own aspect ratio, and its masks' tokens are that grid's)
            grid = sr._grid_of(im.width, im.height) if sr.aspect == "keep" else None
            det.append((n_reg, metas, sr._pool_bits(sr.detected_regions, kept, grid) if self.mode.pool and metas else None, grid))
        return det

    def launch(self, it, results):
        """Queue batch `it` on the device NOW, so that the device holds it while this thread does the bookkeeping of the one
        before: the global vectors of the whole batch in one forward, or the regions' vectors.  They stay on the device."""
        sr, mode, size = self.sr, self.mode, self.model_size
        start = it * self.B
        paths, pils = self.files[start:start + self.B], [im for im, _ in results]
        good = [h for im, h in results if not isinstance(im, Exception)]
        dev_emb = det = None
        if mode.per_region:
            det = self.detect_batch(pils)
            idx = [j for j, d in enumerate(det) if d is not None and d[1]]
            handles = [results[j][1] for j in idx]
            if idx and mode.crop:
                # boxes from the detector, one crop + resize launch, forwards of max_batch crops
                with torch.cuda.device(sr.device), self.slot_frames(it, handles) as frames:
                    dev_emb = sr._embed_regions_batch([(pils[j], det[j][1]) for j in idx], to_host=False, device_frames=frames)
            elif idx:
                # (the simple route: detect the batch's regions, then one embed_regions per batch)
                with torch.cuda.device(sr.device):
                    if mode.host_resize:
                        u8 = torch.stack(handles).to(sr.device, non_blocking=True)
                    else:
                        with sr._lock:
                            with self.slot_frames(it, handles) as frames:
                                pass                    # (the event goes directly behind the copy)
                            if sr.aspect != "keep":
                                u8 = pp.crop_resize_device(frames, None, size)
                    if sr.aspect == "keep":             # one resize and one embed_regions per grid of the batch's frames
                        dev_emb = sr._embed_by_grid(frames, None, bits=[det[j][2] for j in idx], grids=[det[j][3] for j in idx],
                                                    to_host=False)
                    else:
                        dev_emb = sr._embed_pool_batch(u8, [det[j][2] for j in idx], to_host=False)
        elif good:
            with sr._lock, torch.cuda.device(sr.device):
                if mode.pipelined:
                    # every file of the batch has its row in the staging buffer (a failed file's row keeps whatever it
                    # held: embedded and never looked at)
                    dev_in = self.stage[it % NSLOT][:len(paths)].to(sr.device, non_blocking=True)
                    self.h2d_done[it % NSLOT] = torch.cuda.Event()
                    self.h2d_done[it % NSLOT].record()
                    dev_emb = sr.pe_model.embed(dev_in)
                else:
                    # device resize: the decoded frames go up as they are, one crop + resize launch, one forward
                    with self.slot_frames(it, good) as frames:
                        pass
                    if sr.aspect == "keep":             # one resize and one forward per grid of the batch's frames
                        dev_emb = sr._embed_by_grid(frames, None, to_host=False)
                    else:
                        dev_emb = sr.pe_model.embed(pp.crop_resize_device(frames, None, size))
        return Batch(start, paths, pils, dev_emb, start + self.B >= len(self.files), det)

    def settle(self, batch):
        """finalize the batch in flight, if any, under the bookkeeping clock"""
        if batch is not None:
            t_b = time.perf_counter()
            self.finalize(batch)
            self.stats["bookkeeping_s"] += time.perf_counter() - t_b

    def finalize(self, b):
        """bookkeeping of one embedded batch: metadata per image, then the batch's vectors -- still on the device --
        go straight into the collection being built (device-to-device append; nothing visits the host)"""
        sr, log, n_files = self.sr, self.log, len(self.files)
        gi = 0
        batch_items = []                       # (path, metas, row of dev_emb or None)
        for j, (path, im) in enumerate(zip(b.paths, b.pils)):
            i = b.start + j
            filename = os.path.basename(path)
            log(f"🔄 Processing {i + 1}/{n_files}: {filename}", 0.1 + 0.7 * (i / n_files))
            if isinstance(im, Exception):
                log(f"❌ Error processing {filename}: {str(im)}")
                self.done_files.append(path)
                self.failed += 1
                continue
            row = None
            if b.dev_emb is not None and not self.mode.per_region:
                row = j if self.mode.pipelined else gi      # staged batches have one row per file, the others one per decoded file
                gi += 1
            if self.use_direct_pe:
                metas = [sr._full_image_meta(im)]
                log(f"✅ Extracted global embedding for {filename}")
            else:
                if b.det is not None:
                    n_reg, metas = b.det[j][:2]             # crop / pool mode: detected when the batch was queued
                else:
                    n_reg = sr.detect_regions(im, self.text_prompt)
                    metas = sr._region_metadata(im, sr.detected_regions)[1] if n_reg else []
                if n_reg == 0:
                    log(f"⚠️ No regions found in {filename}, skipping")
                    self.done_files.append(path)
                    self.failed += 1
                    continue
                log(f"✅ Found {n_reg} regions, extracted {len(metas)} embeddings in {filename}")
            for m in metas:
                m["image_source"] = path
                m["filename"] = filename
                m["original_region_id"] = m.get("region_id", uuid4())
                m["region_id"] = uuid4()
            batch_items.append((path, metas, row))
        self.store(batch_items, b.dev_emb, b.last)

    def store(self, batch_items, dev_emb, last):
        """the embedded batch enters the collection (and only now counts as processed: a shard never names a file whose
        vectors it does not hold).  Per-region modes: dev_emb is one vector per region, in item order."""
        sr, store_db = self.sr, self.store_db
        metas_all, rows = [], []
        for path, metas, row in batch_items:
            metas_all.extend(metas)
            if not self.mode.per_region:
                rows.extend([row] * len(metas))            # every region of an image stores its global vector (core_system.py:406-408)
            self.done_files.append(path)
            self.processed += 1
            sr._last_processed_file = path
        if metas_all:
            with sr._lock, torch.cuda.device(sr.device):
                if self.mode.per_region or (rows == list(range(len(rows))) and len(rows) == dev_emb.shape[0]):
                    vec = dev_emb
                else:
                    vec = dev_emb.index_select(0, torch.tensor(rows, dtype=torch.int64, device=dev_emb.device))
                rep = store_db.upsert(vec, [m["region_id"] for m in metas_all], metas_all, files=list(self.done_files),
                                      skip_duplicates=sr.skip_duplicates)
                if rep and rep["dropped"]:
                    self.stats["duplicates_skipped"] += len(rep["dropped"])
                    self.log(f"♻️ Skipped {len(rep['dropped'])} near-duplicates of stored vectors "
                             f"(score >= {sr.skip_duplicates:g}); {rep['kept']} of the batch stored")
        else:
            store_db.upsert(torch.zeros((0, store_db.dim)), [], [], files=list(self.done_files))
        self.done_files.clear()
        # a checkpoint writes only what is new: at most one per interval (the end of the build writes the last shard itself)
        if time.monotonic() - self.last_ckpt >= sr.checkpoint_interval_s and not last:
            self.checkpoint()
            self.last_ckpt = time.monotonic()
