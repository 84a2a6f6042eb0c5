"""``SimpleReverso`` façade over the MI355X-native embed + search path.

Same class name, method names, argument meaning, return shapes and ``❌ / ⚠️``
string conventions as the reference's ``core_system.py`` (class at ``:44``), so the
reference's ``ui.py`` / ``main.py`` run on top of it unchanged.
What differs underneath:

* ``encode_image`` (``:341``, ``:442``) is the HIP forward in ``librevo.so``;
* the vector store (``QdrantClient``, ``:100``, ``:521``, ``:600-622``, ``:659-664``) is a
  device-resident gallery with bit-exact fp32 re-scored top-k;
* ``create_database`` embeds in batches (decode threads overlap the device) instead
  of one image per forward (``:541-591``), and its checkpoint/resume works;
* GroundedSAM (``:205-318``) is third-party and out of scope: a detector callable can be
  injected (``detector=``); without one every image is one full-frame region, which
  is also what the reference's embedding of a region amounts to (``:406`` "Use global
  for now": every region receives the global embedding).  ``detector="prompt"`` installs
  the built-in ``PromptDetector`` instead: the text prompt scored against the image's
  token vectors on the device.

There is no CPU fallback: constructing the class without a GPU raises.
"""
import dataclasses
import os
import shutil
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image, ImageDraw, ImageFont

from . import filters
from . import ingest
from . import preprocess as pp
from . import regions as rg
from . import store as st
from .config import DEFAULT_VARIANT, TEXT_VARIANTS, aspect_grid, available_configs, get_config, get_text_config
from .engine import TextEngine, VitEngine
from .ingest import BUILDING, uuid4 as _uuid4
from .tokenizer import ClipTokenizer
from .weights import load_state_dict, load_text_state_dict, resolve_text_config, synth_text_weights, synth_weights

DB_ROOT = "./simple_reverso_db"


class Regions:
    """Minimal stand-in for ``supervision.Detections`` (xyxy, mask, confidence, class_id)."""

    def __init__(self, xyxy, mask=None, confidence=None, class_id=None, class_names=None):
        self.xyxy = np.asarray(xyxy, dtype=np.float32).reshape(-1, 4)
        self.mask = mask
        n = len(self.xyxy)
        self.confidence = np.ones(n, np.float32) if confidence is None else np.asarray(confidence, np.float32)
        self.class_id = np.zeros(n, np.int64) if class_id is None else np.asarray(class_id, np.int64)
        self.class_names = class_names or ["object"]

    def __len__(self):
        return len(self.xyxy)


def split_prompt(text_prompt):
    """``"person . car . building"`` -> ``["person", "car", "building"]``: the reference's prompt format (core_system.py:237,
    :416), phrases separated by `` . ``; a closing `` .`` and empty phrases are dropped, the order and repeats are kept."""
    text = (text_prompt or "").strip()
    if text.endswith(" ."):
        text = text[:-2]
    return [p.strip() for p in text.split(" . ") if p.strip(" .")]


class PromptDetector:
    """The built-in detector (``SimpleReverso(detector="prompt")``): the prompt's phrases and the background prompts through
    the text tower, then ``VitEngine.detect`` -- every patch cell goes to the phrase its token vector scores highest against,
    the label map is cut into connected regions (include/revo.h, DETECT).  Called like any injected
    detector, ``detector(pil, text_prompt) -> Regions``: pixel boxes, pixel masks (``regions.cell_masks``), ``class_names``
    (the phrases), ``class_id`` and ``confidence``.  Not GroundedSAM, which stays out of scope; nothing is claimed about
    detection quality on trained weights."""

    def __init__(self, system, threshold=None, background_prompts=(), min_cells=1, max_regions=50):
        self.system = system
        self.threshold = None if threshold is None else float(threshold)
        self.background_prompts = [str(p) for p in background_prompts]
        self.min_cells, self.max_regions = int(min_cells), int(max_regions)
        self.last = None                    # the engine-level result of the last call (cell boxes, bitmaps; device tensors)

    def __call__(self, image, text_prompt):
        s = self.system
        pil = pp.to_pil(image)
        phrases = split_prompt(text_prompt) or ["object"]
        texts = phrases + self.background_prompts
        if len(texts) > 64:
            raise ValueError(f"a prompt holds at most 64 phrases, background prompts included (got {len(texts)})")
        cfg = s.pe_model.cfg
        prompts = s.embed_text(texts)
        u8 = s._frames_u8([pil])
        with s._lock:
            det = s.pe_model.detect(u8, prompts, thresholds=self.threshold, n_background=len(self.background_prompts),
                                    min_cells=self.min_cells, max_regions=min(self.max_regions, cfg.grid * cfg.grid),
                                    with_vectors=False)
        self.last = det
        bits = det.bits.cpu().numpy()
        return Regions(rg.cell_boxes(cfg, det.boxes.cpu().numpy(), pil.width, pil.height),
                       mask=rg.cell_masks(cfg, bits, pil.width, pil.height), confidence=det.confidence.cpu().numpy(),
                       class_id=det.prompt.cpu().numpy(), class_names=phrases)


NO_QUERY = "❌ No query embeddings available. Please detect/process an image first."
NO_DATABASE = "❌ No database loaded. Please create or load a database first."


def _item(payload, point_id, score=None):
    """What a report says of one stored region: ``{"filename", "image_source", "bbox", "id"}``, then ``"score"`` if given."""
    item = {"filename": payload.get("filename", "Unknown"), "image_source": payload.get("image_source", ""),
            "bbox": payload.get("bbox"), "id": point_id}
    if score is not None:
        item["score"] = score
    return item


def _listing(items):
    """One numbered line per scored item."""
    return "".join(f"{n + 1}. {it['filename']}  score {it['score']:.3f}  (Source: {it['image_source']})\n"
                   for n, it in enumerate(items))


def _no_hits(what, threshold=None):
    """The report of an empty result: "❌ No <what>", and the threshold that cut it if there was one."""
    return f"❌ No {what}" + (f" above threshold {threshold}" if threshold is not None else "")


class SimpleReverso:
    """Simplified visual investigation system (MI355X-native hot path)."""
    # names of the databases create_database calls of this instance are building right now (two UI threads may overlap):
    # list_databases / load_database leave those build directories alone meanwhile.  Guarded by _building_lock.
    _building_lock = threading.Lock()
    _building_names = frozenset()      # (per-instance set from __init__ on)
    aspect, aspect_max_ratio = "squash", 4.0      # (set by __init__; the defaults are the reference's behaviour)

    def __init__(self, model_name=DEFAULT_VARIANT, checkpoint=None, device=0, db_root=DB_ROOT, max_batch=64,
                 detector=None, decode_workers=None, synthetic_seed=0, region_mode="global", device_resize=False,
                 checkpoint_interval_s=30.0, skip_duplicates=None, detect_threshold=None, background_prompts=(),
                 aspect="squash", aspect_max_ratio=4.0):
        print("🚀 Initializing Simple Revers-o...")
        if aspect not in ("squash", "keep"):
            raise ValueError("aspect must be 'squash' (every image resized to the model's square: the reference's behaviour, "
                             "core_system.py:200) or 'keep' (embedded on the token grid nearest its own aspect ratio)")
        if not float(aspect_max_ratio) >= 1.0:
            raise ValueError("aspect_max_ratio must be at least 1")
        # "keep": native-aspect embedding -- a query, a stored frame and a region crop are resized,
        # without crop, to the grid of the tower's menu (config.aspect_grids) nearest their own aspect ratio and embedded on
        # it; the token budget stays the native one.  The prompt detector keeps running on the squashed native image: only the
        # vectors follow the aspect.  A database holds vectors of ONE mode (its build info names it).
        self.aspect, self.aspect_max_ratio = aspect, float(aspect_max_ratio)
        if region_mode not in ("global", "crop", "pool"):
            raise ValueError("region_mode must be 'global' (the reference's behaviour, core_system.py:406), 'crop' or 'pool'")
        # "crop": every region is cropped to its box on the device and embedded on its own -- the
        # feature the reference leaves as a placeholder (:406 "Use global for now", :687-690)
        # "pool": one forward per IMAGE; every region is attention-pooled over the tokens its mask covers
        # (regions.token_masks, VitEngine.embed_regions): the mask's shape counts, not just its box
        self.region_mode = region_mode
        # a score threshold: create_database stores a vector only if no stored vector and no earlier kept vector of its batch
        # scores that high against it (GalleryStore.upsert(skip_duplicates=...): frames of a static camera or a slow pan)
        if skip_duplicates is not None:
            skip_duplicates = float(skip_duplicates)
            if skip_duplicates != skip_duplicates:
                raise ValueError("skip_duplicates must be a score threshold or None, not NaN")
        self.skip_duplicates = skip_duplicates
        # True: decoded frames are uploaded as they are and squash-resized by the HIP kernel
        # (same pixels as the host PIL resize, bit for bit); False: PIL resize in the decode pool
        self.device_resize = bool(device_resize)
        self.checkpoint_interval_s = float(checkpoint_interval_s)     # a checkpoint writes the vectors added since the last one (a delta shard)
        self.db_root = db_root
        self.max_batch = int(max_batch)
        # a callable (image, text_prompt) -> Regions, None (every image is one full-frame region), or "prompt": the built-in
        # PromptDetector -- the prompt's phrases scored against the image's token vectors on the device (a second forward per
        # image in the region modes of create_database); detect_threshold and background_prompts are its settings
        self.detector = PromptDetector(self, detect_threshold, background_prompts) if detector == "prompt" else detector
        # decode threads of a gallery build.  None = by mode (create_database): MORE threads are not better -- PIL's
        # RGBX -> RGB packing of a decoded frame runs under the GIL (0.35 ms per 640 x 480 frame), and the ingest thread,
        # which has to keep the device's queue full, waits its turn behind every thread that wants it: measured on
        # 3 000 JPEGs with device resize 1 950 images/s with 8 threads, 1 620 with 16, 1 720 with 32.  (Decode worker
        # PROCESSES writing into pinned shared memory were built and measured too: 1 975 and 563-598 images/s against
        # 1 950 and 602-649 with threads -- with the right thread count the build waits for the device, not for the GIL.)
        self.decode_workers = None if decode_workers is None else int(decode_workers)
        self._decode_pool = ThreadPoolExecutor(max_workers=self.decode_workers or 8)
        self._lock = threading.RLock()      # ui.py drives one shared instance from worker threads
        self.device = self.setup_device(device)
        self.pe_model, self.preprocess = self.load_pe_model(model_name, checkpoint, synthetic_seed)
        self.text_model = None              # the checkpoint's text tower, built by the first text query (load_text_model)
        self.grounded_sam = None
        self.vector_db = None
        self.current_database = None
        self.detected_regions = []
        self.region_embeddings = None
        self.query_embedding_for_search = None
        self._building_names = set()
        self._building_lock = threading.Lock()
        self._stop_requested = False
        self._last_processed_file = None
        self._partial_embeddings = []
        self._partial_metadata = []
        self._build_store = None        # the collection a create_database call is building (closed when the call returns)
        self.last_ingest_stats = None   # wall-clock stage times of the last create_database call
        print("✅ Simple Revers-o ready!")

    # ------------------------------------------------------------- DB admin --
    def list_databases(self):
        """core_system.py:74-88"""
        if not os.path.exists(self.db_root):
            return []
        for n in os.listdir(self.db_root):              # a crash inside the final swap of a build: put the database back
            for suf in (BUILDING, st.OLD, st.OLD_LEGACY):
                if suf == st.OLD_LEGACY and not st.is_legacy_set_aside(self.db_root, n):
                    continue
                # (not a build this very process is finishing: create_database swaps that one in itself)
                if n.endswith(suf) and not self._is_building(n[: -len(suf)]):
                    st.recover(os.path.join(self.db_root, n[: -len(suf)]), BUILDING)
        return [n for n in os.listdir(self.db_root)
                if os.path.isdir(os.path.join(self.db_root, n)) and n != "checkpoints" and not n.endswith(BUILDING)
                and not n.endswith(st.OLD) and not st.is_legacy_set_aside(self.db_root, n)]

    def _is_building(self, name):
        with self._building_lock:
            return name in self._building_names

    def load_database(self, database_name):
        """core_system.py:90-119"""
        if not database_name:
            return "❌ Please provide a database name"
        db_path = os.path.join(self.db_root, database_name)
        if not self._is_building(database_name):
            st.recover(db_path, BUILDING)
        if not os.path.exists(db_path):
            return f"❌ Database not found: {database_name}"
        try:
            if not (os.path.exists(os.path.join(db_path, st.MANIFEST)) or os.path.exists(os.path.join(db_path, "meta.json"))):
                return f"❌ Collection not found in database: {database_name}"
            with self._lock:
                if self.vector_db is not None:
                    self.vector_db.close()
                self.vector_db = st.GalleryStore.load(db_path, device=self.device.index or 0)
                self.current_database = self.vector_db.collection
                built = (self.vector_db.build_info or {}).get("aspect", "squash")
            if built != self.aspect:
                return (f"✅ Loaded database: {database_name}\n⚠️ It was built with aspect='{built}' and this system embeds "
                        f"queries with aspect='{self.aspect}': their vectors are not made the same way")
            return f"✅ Loaded database: {database_name}"
        except Exception as e:
            return f"❌ Error loading database: {str(e)}"

    def delete_database(self, database_name):
        """core_system.py:121-135"""
        if not database_name:
            return "❌ Please provide a database name"
        db_path = os.path.join(self.db_root, database_name)
        if not os.path.exists(db_path):
            return f"❌ Database not found: {database_name}"
        try:
            shutil.rmtree(db_path)
            # an unfinished build of the same name and its checkpoint note go with it
            shutil.rmtree(db_path + BUILDING, ignore_errors=True)
            shutil.rmtree(db_path + st.OLD, ignore_errors=True)
            if st.is_legacy_set_aside(self.db_root, database_name + st.OLD_LEGACY):
                shutil.rmtree(db_path + st.OLD_LEGACY, ignore_errors=True)
            st.remove_checkpoint(os.path.join(self.db_root, "checkpoints", f"{database_name}_checkpoint"))
            return f"✅ Deleted database: {database_name}"
        except Exception as e:
            return f"❌ Error deleting database: {str(e)}"

    def unlock_database(self, database_name):
        """core_system.py:137-154"""
        if not database_name:
            return "❌ Please provide a database name"
        db_path = os.path.join(self.db_root, database_name)
        if not os.path.exists(db_path):
            return f"❌ Database not found: {database_name}"
        lock_file = os.path.join(db_path, ".lock")
        if os.path.exists(lock_file):
            try:
                os.remove(lock_file)
                return f"✅ Removed lock file from database: {database_name}"
            except Exception as e:
                return f"❌ Error removing lock file: {str(e)}"
        return f"ℹ️ No lock file found for database: {database_name}"

    # -------------------------------------------------------- model lifecycle --
    def setup_device(self, device=0):
        """core_system.py:156-167 — ROCm reports as ``cuda``; no MPS / CPU path here."""
        if not torch.cuda.is_available():
            raise RuntimeError("revers-o_amd needs an MI355X (ROCm) device: the hot path has no CPU fallback")
        dev = torch.device("cuda", int(device))
        print(f"🔥 Using ROCm device: {dev} ({torch.cuda.get_device_name(dev)})")
        return dev

    def load_pe_model(self, target_model=DEFAULT_VARIANT, checkpoint=None, synthetic_seed=0):
        """core_system.py:169-203: the target model first; if it is not among the available configs, or if loading it
        FAILS (:183-191 -- here: a checkpoint that does not fit the architecture, by missing, unexpected or mis-shaped
        tensor, or an engine that cannot be created), the first available config -- whose own failure propagates, as the
        reference's second ``from_config`` would."""
        print(f"📚 Loading {target_model}...")
        configs = available_configs()
        print(f"Available PE configs: {configs}")
        checkpoint = checkpoint or os.environ.get("REVERSO_PE_CHECKPOINT")
        self._checkpoint, self._synthetic_seed = checkpoint, synthetic_seed      # load_text_model reads the same file
        sd = load_state_dict(checkpoint) if checkpoint else None
        if sd is None:
            # no network here: pretrained weights (pe.CLIP.from_config(..., pretrained=True), :181)
            # must be supplied as a file; without one the tower is random-initialised.
            print("⚠️ No checkpoint given (REVERSO_PE_CHECKPOINT): using seeded random-init weights")

        def build(name):
            cfg = get_config(name)
            w = sd if sd is not None else synth_weights(cfg, seed=synthetic_seed, device=self.device)
            # LayerScale follows the checkpoint's ls_* tensors; any other unexpected `visual.*` tensor is an error (weights.py)
            return VitEngine(cfg, w, device=self.device.index or 0, max_batch=self.max_batch)

        known = target_model in configs
        if not known:
            try:
                get_config(target_model)            # the build's own test miniatures are not "available configs"
                known = True
            except KeyError:
                pass
        if known:
            try:
                engine = build(target_model)
                print(f"✅ Loaded {target_model}" + (f" weights from {checkpoint}" if checkpoint else ""))
            except Exception as e:
                print(f"❌ Failed to load {target_model}: {e}")
                engine = build(configs[0])
                print(f"🔄 Using fallback: {configs[0]}")
        else:
            engine = build(configs[0])
            print(f"🔄 Using available: {configs[0]}")
        size = engine.cfg.image_size
        print("⚡ bf16 MFMA matmuls, fp32 residual stream" + (", LayerScale from the checkpoint" if engine.cfg.use_ls else ""))
        return engine, (lambda image: pp.resize_u8(image, size))

    # ------------------------------------------------------------- detection --
    def detect_regions(self, image, text_prompt=None):
        """core_system.py:237-318.  Delegates to the injected detector; without one the
        whole frame is the single region."""
        self.detected_regions = []
        self.region_embeddings = None
        self.query_embedding_for_search = None
        pil = pp.to_pil(image)
        if self.detector is not None:
            det = self.detector(pil, text_prompt or "object")
            self.detected_regions = det
            return len(det)
        w, h = pil.size
        self.detected_regions = Regions([[0, 0, w, h]], mask=None, class_names=["full_image"])
        return 1

    def _region_metadata(self, pil, regions):
        """Per-region metadata exactly as core_system.py:363-425 builds it (cap 50, empty masks
        skipped, missing masks -> full-image bbox); returns (kept indices, metadata)."""
        names = getattr(regions, "class_names", None) or ["object"]
        kept, metas = [], []
        for i in range(min(len(regions), 50)):
            conf = float(regions.confidence[i]) if i < len(regions.confidence) else 0.0
            cid = int(regions.class_id[i]) if i < len(regions.class_id) else -1
            mask = regions.mask[i] if getattr(regions, "mask", None) is not None and i < len(regions.mask) else None
            if mask is None:
                metas.append({"region_id": _uuid4(), "bbox": [0, 0, pil.width, pil.height], "area_ratio": 1.0,
                              "detection_index": i, "confidence": conf,
                              "detected_class": names[cid] if 0 <= cid < len(names) else "unknown",
                              "mask_status": "missing_or_unavailable"})
                kept.append(i)
                continue
            m = np.asarray(mask)
            m = (m > 0.5).astype(np.uint8) if np.issubdtype(m.dtype, np.floating) else m.astype(np.uint8)
            if m.sum() == 0:
                print(f"⚠️ Empty mask for region {i}, skipping")
                continue
            ys, xs = np.where(m)
            metas.append({"region_id": _uuid4(),
                          "bbox": [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())],
                          "area_ratio": float(m.sum() / m.size), "detection_index": i, "confidence": conf,
                          "detected_class": names[cid] if 0 <= cid < len(names) else "object",
                          "mask_status": "processed"})
            kept.append(i)
        return kept, metas

    # ----------------------------------------------------------------- embed --
    def _grid_of(self, width, height):
        """aspect="keep": the token grid of a ``width x height`` image or crop (config.aspect_grid over the tower's menu)"""
        return aspect_grid(self.pe_model.cfg, height, width, self.aspect_max_ratio)

    def _embed_by_grid(self, frames, boxes, bits=None, grids=None, to_host=True):
        """aspect="keep", the one place a batch is split by grid: device frames (uint8 ``[H, W, 3]``) and jobs ``boxes``
        (``(frame_index, x0, y0, x1, y1)``, or None for every frame whole), each embedded on the grid of its box's aspect
        ratio (``grids``: per job, where the caller already chose them).  The jobs are grouped by grid; per group one
        crop + resize launch and one forward of the group's jobs, and the vectors are scattered back: fp32 ``[n, D]`` in job
        order.  With ``bits`` (pool mode: per job the token bitmaps of its regions ON ITS GRID) the forward is
        ``embed_regions`` and the result one row per region, jobs in order, regions in theirs."""
        cfg = self.pe_model.cfg
        if boxes is None:
            boxes = [(i, 0, 0, f.shape[1], f.shape[0]) for i, f in enumerate(frames)]
        if grids is None:
            grids = [self._grid_of(b[3] - b[1], b[4] - b[2]) for b in boxes]
        counts = [1] * len(boxes) if bits is None else [len(b) for b in bits]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out = torch.empty((int(starts[-1]), cfg.out_dim), dtype=torch.float32, device=self.device)
        groups = {}
        for i, g in enumerate(grids):
            if counts[i]:
                groups.setdefault(tuple(g), []).append(i)
        P = cfg.patch_size
        with self._lock, torch.cuda.device(self.device):
            for (gh, gw), idx in groups.items():
                u8 = pp.crop_resize_device(frames, [boxes[i] for i in idx], (gh * P, gw * P))
                if bits is None:
                    emb = self.pe_model.embed(u8, grid=(gh, gw))
                else:
                    ri = np.concatenate([np.full(counts[i], j, dtype=np.int64) for j, i in enumerate(idx)])
                    _, emb = self.pe_model.embed_regions(u8, ri, np.concatenate([bits[i] for i in idx]), with_global=False,
                                                         grid=(gh, gw))
                rows = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in idx])
                out.index_copy_(0, torch.from_numpy(rows).to(self.device), emb)
        return out.cpu() if to_host else out

    def _device_frames(self, pils):
        return [torch.from_numpy(np.array(pp.to_pil(im), dtype=np.uint8)).to(self.device, non_blocking=True) for im in pils]

    def _embed_pils(self, pils):
        """list of PIL images -> fp32 CPU tensor [n, D] (L2-normalised)."""
        if self.aspect == "keep":
            return self._embed_by_grid(self._device_frames(pils), None)
        u8 = self._frames_u8(pils)
        with self._lock:
            emb = self.pe_model.embed(u8)
        return emb.cpu()

    def _embed_regions_batch(self, items, to_host=True, device_frames=None):
        """items: [(pil, metas)].  One vector per region of every image: the frames go to the device once,
        every region's bbox is cropped + squash-resized there in one launch (bit-identical to PIL
        crop().resize()), then forwards of max_batch crops.  Mask-derived boxes are inclusive
        (core_system.py:411).  Returns fp32 [n_regions, D] in item order: a CPU tensor, or with
        to_host=False the device tensor (the launches are asynchronous)."""
        frames, boxes = [], []
        for n_item, (pil, metas) in enumerate(items):
            if not metas:
                continue
            fi = len(frames)
            if device_frames is not None:
                frames.append(device_frames[n_item])                    # already uploaded (create_database: one copy per batch)
            else:
                frames.append(torch.from_numpy(np.array(pil, dtype=np.uint8)).to(self.device, non_blocking=True))
            for m in metas:
                x0, y0, x1, y1 = m["bbox"]
                if m.get("mask_status") == "processed":
                    x1, y1 = x1 + 1, y1 + 1
                boxes.append((fi,) + pp.clamp_box((x0, y0, x1, y1), pil.width, pil.height))
        if not boxes:
            return torch.empty((0, self.pe_model.cfg.out_dim), device=None if to_host else self.device)
        if self.aspect == "keep":                  # every crop on the grid of its own box
            return self._embed_by_grid(frames, boxes, to_host=to_host)
        with self._lock:
            u8 = pp.crop_resize_device(frames, boxes, self.pe_model.cfg.image_size)
            emb = self.pe_model.embed(u8)
        return emb.cpu() if to_host else emb

    def _embed_regions(self, pil, metas):
        """One vector per region of one image (see _embed_regions_batch)."""
        return self._embed_regions_batch([(pil, metas)])

    def _pool_bits(self, regions, kept, grid=None):
        """pool mode: the token bitmap of every kept region (uint32 [len(kept), words]).  A processed mask is pooled over
        the tokens it covers (regions.token_masks; binarised as _region_metadata does); a region without a mask gets every
        token, class token included -- its image's global vector bit for bit, the reference's own fallback
        (core_system.py:367-389).  ``grid``: the token grid the image is embedded on (aspect="keep"; None: the native one)."""
        cfg = self.pe_model.cfg
        out = np.zeros((len(kept), rg.words_per_region(cfg, grid)), dtype=np.uint32)
        by_shape = {}                                  # masks of one shape (the usual case: the image's) share the cell tables
        for j, i in enumerate(kept):
            mask = regions.mask[i] if getattr(regions, "mask", None) is not None and i < len(regions.mask) else None
            if mask is None:
                out[j] = rg.full_mask(cfg, include_cls=True, grid=grid)
                continue
            m = np.asarray(mask)
            m = (m > 0.5) if np.issubdtype(m.dtype, np.floating) else (m.astype(np.uint8) != 0)
            by_shape.setdefault(m.shape, []).append((j, m))
        for (h, w), items in by_shape.items():
            out[[j for j, _ in items]] = rg.token_masks(cfg, [m for _, m in items], w, h, grid=grid)
        return out

    def _embed_pool_batch(self, u8, bits_per_image, to_host=True):
        """pool mode: u8 [n, 3, size, size] device frames at the model resolution, bits_per_image: a bitmap array per
        frame.  One forward per frame, one vector per region in frame order."""
        region_image = np.concatenate([np.full(len(b), j, dtype=np.int64) for j, b in enumerate(bits_per_image)])
        with self._lock:
            _, emb = self.pe_model.embed_regions(u8, region_image, np.concatenate(list(bits_per_image)), with_global=False)
        return emb.cpu() if to_host else emb

    def _frames_u8(self, pils):
        """PIL images -> device uint8 [n, 3, size, size] at the model resolution (the pixels _embed_pils embeds)"""
        size = self.pe_model.cfg.image_size
        if self.device_resize:
            frames = [torch.from_numpy(np.array(pp.to_pil(im), dtype=np.uint8)).to(self.device, non_blocking=True)
                      for im in pils]
            with self._lock:
                return pp.crop_resize_device(frames, None, size)
        u8 = torch.stack(list(self._decode_pool.map(lambda im: pp.resize_u8(im, size), pils)))
        return u8.to(self.device, non_blocking=True)

    def extract_embeddings(self, image):
        """core_system.py:320-429: one forward of the full image, every kept region receives
        the global embedding (:406) with its own mask-derived metadata.  With
        ``region_mode="crop"`` every region is embedded from its own crop instead, with ``region_mode="pool"`` from the
        tokens of that one forward which its mask covers."""
        if not self.detected_regions or len(self.detected_regions) == 0:
            print("❌ No regions detected")
            return [], []
        pil = pp.to_pil(image)
        kept, metas = self._region_metadata(pil, self.detected_regions)
        if self.region_mode == "crop":
            embeddings = list(self._embed_regions(pil, metas))
        elif self.region_mode == "pool":
            if not kept:
                embeddings = []
            elif self.aspect == "keep":            # the image's own grid; the masks' tokens on that grid
                grid = self._grid_of(pil.width, pil.height)
                embeddings = list(self._embed_by_grid(self._device_frames([pil]), None, grids=[grid],
                                                      bits=[self._pool_bits(self.detected_regions, kept, grid)]))
            else:
                embeddings = list(self._embed_pool_batch(self._frames_u8([pil]), [self._pool_bits(self.detected_regions, kept)]))
        else:
            g = self._embed_pils([pil])[0]
            embeddings = [g.clone() for _ in kept]
        self.region_embeddings = embeddings
        print(f"🎯 Extracted {len(embeddings)} region embeddings")
        return embeddings, metas

    def process_image_direct_pe(self, image):
        """core_system.py:431-455"""
        pil = pp.to_pil(image)
        e = self._embed_pils([pil])[0]
        if e.dim() != 1:
            raise ValueError(f"Unexpected feature shape: {tuple(e.shape)}")
        self.region_embeddings = [e]
        return [e.clone()], [self._full_image_meta(pil)]

    @staticmethod
    def _full_image_meta(pil):
        """The metadata of a direct-PE vector: the whole frame as its one region (core_system.py:449-453)"""
        return {"region_id": _uuid4(), "bbox": [0, 0, pil.width, pil.height], "area_ratio": 1.0,
                "detection_index": 0, "confidence": 1.0, "detected_class": "full_image"}

    def request_stop(self):
        """core_system.py:457-459"""
        self._stop_requested = True

    # ------------------------------------------------------- gallery build ----
    def create_database(self, folder_path, database_name, text_prompt="person . car . building", use_direct_pe=False,
                        progress_callback=None, resume_from_checkpoint=False, include_subfolders=False):
        """core_system.py:461-648, with batched embedding and a working checkpoint."""
        # while this call builds <name>.building, a list_databases / load_database from another thread (a UI refresh) must
        # not adopt that directory as a crashed build's left-over (store.recover): the call swaps it in itself
        with self._building_lock:
            mine = database_name not in self._building_names      # (a second overlapping build of the SAME name: the first
            self._building_names.add(database_name)               #  one to enter keeps the entry until it returns)
        try:
            return self._create_database(folder_path, database_name, text_prompt, use_direct_pe, progress_callback,
                                         resume_from_checkpoint, include_subfolders)
        finally:
            if mine:
                with self._building_lock:
                    self._building_names.discard(database_name)

    def _create_database(self, folder_path, database_name, text_prompt, use_direct_pe, progress_callback,
                         resume_from_checkpoint, include_subfolders):
        if self.skip_duplicates is not None and self.region_mode == "global" and not use_direct_pe:
            # every region of an image stores the image's global vector (core_system.py:406-408): all but the first would
            # be "duplicates" of it
            msg = ("❌ skip_duplicates needs one vector per stored point: with the detector in region_mode='global' every "
                   "region of an image shares the image's vector (use use_direct_pe=True, region_mode='crop' or 'pool')")
            if progress_callback:
                progress_callback(msg, None)
            return msg
        if self.aspect == "keep" and not self.device_resize:
            # the frames of a batch have different grids: they go up as decoded and are resized on the device, group by group
            msg = ("❌ aspect='keep' builds a database through the device resize: create the system with device_resize=True "
                   "(the host-resize route stages one square row per file)")
            if progress_callback:
                progress_callback(msg, None)
            return msg
        log_status = ingest.StatusLog(progress_callback)
        os.makedirs(self.db_root, exist_ok=True)
        processed_files = set()
        # The collection is built in <db>.building (the finished one, if any, stays searchable until the new one is
        # complete) and its manifest of delta shards is the checkpoint: a resume re-opens it.
        self._partial_embeddings, self._partial_metadata = [], []          # (kept for callers that look at them: always empty now)
        build_path = os.path.join(self.db_root, database_name) + BUILDING
        self._build_store = None
        if resume_from_checkpoint and os.path.exists(os.path.join(build_path, st.MANIFEST)):
            build_info = self._build_info(folder_path, use_direct_pe, include_subfolders)
            try:
                header = st.read_manifest(os.path.join(build_path, st.MANIFEST))[0]
                diff = [k for k in build_info if header.get("build", {}).get(k) != build_info[k]]
                if header.get("build", {}).get("aspect", "squash") != self.aspect and "aspect" not in diff:
                    diff.append("aspect")
                if header.get("dim") != self.pe_model.cfg.out_dim:
                    diff.append("dim")
                if diff:
                    # another folder, model or mode: its rows must not be mixed with this build's
                    raise ValueError(f"the unfinished build was made with a different {', '.join(diff)}")
                n_files = len(os.listdir(folder_path)) if os.path.isdir(folder_path) else 0
                self._build_store = st.GalleryStore.load(build_path, device=self.device.index or 0, allow_partial=True,
                                                         capacity=n_files)        # room for the rest: no regrow right away
                processed_files = set(self._build_store.files_done)
                log_status(f"📋 Resuming from checkpoint: {len(processed_files)} files already processed")
            except Exception as e:
                log_status(f"⚠️ Error loading checkpoint: {str(e)}. Starting fresh.")
                processed_files, self._build_store = set(), None
        try:
            return ingest.IngestRun(self, folder_path, database_name, text_prompt, use_direct_pe, resume_from_checkpoint,
                                    include_subfolders, log_status, processed_files).run()
        finally:
            self._stop_requested = False
            self._partial_embeddings, self._partial_metadata = [], []
            if self._build_store is not None:               # stopped or failed: the shards on disk are the checkpoint
                self._build_store.close()
                self._build_store = None

    def _build_info(self, folder_path, use_direct_pe, include_subfolders):
        """What a collection is made from and how: written into the build's manifest header, compared on resume."""
        info = {"folder_path": os.path.abspath(folder_path), "model": self.pe_model.cfg.name,
                "use_ls": bool(self.pe_model.cfg.use_ls), "region_mode": self.region_mode,
                "use_direct_pe": bool(use_direct_pe), "include_subfolders": bool(include_subfolders),
                "skip_duplicates": self.skip_duplicates}      # (an older manifest has no such key: the same as None)
        if self.aspect != "squash":                           # (no key: "squash", what every older manifest is)
            info.update(aspect=self.aspect, aspect_max_ratio=self.aspect_max_ratio)
        return info

    # ---------------------------------------------------------------- search --
    def search_similar_boosted(self, formula, similarity_threshold=0.7, max_results=5, query_filter=None):
        """:meth:`search_similar` with the ranking rescored by ``formula`` over ``$score`` and the stored payloads (boost.py:
        "like this region, but prefer images taken near this date / place").  ``similarity_threshold`` is what the
        reference's slider means: a cut on the plain similarity (None: none), not on the boosted score; every stored region
        that passes it (and ``query_filter``) competes, not a prefetched short list.  Returns ``(text, items)``, items
        ``{"filename", "image_source", "bbox", "id", "score", "similarity"}``, best boosted score first.  No thumbnails."""
        if err := self._not_ready(need_query=True):
            return err, []
        query = self.region_embeddings[0]
        min_similarity = None if similarity_threshold is None else float(similarity_threshold)
        try:
            with self._lock:
                hits = self.vector_db.search_boosted(query, int(max_results), formula, min_similarity=min_similarity,
                                                     query_filter=query_filter)
        except ValueError as e:
            return f"❌ {e.args[0]}", []
        if not hits:
            return _no_hits("similar regions found", similarity_threshold), []
        items = [dict(_item(r.payload, r.id, r.score), similarity=r.similarity) for r in hits]
        text = f"🎯 Found {len(items)} similar regions (boosted):\n\n"
        return text + _listing(items), items

    def search_similar(self, similarity_threshold=0.7, max_results=5, query_filter=None, group_by=None):
        """core_system.py:650-717: first region embedding as the query, limit + score
        threshold, results best first with the same text and thumbnail formatting.  ``query_filter``: a Qdrant-style
        payload filter (filters.Filter or its dict form) restricting the search to the points it selects.  ``group_by``
        (a payload key, e.g. ``"image_source"``): at most ``max_results`` distinct values of it, each by its best region
        (a region-mode database holds several rows per image; without it one image can fill every place)."""
        if err := self._not_ready(need_query=True):
            return err, []
        return self._search_with_query(self.region_embeddings[0], similarity_threshold, max_results, query_filter, group_by)

    def _not_ready(self, need_query=False):
        """What a search says instead of starting -- no query embedding (asked first, where a method needs one) or no
        database -- or None."""
        if need_query and not self.region_embeddings:
            return NO_QUERY
        if not self.vector_db or not self.current_database:
            return NO_DATABASE
        return None

    def _search_with_query(self, query, similarity_threshold, max_results, query_filter, group_by):
        """The search and the result formatting of :meth:`search_similar` for a query vector (an image region's or a
        prompt's); ``similarity_threshold`` None: no cut."""
        score_threshold = None if similarity_threshold is None else float(similarity_threshold)
        with self._lock:
            if group_by is not None:
                res = self.vector_db.search_groups(query, group_by, limit=int(max_results),
                                                   score_threshold=score_threshold, query_filter=query_filter)
                hits = [grp.hits[0] for grp in res.groups]
            elif query_filter is None:
                hits = self.vector_db.search(query, limit=int(max_results), score_threshold=score_threshold)
            else:
                hits = self.vector_db.search(query, limit=int(max_results), score_threshold=score_threshold,
                                             query_filter=query_filter)
        if not hits:
            return _no_hits("similar regions found", similarity_threshold), []
        text = f"🎯 Found {len(hits)} similar regions:\n\n"

        def thumbnail(r):
            """the hit's source image with its score label, at most 400 px (core_system.py:682-706); None when the file
            is gone or unreadable.  One pool task per hit: decoding and resampling release the GIL, and ten hits were
            40 ms of a 50 ms interactive query when done one after the other."""
            image_path = r.payload.get("image_source", "")
            if not os.path.exists(image_path):
                return None
            try:
                img = Image.open(image_path).convert("RGB")
                draw = ImageDraw.Draw(img)
                try:
                    font = ImageFont.truetype("Arial.ttf", max(15, int(min(img.height, img.width) * 0.05)))
                except IOError:
                    font = ImageFont.load_default()
                label = f"Score: {r.score:.3f}"
                box = draw.textbbox((5, 5), label, font=font)
                draw.rectangle([box[0] - 2, box[1] - 2, box[2] + 2, box[3] + 2], fill="black")
                draw.text((5, 5), label, fill="white", font=font)
                img.thumbnail((400, 400), Image.Resampling.LANCZOS)
                return img
            except Exception as e:
                print(f"❌ Error loading/processing image {image_path}: {e}")
                return None

        try:
            images = list(self._decode_pool.map(thumbnail, hits)) if len(hits) > 1 else [thumbnail(hits[0])]
        except RuntimeError:                     # the pool is being replaced by a build on another thread
            images = [thumbnail(r) for r in hits]
        items = []
        for i, (r, img) in enumerate(zip(hits, images)):
            payload = r.payload
            filename = payload.get("filename", "Unknown")
            image_path = payload.get("image_source", "")
            text += f"{i + 1}. {filename} (Similarity: {r.score:.3f})\n"
            text += f"   Source: {image_path}\n"
            text += f"   📍 Bounding box: {str(payload.get('bbox', '[0,0,0,0]'))}\n\n"
            items.append({"image": img, "score": r.score, "filename": filename, "bbox": payload.get("bbox")})
        return text, items

    # ------------------------------------------------------------ text queries --
    def load_text_model(self, checkpoint=None, vocab=None):
        """The text tower of the same CLIP checkpoint (the reference loads it at core_system.py:181 and never uses it), built
        on first use.  ``checkpoint``: the file to read it from -- by default the one the image tower came from; without
        one: seeded random-init weights and a warning, as :meth:`load_pe_model` does.  ``vocab``: the BPE merges file
        (``REVERSO_BPE_VOCAB`` otherwise); without one only token arrays can be embedded."""
        with self._lock:
            if getattr(self, "text_model", None) is not None and checkpoint is None and vocab is None:
                return self.text_model
            checkpoint = checkpoint or self._checkpoint or os.environ.get("REVERSO_PE_CHECKPOINT")
            name = self.pe_model.cfg.name
            if checkpoint:
                sd = load_text_state_dict(checkpoint)
                cfg = resolve_text_config(sd, name=name)
            else:
                print("⚠️ No checkpoint given (REVERSO_PE_CHECKPOINT): the text tower uses seeded random-init weights")
                cfg = get_text_config(name if name in TEXT_VARIANTS else DEFAULT_VARIANT)
                if cfg.out_dim != self.pe_model.cfg.out_dim:      # (a test miniature of the image tower: match its width)
                    cfg = dataclasses.replace(get_text_config("PE-Tiny-Text-16"), out_dim=self.pe_model.cfg.out_dim)
                sd = synth_text_weights(cfg, seed=self._synthetic_seed, device=self.device)
            if cfg.out_dim != self.pe_model.cfg.out_dim:
                raise ValueError(f"the text tower embeds into {cfg.out_dim} dimensions, the image tower into {self.pe_model.cfg.out_dim}")
            tok = None
            vocab = vocab or os.environ.get("REVERSO_BPE_VOCAB")
            if vocab:
                tok = ClipTokenizer(vocab, context_length=cfg.context_length, vocab_size=cfg.vocab_size)
            if getattr(self, "text_model", None) is not None:
                self.text_model.close()
            self.text_model = TextEngine(cfg, sd, device=self.device.index or 0, tokenizer=tok)
            print(f"✅ Loaded the text tower of {name}" + (f" from {checkpoint}" if checkpoint else ""))
            return self.text_model

    def embed_text(self, texts):
        """Prompts (a string, a list of strings, or an integer token array ``[n, seq_len]``) -> normalised fp32 ``[n, out_dim]``
        on the device, in the space of the image embeddings."""
        eng = self.load_text_model()
        if isinstance(texts, str) or (len(texts) and isinstance(texts[0], str)):
            return eng.embed(texts)
        return eng.embed_tokens(texts, trim=True)

    def search_by_text(self, text, similarity_threshold=None, max_results=5, query_filter=None, group_by=None):
        """:meth:`search_similar` with a prompt as the query: the same results and strings.  No default threshold: the
        text-image cosines of a CLIP model lie far below the 0.7 that suits image-image scores."""
        if err := self._not_ready():
            return err, []
        try:
            query = self.embed_text([text] if isinstance(text, str) else text)[0].cpu()
        except Exception as e:
            return f"❌ Error embedding the text query: {str(e)}", []
        return self._search_with_query(query, similarity_threshold, max_results, query_filter, group_by)

    def search_by_text_and_image(self, text, max_results=5, candidates=100, fusion="rrf", text_weight=1.0, image_weight=1.0,
                                 image_threshold=None, query_filter=None):
        """"Regions that look like this picture AND match these words": the first region embedding of the query image and the
        embedding of ``text`` (a string, or several: one list each) are searched for their best ``candidates`` regions each,
        and the lists are fused by rank (``fusion="rrf"``) or by each list's standardised scores (``"dbsf"``) -- adding the
        raw scores, or searching with the averaged vector, would rank by the image alone, because the text-image cosines
        of a CLIP model lie far below the image-image ones.  ``image_threshold`` drops image-list members scoring below it;
        the ranks in the text lists are untouched.  Returns ``(text, items)``, items ``{"filename", "image_source", "bbox",
        "id", "score", "ranks", "scores"}`` best first: list 0 is the image, lists 1.. the prompts; ``ranks[j]`` is the
        region's rank in list j (0: not among its candidates), ``scores[j]`` its cosine against that query.  No thumbnails."""
        if err := self._not_ready(need_query=True):
            return err, []
        try:
            prompts = self.embed_text([text] if isinstance(text, str) else text)
        except Exception as e:
            return f"❌ Error embedding the text query: {str(e)}", []
        image = torch.as_tensor(self.region_embeddings[0], dtype=torch.float32).reshape(-1)
        n_text = int(prompts.shape[0])
        thresholds = None if image_threshold is None else [float(image_threshold)] + [None] * n_text
        with self._lock:
            hits = self.vector_db.query_fusion([image] + list(prompts), limit=int(max_results), prefetch_limit=int(candidates),
                                               fusion=fusion, weights=[float(image_weight)] + [float(text_weight)] * n_text,
                                               prefetch_thresholds=thresholds, query_filter=query_filter)
        if not hits:
            return _no_hits("regions found for this picture and text"), []
        items = [dict(_item(r.payload, r.id, r.score), ranks=r.ranks, scores=r.scores) for r in hits]
        out = f"🎯 Found {len(items)} regions for the picture and the text ({fusion}):\n\n"
        for n, it in enumerate(items):
            out += f"{n + 1}. {it['filename']}  fused {it['score']:.4f}  ranks {it['ranks']}  (Source: {it['image_source']})\n"
        return out, items

    def label_database(self, labels, query_filter=None, members=5):
        """Zero-shot labelling: every stored region (those a Qdrant-style ``query_filter`` selects, if given) gets the best
        of the prompts ``labels`` -- the exact assignment of ``Gallery.kmeans(max_iter=0)`` with the prompts' embeddings as
        centroids.  Returns ``(text, out)``: per label ``{"label", "count", "members": [{"filename", "image_source", "bbox",
        "id", "score"}]}`` with its ``members`` best-scoring regions, in the order of ``labels``."""
        if err := self._not_ready():
            return err, []
        labels = [labels] if isinstance(labels, str) else list(labels)
        if not labels:
            return "❌ Please provide at least one label", []
        try:
            with self._lock:
                db = self.vector_db
                if len(db) == 0:
                    return "⚠️ The database holds no regions", []
                lab, sc = db.assign(self.embed_text(labels), query_filter=query_filter)
                lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
                out = []
                for j, name in enumerate(labels):
                    rows = np.nonzero(lab == j)[0]
                    best = rows[np.lexsort((rows, -sc[rows]))][:int(members)]        # score desc, row asc
                    out.append({"label": name, "count": int(rows.size),
                                "members": [_item(db.payloads[r], db.ids[r], float(sc[r])) for r in best.tolist()]})
        except Exception as e:
            return f"❌ Error labelling the database: {str(e)}", []
        total = sum(o["count"] for o in out)
        text = f"🎯 {total} regions over {len(out)} labels:\n\n"
        for o in out:
            eg = f", e.g. {o['members'][0]['filename']} ({o['members'][0]['score']:.3f})" if o["members"] else ""
            text += f"- {o['label']}: {o['count']} regions{eg}\n"
        return text, out

    def search_similar_all_regions(self, similarity_threshold=None, max_results=5, query_filter=None, group_by="image_source"):
        """"Which images contain ALL of what this image shows?": EVERY region embedding of the query image is a query
        vector, the stored regions are grouped by payload key ``group_by``, and a group's score is the sum over the query
        regions of its best score among the group's regions (late-interaction MaxSim; up to 64 query regions).
        ``similarity_threshold`` cuts that SUM (it lies in [-n, n] for n query regions).  Returns ``(text, items)``: items
        ``{"image": the group's value, "score", "regions": [{"bbox", "score", "id", "filename"} per query region]}`` best first."""
        if err := self._not_ready(need_query=True):
            return err, []
        queries = torch.stack([torch.as_tensor(e, dtype=torch.float32).reshape(-1) for e in self.region_embeddings])
        if queries.shape[0] > 64:
            return f"❌ {queries.shape[0]} query regions: a multi-region search takes at most 64.", []
        with self._lock:
            res = self.vector_db.search_multivector(queries, group_by, limit=int(max_results),
                                                    score_threshold=None if similarity_threshold is None else float(similarity_threshold),
                                                    query_filter=query_filter)
        if not res:
            return _no_hits("images found for these regions", similarity_threshold), []
        items = [{"image": r.value, "score": r.score,
                  "regions": [{"bbox": h.payload.get("bbox"), "score": h.score, "id": h.id,
                               "filename": h.payload.get("filename", "Unknown")} for h in r.hits]} for r in res]
        text = f"🎯 Found {len(items)} images matching all {queries.shape[0]} query regions:\n\n"
        for n, it in enumerate(items):
            text += f"{n + 1}. {it['image']}  score {it['score']:.3f}\n"
            for q, reg in enumerate(it["regions"]):
                text += f"   region {q + 1}: 📍 {reg['bbox']}  score {reg['score']:.3f}\n"
        return text, items

    def search_all_similar(self, similarity_threshold=0.7, query_filter=None):
        """:meth:`search_similar` without ``max_results``: EVERY stored region whose vector scores at least
        ``similarity_threshold`` against the first region embedding (``query_filter``: only the points a Qdrant-style payload
        filter selects).  Returns ``(text, items)``, items ``{"filename", "image_source", "bbox", "id", "score"}`` best first.
        No thumbnails: the list can hold thousands of hits."""
        if err := self._not_ready(need_query=True):
            return err, []
        query = self.region_embeddings[0]
        with self._lock:
            hits = self.vector_db.search_range(query, float(similarity_threshold), query_filter=query_filter)
        if not hits:
            return _no_hits("similar regions found", similarity_threshold), []
        items = [_item(r.payload, r.id, r.score) for r in hits]
        text = f"🎯 Found {len(items)} similar regions:\n\n"
        return text + _listing(items), items

    def search_by_examples(self, positive, negative=(), similarity_threshold=None, max_results=5, query_filter=None):
        """Relevance feedback: "more like these, and not like those".  Each example is the ``id`` of a stored region (as
        earlier results return it), an embedding (tensor / array of the model's width) or an image (PIL image, array or
        path: embedded whole through the loaded model).  A region's score is its best score against a positive example
        when that beats its best score against a negative one, else minus the square of the latter; examples given by id
        are not returned.  Returns ``(text, items)``, items ``{"filename", "image_source", "bbox", "id", "score"}`` best first."""
        if err := self._not_ready():
            return err, []

        def examples(given):
            single = isinstance(given, (str, bytes)) or torch.is_tensor(given) or isinstance(given, (np.ndarray, Image.Image))
            return self._resolve_examples([given] if single else given or ())

        pos, neg = examples(positive), examples(negative)
        if not pos:
            return "❌ No positive examples given. Please pick at least one result or image.", []
        try:
            with self._lock:
                hits = self.vector_db.recommend(pos, neg, limit=int(max_results),
                                                score_threshold=None if similarity_threshold is None else float(similarity_threshold),
                                                query_filter=query_filter)
        except KeyError as e:
            return f"❌ {e.args[0]}", []
        if not hits:
            return _no_hits("regions found for these examples", similarity_threshold), []
        items = [_item(r.payload, r.id, r.score) for r in hits]
        text = f"🎯 Found {len(items)} regions like the {len(pos)} positive and unlike the {len(neg)} negative examples:\n\n"
        return text + _listing(items), items

    def _resolve_examples(self, examples):
        """Examples as the store takes them: an ``id`` or a vector stays, every image (PIL image, array or path) becomes
        its embedding -- all images in one batch."""
        out, images, slots = [], [], []
        for e in examples:
            is_id = isinstance(e, str) and not os.path.exists(e)
            is_vec = (torch.is_tensor(e) or isinstance(e, np.ndarray)) and np.ndim(e) == 1
            if is_id or is_vec:
                out.append(e)
            else:
                slots.append(len(out))
                out.append(None)
                images.append(pp.to_pil(Image.open(e).convert("RGB") if isinstance(e, str) else e))
        if images:
            for slot, v in zip(slots, self._embed_pils(images)):
                out[slot] = v
        return out

    def search_by_context(self, target, pairs, similarity_threshold=None, max_results=5, query_filter=None):
        """Discovery: matches for ``target`` under judgements of the form "this is the kind of thing I mean, that is not".
        ``pairs`` is a list of ``(positive, negative)``; ``target`` and every member of a pair is the ``id`` of a stored
        region, an embedding or an image, as in :meth:`search_by_examples`.  A region is ranked first by the number of
        pairs it lies on the positive side of, then by its similarity to the target; ``target=None`` returns the regions
        that satisfy the pairs (score 0: all of them).  Regions given by id are not returned.  Returns ``(text, items)``,
        items ``{"filename", "image_source", "bbox", "id", "score"}`` best first."""
        if err := self._not_ready():
            return err, []
        pairs = list(pairs or ())
        if any(not isinstance(p, (tuple, list)) or len(p) != 2 for p in pairs):
            return "❌ Every context entry must be a (positive, negative) pair.", []
        if target is None and not pairs:
            return "❌ No target and no context pairs given. Please pick a target or at least one pair.", []
        flat = self._resolve_examples([e for pair in pairs for e in pair] + ([] if target is None else [target]))
        context = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(pairs))]
        try:
            with self._lock:
                hits = self.vector_db.discover(None if target is None else flat[-1], context, limit=int(max_results),
                                               score_threshold=None if similarity_threshold is None else float(similarity_threshold),
                                               query_filter=query_filter)
        except KeyError as e:
            return f"❌ {e.args[0]}", []
        if not hits:
            return _no_hits("regions found for this context", similarity_threshold), []
        items = [_item(r.payload, r.id, r.score) for r in hits]
        text = (f"🎯 Found {len(items)} regions for the {'target' if target is not None else 'context'} under "
                f"{len(pairs)} context pairs:\n\n")
        return text + _listing(items), items

    def search_similar_diverse(self, similarity_threshold=0.7, max_results=5, diversity=0.5, candidates_limit=None,
                               query_filter=None):
        """:meth:`search_similar` without the near-copies: of the stored regions scoring at least ``similarity_threshold``
        against the first region embedding (the best ``candidates_limit`` of them, default ``max(max_results, 100)``),
        ``max_results`` are picked by maximal marginal relevance -- each pick trades its score against its similarity to
        the regions already picked (``diversity`` 0: the plain search, 1: as different as possible).  A database built from
        video frames or region crops otherwise answers with copies of one frame.  Returns ``(text, items)``, items
        ``{"filename", "image_source", "bbox", "id", "score"}`` in pick order.  No thumbnails."""
        if err := self._not_ready(need_query=True):
            return err, []
        query = self.region_embeddings[0]
        with self._lock:
            hits = self.vector_db.search_mmr(query, limit=int(max_results), diversity=float(diversity),
                                             candidates_limit=candidates_limit, score_threshold=float(similarity_threshold),
                                             query_filter=query_filter)
        if not hits:
            return _no_hits("similar regions found", similarity_threshold), []
        items = [_item(r.payload, r.id, r.score) for r in hits]
        text = f"🎯 Found {len(items)} similar regions (diversity {float(diversity):g}):\n\n"
        return text + _listing(items), items

    def find_duplicates(self, similarity_threshold=0.95, query_filter=None):
        """Groups of near-duplicate regions in the loaded database: every stored region whose vector scores at least
        ``similarity_threshold`` against another one, joined transitively (re-posted, re-compressed or re-cropped copies of
        one picture).  ``query_filter`` restricts it to the points a Qdrant-style payload filter selects.  Returns
        ``(text, groups)``: ``groups`` is a list of groups, each a list of ``{"filename", "image_source", "bbox", "id"}`` in
        storage order.  The default 0.95 is a guess: no trained checkpoint has been run here (parity
        unpinned), so what score separates copies from look-alikes is not measured."""
        if err := self._not_ready():
            return err, []
        with self._lock:
            db = self.vector_db
            rows = db.duplicate_row_groups(float(similarity_threshold), query_filter=query_filter)
            return self._duplicates_report(db, rows, similarity_threshold)

    @staticmethod
    def _duplicates_report(db, row_groups, similarity_threshold):
        """``(text, groups)`` of :meth:`find_duplicates` for groups given as lists of rows (the caller holds the lock)."""
        out = [[_item(db.payloads[r], db.ids[r]) for r in grp] for grp in row_groups]
        if not out:
            return f"No near-duplicates found at similarity threshold {similarity_threshold}", []
        text = f"🎯 Found {len(out)} groups of near-duplicates:\n\n"
        for g, members in enumerate(out):
            text += f"{g + 1}. {len(members)} regions\n"
            for m in members:
                text += f"   {m['filename']}  (Source: {m['image_source']})\n"
            text += "\n"
        return text, out

    def find_duplicate_clusters(self, similarity_threshold=0.95, query_filter=None, largest_first=True):
        """:meth:`find_duplicates` by the device route (``GalleryStore.duplicate_row_clusters``): the same groups in the same
        ``(text, groups)`` format, found without listing the pairs, so a group of tens of thousands of regions (the frames
        of a static shot) is returned where :meth:`find_duplicates` is refused.  ``largest_first`` orders the groups by
        (size descending, first region ascending) instead of by their first region."""
        if err := self._not_ready():
            return err, []
        with self._lock:
            db = self.vector_db
            rows = db.duplicate_row_clusters(float(similarity_threshold), query_filter=query_filter)
            if largest_first:
                rows = st.largest_first(rows)
            return self._duplicates_report(db, rows, similarity_threshold)

    def similarity_graph(self, max_neighbors=5, similarity_threshold=None, query_filter=None):
        """Every stored region's ``max_neighbors`` (at most 64) most similar other regions in the loaded database, cut at
        ``similarity_threshold`` if given (``GalleryStore.neighbor_graph``: the exact kNN graph, a level per region rather
        than the one threshold of :meth:`find_duplicates`).  ``query_filter`` restricts both ends to the points a
        Qdrant-style payload filter selects.  Returns ``(text, graph)``: ``graph`` has one entry per region, in storage
        order: ``{"filename", "image_source", "bbox", "id", "neighbors": [{"filename", "image_source", "id", "score"}]}``,
        neighbours best first."""
        if err := self._not_ready():
            return err, []
        try:
            with self._lock:
                db = self.vector_db
                g = db.neighbor_graph(limit=int(max_neighbors), score_threshold=similarity_threshold, query_filter=query_filter)
                payload_of = {i: p for i, p in zip(db.ids, db.payloads)}
        except Exception as e:
            return f"❌ Error building the similarity graph: {str(e)}", []
        out = [dict(_item(payload_of[i], i), neighbors=[]) for i in g.ids]
        for a, b, s in zip(g.offsets_row.tolist(), g.offsets_col.tolist(), g.scores.tolist()):
            nb = out[b]
            out[a]["neighbors"].append({"filename": nb["filename"], "image_source": nb["image_source"], "id": nb["id"],
                                        "score": float(s)})
        if not out:
            return "No regions to relate", []
        text = f"🎯 Neighbours of {len(out)} regions (up to {int(max_neighbors)} each):\n\n"
        for n, it in enumerate(out):
            near = ", ".join(f"{m['filename']} {m['score']:.3f}" for m in it["neighbors"]) or "none"
            text += f"{n + 1}. {it['filename']}: {near}\n"
        return text, out

    def summarize_database(self, n_themes=20, max_iter=10, seed=0, query_filter=None):
        """What is in the loaded database: its stored regions (those a Qdrant-style ``query_filter`` selects, if given)
        partitioned into ``n_themes`` themes by exact spherical k-means (``GalleryStore.themes``), largest first.  Returns
        ``(text, themes)``: each theme is ``{"size", "ids", "representative": {"filename", "image_source", "bbox", "id",
        "score"}}``, the representative being the member closest to the theme's centre."""
        if err := self._not_ready():
            return err, []
        try:
            with self._lock:
                db = self.vector_db
                if len(db) == 0:
                    return "⚠️ The database holds no regions", []
                themes = db.themes(int(n_themes), max_iter=int(max_iter), seed=int(seed), query_filter=query_filter)
        except Exception as e:
            return f"❌ Error summarizing the database: {str(e)}", []
        out = [{"size": t.size, "ids": t.ids,
                "representative": _item(t.representative_payload, t.representative_id, float(t.representative_score))}
               for t in themes]
        if not out:
            return "⚠️ No regions to summarize", []
        total = sum(t["size"] for t in out)
        text = f"🎯 {len(out)} themes over {total} regions:\n\n"
        for n, t in enumerate(out):
            text += f"{n + 1}. {t['size']} regions, e.g. {t['representative']['filename']} ({t['representative']['score']:.3f})\n"
        return text, out

    def delete_images(self, image_sources=None, query_filter=None):
        """Remove stored regions from the loaded database, in place: every region of the source images ``image_sources``
        (one path or a list; payload key ``image_source``) or every region a Qdrant-style ``query_filter`` selects (both
        given: regions that meet both).  The database behind the reference does this with ``delete(points_selector=...)``;
        here the rows move on the device and the database directory gets one ``delete`` line (``GalleryStore.delete``).
        Returns a status string with the number of regions removed."""
        if err := self._not_ready():
            return err
        if isinstance(image_sources, str):
            image_sources = [image_sources]
        image_sources = list(image_sources or [])
        if not image_sources and query_filter is None:
            return "❌ Please provide image sources or a filter"
        try:
            must = []
            if image_sources:
                must.append(filters.FieldCondition("image_source", match=filters.MatchAny(image_sources)))
            if query_filter is not None:
                must.append(filters.as_filter(query_filter))
            with self._lock:
                n = self.vector_db.delete(filters.Filter(must=must))
                if n and self.vector_db.path:
                    self.vector_db.save()                # the manifest is a finished database again
                left = len(self.vector_db)
        except Exception as e:
            return f"❌ Error deleting regions: {str(e)}"
        if n == 0:
            return "⚠️ No stored regions matched: nothing deleted"
        return f"✅ Deleted {n} regions ({left} left in database: {self.current_database})"

    def visualize_detections(self, image, selected_region_index=None):
        """core_system.py:719-757 draws mask contours with OpenCV (UI cosmetics, out of scope);
        boxes are outlined with PIL so the UI keeps working."""
        pil = pp.to_pil(image).copy()
        if not self.detected_regions or len(self.detected_regions) == 0:
            return pil
        draw = ImageDraw.Draw(pil)
        for i, box in enumerate(self.detected_regions.xyxy):
            sel = i == selected_region_index
            draw.rectangle([float(v) for v in box], outline=(0, 255, 0) if sel else (255, 0, 0), width=3 if sel else 1)
            draw.text((float(box[0]) + 3, float(box[1]) + 3), f"{i + 1}", fill=(0, 0, 0) if sel else (255, 0, 0))
        return pil
