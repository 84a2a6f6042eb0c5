"""Host side of the hot path: ``embed()`` / ``search()`` over librevo's C ABI.

Python owns orchestration only (device tensors, streams, weight hand-over); every
kernel on the path is HIP inside ``librevo.so``.  The entry points mirror what
the reference does at

* ``core_system.py:431-455`` ``process_image_direct_pe``  ->  :meth:`VitEngine.embed`
* ``core_system.py:596-622`` collection create + upsert     ->  :class:`Gallery`
* ``core_system.py:650-664`` ``search_similar`` / ``vector_db.search``  ->  :meth:`Gallery.search`
"""
import contextlib
import ctypes as C
import dataclasses
import json
import threading

import torch

from . import _lib
from .config import PEConfig, PETextConfig, get_config, get_text_config
from .weights import (check_state_dict, check_text_state_dict, expected_text_shapes, resolve_config, strip_non_parameters,
                      synth_text_weights, synth_weights)

IMAGE_F32 = 0
IMAGE_U8 = 1


def _require_cuda(t, name, device=None):
    if not t.is_cuda:
        raise _lib.RevoError(f"{name} must be a device tensor (the hot path has no CPU fallback)")
    if device is not None and t.device != device:
        raise _lib.RevoError(f"{name} is on {t.device} but the handle is bound to {device}")


def _f32(t, name, device=None, host_ok=False):
    """A caller's tensor as the ABI reads it: checked to be on ``device`` (a host tensor passes with ``host_ok``), fp32,
    contiguous."""
    if t.is_cuda or not host_ok:
        _require_cuda(t, name, device)
    return t.detach().to(torch.float32).contiguous()


def _rows(t, name, dim, device, form="n", host_ok=False, one_row=True):
    """A caller's vectors as fp32 contiguous rows ``[n, dim]`` for a handle on ``device`` (:func:`_f32`); a single vector
    ``[dim]`` is one row where the method takes that (``one_row``).  ``form`` is how the message names the row count."""
    t = _f32(t, name, device, host_ok)
    if one_row and t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[1] != dim:
        raise ValueError(f"{name} must be [{form}, {dim}], got {tuple(t.shape)}")
    return t


def _threshold(score_threshold):
    """``(has_threshold, threshold)`` as the ABI takes an optional score threshold: 0.0 is a threshold, None is none."""
    return (0, 0.0) if score_threshold is None else (1, float(score_threshold))


def _as_device(device):
    d = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


def _tensor_array(state_dict, names):
    """The ``revo_tensor`` array of ``names`` for a create call, and the fp32 tensors it points into (keep them alive until
    the call returns)."""
    keep = []
    arr = (_lib.Tensor * len(names))()
    for i, n in enumerate(names):
        t = state_dict[n].detach().to(torch.float32).contiguous()
        keep.append(t)
        arr[i].name = n.encode()
        arr[i].data = t.data_ptr()
        arr[i].numel = t.numel()
    return arr, keep


class _Handle:
    """A handle of the library held by ``self._h`` in ``self._lib``, destroyed by the entry point ``_destroy`` names."""
    _destroy = None

    @contextlib.contextmanager
    def _frame(self):
        """Inside: the handle's lock is held and its device is the current one."""
        with self._lock, torch.cuda.device(self.device):
            yield

    def _call(self, name, *args):
        """The library's entry point ``name`` with this handle first; a status other than 0 raises, naming it."""
        _lib.check(getattr(self._lib, name)(self._h, *args), name)

    def _chunks(self, n):
        """``(start, end)`` of ``n`` inputs in forwards of at most ``max_batch``."""
        for s in range(0, n, self.max_batch):
            yield s, min(n, s + self.max_batch)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _need_hooks(engine, what):
    if not engine.experiments:
        raise _lib.RevoError(f"{what} is a parity-test hook of librevo_exp.so: create the engine with experiments=True")


@dataclasses.dataclass
class Detections:
    """The result of :meth:`VitEngine.detect` (include/revo.h, DETECT): one entry per region, images ascending, device
    tensors.  ``image`` / ``prompt`` / ``cells`` int32 ``[n]``, ``boxes`` int32 ``[n, 4]`` (gx0, gy0, gx1, gy1, inclusive, in
    cells), ``confidence`` fp32 ``[n]``, ``bits`` int32 ``[n, ceil(S / 32)]`` (the uint32 token bitmaps reinterpreted: what
    :meth:`VitEngine.embed_regions` takes), ``vectors`` fp32 ``[n, out_dim]`` or ``None``; with maps, ``scores`` fp32
    ``[B, P, g * g]`` and ``labels`` int32 ``[B, g * g]``; ``global_vectors`` fp32 ``[B, out_dim]`` when asked for."""
    image: torch.Tensor
    prompt: torch.Tensor
    boxes: torch.Tensor
    cells: torch.Tensor
    confidence: torch.Tensor
    bits: torch.Tensor
    vectors: torch.Tensor = None
    scores: torch.Tensor = None
    labels: torch.Tensor = None
    global_vectors: torch.Tensor = None

    def __len__(self):
        return int(self.image.shape[0])


class VitEngine(_Handle):
    """A PE vision tower resident on one GPU (weights bf16, fp32 residual stream)."""

    _destroy = "revo_vit_destroy"

    def __init__(self, cfg: PEConfig, state_dict, device=0, max_batch=64, experiments=False):
        # LayerScale follows the checkpoint; unknown `visual.*` tensors are rejected by name
        cfg = resolve_config(cfg, state_dict)
        self.cfg = cfg
        self.device = _as_device(device)
        self.max_batch = int(max_batch)
        self._lock = threading.Lock()
        # experiments=True: the handle lives in librevo_exp.so, the only library with the parity-test hooks
        # (residual_after / taps); the product library cannot stop a forward early or hand out intermediates
        self.experiments = bool(experiments) or _lib.product_is_experiment_build()
        lib = _lib.load_exp() if experiments else _lib.load()
        check_state_dict(cfg, state_dict)
        # the image tower only (a whole-CLIP state dict also holds the text tower), without registered buffers
        state_dict = strip_non_parameters({k: v for k, v in state_dict.items() if k.startswith("visual.")})
        names = sorted(state_dict)
        arr, keep = _tensor_array(state_dict, names)          # keep: alive until create returns
        c = _lib.VitCfg(cfg.image_size, cfg.patch_size, cfg.width, cfg.layers, cfg.heads, cfg.mlp_dim, cfg.out_dim,
                        cfg.pool_heads, int(cfg.use_cls), int(cfg.use_ls), cfg.ln_eps, cfg.rope_theta, cfg.pool_mlp_dim)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _lib.check(lib.revo_vit_create(C.byref(c), arr, len(names), self.device.index or 0, self.max_batch,
                                           C.byref(h)), "revo_vit_create")
        self._h = h
        self._lib = lib

    @classmethod
    def synthetic(cls, name_or_cfg="PE-Core-L14-336", seed=0, device=0, max_batch=64, experiments=False, **kw):
        cfg = name_or_cfg if isinstance(name_or_cfg, PEConfig) else get_config(name_or_cfg)
        dev = torch.device("cuda", device)
        sd = synth_weights(cfg, seed=seed, device=dev, **kw)
        return cls(cfg, sd, device=device, max_batch=max_batch, experiments=experiments)

    def _grid(self, grid):
        """``grid=None | (gh, gw)`` -> ``(gh, gw, S)``: the token grid of a call (include/revo.h, GRIDS) and its tokens per
        image.  ``None`` is the tower's native ``g x g``; any shape within its ``g * g`` cells is accepted
        (``config.aspect_grid`` chooses one for an image)."""
        g = self.cfg.grid
        if grid is None:
            gh = gw = g
        else:
            gh, gw = (int(v) for v in grid)
            if gh < 1 or gw < 1 or gh * gw > g * g:
                raise ValueError(f"grid must be (gh, gw) with positive sides and gh * gw <= {g} * {g}, got {tuple(grid)!r}")
        return gh, gw, gh * gw + (1 if self.cfg.use_cls else 0)

    @contextlib.contextmanager
    def _grid_frame(self, grid):
        """:meth:`_frame` with the handle set to ``grid`` inside -- yields the stream -- and back to native on the way out,
        whatever happened: a call without ``grid`` always runs native."""
        gh, gw, _ = self._grid(grid)
        with self._frame():
            st = _lib.current_stream()
            self._call("revo_vit_set_grid", gh, gw, st)
            try:
                yield st
            finally:
                self._lib.revo_vit_set_grid(self._h, 0, 0, st)

    def _images(self, images, grid=None):
        """``images`` validated for a forward on ``grid``: contiguous, and its ``image_dtype``."""
        _require_cuda(images, "images", self.device)
        gh, gw, _ = self._grid(grid)
        h, w = gh * self.cfg.patch_size, gw * self.cfg.patch_size
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != h or images.shape[3] != w:
            raise ValueError(f"images must be [B,3,{h},{w}]" + (f" for grid ({gh}, {gw})" if grid is not None else "") +
                             f", got {tuple(images.shape)}")
        if images.dtype == torch.uint8:
            kind = IMAGE_U8
        elif images.dtype == torch.float32:
            kind = IMAGE_F32
        else:
            raise ValueError("images must be uint8 or float32")
        return images.contiguous(), kind

    # -- the embed entry point ------------------------------------------------
    def embed(self, images, normalize=True, out=None, grid=None):
        """images: uint8 or float32 ``[B,3,H,W]`` device tensor at the model
        resolution (float input already normalised to [-1,1], i.e. what
        ``self.preprocess`` yields at core_system.py:439).  Returns fp32
        ``[B, out_dim]`` on the device, L2-normalised (core_system.py:447).
        ``grid=(gh, gw)``: native-aspect embedding (include/revo.h, GRIDS) -- the images are
        ``[B,3,gh * patch,gw * patch]`` and the forward runs on that token grid."""
        images, kind = self._images(images, grid)
        cfg = self.cfg
        B = images.shape[0]
        if out is None:
            out = torch.empty((B, cfg.out_dim), dtype=torch.float32, device=images.device)
        with self._grid_frame(grid) as st:
            for s, e in self._chunks(B):
                self._call("revo_vit_forward", _lib.ptr(images[s:e]), kind, e - s, _lib.ptr(out[s:e]), int(bool(normalize)), st)
        return out

    def embed_regions(self, images, region_image, token_bits, normalize=True, with_global=True, grid=None):
        """A vector per region for one forward per image (include/revo.h, REGIONS): region ``r`` is pooled over the tokens
        of image ``region_image[r]`` that ``token_bits[r]`` allows (``regions.token_masks``: ``[R, ceil(S / 32)]`` as a
        uint32 / int32 numpy array, or an int32 torch tensor on the host or on this device).  ``images`` as in
        :meth:`embed`.  Returns ``(global, regions)``: fp32 ``[B, out_dim]`` (exactly :meth:`embed`'s rows; ``None``
        without ``with_global``) and fp32 ``[R, out_dim]`` in the caller's order.  A region that allows every token has
        its image's global vector bit for bit, one that allows none is all zeros.  Batches above ``max_batch`` are split
        and every region goes with its image.  Under ``grid=(gh, gw)`` the bitmaps are those of that grid
        (``regions.token_masks(..., grid=grid)``)."""
        import numpy as np
        images, kind = self._images(images, grid)
        cfg = self.cfg
        seq = self._grid(grid)[2]
        B, words = images.shape[0], (seq + 31) // 32
        ri = torch.as_tensor(np.asarray(region_image.cpu() if isinstance(region_image, torch.Tensor) else region_image,
                                        dtype=np.int64).reshape(-1))
        R = ri.shape[0]
        if R and (int(ri.min()) < 0 or int(ri.max()) >= B):
            raise IndexError(f"region_image must name images of the batch, 0 <= index < {B}")
        if isinstance(token_bits, torch.Tensor):
            if token_bits.dtype != torch.int32:
                raise ValueError("token_bits as a tensor must be int32 (the uint32 words reinterpreted)")
            bits = token_bits.contiguous()
            if bits.is_cuda:
                _require_cuda(bits, "token_bits", self.device)
        else:
            bits = torch.from_numpy(np.ascontiguousarray(np.asarray(token_bits)).astype(np.uint32, copy=False).view(np.int32))
        if bits.dim() != 2 or bits.shape[0] != R or bits.shape[1] != words:
            raise ValueError(f"token_bits must be [{R}, {words}] (one bitmap of ceil({seq} / 32) words per region), "
                             f"got {tuple(bits.shape)}")
        if B == 0 or (R == 0 and not with_global):
            return (torch.empty((B, cfg.out_dim), dtype=torch.float32, device=images.device) if with_global else None,
                    torch.empty((R, cfg.out_dim), dtype=torch.float32, device=images.device))
        out_g = torch.empty((B, cfg.out_dim), dtype=torch.float32, device=images.device) if with_global else None
        out_r = torch.empty((R, cfg.out_dim), dtype=torch.float32, device=images.device)
        with self._grid_frame(grid) as st:
            for s, e in self._chunks(B):
                whole = s == 0 and e == B
                sel = None if whole else torch.nonzero((ri >= s) & (ri < e)).reshape(-1)
                n = R if whole else int(sel.shape[0])
                if n == 0 and not with_global:
                    continue
                idx = (ri if whole else ri[sel] - s).to(torch.int32).contiguous()
                cb = bits if whole else bits[sel.to(bits.device)].contiguous()
                dst = out_r if whole else torch.empty((n, cfg.out_dim), dtype=torch.float32, device=images.device)
                self._call("revo_vit_forward_regions", _lib.ptr(images[s:e]), kind, e - s, _lib.ptr(idx) if n else None,
                           _lib.ptr(cb) if n else None, int(cb.is_cuda), n, _lib.ptr(out_g[s:e]) if with_global else None,
                           _lib.ptr(dst) if n else None, int(bool(normalize)), st)
                if not whole and n:
                    out_r.index_copy_(0, sel.to(out_r.device), dst)
        return out_g, out_r

    def embed_tokens(self, images, normalize=True, with_global=True, grid=None):
        """A vector per token from one forward per image (include/revo.h, TOKENS): returns ``(global, tokens)``, fp32
        ``[B, out_dim]`` (exactly :meth:`embed`'s rows; ``None`` without ``with_global``) and fp32 ``[B, S, out_dim]``.
        Token ``s`` of image ``b`` has, bit for bit, the vector :meth:`embed_regions` gives the region that allows token ``s``
        alone.  Token 0 is the class token on towers that have one; patch ``(gy, gx)`` is token ``use_cls + gy * g + gx``
        (``use_cls + gy * gw + gx`` and ``S = gh * gw + use_cls`` under ``grid=(gh, gw)``)."""
        images, kind = self._images(images, grid)
        cfg = self.cfg
        B = images.shape[0]
        out_g = torch.empty((B, cfg.out_dim), dtype=torch.float32, device=images.device) if with_global else None
        out_t = torch.empty((B, self._grid(grid)[2], cfg.out_dim), dtype=torch.float32, device=images.device)
        with self._grid_frame(grid) as st:
            for s, e in self._chunks(B):
                self._call("revo_vit_forward_tokens", _lib.ptr(images[s:e]), kind, e - s,
                           _lib.ptr(out_g[s:e]) if with_global else None, _lib.ptr(out_t[s:e]), int(bool(normalize)), st)
        return out_g, out_t

    def detect(self, images, prompts, thresholds=None, n_background=0, min_cells=1, max_regions=50, with_vectors=True,
               with_maps=False, normalize=True, with_global=False):
        """Text-prompted regions (include/revo.h, DETECT): every patch cell goes to the prompt vector its token vector scores
        highest against, and the label map is cut into 4-connected regions.  ``prompts``: fp32 ``[P, out_dim]`` on this
        device (``TextEngine.embed``'s rows, or any vectors of the space), the last ``n_background`` of them background
        prompts that take cells and give no region; ``thresholds``: ``None`` (-inf for every prompt), a number, or ``P``
        numbers.  Regions of fewer than ``min_cells`` cells are dropped; per image the best ``max_regions`` by
        (confidence, lowest cell) are kept -- 50 is the reference's region cap.  Returns a :class:`Detections`: images
        ascending, device tensors.  Synchronous.  The contract is numerical: nothing is claimed about detection quality."""
        import numpy as np
        images, kind = self._images(images)
        cfg = self.cfg
        pr = _rows(prompts, "prompts", cfg.out_dim, self.device, "P", one_row=False)
        P = pr.shape[0]
        if thresholds is None:
            thr = np.full(P, -np.inf, dtype=np.float32)
        else:
            thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (P,)))
        B, words, G2 = images.shape[0], (cfg.seq + 31) // 32, cfg.grid * cfg.grid
        if B == 0:
            raise ValueError("detect: images holds no image")
        dev = images.device
        parts = []
        out_g = torch.empty((B, cfg.out_dim), dtype=torch.float32, device=dev) if with_global else None
        with self._frame():
            st = _lib.current_stream()
            for s, e in self._chunks(B):
                n = C.c_int64()
                self._call("revo_vit_detect", _lib.ptr(images[s:e]), kind, e - s, _lib.ptr(pr), P, C.c_void_p(thr.ctypes.data),
                           int(n_background), int(min_cells), int(max_regions), _lib.ptr(out_g[s:e]) if with_global else None,
                           int(bool(with_vectors)), int(bool(normalize)), C.byref(n), st)
                n = int(n.value)
                d = Detections(
                    image=torch.empty((n,), dtype=torch.int32, device=dev), prompt=torch.empty((n,), dtype=torch.int32, device=dev),
                    boxes=torch.empty((n, 4), dtype=torch.int32, device=dev), cells=torch.empty((n,), dtype=torch.int32, device=dev),
                    confidence=torch.empty((n,), dtype=torch.float32, device=dev),
                    bits=torch.empty((n, words), dtype=torch.int32, device=dev),
                    vectors=torch.empty((n, cfg.out_dim), dtype=torch.float32, device=dev) if with_vectors else None)
                if n:
                    self._call("revo_vit_detect_read", 0, n, _lib.ptr(d.image), _lib.ptr(d.prompt), _lib.ptr(d.boxes),
                               _lib.ptr(d.cells), _lib.ptr(d.confidence), _lib.ptr(d.bits), _lib.ptr(d.vectors), 1)
                if with_maps:
                    d.scores = torch.empty((e - s, P, G2), dtype=torch.float32, device=dev)
                    d.labels = torch.empty((e - s, G2), dtype=torch.int32, device=dev)
                    self._call("revo_vit_detect_maps", _lib.ptr(d.scores), _lib.ptr(d.labels), 1)
                d.image += s
                parts.append(d)
        if len(parts) == 1:
            out = parts[0]
        else:
            cat = lambda name: (None if getattr(parts[0], name) is None else torch.cat([getattr(p, name) for p in parts]))
            out = Detections(**{f.name: cat(f.name) for f in dataclasses.fields(Detections) if f.name != "global_vectors"})
        out.global_vectors = out_g
        return out

    def ln_fold_stats(self, reset=False):
        """Telemetry of the LayerNorm folded into qkv / fc1 (include/revo.h revo_vit_stats; synchronises the current stream):
        rows whose statistics the consuming GEMMs merged since the last reset, how many of them had |mean| / std above
        ``ratio`` (and above four times it) -- the regime in which the fold's rounding error exceeds the LayerNorm kernel's."""
        out = (C.c_double * 4)()
        with self._frame():
            self._call("revo_vit_stats", out, int(bool(reset)), _lib.current_stream())
        return {"rows": int(out[0]), "rows_above_ratio": int(out[1]), "rows_above_4x_ratio": int(out[2]), "ratio": float(out[3])}

    # -- parity-test hook -----------------------------------------------------
    def residual_after(self, images, n_layers, grid=None):
        """fp32 residual stream [B, S, W] after ln_pre and the first n blocks."""
        _need_hooks(self, "residual_after")
        images, kind = self._images(images, grid)
        B = images.shape[0]
        assert B <= self.max_batch
        x = torch.empty((B, self._grid(grid)[2], self.cfg.width), dtype=torch.float32, device=images.device)
        dummy = torch.empty((B, self.cfg.out_dim), dtype=torch.float32, device=images.device)
        with self._grid_frame(grid) as st:
            self._call("revo_vit_set_debug_layers", int(n_layers))
            try:
                self._call("revo_vit_forward", _lib.ptr(images), kind, B, _lib.ptr(dummy), 0, st)
                self._call("revo_vit_read_residual", B, _lib.ptr(x), st)
            finally:
                self._lib.revo_vit_set_debug_layers(self._h, -1)
        return x


    def taps(self, images, grid=None):
        """Parity-test hook: intermediate activations of one forward as fp32 CPU-comparable tensors:
        ``embed`` [B,S,W] (patch embed + position + class token, before ln_pre), ``ln_post`` [B,S,W] (fp32: the head
        works in fp32), ``pooled`` [B,W] (attention-pool output before proj) and the ``embedding`` [B,D]."""
        _need_hooks(self, "taps")
        _require_cuda(images, "images", self.device)
        B = images.shape[0]
        assert B <= self.max_batch
        cfg = self.cfg
        out = {"embed": self.residual_after(images, -2, grid=grid)}
        emb = self.embed(images, grid=grid)
        lnp = torch.empty((B, self._grid(grid)[2], cfg.width), dtype=torch.float32, device=self.device)
        pooled = torch.empty((B, cfg.width), dtype=torch.float32, device=self.device)
        with self._grid_frame(grid) as st:          # (the rows of the forward just run: the tap's size follows the grid)
            self._call("revo_vit_read_tap", 1, B, _lib.ptr(lnp), st)
            self._call("revo_vit_read_tap", 2, B, _lib.ptr(pooled), st)
        out.update(ln_post=lnp, pooled=pooled, embedding=emb)
        return out


class TextEngine(_Handle):
    """The text tower of the same CLIP checkpoint resident on one GPU (include/revo.h, TEXT): prompts -> vectors in the
    image embeddings' space.  ``state_dict``: the tower's tensors under their upstream names without a prefix
    (``weights.load_text_state_dict`` / ``weights.text_state_dict``)."""

    _destroy = "revo_text_destroy"

    def __init__(self, cfg: PETextConfig, state_dict, device=0, max_batch=256, experiments=False, tokenizer=None):
        self.cfg = cfg
        self.device = _as_device(device)
        self.max_batch = int(max_batch)
        self.tokenizer = tokenizer
        self._lock = threading.Lock()
        self.experiments = bool(experiments) or _lib.product_is_experiment_build()
        lib = _lib.load_exp() if experiments else _lib.load()
        check_text_state_dict(cfg, state_dict)
        names = sorted(k for k in state_dict if k in expected_text_shapes(cfg))
        arr, keep = _tensor_array(state_dict, names)          # keep: alive until create returns
        c = _lib.TextCfg(cfg.context_length, cfg.vocab_size, cfg.width, cfg.layers, cfg.heads, cfg.mlp_dim, cfg.out_dim,
                         int(cfg.use_ls), cfg.ln_eps)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _lib.check(lib.revo_text_create(C.byref(c), arr, len(names), self.device.index or 0, self.max_batch,
                                            C.byref(h)), "revo_text_create")
        self._h = h
        self._lib = lib

    @classmethod
    def synthetic(cls, name_or_cfg="PE-Core-L14-336", seed=0, device=0, max_batch=256, experiments=False, tokenizer=None, **kw):
        cfg = name_or_cfg if isinstance(name_or_cfg, PETextConfig) else get_text_config(name_or_cfg)
        sd = synth_text_weights(cfg, seed=seed, device=torch.device("cuda", device), **kw)
        return cls(cfg, sd, device=device, max_batch=max_batch, experiments=experiments, tokenizer=tokenizer)

    @staticmethod
    def _host_tokens(tokens):
        import numpy as np
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.detach().cpu().numpy()
        t = np.asarray(tokens)
        if t.ndim != 2 or t.dtype.kind not in "iu":
            raise ValueError(f"tokens must be an integer array [n, seq_len], got {t.dtype} {t.shape}")
        if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
            raise ValueError("token ids must fit int32")
        return np.ascontiguousarray(t.astype(np.int32, copy=False))

    def embed_tokens(self, tokens, normalize=True, trim=False, out=None):
        """tokens: integer ``[n, seq_len]`` on the host, ``1 <= seq_len <= context_length``, every id in ``[0, vocab)``
        (anything else raises, naming the prompt and the position; nothing reaches the device).  Returns fp32
        ``[n, out_dim]`` on the device.  ``trim=True`` cuts the columns behind the batch's longest prompt (its end token:
        the largest id) before the call -- the same rows, fewer of them."""
        t = self._host_tokens(tokens)
        n, L = t.shape
        if trim and n:
            L = int((t.argmax(axis=1)).max()) + 1
            t = t[:, :L].copy()
        if out is None:
            out = torch.empty((n, self.cfg.out_dim), dtype=torch.float32, device=self.device)
        _require_cuda(out, "out", self.device)
        with self._frame():
            st = _lib.current_stream()
            for s, e in self._chunks(n):
                part = t[s:e]
                self._call("revo_text_forward", C.c_void_p(part.ctypes.data), e - s, L, _lib.ptr(out[s:e]), int(bool(normalize)), st)
        return out

    def embed(self, texts, normalize=True, trim=True):
        """Prompts (a string or a list of strings) through the tokenizer and :meth:`embed_tokens`."""
        if self.tokenizer is None:
            from .tokenizer import ClipTokenizer
            try:
                self.tokenizer = ClipTokenizer(None, context_length=self.cfg.context_length, vocab_size=self.cfg.vocab_size)
            except FileNotFoundError as exc:
                raise _lib.RevoError(f"embedding strings needs a tokenizer: {exc}") from exc
        return self.embed_tokens(self.tokenizer(texts, self.cfg.context_length), normalize=normalize, trim=trim)

    # -- parity-test hook -----------------------------------------------------
    def residual_after(self, tokens, n_layers):
        """fp32 residual stream [n, seq_len, W] after the first n blocks (-2: the embedded tokens)."""
        _need_hooks(self, "residual_after")
        t = self._host_tokens(tokens)
        n, L = t.shape
        assert 1 <= n <= self.max_batch
        x = torch.empty((n, L, self.cfg.width), dtype=torch.float32, device=self.device)
        dummy = torch.empty((n, self.cfg.out_dim), dtype=torch.float32, device=self.device)
        with self._frame():
            st = _lib.current_stream()
            self._call("revo_text_set_debug_layers", int(n_layers))
            try:
                self._call("revo_text_forward", C.c_void_p(t.ctypes.data), n, L, _lib.ptr(dummy), 0, st)
                self._call("revo_text_read_residual", n, _lib.ptr(x), st)
            finally:
                self._lib.revo_text_set_debug_layers(self._h, -1)
        return x


class Gallery(_Handle):
    """Device-resident cosine gallery: normalised rows as bf16 (scan copy) plus an
    fp32 master copy used for exact re-scoring and persistence."""

    _destroy = "revo_gallery_destroy"

    def __init__(self, dim, capacity, device=0, keep_f32=True, experiments=False):
        self.dim = int(dim)
        self.capacity = int(capacity)
        self.device = _as_device(device)
        self._lock = threading.Lock()
        self._total_rows = 0                      # set_total_rows: rows of the sharded gallery this handle is a shard of (0: none)
        # experiments=True: a handle of librevo_exp.so, the only library in which a search can be forced through (or
        # kept from) its exact fallbacks (set_search_mode: parity tests and timing scripts)
        self.experiments = bool(experiments) or _lib.product_is_experiment_build()
        self._lib = _lib.load_exp() if experiments else _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.revo_gallery_create(self.dim, self.capacity, self.device.index or 0, int(keep_f32),
                                                     C.byref(h)), "revo_gallery_create")
        self._h = h

    def __len__(self):
        return int(self._lib.revo_gallery_size(self._h))

    def clear(self):
        self._call("revo_gallery_clear")

    def add(self, vectors, normalize=True):
        """Append fp32 rows [n, dim] (device or host tensor).  Rows are normalised
        at insert like qdrant's COSINE collections (core_system.py:600-603)."""
        v = _rows(vectors, "vectors", self.dim, self.device, host_ok=True, one_row=False)
        start = len(self)
        with self._frame():
            # a device source is read by kernels on torch's current stream: its memory is not reused before they have
            # run (the caching allocator is stream-ordered), so nothing waits here -- an ingest appends batch after
            # batch without a host round trip; a host source is staged and synchronised inside the call
            self._call("revo_gallery_append", _lib.ptr(v), v.shape[0], int(bool(normalize)), int(v.is_cuda), _lib.current_stream())
        return start

    ADD_UNIQUE_MAX = 16384                        # rows of one revo_gallery_append_unique call (DEDUP_MAX_BATCH, kernels.h)

    def add_unique(self, vectors, threshold, normalize=True):
        """Append only the rows that are no near-duplicate (include/revo.h, DEDUP): row by row, a vector whose exact fp32
        score against a gallery row or an earlier kept row of ``vectors`` reaches ``threshold`` is dropped.  Returns
        ``(rows int64 [n], scores fp32 [n], kept bool [n])`` on the device: a kept row's new row index and -inf, a dropped
        row's representative (the first such row) and its score.  The gallery needs room for every row of a call, kept or
        not; inputs above ``ADD_UNIQUE_MAX`` rows go in consecutive calls, which gives the same result.  Synchronous."""
        v = _rows(vectors, "vectors", self.dim, self.device, host_ok=True, one_row=False)
        n = int(v.shape[0])
        rows = torch.empty((n,), dtype=torch.int64, device=self.device)
        scores = torch.empty((n,), dtype=torch.float32, device=self.device)
        kept = C.c_int64()
        with self._frame():
            for a in range(0, n, self.ADD_UNIQUE_MAX):
                b = min(n, a + self.ADD_UNIQUE_MAX)
                self._call("revo_gallery_append_unique", _lib.ptr(v[a:b]), b - a, int(bool(normalize)), int(v.is_cuda),
                           float(threshold), _lib.ptr(rows[a:b]), _lib.ptr(scores[a:b]), 1, C.byref(kept), _lib.current_stream())
        return rows, scores, torch.isinf(scores) & (scores < 0)

    def remove(self, rows):
        """Take rows out in place (include/revo.h, EDIT): ``rows`` is a ``bool [len]`` mask, a packed int32 bitmap
        ``[ceil(len / 32)]`` (bit ``r & 31`` of word ``r >> 5``) or an int64 index tensor, on the device or the host.  The
        remaining rows keep their order and close up: every search afterwards returns exactly what it returns on a gallery
        built from the remaining rows alone.  Returns the number of rows removed.  Synchronous."""
        n = len(self)
        rows = torch.as_tensor(rows)
        if rows.is_cuda:
            _require_cuda(rows, "rows", self.device)
        if rows.dtype == torch.int64:
            idx = rows.reshape(-1)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
                raise IndexError(f"remove: row index outside the gallery of {n} rows")
            rows = torch.zeros(n, dtype=torch.bool, device=idx.device)
            rows[idx] = True
        words = (n + 31) // 32
        if rows.dtype == torch.bool:
            if rows.dim() != 1 or rows.shape[0] != n:
                raise ValueError(f"rows must be bool [{n}] (one entry per gallery row), got {tuple(rows.shape)}")
            if rows.is_cuda:
                bits = self.allow_bits(rows)
            else:
                from .filters import pack_bits
                bits = torch.from_numpy(pack_bits(rows.numpy()))
        elif rows.dtype == torch.int32 and rows.dim() == 1 and rows.shape[0] == words:
            bits = rows.contiguous()
        else:
            raise ValueError(f"rows must be bool [{n}], a packed int32 bitmap [{words}] or int64 indices, got {rows.dtype} "
                             f"{tuple(rows.shape)}")
        removed = C.c_int64()
        with self._frame():
            self._call("revo_gallery_remove", _lib.ptr(bits), n, int(bits.is_cuda), C.byref(removed), _lib.current_stream())
        return int(removed.value)

    def update(self, rows, vectors, normalize=True):
        """Overwrite row ``rows[i]`` with ``vectors[i]`` (fp32 ``[n, dim]``, device or host) exactly as :meth:`add` would
        have written it (include/revo.h, EDIT).  ``rows``: int64 indices (tensor or list), each inside the gallery and given
        once.  A filter or group ids stay valid: no row moves."""
        idx = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu().contiguous()
        v = _rows(vectors, "vectors", self.dim, self.device, idx.shape[0], host_ok=True, one_row=False)
        if v.shape[0] != idx.shape[0]:
            raise ValueError(f"vectors must be [{idx.shape[0]}, {self.dim}] (one per row index), got {tuple(v.shape)}")
        with self._frame():
            self._call("revo_gallery_update", _lib.ptr(idx), _lib.ptr(v), idx.shape[0], int(bool(normalize)), int(v.is_cuda),
                       _lib.current_stream())

    def read(self, start=0, n=None):
        n = len(self) - start if n is None else n
        out = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            self._call("revo_gallery_read", start, n, _lib.ptr(out), 1)
        return out

    def cert_stats(self):
        """The certificate's maxima as the searches read them: ``(G, Eg)`` with ``G >= ||g||`` and ``Eg >= ||bf16(g) - g||``
        for every row now present (include/revo.h, revo_op_gallery_cert_stats).  Synchronous."""
        out = (C.c_float * 2)()
        with self._frame():
            self._call("revo_op_gallery_cert_stats", out, _lib.current_stream())
        return float(out[0]), float(out[1])

    def allow_bits(self, allow):
        """The device allow-bitmap (int32 ``[ceil(len / 32)]``, bit ``r & 31`` of word ``r >> 5``) of ``allow``: a device
        tensor, either ``torch.bool [len(self)]`` or that bitmap already packed."""
        n = len(self)
        _require_cuda(allow, "allow", self.device)
        words = (n + 31) // 32
        if allow.dtype == torch.bool:
            if allow.dim() != 1 or allow.shape[0] != n:
                raise ValueError(f"allow must be bool [{n}] (one entry per gallery row), got {tuple(allow.shape)}")
            m = torch.zeros(words * 32, dtype=torch.int64, device=allow.device)
            m[:n] = allow.to(torch.int64)
            w = (m.view(words, 32) << torch.arange(32, device=allow.device, dtype=torch.int64)).sum(1)
            return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
        if allow.dtype != torch.int32 or allow.dim() != 1 or allow.shape[0] != words:
            raise ValueError(f"allow must be bool [{n}] or a packed int32 bitmap [{words}], got {allow.dtype} "
                             f"{tuple(allow.shape)}")
        return allow.contiguous()

    @contextlib.contextmanager
    def _frame(self, allow=None, groups=None):
        """Inside: the lock is held and the device current (:meth:`_Handle._frame`); then the handle's searches see only
        the rows ``allow`` selects (revo_search_set_filter) and its grouped searches the group ids ``groups``
        (revo_search_set_groups).  Both are cleared again on the way out."""
        with super()._frame():
            try:
                if allow is not None:
                    bits = self.allow_bits(allow)
                    self._call("revo_search_set_filter", _lib.ptr(bits), len(self), 1, _lib.current_stream())
                if groups is not None:
                    n = len(self)
                    _require_cuda(groups, "groups", self.device)
                    if groups.dtype != torch.int32 or groups.dim() != 1 or groups.shape[0] != n:
                        raise ValueError(f"groups must be int32 [{n}] (one group id per gallery row, -1 = none), got "
                                         f"{groups.dtype} {tuple(groups.shape)}")
                    groups = groups.contiguous() if n else torch.full((1,), -1, dtype=torch.int32, device=self.device)   # (non-null)
                    self._call("revo_search_set_groups", _lib.ptr(groups), n, 1, _lib.current_stream())
                yield
            finally:
                if groups is not None:
                    self._lib.revo_search_set_groups(self._h, None, 0, 0, None)
                if allow is not None:
                    self._lib.revo_search_set_filter(self._h, None, 0, 0, None)

    def search(self, queries, k=5, score_threshold=None, index_offset=0, allow=None):
        """queries: fp32 [Q, dim] device tensor.  Returns (scores [Q,k] fp32,
        indices [Q,k] int64, counts [Q] int32), best first, padded with -inf/-1
        past ``counts`` (the reference's ``limit`` / ``score_threshold`` semantics,
        core_system.py:659-664).  ``allow`` (device tensor, bool [len] or a packed int32 bitmap): search only those
        rows -- exactly the result an unfiltered search of a gallery holding just the allowed rows would give.  k <= 1024
        (51 and up: include/revo.h, LARGE K)."""
        q = _rows(queries, "queries", self.dim, self.device, "Q")
        Q = q.shape[0]
        scores = torch.empty((Q, k), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=q.device)
        counts = torch.empty((Q,), dtype=torch.int32, device=q.device)
        # k <= 50: the certified scan; 51 <= k <= 1024: the large-k path (include/revo.h, LARGE K), same result contract
        fn = "revo_search_topk" if k <= 50 else "revo_search_topk_large"
        with self._frame(allow):
            self._call(fn, _lib.ptr(q), Q, int(k), *_threshold(score_threshold), int(index_offset),
                       _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts), _lib.current_stream())
        return scores, idx, counts

    def pairs(self, threshold, allow=None):
        """Near-duplicate pairs of the gallery (include/revo.h, PAIRS): every pair of rows ``i < j`` whose fp32 score
        reaches ``threshold``, both allowed by ``allow`` (as in :meth:`search`).  Returns ``(pairs [n, 2] int64, scores [n]
        fp32)`` device tensors ordered by ``(i, j)``, exactly what an exhaustive fp32 scoring of every pair would give.
        Synchronous (the kernels read the candidate count between their passes)."""
        n = C.c_int64()
        with self._frame(allow):
            self._call("revo_gallery_pairs", float(threshold), C.byref(n), _lib.current_stream())
            n = int(n.value)
            pairs = torch.empty((n, 2), dtype=torch.int64, device=self.device)
            scores = torch.empty((n,), dtype=torch.float32, device=self.device)
            self._call("revo_gallery_pairs_read", 0, n, _lib.ptr(pairs), _lib.ptr(scores), 1)
        return pairs, scores

    def clusters(self, threshold, allow=None):
        """Duplicate clusters of the gallery (include/revo.h, CLUSTERS): the connected components of the graph whose edges
        are the pairs of :meth:`pairs` at ``threshold``, computed on the device without storing those pairs, so a cluster's
        size sets no limit.  Returns ``(labels [len] int64, offsets [n_clusters + 1] int64, members [n_members] int64)``
        device tensors: ``labels[r]`` is the lowest row of r's component (-1: ``allow`` excludes r), cluster c (a component of
        at least two rows; clusters ordered by their lowest row) is ``members[offsets[c]:offsets[c + 1]]``, ascending.
        Synchronous."""
        nc, nm = C.c_int64(), C.c_int64()
        with self._frame(allow):
            self._call("revo_gallery_clusters", float(threshold), C.byref(nc), C.byref(nm), _lib.current_stream())
            labels = torch.empty((len(self),), dtype=torch.int64, device=self.device)
            offsets = torch.empty((int(nc.value) + 1,), dtype=torch.int64, device=self.device)
            members = torch.empty((int(nm.value),), dtype=torch.int64, device=self.device)
            self._call("revo_gallery_clusters_read", _lib.ptr(labels), _lib.ptr(offsets), _lib.ptr(members), 1)
        return labels, offsets, members

    def knn(self, k, score_threshold=None, allow=None):
        """Exact kNN graph of the gallery (include/revo.h, KNN): for every row ``allow`` selects (as in :meth:`search`) its
        best ``k <= 64`` other allowed rows by (score desc, index asc), cut at ``score_threshold`` if given.  Returns
        ``(scores [len, k] fp32, indices [len, k] int64, counts [len] int32)`` device tensors, padded with -inf / -1 past
        ``counts``; a row ``allow`` excludes has count 0 and is nobody's neighbour.  A score has the bits :meth:`pairs`
        gives the same two rows; a row is never its own neighbour, identical rows at other indices are.  Synchronous."""
        n = C.c_int64()
        with self._frame(allow):
            self._call("revo_gallery_knn", int(k), *_threshold(score_threshold), C.byref(n), _lib.current_stream())
            n = int(n.value)
            scores = torch.empty((n, int(k)), dtype=torch.float32, device=self.device)
            idx = torch.empty((n, int(k)), dtype=torch.int64, device=self.device)
            counts = torch.empty((n,), dtype=torch.int32, device=self.device)
            self._call("revo_gallery_knn_read", 0, n, _lib.ptr(idx), _lib.ptr(scores), _lib.ptr(counts), 1)
        return scores, idx, counts

    def kmeans(self, centroids, max_iter=10, normalize=True, allow=None):
        """Exact spherical k-means over the gallery (include/revo.h, KMEANS): the rows ``allow`` selects (as in
        :meth:`search`) are assigned to the best of the ``C`` centroids under the fp32 score (ties to the lowest centroid),
        the centroids are re-computed from their members in a fixed summation order, for at most ``max_iter`` updates
        (``max_iter=0``: a pure assignment).  ``centroids``: fp32 ``[C, dim]`` device tensor, normalised like appended rows
        unless ``normalize=False``.  Returns ``(centroids [C, dim] fp32, labels [len] int32, scores [len] fp32, sizes [C]
        int64, n_iter, converged)``, all tensors on the device; the labels are the exact assignment against the returned
        centroids, a row ``allow`` excludes has label -1 and score -inf.  Labels and scores are what
        ``search(self.read(), k=1)`` gives on a gallery of the returned centroids.  Synchronous."""
        c = _rows(centroids, "centroids", self.dim, self.device, "C", one_row=False)
        if c.shape[0] < 1:
            raise ValueError(f"centroids must be [C, {self.dim}] with C >= 1, got {tuple(c.shape)}")
        n_c = int(c.shape[0])
        n, it, conv = C.c_int64(), C.c_int32(), C.c_int32()
        with self._frame(allow):
            self._call("revo_gallery_kmeans", _lib.ptr(c), n_c, int(bool(normalize)), 1, int(max_iter), C.byref(it),
                       C.byref(conv), C.byref(n), _lib.current_stream())
            n = int(n.value)
            out = torch.empty((n_c, self.dim), dtype=torch.float32, device=self.device)
            sizes = torch.empty((n_c,), dtype=torch.int64, device=self.device)
            labels = torch.empty((n,), dtype=torch.int32, device=self.device)
            scores = torch.empty((n,), dtype=torch.float32, device=self.device)
            self._call("revo_gallery_kmeans_centroids", _lib.ptr(out), _lib.ptr(sizes), 1)
            self._call("revo_gallery_kmeans_read", 0, n, _lib.ptr(labels), _lib.ptr(scores), 1)
        return out, labels, scores, sizes, int(it.value), bool(conv.value)

    def search_range(self, queries, score_threshold, index_offset=0, allow=None):
        """Range search (include/revo.h, RANGE): for each query every row (allowed by ``allow``, as in :meth:`search`) whose
        fp32 score reaches ``score_threshold`` -- the reference's threshold without its ``limit``.  Returns ``(offsets [Q + 1]
        int64, indices [n] int64, scores [n] fp32)`` device tensors: query q's results are ``offsets[q] .. offsets[q + 1]``,
        best first (score desc, index asc), with the bits :meth:`search` returns.  Synchronous."""
        q = _rows(queries, "queries", self.dim, self.device, "Q")
        Q = q.shape[0]
        n = C.c_int64()
        offsets = torch.empty((Q + 1,), dtype=torch.int64, device=self.device)
        with self._frame(allow):
            self._call("revo_search_range", _lib.ptr(q), Q, float(score_threshold), int(index_offset), C.byref(n),
                       _lib.current_stream())
            n = int(n.value)
            idx = torch.empty((n,), dtype=torch.int64, device=self.device)
            scores = torch.empty((n,), dtype=torch.float32, device=self.device)
            self._call("revo_search_range_read", _lib.ptr(offsets), 0, n, _lib.ptr(idx), _lib.ptr(scores), 1)
        return offsets, idx, scores

    def recommend(self, positive, negative=None, k=5, score_threshold=None, index_offset=0, allow=None):
        """Search by examples (include/revo.h, RECOMMEND): ``positive`` fp32 ``[P, dim]`` and ``negative`` fp32 ``[N, dim]``
        (or None) device tensors, ``P >= 1``, ``P + N <= 128``.  A row's score is its best score ``sp`` against a positive if
        that exceeds its best score ``sn`` against a negative, else ``-(sn * sn)``; returns the best ``k <= 1024`` rows
        (allowed by ``allow``, as in :meth:`search`) as ``(scores [k] fp32, indices [k] int64, count)`` device tensors
        (``count`` a 0-d int32), best first, padded with -inf / -1 -- exactly what scoring every row that way in fp32 and
        sorting gives.  Synchronous."""
        pos = _rows(positive, "positive", self.dim, self.device)
        neg = _rows(negative, "negative", self.dim, self.device) if negative is not None and negative.numel() > 0 else None
        ex = pos if neg is None else torch.cat([pos, neg]).contiguous()
        k = int(k)
        scores = torch.empty((max(k, 1),), dtype=torch.float32, device=self.device)
        idx = torch.empty((max(k, 1),), dtype=torch.int64, device=self.device)
        counts = torch.empty((1,), dtype=torch.int32, device=self.device)
        with self._frame(allow):
            self._call("revo_search_recommend", _lib.ptr(ex), pos.shape[0], 0 if neg is None else neg.shape[0], k,
                       *_threshold(score_threshold), int(index_offset), _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts),
                       _lib.current_stream())
        return scores, idx, counts[0]

    def discover(self, target, positives, negatives, k=5, score_threshold=None, index_offset=0, allow=None):
        """Discovery / context search (include/revo.h, DISCOVER): ``positives`` and ``negatives`` fp32 ``[n, dim]`` device
        tensors, pair ``i`` being ``(positives[i], negatives[i])`` (both None or empty: no pairs), and ``target`` an fp32
        ``[dim]`` device tensor or None.  With a target (``n <= 63``) a row's score is ``R + sig``: ``R`` counts +1 for every
        pair whose positive it scores higher against than its negative and -1 otherwise, ``0 < sig < 1`` grows with its
        score against the target.  Without one (context search, ``1 <= n <= 64``) the score is the sum over the pairs of
        ``fs(min(sp - sn - FLT_EPSILON, 0))``, ``fs(x) = x / (1 + |x|)``: 0 for a row on the positive side of every pair.
        Returns the best ``k <= 1024`` rows (allowed by ``allow``, as in :meth:`search`) as ``(scores [k] fp32, indices [k]
        int64, count)`` device tensors, best first, padded with -inf / -1 -- exactly what scoring every row that way in
        fp32 and sorting gives.  Synchronous."""
        pos = _rows(positives, "positives", self.dim, self.device) if positives is not None and positives.numel() > 0 else None
        neg = _rows(negatives, "negatives", self.dim, self.device) if negatives is not None and negatives.numel() > 0 else None
        n = 0 if pos is None else pos.shape[0]
        if n != (0 if neg is None else neg.shape[0]):
            raise ValueError("discover: positives and negatives must hold the same number of rows (one of each per pair)")
        tgt = None
        if target is not None:
            tgt = _rows(target, "target", self.dim, self.device)
            if tgt.shape[0] != 1:
                raise ValueError(f"target must be one vector of {self.dim} elements, got {tuple(target.shape)}")
        k = int(k)
        scores = torch.empty((max(k, 1),), dtype=torch.float32, device=self.device)
        idx = torch.empty((max(k, 1),), dtype=torch.int64, device=self.device)
        counts = torch.empty((1,), dtype=torch.int32, device=self.device)
        with self._frame(allow):
            self._call("revo_search_discover", _lib.ptr(tgt), _lib.ptr(pos), _lib.ptr(neg), n, k, *_threshold(score_threshold),
                       int(index_offset), _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts), _lib.current_stream())
        return scores, idx, counts[0]

    def search_boosted(self, query, mult=None, bias=None, k=5, score_threshold=None, min_similarity=None, index_offset=0,
                       allow=None):
        """Boosted search (include/revo.h, BOOSTED): ``query`` one fp32 ``[dim]`` device vector; ``mult`` and ``bias`` fp32
        ``[len]`` device tensors, one entry per gallery row, or None (1 / 0).  A row's final score is
        ``fma(mult[r], s(r), bias[r])``, one correctly rounded operation, with ``s`` the similarity :meth:`search` returns.
        Returns the best ``k <= 1024`` rows (allowed by ``allow``, as in :meth:`search`) with ``s >= min_similarity`` and
        ``final >= score_threshold`` where given, as ``(scores [k] fp32, similarities [k] fp32, indices [k] int64, count)``
        device tensors (``count`` a 0-d int32), best final score first, padded with -inf / -inf / -1 -- exactly what computing
        the final score of every row and sorting gives.  On every allowed row ``mult`` must be finite and >= 0 and ``bias``
        finite: the call raises otherwise.  Synchronous."""
        q = _rows(query, "query", self.dim, self.device)
        if q.shape[0] != 1:
            raise ValueError(f"query must be one vector of {self.dim} elements, got {tuple(query.shape)}")
        n = len(self)

        def per_row(t, name):
            if t is None:
                return None
            _require_cuda(t, name, self.device)
            if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n:
                raise ValueError(f"{name} must be fp32 [{n}] (one entry per gallery row), got {t.dtype} {tuple(t.shape)}")
            return t.contiguous() if n else None
        m, b = per_row(mult, "mult"), per_row(bias, "bias")
        k = int(k)
        scores = torch.empty((max(k, 1),), dtype=torch.float32, device=self.device)
        sims = torch.empty((max(k, 1),), dtype=torch.float32, device=self.device)
        idx = torch.empty((max(k, 1),), dtype=torch.int64, device=self.device)
        counts = torch.empty((1,), dtype=torch.int32, device=self.device)
        with self._frame(allow):
            self._call("revo_search_boosted", _lib.ptr(q), _lib.ptr(m), _lib.ptr(b), k, *_threshold(score_threshold),
                       *_threshold(min_similarity), int(index_offset), _lib.ptr(scores), _lib.ptr(sims), _lib.ptr(idx),
                       _lib.ptr(counts), _lib.current_stream())
        return scores, sims, idx, counts[0]

    def search_maxsim(self, queries, groups, k=5, score_threshold=None, index_offset=0, allow=None, with_parts=False):
        """Multi-vector search (include/revo.h, MAXSIM): ``queries`` fp32 ``[n, dim]`` device tensor, ``1 <= n <= 64``;
        ``groups`` int32 ``[len]`` device tensor, the group of every row (-1 = none), as in :meth:`search_groups`.  A
        group's score is the sum over the query vectors (in order, fp32) of its best score against the group's rows that
        ``allow`` selects.  Returns the best ``k <= 1024`` groups as ``(scores [k] fp32, group_ids [k] int32, count)``
        device tensors (``count`` a 0-d int32), best first (score desc, group id asc), padded with -inf / -1 -- exactly
        what scoring every group that way in fp32 and sorting gives.  ``with_parts``: also ``part_scores [k, n]`` fp32 (the
        best score per query vector) and ``part_rows [k, n]`` int64 (``index_offset`` + the lowest row attaining it),
        padded with -inf / -1.  Synchronous."""
        q = _rows(queries, "queries", self.dim, self.device)
        n, k = q.shape[0], int(k)
        scores = torch.empty((max(k, 1),), dtype=torch.float32, device=self.device)
        gids = torch.empty((max(k, 1),), dtype=torch.int32, device=self.device)
        counts = torch.empty((1,), dtype=torch.int32, device=self.device)
        ps = torch.empty((max(k, 1), max(n, 1)), dtype=torch.float32, device=self.device) if with_parts else None
        pr = torch.empty((max(k, 1), max(n, 1)), dtype=torch.int64, device=self.device) if with_parts else None
        with self._frame(allow, groups):
            self._call("revo_search_maxsim", _lib.ptr(q), n, k, *_threshold(score_threshold), int(index_offset), _lib.ptr(scores),
                       _lib.ptr(gids), _lib.ptr(counts), _lib.ptr(ps), _lib.ptr(pr), _lib.current_stream())
        return (scores, gids, counts[0], ps, pr) if with_parts else (scores, gids, counts[0])

    def search_mmr(self, queries, k=5, candidates=None, diversity=0.5, score_threshold=None, index_offset=0, allow=None):
        """Diverse search (include/revo.h, MMR): for each query the best ``candidates`` rows of :meth:`search` (default
        ``min(1024, max(k, 100))``; same filter and threshold semantics), of which ``k`` are picked greedily by maximal
        marginal relevance: each pick maximises ``(1 - diversity) * score - diversity * (largest score against a row already
        picked)``.  ``diversity = 0`` is the plain top-k, ``1`` ignores relevance after the first pick.  Returns ``(scores
        [Q, k] fp32, mmr_values [Q, k] fp32, indices [Q, k] int64, counts [Q] int32)`` device tensors in pick order
        (``scores``: the rows' plain search scores; ``mmr_values``: the value each row was picked with), padded with
        -inf / -inf / -1.  Exact: the candidates are those of the exhaustive fp32 search, every similarity has the bits
        :meth:`pairs` reports, the selection is the fp32 arithmetic the header states.  Asynchronous like :meth:`search`."""
        q = _rows(queries, "queries", self.dim, self.device, "Q")
        k = int(k)
        candidates = min(1024, max(k, 100)) if candidates is None else int(candidates)
        Q = q.shape[0]
        scores = torch.empty((Q, max(k, 1)), dtype=torch.float32, device=q.device)
        values = torch.empty((Q, max(k, 1)), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, max(k, 1)), dtype=torch.int64, device=q.device)
        counts = torch.empty((Q,), dtype=torch.int32, device=q.device)
        with self._frame(allow):
            self._call("revo_search_mmr", _lib.ptr(q), Q, k, candidates, float(diversity), *_threshold(score_threshold),
                       int(index_offset), _lib.ptr(scores), _lib.ptr(values), _lib.ptr(idx), _lib.ptr(counts), _lib.current_stream())
        return scores, values, idx, counts

    def search_fusion(self, queries, k=5, limit=100, method="rrf", rrf_k=60.0, weights=None, list_thresholds=None,
                      score_threshold=None, index_offset=0, allow=None, with_ranks=True, with_list_scores=False):
        """Hybrid query (include/revo.h, FUSION): ``queries`` is ``[n, m, dim]`` (or ``[m, dim]`` for one fused search) --
        m query vectors of possibly different kinds, e.g. an image embedding and a text embedding.  Each is searched for its
        best ``limit`` rows as :meth:`search` would (same filter semantics); the m lists are fused by ``method``: ``"rrf"``
        (each member adds ``weight / (rrf_k + rank)``) or ``"dbsf"`` (each member adds ``weight * (score - (mean - 3 sd)) /
        (6 sd)`` with the list's own mean and deviation).  ``list_thresholds[j]`` drops list j's entries below it without
        renumbering the ranks behind them; ``score_threshold`` cuts on the fused score.  Returns ``(scores [n, k] fp32,
        indices [n, k] int64, counts [n] int32)``, then ``ranks [n, k, m] int32`` (1-based position in list j, 0 = not in
        it) if ``with_ranks`` and ``list_scores [n, k, m] fp32`` (the row's exact score against every one of the m queries,
        member or not) if ``with_list_scores``; padding -inf / -1 / 0 / -inf.  Exact and asynchronous like :meth:`search`."""
        q = _f32(queries, "queries", self.device)
        if q.dim() == 2:
            q = q[None]
        if q.dim() != 3 or q.shape[2] != self.dim:
            raise ValueError(f"queries must be [n, m, {self.dim}], got {tuple(q.shape)}")
        n, m = int(q.shape[0]), int(q.shape[1])
        k = int(k)
        w, t = _fusion_host_arrays(m, weights, list_thresholds)
        scores = torch.empty((n, max(k, 1)), dtype=torch.float32, device=q.device)
        idx = torch.empty((n, max(k, 1)), dtype=torch.int64, device=q.device)
        counts = torch.empty((n,), dtype=torch.int32, device=q.device)
        ranks = torch.empty((n, max(k, 1), m), dtype=torch.int32, device=q.device) if with_ranks else None
        ls = torch.empty((n, max(k, 1), m), dtype=torch.float32, device=q.device) if with_list_scores else None
        with self._frame(allow):
            self._call("revo_search_fusion", _lib.ptr(q), n, m, int(limit), _fusion_method(method), float(rrf_k), w, t, k,
                       *_threshold(score_threshold), int(index_offset), _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts),
                       _lib.ptr(ranks), _lib.ptr(ls), _lib.current_stream())
        return (scores, idx, counts) + ((ranks,) if with_ranks else ()) + ((ls,) if with_list_scores else ())

    def search_groups(self, queries, groups, limit=5, group_size=1, score_threshold=None, index_offset=0, allow=None):
        """The best ``limit`` groups of rows for each query (Qdrant's ``search_groups``; include/revo.h, GROUPED).
        ``groups``: int32 ``[len]`` device tensor, the group of every row (-1 = none: never returned).  A group ranks by
        its best row; each carries its best ``group_size`` rows (``limit * group_size <= 50``).  Exactly the grouping of an
        exhaustive fp32 scoring of the rows ``allow`` selects (see :meth:`search`).  Returns (scores ``[Q, limit,
        group_size]`` fp32, indices (same, int64), hit_counts ``[Q, limit]`` int32, group_ids ``[Q, limit]`` int32,
        group_counts ``[Q]`` int32), padded with -inf / -1 / 0 / -1."""
        q = _rows(queries, "queries", self.dim, self.device, "Q")
        Q, L, S = q.shape[0], int(limit), int(group_size)
        scores = torch.empty((Q, L, S), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, L, S), dtype=torch.int64, device=q.device)
        hits = torch.empty((Q, L), dtype=torch.int32, device=q.device)
        gids = torch.empty((Q, L), dtype=torch.int32, device=q.device)
        ngroups = torch.empty((Q,), dtype=torch.int32, device=q.device)
        with self._frame(allow, groups):
            self._call("revo_search_groups", _lib.ptr(q), Q, L, S, *_threshold(score_threshold), int(index_offset),
                       _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(hits), _lib.ptr(gids), _lib.ptr(ngroups), _lib.current_stream())
        return scores, idx, hits, gids, ngroups

    # -- the exactness certificate (include/revo.h, "EXACTNESS") ------------------------------------------
    MODES = {"certified": 0, "collect": 1, "bruteforce": 2, "uncertified": 3}

    def set_search_mode(self, mode="certified"):
        """``certified`` (default): every query's result is certified exact or re-done exactly; ``collect`` /
        ``bruteforce``: every query takes that fallback (parity tests; ``bruteforce`` also sends every query of a grouped
        search through the grouped fallback); ``uncertified``: certificate counted only."""
        if not self.experiments:
            raise _lib.RevoError("set_search_mode is a parity-test hook of librevo_exp.so: create the gallery with "
                                 "experiments=True (the product library's searches are always certified exact)")
        self._call("revo_search_set_mode", self.MODES[mode] if isinstance(mode, str) else int(mode))

    def search_stats(self):
        """Counters of the last search on this handle (synchronises the current stream)."""
        out = (C.c_int32 * 8)()
        with torch.cuda.device(self.device):
            self._call("revo_search_stats", out, _lib.current_stream())
        return {"uncertified": int(out[0]), "bruteforced": int(out[1]), "checked": int(out[2]), "collected_rows": int(out[3]),
                "from_segments": int(out[4]), "grouped_fallback": int(out[5]), "large_k_fallback": int(out[6]),
                "join_passes": int(out[7])}

    def set_total_rows(self, total_rows):
        """This handle holds ONE SHARD of a row-sharded gallery of ``total_rows`` rows (0: forget): its two-phase scans
        start from an estimate of the whole gallery's admission level (include/revo.h, revo_search_set_total_rows)."""
        self._call("revo_search_set_total_rows", int(total_rows))
        self._total_rows = int(total_rows)

    def search_plan(self, n_queries, k=5):
        """How a search would run (reporting): dict with the scan form, the pre-pass rows, slices and ksel."""
        out = (C.c_int64 * 4)()
        self._call("revo_search_plan", int(n_queries), int(k), out)
        return {"scan256": bool(out[0]), "prepass_rows": int(out[1]), "slices": int(out[2]), "ksel": int(out[3])}

    # -- the same search in two phases (row-sharded gallery; see sharded.py and include/revo.h) --------------
    def search_candidates(self, queries, k=5, top_m=8, allow=None):
        """Phase 1: scan this shard, keep the candidates in the handle.  Returns int32 ``[Q, top_m]``: the bit
        patterns of the order-preserving uint32 scan scores of each query's best ``top_m`` candidates."""
        q = _rows(queries, "queries", self.dim, self.device, "Q")
        bounds = torch.empty((q.shape[0], int(top_m)), dtype=torch.int32, device=q.device)
        with self._frame(allow):
            self._call("revo_search_candidates", _lib.ptr(q), q.shape[0], int(k), int(top_m), _lib.ptr(bounds), _lib.current_stream())
        return bounds

    def search_finish(self, n_queries, k, all_bounds=None, score_threshold=None, index_offset=0, out_packed=None, allow=None):
        """Phase 2: fp32 re-score of the candidates that can still be among the best of the whole gallery
        (``all_bounds``: int32 ``[parts, Q, top_m]``, the all-gathered phase-1 outputs; None = every candidate).
        Returns (scores, indices, counts); with ``out_packed`` (uint8 ``[packed_bytes(Q, k)]``) scores and indices
        are views into that buffer, laid out for :func:`merge_topk_packed`."""
        Q, k = int(n_queries), int(k)
        cert = None
        # (after a scan that dropped rows against an ESTIMATED level -- set_total_rows on a shard large enough to estimate --
        #  only the packed block's certificate makes the result exhaustive: revo_search_finish itself refuses
        #  cert = NULL then, status -2, and says so; a shard that never estimated is served either way)
        if out_packed is not None:
            idx = out_packed[: Q * k * 8].view(torch.int64).view(Q, k)
            scores = out_packed[Q * k * 8: Q * k * 12].view(torch.float32).view(Q, k)
            cert = out_packed[Q * k * 12: Q * k * 12 + Q * 4].view(torch.float32)     # this shard's certificate bounds
        else:
            scores = torch.empty((Q, k), dtype=torch.float32, device=self.device)
            idx = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        counts = torch.empty((Q,), dtype=torch.int32, device=self.device)
        parts = top_m = 0
        if all_bounds is not None:
            _require_cuda(all_bounds, "all_bounds", self.device)
            all_bounds = all_bounds.contiguous()
            parts, top_m = int(all_bounds.shape[0]), int(all_bounds.shape[2])
            if all_bounds.dtype != torch.int32 or all_bounds.shape[1] != Q:
                raise ValueError("all_bounds must be int32 [parts, Q, top_m]")
        with self._frame(allow):
            self._call("revo_search_finish", Q, k, *_threshold(score_threshold), int(index_offset), _lib.ptr(all_bounds), parts,
                       top_m, _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts), _lib.ptr(cert), _lib.current_stream())
        return scores, idx, counts

    def search_exact(self, q_idx, need, k, index_offset=0, out_packed=None, allow=None):
        """Second round of a row-sharded search: exact local top-k of the queries ``q_idx`` (int32 ``[n]``, rows of the
        last :meth:`search_candidates` call) given ``need`` (fp32 ``[n]``: the score a row must reach to change the
        merged result).  Results in compact rows ``[n, k]``; with ``out_packed`` laid out for :func:`merge_topk_packed`."""
        n, k = int(q_idx.shape[0]), int(k)
        _require_cuda(q_idx, "q_idx", self.device)
        _require_cuda(need, "need", self.device)
        assert q_idx.dtype == torch.int32 and need.dtype == torch.float32 and need.shape[0] == n
        if out_packed is not None:
            idx = out_packed[: n * k * 8].view(torch.int64).view(n, k)
            scores = out_packed[n * k * 8: n * k * 12].view(torch.float32).view(n, k)
            out_packed[n * k * 12: n * k * 12 + n * 4].view(torch.float32).fill_(float("-inf"))   # exact: nothing left to certify
        else:
            scores = torch.empty((n, k), dtype=torch.float32, device=self.device)
            idx = torch.empty((n, k), dtype=torch.int64, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        with self._frame(allow):
            self._call("revo_search_exact", n, _lib.ptr(q_idx.contiguous()), _lib.ptr(need.contiguous()), k, 0, 0.0,
                       int(index_offset), _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts), _lib.current_stream())
        return scores, idx, counts


def search_estimates(k):
    """True if shards that know the whole gallery's row count scan a best-k search against its estimated admission level."""
    return int(_lib.load().revo_search_estimates(int(k))) == 1


def search_ksel(k):
    """Candidates the scan keeps per query for a top-k search (32 or 64)."""
    return int(_lib.load().revo_search_ksel(int(k)))


def packed_bytes(n_queries, k):
    """Size of one packed result block ([Q, k] int64 indices, [Q, k] fp32 scores, [Q] fp32 certificate bounds,
    padded to 16 bytes)."""
    return int(_lib.load().revo_topk_packed_bytes(int(n_queries), int(k)))


def merge_topk_packed(packed, parts, n_queries, k, score_threshold=None, certify=False):
    """Merge ``parts`` packed result blocks (uint8, back to back: one all-gather) into [Q, k]; K14.
    ``certify``: also check every query's exactness certificate over all shards; returns a fourth item
    ``(unc_count int32 [1], unc_q int32 [Q], unc_need fp32 [Q])`` (device; the first ``unc_count`` entries are valid)."""
    _require_cuda(packed, "packed")
    Q, k = int(n_queries), int(k)
    assert packed.dtype == torch.uint8 and packed.numel() == parts * packed_bytes(Q, k)
    scores = torch.empty((Q, k), dtype=torch.float32, device=packed.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=packed.device)
    counts = torch.empty((Q,), dtype=torch.int32, device=packed.device)
    unc = None
    if certify:
        unc = (torch.zeros((1,), dtype=torch.int32, device=packed.device),
               torch.empty((max(Q, 1),), dtype=torch.int32, device=packed.device),
               torch.empty((max(Q, 1),), dtype=torch.float32, device=packed.device))
    lib = _lib.load()
    with torch.cuda.device(packed.device):
        _lib.check(lib.revo_topk_merge_packed(_lib.ptr(packed), int(parts), Q, k, *_threshold(score_threshold),
                                              _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts),
                                              _lib.ptr(unc[0]) if unc else None, _lib.ptr(unc[1]) if unc else None,
                                              _lib.ptr(unc[2]) if unc else None, _lib.current_stream()),
                   "revo_topk_merge_packed")
    return (scores, idx, counts, unc) if certify else (scores, idx, counts)


def merge_topk(part_scores, part_indices, k, score_threshold=None):
    """Merge per-shard results [P,Q,k] (device) into [Q,k]; K14."""
    _require_cuda(part_scores, "part_scores")
    P, Q, kk = part_scores.shape
    assert kk == k
    ps = part_scores.contiguous()
    pi = part_indices.contiguous()
    scores = torch.empty((Q, k), dtype=torch.float32, device=ps.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=ps.device)
    counts = torch.empty((Q,), dtype=torch.int32, device=ps.device)
    lib = _lib.load()
    with torch.cuda.device(ps.device):
        _lib.check(lib.revo_topk_merge(_lib.ptr(ps), _lib.ptr(pi), P, Q, k, *_threshold(score_threshold),
                                       _lib.ptr(scores), _lib.ptr(idx), _lib.ptr(counts), _lib.current_stream()),
                   "revo_topk_merge")
    return scores, idx, counts


FUSION_METHODS = {"rrf": 0, "dbsf": 1}


def _fusion_method(method):
    if method not in FUSION_METHODS:
        raise ValueError(f"fusion method must be one of {sorted(FUSION_METHODS)}, got {method!r}")
    return FUSION_METHODS[method]


def _fusion_host_arrays(m, weights, list_thresholds):
    """The host float[m] arrays of revo_search_fusion / revo_topk_fuse (None stays NULL; a threshold of None: -inf)."""
    def arr(values, name, none_value):
        if values is None:
            return None
        values = [none_value if v is None else float(v) for v in values]
        if len(values) != m:
            raise ValueError(f"{name} must have one entry per list ({m}), got {len(values)}")
        return (C.c_float * m)(*values)
    return arr(weights, "weights", 1.0), arr(list_thresholds, "list_thresholds", float("-inf"))


def fuse_topk(scores, indices, counts, k=5, method="rrf", rrf_k=60.0, weights=None, list_thresholds=None, score_threshold=None,
              with_ranks=True):
    """Fuse result lists the caller already holds (include/revo.h, FUSION: revo_topk_fuse): ``scores`` fp32 and ``indices``
    int64 ``[n, m, C]``, ``counts`` int32 ``[n, m]``, device tensors -- e.g. the merged lists of a row-sharded search.  The
    arithmetic, order and outputs of :meth:`Gallery.search_fusion`: returns ``(scores [n, k], indices [n, k], counts [n])``
    and ``ranks [n, k, m]`` if ``with_ranks``."""
    s = _f32(scores, "scores")
    _require_cuda(indices, "indices", scores.device)
    _require_cuda(counts, "counts", scores.device)
    i = indices.detach().to(torch.int64).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    if s.dim() != 3 or i.shape != s.shape or tuple(c.shape) != tuple(s.shape[:2]):
        raise ValueError(f"scores and indices must be [n, m, C] and counts [n, m], got {tuple(s.shape)}, {tuple(i.shape)}, "
                         f"{tuple(c.shape)}")
    n, m, limit = (int(x) for x in s.shape)
    k = int(k)
    w, t = _fusion_host_arrays(m, weights, list_thresholds)
    out_s = torch.empty((n, max(k, 1)), dtype=torch.float32, device=s.device)
    out_i = torch.empty((n, max(k, 1)), dtype=torch.int64, device=s.device)
    out_c = torch.empty((n,), dtype=torch.int32, device=s.device)
    ranks = torch.empty((n, max(k, 1), m), dtype=torch.int32, device=s.device) if with_ranks else None
    lib = _lib.load()
    with torch.cuda.device(s.device):
        _lib.check(lib.revo_topk_fuse(_lib.ptr(s), _lib.ptr(i), _lib.ptr(c), n, m, limit, _fusion_method(method), float(rrf_k),
                                      w, t, k, *_threshold(score_threshold), _lib.ptr(out_s),
                                      _lib.ptr(out_i), _lib.ptr(out_c), _lib.ptr(ranks), _lib.current_stream()),
                   "revo_topk_fuse")
    return (out_s, out_i, out_c, ranks) if with_ranks else (out_s, out_i, out_c)


# ---- module-level convenience API named by the north star ------------------
_default_engine = None
_default_gallery = None


def set_default(engine=None, gallery=None):
    global _default_engine, _default_gallery
    if engine is not None:
        _default_engine = engine
    if gallery is not None:
        _default_gallery = gallery


def embed(images, engine=None):
    """images: uint8 / float32 ``[B,3,H,W]`` device tensor at the model resolution, or a list of PIL images / arrays /
    paths (squash-resized on the host like ``self.preprocess`` at core_system.py:439, uploaded as uint8).
    Returns fp32 ``[B, D]`` on the device, L2-normalised."""
    eng = engine or _default_engine
    if eng is None:
        raise _lib.RevoError("embed(): no engine; create a VitEngine and call set_default(engine=...)")
    if isinstance(images, (list, tuple)):
        from . import preprocess as pp
        images = pp.batch_u8(list(images), eng.cfg.image_size, pin=True).to(eng.device, non_blocking=True)
    return eng.embed(images)


def search(queries, k=5, score_threshold=None, gallery=None, allow=None):
    gal = gallery or _default_gallery
    if gal is None:
        raise _lib.RevoError("search(): no gallery; create a Gallery and call set_default(gallery=...)")
    return gal.search(queries, k=k, score_threshold=score_threshold, allow=allow)


# ---- profiler ---------------------------------------------------------------
def prof_enable(on=True):
    """on: False/0 off, True/1 every kernel class, 2 only the body GEMMs, 3 every fourth launch of each
    body-GEMM class (cheap enough for a timed region)."""
    _lib.load().revo_prof_enable(int(on))


def prof_reset():
    _lib.load().revo_prof_reset()


def prof_report():
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.load().revo_prof_report(buf, len(buf)), "revo_prof_report")
    return json.loads(buf.value.decode())
