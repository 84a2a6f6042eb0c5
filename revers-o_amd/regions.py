"""Token bitmaps of image regions for ``VitEngine.embed_regions`` (masked attention pooling).

A region -- a pixel mask or a box in the SOURCE image -- becomes the set of ViT tokens whose patch it covers, as the
bitmap ``revo_vit_forward_regions`` reads: ``uint32 [ceil(S / 32)]``, token ``s`` allowed iff bit ``s & 31`` of word
``s >> 5`` is set (the layout of the search filters, :func:`reverso_amd.filters.pack_bits`).  Everything here is host
arithmetic on integers and float64: the same region gives the same bitmap on every machine.

The rule.  The embed path squash-resizes the source image to the model's square (``preprocess.resize_u8``), a linear map
per axis, so source pixel ``(px, py)`` of a ``width x height`` image belongs to the cell ``(px * g // width, py * g //
height)`` of the ``g x g`` patch grid.  ``cell_pixels`` is the number of source pixels of a cell, ``count`` how many of them
the region holds.  A cell's token is allowed iff ``count > 0`` and ``count >= min_cover * cell_pixels``; if no cell
qualifies, the one cell with the largest ``count / cell_pixels`` is allowed (ties: the lowest token), so a non-empty region
never gives an empty bitmap.  A region without a pixel raises ``ValueError``.  Token index: ``use_cls + gy * g + gx``
(token 0 is the class token on towers that have one; ``include_cls`` adds it to every region).

A box ``(x0, y0, x1, y1)`` stands for its rectangle: the pixels whose centre ``(px + 0.5, py + 0.5)`` lies in
``[x0, x1) x [y0, y1)``, clipped to the image.

Under a rectangular token grid (``grid=(gh, gw)``: native-aspect embedding) the same rule holds with
``gw`` columns and ``gh`` rows: the cell is ``(px * gw // width, py * gh // height)``, the token ``use_cls + gy * gw + gx``,
``S = gh * gw + use_cls``.  ``grid=None`` is the tower's native ``g x g``."""
import math

import numpy as np

__all__ = ["token_masks", "full_mask", "words_per_region", "cell_masks", "cell_boxes"]


def _grid(cfg, grid):
    """grid=None | (gh, gw) -> (gh, gw, S)"""
    if grid is None:
        gh = gw = int(cfg.grid)
    else:
        gh, gw = (int(v) for v in grid)
        if gh < 1 or gw < 1:
            raise ValueError(f"grid must be (gh, gw) with positive sides, got {grid!r}")
    return gh, gw, gh * gw + (1 if cfg.use_cls else 0)


def words_per_region(cfg, grid=None):
    return (_grid(cfg, grid)[2] + 31) // 32


def full_mask(cfg, include_cls=True, grid=None):
    """``uint32 [ceil(S / 32)]`` allowing every patch token, and the class token with ``include_cls`` (then the region's
    vector is the image's global vector, bit for bit)."""
    allow = np.ones(_grid(cfg, grid)[2], dtype=bool)
    if cfg.use_cls and not include_cls:
        allow[0] = False
    return _pack(allow[None])[0]


def _pack(allow):
    """bool [R, S] -> uint32 [R, ceil(S / 32)], bit s & 31 of word s >> 5"""
    R, S = allow.shape
    words = (S + 31) // 32
    padded = np.zeros((R, words * 32), dtype=np.uint64)
    padded[:, :S] = allow
    shifts = np.arange(32, dtype=np.uint64)
    return (padded.reshape(R, words, 32) << shifts).sum(axis=2).astype(np.uint32)


def _axis_cells(n, g):
    """cell of every pixel along an axis of n pixels, and the pixels per cell"""
    cell = (np.arange(n, dtype=np.int64) * g) // n
    return cell, np.bincount(cell, minlength=g).astype(np.int64)


def _box_range(lo, hi, n):
    """pixels p of [0, n) whose centre p + 0.5 lies in [lo, hi)"""
    a = max(0, int(math.ceil(float(lo) - 0.5)))
    b = min(n, int(math.ceil(float(hi) - 0.5)))
    return a, max(a, b)


def _is_box(region):
    a = np.asarray(region)
    return a.ndim == 1 and a.shape[0] == 4


def token_masks(cfg, regions, width, height, min_cover=0.5, include_cls=False, grid=None):
    """regions: a sequence of boolean pixel masks ``[height, width]`` and / or boxes ``(x0, y0, x1, y1)`` in source pixels
    of a ``width x height`` image.  Returns ``uint32 [R, ceil(S / 32)]`` for the tower ``cfg`` (module docstring)."""
    width, height = int(width), int(height)
    gh, gw, seq = _grid(cfg, grid)
    if width <= 0 or height <= 0:
        raise ValueError("token_masks: width and height must be positive")
    if not 0.0 <= float(min_cover) <= 1.0:
        raise ValueError("token_masks: min_cover must be in [0, 1]")
    first = 1 if cfg.use_cls else 0
    cx, nx = _axis_cells(width, gw)
    cy, ny = _axis_cells(height, gh)
    cell_pixels = np.outer(ny, nx)                                    # [gy, gx]
    contiguous = bool((nx > 0).all() and (ny > 0).all())
    x_start, y_start = np.cumsum(nx) - nx, np.cumsum(ny) - ny       # first pixel of every cell
    allow = np.zeros((len(regions), seq), dtype=bool)
    for r, region in enumerate(regions):
        if _is_box(region):
            x0, y0, x1, y1 = (float(v) for v in np.asarray(region, dtype=np.float64))
            xa, xb = _box_range(x0, x1, width)
            ya, yb = _box_range(y0, y1, height)
            count = np.outer(np.bincount(cy[ya:yb], minlength=gh), np.bincount(cx[xa:xb], minlength=gw)).astype(np.int64)
        else:
            m = np.asarray(region)
            if m.shape != (height, width):
                raise ValueError(f"token_masks: region {r} must be a mask [{height}, {width}] or a box of 4 numbers, got "
                                 f"shape {m.shape}")
            m = m.astype(bool)
            if contiguous:      # every cell holds pixels: the cells are runs of rows / columns, summed run by run
                count = np.add.reduceat(np.add.reduceat(m.view(np.uint8), x_start, axis=1, dtype=np.int32), y_start,
                                        axis=0).astype(np.int64)
            else:               # fewer pixels than cells along an axis: some cells are empty
                count = np.bincount((cy[:, None] * gw + cx[None, :])[m], minlength=gh * gw).astype(np.int64).reshape(gh, gw)
        if count.sum() == 0:
            raise ValueError(f"token_masks: region {r} holds no pixel of the image")
        ok = (count > 0) & (count.astype(np.float64) >= float(min_cover) * cell_pixels.astype(np.float64))
        if not ok.any():
            ratio = np.where(cell_pixels > 0, count.astype(np.float64) / np.maximum(cell_pixels, 1).astype(np.float64), 0.0)
            ok = np.zeros_like(ok)
            ok.reshape(-1)[int(np.argmax(ratio.reshape(-1)))] = True     # argmax: the first, i.e. lowest, token of a tie
        allow[r, first:] = ok.reshape(-1)
        if include_cls and cfg.use_cls:
            allow[r, 0] = True
    return _pack(allow)


def _unpack_cells(cfg, bits, grid=None):
    """uint32 [R, ceil(S / 32)] -> bool [R, gh, gw]: the patch-token bits (the class token's bit is dropped)"""
    gh, gw, _ = _grid(cfg, grid)
    first = 1 if cfg.use_cls else 0
    b = np.ascontiguousarray(np.asarray(bits))
    b = b.view(np.uint32) if b.dtype == np.int32 else b.astype(np.uint32, copy=False)
    if b.ndim != 2 or b.shape[1] != words_per_region(cfg, grid):
        raise ValueError(f"bits must be [R, {words_per_region(cfg, grid)}], got {b.shape}")
    allow = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(b.shape[0], -1)
    return allow[:, first:first + gh * gw].reshape(b.shape[0], gh, gw)


def cell_masks(cfg, bits, width, height, grid=None):
    """The inverse of :func:`token_masks`' pixel -> cell rule: token bitmaps ``uint32 [R, ceil(S / 32)]`` (a detection's
    ``bits``; int32 words are reinterpreted) -> boolean pixel masks ``[R, height, width]`` of a ``width x height`` source
    image.  Pixel ``(px, py)`` is set iff cell ``(px * g // width, py * g // height)`` is; the class token's bit is ignored.
    For ``width, height >= g`` every cell holds a pixel and ``token_masks(cfg, cell_masks(cfg, bits, w, h), w, h) == bits``
    (patch bits).  When an axis has fewer pixels than cells, the cells no pixel maps to vanish: the mask cannot show them,
    and a region made only of such cells gives an empty mask."""
    width, height = int(width), int(height)
    gh, gw, _ = _grid(cfg, grid)
    if width <= 0 or height <= 0:
        raise ValueError("cell_masks: width and height must be positive")
    cells = _unpack_cells(cfg, bits, grid)
    cx, _ = _axis_cells(width, gw)
    cy, _ = _axis_cells(height, gh)
    return cells[:, cy[:, None], cx[None, :]]


def cell_boxes(cfg, boxes, width, height, grid=None):
    """Inclusive cell boxes ``[R, 4]`` (gx0, gy0, gx1, gy1: a detection's ``boxes``) -> source-pixel ``xyxy`` ``int64 [R, 4]``
    by the same integer map: ``x0`` is the first pixel of column ``gx0``, ``x1`` one past the last pixel of column ``gx1``
    (half-open, like the full-frame box ``[0, 0, width, height]``), so the box encloses :func:`cell_masks`' pixels.  Pixel
    ``px`` lies in column ``gx`` iff ``ceil(gx * width / g) <= px < ceil((gx + 1) * width / g)``.  When an axis has fewer
    pixels than cells a box of cells without a pixel is empty (``x1 == x0``)."""
    width, height = int(width), int(height)
    gh, gw, _ = _grid(cfg, grid)
    if width <= 0 or height <= 0:
        raise ValueError("cell_boxes: width and height must be positive")
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    if b.size and (b.min() < 0 or b[:, [0, 2]].max() >= gw or b[:, [1, 3]].max() >= gh or (b[:, 0] > b[:, 2]).any()
                   or (b[:, 1] > b[:, 3]).any()):
        raise ValueError(f"cell_boxes: boxes must be inclusive cell ranges inside the {gh} x {gw} grid")
    start = lambda c, n, g: -((-c * n) // g)                  # ceil(c * n / g): the first pixel of cell c
    return np.stack([start(b[:, 0], width, gw), start(b[:, 1], height, gh), start(b[:, 2] + 1, width, gw),
                     start(b[:, 3] + 1, height, gh)], axis=1)
