"""numpy restatement of the DETECT contract (include/revo.h): score maps -> labels -> 4-connected regions -> the selected,
ordered regions with their bitmaps.  The yardstick of tests/test_gpu_detect.py; tests/test_detect_host.py holds its two
independently written component labellings (a BFS flood fill and a union-find) against each other.  No GPU, no library."""
from collections import deque

import numpy as np


# ------------------------------------------------------------------ labels ----
def label_cells(scores, thresholds, n_background):
    """scores fp32 [B, P, G2] -> (labels int32 [B, G2], winning score fp32 [B, G2]).  The winner of a cell is the prompt with
    the largest score, ties to the lowest prompt, -0 == +0, NaN never wins; it labels the cell if it is no background prompt
    and its score reaches its threshold (equality keeps)."""
    s = np.asarray(scores, dtype=np.float32)
    B, P, G2 = s.shape
    thr = np.asarray(thresholds, dtype=np.float32).reshape(P)
    w = np.full((B, G2), -1, dtype=np.int64)
    best = np.zeros((B, G2), dtype=np.float32)
    for p in range(P):
        sp = s[:, p, :]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(sp) & ((w < 0) | (sp > best))
        w[take] = p
        best[take] = sp[take]
    ok = (w >= 0) & (w < P - n_background)
    with np.errstate(invalid="ignore"):
        ok &= best >= thr[np.clip(w, 0, P - 1)]
    return np.where(ok, w, -1).astype(np.int32), best


# -------------------------------------------------------------- components ----
def components_bfs(lab):
    """lab int [g, g] -> the 4-connected components of equal label >= 0, each a sorted list of cell indices; a flood fill."""
    g = lab.shape[0]
    seen = np.zeros((g, g), dtype=bool)
    out = []
    for y0 in range(g):
        for x0 in range(g):
            if lab[y0, x0] < 0 or seen[y0, x0]:
                continue
            l, cells, todo = lab[y0, x0], [], deque([(y0, x0)])
            seen[y0, x0] = True
            while todo:
                y, x = todo.popleft()
                cells.append(y * g + x)
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < g and 0 <= xx < g and not seen[yy, xx] and lab[yy, xx] == l:
                        seen[yy, xx] = True
                        todo.append((yy, xx))
            out.append(sorted(cells))
    return sorted(out)


def components_unionfind(lab):
    """The same components from a union-find over the right and down neighbours (no traversal order shared with the BFS)."""
    g = lab.shape[0]
    flat = lab.reshape(-1)
    parent = list(range(g * g))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for c in range(g * g):
        if flat[c] < 0:
            continue
        for d, ok in ((1, c % g + 1 < g), (g, c + g < g * g)):
            if ok and flat[c + d] == flat[c]:
                a, b = find(c), find(c + d)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    groups = {}
    for c in range(g * g):
        if flat[c] >= 0:
            groups.setdefault(find(c), []).append(c)
    return sorted(sorted(v) for v in groups.values())


# ----------------------------------------------------------------- regions ----
def _orderable(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def detect_reference(scores, g, use_cls, thresholds, n_background, min_cells, max_regions, components=components_bfs):
    """The regions of DETECT for score maps fp32 [B, P, g * g].  Returns a dict of numpy arrays: labels int32 [B, g * g], counts
    int32 [B], and per region image, prompt, cells (int32 [n]), boxes int32 [n, 4], confidence fp32 [n], bits uint32
    [n, ceil((g * g + use_cls) / 32)] -- images ascending, within an image (confidence desc with -0 == +0, first cell asc),
    cut at max_regions."""
    s = np.asarray(scores, dtype=np.float32)
    B, P, G2 = s.shape
    assert G2 == g * g
    labels, _ = label_cells(s, thresholds, n_background)
    words = (G2 + use_cls + 31) // 32
    img, prm, cnt, box, conf, bits, counts = [], [], [], [], [], [], []
    for b in range(B):
        regs = []
        for cells in components(labels[b].reshape(g, g)):
            if len(cells) < min_cells:
                continue
            l = int(labels[b, cells[0]])
            v = s[b, l, cells]
            c = v[int(np.argmax(_orderable(v)))]            # the largest score, +0 above -0: the bits are defined
            regs.append((cells, l, c))
        regs.sort(key=lambda r: (-float(r[2]), r[0][0]))    # (-(-0.0) == -(+0.0) in this comparison)
        regs = regs[:max_regions]
        counts.append(len(regs))
        for cells, l, c in regs:
            ys, xs = np.asarray(cells) // g, np.asarray(cells) % g
            word = np.zeros(words, dtype=np.uint32)
            for t in np.asarray(cells) + use_cls:
                word[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
            img.append(b); prm.append(l); cnt.append(len(cells)); conf.append(c); bits.append(word)
            box.append([xs.min(), ys.min(), xs.max(), ys.max()])
    n = len(img)
    return {"labels": labels, "counts": np.asarray(counts, dtype=np.int32),
            "image": np.asarray(img, dtype=np.int32), "prompt": np.asarray(prm, dtype=np.int32),
            "cells": np.asarray(cnt, dtype=np.int32), "boxes": np.asarray(box, dtype=np.int32).reshape(n, 4),
            "confidence": np.asarray(conf, dtype=np.float32), "bits": np.asarray(bits, dtype=np.uint32).reshape(n, words)}


# ------------------------------------------------------------ planted maps ----
def spiral(g):
    """A one-cell-wide spiral of label 0 from the corner inwards (walls of -1 one cell wide): one component, the longest
    winding path a g x g grid holds."""
    lab = np.full((g, g), -1, dtype=np.int32)
    y = x = 0
    dy, dx = 0, 1
    lab[0, 0] = 0
    while True:
        moved = False
        for _ in range(4):
            yy, xx, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= yy < g and 0 <= xx < g and lab[yy, xx] < 0
            ahead = not (0 <= y2 < g and 0 <= x2 < g) or lab[y2, x2] < 0      # the cell behind the next one is not path
            sides = all(not (0 <= yy + sy < g and 0 <= xx + sx < g) or lab[yy + sy, xx + sx] < 0
                        for sy, sx in ((dx, dy), (-dx, -dy)))                  # nor are the next cell's side neighbours
            if free and ahead and sides:
                y, x = yy, xx
                lab[y, x] = 0
                moved = True
                break
            dy, dx = dx, -dy                                                   # turn right
        if not moved:
            return lab


def serpentine(g):
    """Label 0 on the even rows and on one end cell of every odd row, alternating ends; label 1 elsewhere: label 0 is one
    path through the whole grid, label 1 the bars between its turns."""
    lab = np.ones((g, g), dtype=np.int32)
    lab[0::2, :] = 0
    for y in range(1, g, 2):
        lab[y, g - 1 if (y // 2) % 2 == 0 else 0] = 0
    return lab


def u_shape(g):
    """Two arms (the outer columns) that meet only in the last row."""
    lab = np.full((g, g), -1, dtype=np.int32)
    lab[:, 0] = 0
    lab[:, g - 1] = 0
    lab[g - 1, :] = 0
    return lab


def diagonal(g):
    """Cells that touch only diagonally: g components of one cell."""
    lab = np.full((g, g), -1, dtype=np.int32)
    lab[np.arange(g), np.arange(g)] = 0
    return lab


def checkerboard(g):
    """Two prompts in a checkerboard: g * g one-cell components."""
    return ((np.arange(g)[:, None] + np.arange(g)[None, :]) % 2).astype(np.int32)


def scores_from_labels(labs, P, rng, conf=None):
    """Score maps fp32 [B, P, g * g] whose labelling at threshold 0 is `labs` ([B, g, g], -1 = none): every score in
    [-1, -0.5) except the labelled prompt's, which is `conf` (a number, or None: random in [0.5, 1), rounded to 1/16 so that
    confidences tie)."""
    labs = np.asarray(labs)
    B, g = labs.shape[0], labs.shape[1]
    s = rng.uniform(-1.0, -0.5, size=(B, P, g * g)).astype(np.float32)
    flat = labs.reshape(B, -1)
    for b in range(B):
        c = np.nonzero(flat[b] >= 0)[0]
        v = (np.floor(rng.uniform(8, 16, size=c.shape)) / 16).astype(np.float32) if conf is None else np.float32(conf)
        s[b, flat[b, c], c] = v
    return s


def blob_scores(B, P, g, rng):
    """Random score maps with blobs and many exact ties: values on a coarse lattice, constant on 2 x 2 blocks."""
    h = (g + 1) // 2
    coarse = np.floor(rng.uniform(0, 6, size=(B, P, h, h))) / 4 - 0.5
    return np.repeat(np.repeat(coarse, 2, axis=2), 2, axis=3)[:, :, :g, :g].reshape(B, P, g * g).astype(np.float32)


def planted_cases(seed=0):
    """[(name, scores [B, P, g * g], g, use_cls, thresholds [P], n_background, min_cells, max_regions)]: the cases of the
    region kernel's tests."""
    rng = np.random.default_rng(seed)
    zero = lambda P: np.zeros(P, dtype=np.float32)
    cases = []
    add = lambda name, s, g, cls=1, thr=None, nbg=0, mc=1, mr=None: cases.append(
        (name, np.ascontiguousarray(s, dtype=np.float32), g, cls, zero(s.shape[1]) if thr is None else np.asarray(thr, np.float32),
         nbg, mc, g * g if mr is None else mr))
    add("spiral32", scores_from_labels(spiral(32)[None], 2, rng), 32)
    add("serpentine32", scores_from_labels(serpentine(32)[None], 2, rng), 32)
    add("spiral_serpentine_batch", scores_from_labels(np.stack([spiral(32), serpentine(32), spiral(32).T]), 3, rng), 32, cls=0)
    for g in (4, 14, 24):
        add(f"u{g}", scores_from_labels(u_shape(g)[None], 2, rng), g)
        add(f"diagonal{g}", scores_from_labels(diagonal(g)[None], 1, rng), g, cls=0)
        add(f"diagonal_equal_confidence{g}", scores_from_labels(diagonal(g)[None], 1, rng, conf=0.75), g, mr=max(1, g // 2))
    ck = scores_from_labels(checkerboard(32)[None], 2, rng)
    add("checkerboard32_all", ck, 32)
    add("checkerboard32_cut50", ck, 32, mr=50)
    add("checkerboard32_equal_cut7", scores_from_labels(checkerboard(32)[None], 2, rng, conf=0.5), 32, cls=0, mr=7)
    # equal scores across prompts: the lowest prompt wins every cell -> one region per image
    add("equal_prompts", np.full((2, 5, 14 * 14), 0.25, dtype=np.float32), 14, thr=np.full(5, 0.25))
    # s == threshold keeps the cell, one ulp below drops it
    s = np.full((1, 2, 16), -1.0, dtype=np.float32)
    s[0, 0, :8] = 0.5
    s[0, 0, 8:] = np.nextafter(np.float32(0.5), np.float32(0))
    add("score_equals_threshold", s, 4, thr=[0.5, 0.5])
    # -0 against +0: a tie (prompt 0 wins), equal to a threshold of either sign; a region's confidence is +0 when it holds both
    s = np.full((2, 2, 16), -1.0, dtype=np.float32)
    s[0, 0, :] = -0.0
    s[0, 1, :] = 0.0
    s[1, 0, 0::2] = -0.0
    s[1, 0, 1::2] = 0.0
    add("minus_zero_tie", s, 4, thr=[0.0, -0.0])
    add("minus_zero_threshold", s, 4, cls=0, thr=[-0.0, 0.0])
    # NaN: never wins; a cell of NaNs has no label
    s = blob_scores(3, 3, 14, rng)
    s[0, 0, ::3] = np.nan
    s[1, :, 5:40] = np.nan
    s[2, 2, :] = np.nan
    add("nan_cells", s, 14, thr=np.full(3, -np.inf))
    for g in (1, 4, 14, 24, 32):
        for cls in (0, 1):
            s = blob_scores(1 if g == 1 else 5, 4, g, rng)
            add(f"blobs{g}_cls{cls}", s, g, cls=cls, thr=np.full(4, -np.inf), nbg=0)
    s = blob_scores(5, 4, 24, rng)
    for nbg in (0, 1, 3):
        add(f"background{nbg}", s, 24, thr=[-0.25, 0.0, 0.25, -np.inf], nbg=nbg)
    for mc in (1, 2, 24 * 24):
        add(f"min_cells{mc}", s, 24, thr=np.full(4, -np.inf), mc=mc, mr=9)
    add("nothing_labelled", s, 24, thr=np.full(4, np.inf))
    one = np.full((5, 2, 14 * 14), -1.0, dtype=np.float32)
    one[:, 1, :] = rng.uniform(0.1, 0.9, size=(5, 14 * 14)).astype(np.float32)
    add("one_label", one, 14, mc=14 * 14)
    add("one_label_g1", np.full((1, 1, 1), 0.5, dtype=np.float32), 1, mr=1)
    return cases
