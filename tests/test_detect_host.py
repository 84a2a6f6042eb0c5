"""CPU: the host side of text-prompted regions -- regions.cell_masks / cell_boxes against token_masks, the prompt split, and
the numpy restatement the GPU tests compare with (tests/_detect_reference.py), whose two component labellings are held against
each other here so that the yardstick is not wrong in one way."""
import os
import sys

import numpy as np
import pytest

import reverso_amd
from reverso_amd import regions as rg
from reverso_amd.core_system import split_prompt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _detect_reference as dr  # noqa: E402


def _random_bits(cfg, n, rng):
    allow = np.zeros((n, cfg.seq), dtype=bool)
    first = 1 if cfg.use_cls else 0
    allow[:, first:] = rng.random((n, cfg.grid * cfg.grid)) < 0.3
    allow[0, first:] = True
    allow[1, first:] = False
    allow[1, first + 3] = True
    return rg._pack(allow)


@pytest.mark.parametrize("name", ["PE-Tiny-T14-56", "PE-Tiny-N14-56", "PE-Core-B16-224", "PE-Core-L14-336"])
@pytest.mark.parametrize("size", [(640, 480), (97, 301), (24, 24), (1023, 25)])
def test_cell_masks_round_trip_through_token_masks(name, size):
    cfg = reverso_amd.get_config(name)
    w, h = max(size[0], cfg.grid), max(size[1], cfg.grid)        # width, height >= g: every cell holds a pixel
    bits = _random_bits(cfg, 6, np.random.default_rng(3))
    masks = rg.cell_masks(cfg, bits, w, h)
    assert masks.shape == (6, h, w) and masks.dtype == bool
    # pixel (px, py) is set iff its cell is
    g, first = cfg.grid, 1 if cfg.use_cls else 0
    for px, py in ((0, 0), (w - 1, h - 1), (w // 3, h // 2), (w - 1, 0)):
        t = first + (py * g // h) * g + (px * g // w)
        assert np.array_equal(masks[:, py, px], (bits[:, t >> 5] >> np.uint32(t & 31)) & 1 == 1)
    for min_cover in (0.5, 1.0):
        assert np.array_equal(rg.token_masks(cfg, list(masks), w, h, min_cover=min_cover), bits)
    # int32 words (a device tensor's) are the same bitmaps
    assert np.array_equal(rg.cell_masks(cfg, bits.view(np.int32), w, h), masks)


@pytest.mark.parametrize("size", [(640, 480), (97, 301), (14, 14), (15, 1000)])
def test_cell_boxes_enclose_the_masks_exactly(size):
    cfg = reverso_amd.get_config("PE-Tiny-N14-56")      # g = 4, no class token
    g = cfg.grid
    w, h = max(size[0], g), max(size[1], g)
    boxes = np.array([[0, 0, 0, 0], [0, 0, g - 1, g - 1], [1, 2, 3, 2], [g - 1, g - 1, g - 1, g - 1], [2, 0, 2, 3]])
    px = rg.cell_boxes(cfg, boxes, w, h)
    assert px.dtype == np.int64 and px.shape == (5, 4)
    assert list(px[1]) == [0, 0, w, h]
    for (gx0, gy0, gx1, gy1), (x0, y0, x1, y1) in zip(boxes, px):
        allow = np.zeros((1, g, g), dtype=bool)
        allow[0, gy0:gy1 + 1, gx0:gx1 + 1] = True
        m = rg.cell_masks(cfg, rg._pack(allow.reshape(1, -1)), w, h)[0]
        ys, xs = np.nonzero(m)
        assert (x0, y0, x1, y1) == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)     # the tight half-open box of the mask
    with pytest.raises(ValueError):
        rg.cell_boxes(cfg, [[0, 0, g, 0]], w, h)
    with pytest.raises(ValueError):
        rg.cell_boxes(cfg, [[2, 0, 1, 0]], w, h)


def test_fewer_pixels_than_cells_is_pinned():
    """An axis with fewer pixels than cells: the cells no pixel maps to vanish from the mask, a box of such cells is empty,
    and the round trip loses exactly those cells."""
    cfg = reverso_amd.get_config("PE-Tiny-N14-56")      # g = 4
    w, h = 2, 8                                         # two pixel columns: they map to cell columns 0 and 2
    allow = np.ones((1, 4, 4), dtype=bool)
    bits = rg._pack(allow.reshape(1, -1))
    m = rg.cell_masks(cfg, bits, w, h)
    assert m.shape == (1, 8, 2) and m.all()
    back = rg.token_masks(cfg, list(m), w, h)
    want = np.zeros((4, 4), dtype=bool)
    want[:, [0, 2]] = True
    assert np.array_equal(back, rg._pack(want.reshape(1, -1)))
    only_empty = np.zeros((1, 4, 4), dtype=bool)
    only_empty[0, :, 1] = True                           # column 1 holds no pixel
    assert not rg.cell_masks(cfg, rg._pack(only_empty.reshape(1, -1)), w, h).any()
    assert list(rg.cell_boxes(cfg, [[1, 0, 1, 3]], w, h)[0]) == [1, 0, 1, 8]      # x1 == x0: empty
    assert list(rg.cell_boxes(cfg, [[0, 0, 3, 3]], w, h)[0]) == [0, 0, 2, 8]
    with pytest.raises(ValueError):
        rg.cell_masks(cfg, bits, 0, 8)
    with pytest.raises(ValueError):
        rg.cell_masks(cfg, bits[:, :0], 8, 8)


def test_prompt_split():
    assert split_prompt("person . car . building") == ["person", "car", "building"]
    assert split_prompt("  a red car  .  the dog . ") == ["a red car", "the dog"]
    assert split_prompt("person . car .") == ["person", "car"]
    assert split_prompt("a.b . 3.5 litres") == ["a.b", "3.5 litres"]       # only " . " separates
    assert split_prompt("car . car") == ["car", "car"]
    assert split_prompt("one phrase") == ["one phrase"]
    assert split_prompt("") == [] and split_prompt(None) == [] and split_prompt(" . ") == []


# ------------------------------------------------------- the reference itself ----
def test_planted_shapes_are_what_they_claim():
    for g in (4, 14, 32):
        sp = dr.spiral(g)
        comps = dr.components_bfs(sp)
        assert len(comps) == 1 and len(comps[0]) == int((sp == 0).sum()) > g * g // 3
        # one cell wide: every path cell has at most two path neighbours, the two ends one
        pad = np.pad(sp == 0, 1)
        nb = (pad[:-2, 1:-1].astype(int) + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:])[sp == 0]
        assert nb.max() <= 2 and (nb == 1).sum() == 2
        se = dr.serpentine(g)
        zero = [c for c in dr.components_bfs(se) if se.reshape(-1)[c[0]] == 0]
        assert len(zero) == 1 and len(zero[0]) == int((se == 0).sum())
        assert len(dr.components_bfs(dr.u_shape(g))) == 1
        assert len(dr.components_bfs(dr.diagonal(g))) == g
        assert len(dr.components_bfs(dr.checkerboard(g))) == g * g
    # the arms of the U meet only in the last row
    u = dr.u_shape(14)
    u[13, 5] = -1
    assert len(dr.components_bfs(u)) == 2


def test_two_labellings_agree_on_random_and_planted_maps():
    rng = np.random.default_rng(11)
    maps = [dr.spiral(32), dr.serpentine(32), dr.u_shape(24), dr.diagonal(14), dr.checkerboard(32), dr.spiral(32).T,
            np.full((1, 1), 0), np.full((1, 1), -1), np.full((14, 14), 2), np.full((4, 4), -1)]
    for g in (1, 2, 4, 14, 24, 32):
        for n_labels in (1, 2, 5):
            for _ in range(6):
                maps.append(rng.integers(-1, n_labels, size=(g, g)))
    for m in maps:
        m = np.asarray(m, dtype=np.int32)
        a, b = dr.components_bfs(m), dr.components_unionfind(m)
        assert a == b
        cells = sorted(c for comp in a for c in comp)
        assert cells == list(np.nonzero(m.reshape(-1) >= 0)[0])          # a partition of the labelled cells


def test_reference_is_the_same_under_either_labelling_and_keeps_its_rules():
    for name, s, g, cls, thr, nbg, mc, mr in dr.planted_cases():
        a = dr.detect_reference(s, g, cls, thr, nbg, mc, mr, components=dr.components_bfs)
        b = dr.detect_reference(s, g, cls, thr, nbg, mc, mr, components=dr.components_unionfind)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                  b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), (name, k)
        assert a["counts"].sum() == len(a["image"]) and (a["counts"] <= mr).all() and (a["cells"] >= mc).all(), name
        assert (np.diff(a["image"]) >= 0).all(), name
        P = s.shape[1]
        assert ((a["prompt"] >= 0) & (a["prompt"] < P - nbg)).all(), name
        if cls:
            assert (a["bits"][:, 0] & 1 == 0).all(), name                 # only patch-token bits
        pop = np.array([sum(bin(int(w)).count("1") for w in row) for row in a["bits"]], dtype=np.int32)
        assert np.array_equal(pop, a["cells"]), name
    by_name = {c[0]: c for c in dr.planted_cases()}
    run = lambda n: dr.detect_reference(*by_name[n][1:])
    assert list(run("spiral32")["counts"]) == [1] and list(run("serpentine32")["prompt"]).count(0) == 1
    r = run("checkerboard32_cut50")
    assert len(r["image"]) == 50 and (np.diff(r["confidence"]) <= 0).all()
    r = run("checkerboard32_equal_cut7")
    assert list(r["boxes"][:, 0] + 32 * r["boxes"][:, 1]) == list(range(7))          # equal confidences: lowest first cell first
    assert list(run("equal_prompts")["prompt"]) == [0, 0]
    assert list(run("score_equals_threshold")["cells"]) == [8]
    r = run("minus_zero_tie")
    assert list(r["prompt"]) == [0, 0] and list(r["cells"]) == [16, 16]
    assert list(r["confidence"].view(np.uint32)) == [0x80000000, 0]                   # all -0; -0 and +0 mixed: +0
    assert run("nothing_labelled")["counts"].sum() == 0
    assert list(run("one_label")["counts"]) == [1] * 5
    assert (run("nan_cells")["labels"][1, 5:40] == -1).all()


def test_entry_points_refuse_before_the_device_is_touched():
    """No GPU in this tier: every call below returns -2 from its argument checks, naming the argument."""
    import ctypes as C
    from reverso_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    cnt = (C.c_int32 * 4)(-7, -7, -7, -7)
    p = lambda a: C.cast(a, C.c_void_p)
    regs = lambda P=2, g=4, cls=1, nbg=0, mc=1, mr=4, s=p(buf), t=p(buf), c=p(cnt), B=1: lib.revo_op_detect_regions(
        s, B, P, g, cls, t, nbg, mc, mr, None, None, None, None, None, None, None, c, None)
    for kw, word in ((dict(P=0), "n_prompts"), (dict(P=65), "n_prompts"), (dict(nbg=2), "n_background"), (dict(mc=0), "min_cells"),
                     (dict(mr=0), "max_regions"), (dict(mr=17), "max_regions"), (dict(g=0), "g * g"), (dict(g=33), "g * g"),
                     (dict(cls=-1), "use_cls"), (dict(s=None), "null"), (dict(t=None), "null"), (dict(c=None), "null"),
                     (dict(B=-1), "batch")):
        assert regs(**kw) == -2 and word in lib.revo_last_error().decode(), kw
    assert regs(B=0) == 0 and list(cnt) == [-7] * 4
    sc = lambda rows=4, P=2, dim=16, tk=p(buf), pr=p(buf), pn=p(buf), out=p(buf): lib.revo_op_detect_scores(
        tk, rows, pr, P, dim, pn, out, None)
    for kw, word in ((dict(P=0), "n_prompts"), (dict(P=65), "n_prompts"), (dict(dim=6), "dim"), (dict(dim=0), "dim"),
                     (dict(rows=-1), "rows"), (dict(tk=None), "null"), (dict(pr=None), "null"), (dict(pn=None), "null"),
                     (dict(out=None), "null")):
        assert sc(**kw) == -2 and word in lib.revo_last_error().decode(), kw
    n = C.c_int64(-7)
    assert lib.revo_vit_detect(None, p(buf), 1, 1, p(buf), 1, p(buf), 0, 1, 1, None, 0, 1, C.byref(n), None) == -2
    assert b"handle" in lib.revo_last_error() and n.value == -7
    assert lib.revo_vit_forward_tokens(None, p(buf), 1, 1, None, p(buf), 1, None) == -2
    assert lib.revo_vit_detect_read(None, 0, 0, None, None, None, None, None, None, None, 0) == -2
    assert lib.revo_vit_detect_maps(None, None, None, 0) == -2


def test_detect_entry_points_under_address_and_ub_sanitizers():
    """tests/native/detect_host_check.cpp: the same refusals from a stand-alone program whose host code (api.hip, vit.hip and
    the other translation units of the C ABI) is compiled with -fsanitize=address,undefined; no device is touched."""
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "revers-o_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "4", "all", "detect_check"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "detect_host_check")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("tower entry points: null handle", "op scores: sizes and null arguments", "op regions: limits",
                 "op regions: null arguments"):
        assert case in r.stdout
