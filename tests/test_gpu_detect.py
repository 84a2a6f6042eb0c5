"""GPU: text-prompted regions (include/revo.h TOKENS and DETECT).  The contract is numerical and every
comparison is exact: token vectors against one-token regions (torch.equal), score bits against the range search (uint32),
the region kernel against the numpy restatement of tests/_detect_reference.py (np.array_equal), revo_vit_detect end to end
against that restatement applied to embed_tokens plus range-search scores, its refusals, and the facade's prompt detector."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import reverso_amd
from reverso_amd import _lib, engine, regions
from reverso_amd.core_system import PromptDetector, SimpleReverso
from reverso_amd.tokenizer import ClipTokenizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _detect_reference as dr  # noqa: E402
import _text_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu


def _images(cfg, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8).to(dev)


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def b16(dev):
    eng = engine.VitEngine.synthetic("PE-Core-B16-224", seed=7, device=0, max_batch=3, randomize_affine=True)
    yield eng
    eng.close()


# ------------------------------------------------------------- token vectors ----
def _check_tokens(eng, B, seed, dev):
    cfg = eng.cfg
    S, words = cfg.seq, (cfg.seq + 31) // 32
    u8 = _images(cfg, B, seed, dev)
    one = np.zeros((B * S, words), dtype=np.uint32)
    tok = np.tile(np.arange(S), B)
    one[np.arange(B * S), tok >> 5] = np.uint32(1) << (tok & 31).astype(np.uint32)
    ri = np.repeat(np.arange(B), S)
    for normalize in (False, True):
        glob = eng.embed(u8, normalize=normalize)
        _, reg = eng.embed_regions(u8, ri, one, normalize=normalize, with_global=False)
        g2, t = eng.embed_tokens(u8, normalize=normalize)
        assert t.shape == (B, S, cfg.out_dim)
        assert torch.equal(t.reshape(B * S, -1), reg), f"normalize={normalize}"
        assert torch.equal(g2, glob)
        g3, t3 = eng.embed_tokens(u8, normalize=normalize, with_global=False)
        assert g3 is None and torch.equal(t3, t)
    assert torch.isfinite(t).all() and float((t.norm(dim=-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("name", ["PE-Tiny-T14-56", "PE-Tiny-N14-56"])
def test_token_vectors_are_the_one_token_regions_tiny(name, dev):
    eng = engine.VitEngine.synthetic(name, seed=3, device=0, max_batch=2, randomize_affine=True)
    try:
        _check_tokens(eng, 2, 5, dev)
    finally:
        eng.close()


def test_token_vectors_are_the_one_token_regions_across_the_chunk(b16, dev):
    assert 3 * b16.cfg.seq == 591                       # crosses the head's 512-row chunk
    _check_tokens(b16, 3, 6, dev)


# ---------------------------------------------------------------- score bits ----
def _range_scores(prompts, rows, dev):
    """s[p, r] from parent-commit code: Gallery.search_range(prompts, -2.0) over the rows appended with normalize=False.  The
    gallery takes dimensions that are multiples of 64 only: other rows and prompts are padded with zeros, which neither the
    query normalisation (an fma of 0 * 0 onto the sum) nor the re-score's chain (lanes that hold only zeros add +0) sees."""
    P, D = prompts.shape
    pad = (-D) % 64
    if pad:
        prompts = torch.cat([prompts, torch.zeros((P, pad), device=dev)], dim=1)
        rows = torch.cat([rows, torch.zeros((rows.shape[0], pad), device=dev)], dim=1)
    G = engine.Gallery(D + pad, rows.shape[0], device=0)
    try:
        G.add(rows, normalize=False)
        off, idx, sc = G.search_range(prompts, -2.0)
    finally:
        G.close()
    off, idx, sc = off.cpu().numpy(), idx.cpu().numpy(), _u32(sc)
    out = np.zeros((P, rows.shape[0]), dtype=np.uint32)
    for p in range(P):
        assert off[p + 1] - off[p] == rows.shape[0]
        out[p, idx[off[p]:off[p + 1]]] = sc[off[p]:off[p + 1]]
    return out


@pytest.mark.parametrize("dim", [64, 96, 1024])
@pytest.mark.parametrize("n_prompts", [1, 64])
def test_score_bits_are_the_range_search_bits(lib, dev, dim, n_prompts):
    g = torch.Generator().manual_seed(dim + n_prompts)
    prompts = (torch.randn((n_prompts, dim), generator=g) * 3).to(dev)            # not unit: the op normalises them
    rows = torch.randn((600, dim), generator=g).to(dev)
    rows = rows / rows.norm(dim=1, keepdim=True)
    planted = prompts[: min(n_prompts, 8)] / prompts[: min(n_prompts, 8)].norm(dim=1, keepdim=True)
    rows = torch.cat([rows, planted]).contiguous()
    R = rows.shape[0]
    pn = torch.full((n_prompts, dim), float("nan"), device=dev)
    sc = torch.full((n_prompts, R), float("nan"), device=dev)
    _lib.check(lib.revo_op_detect_scores(_lib.ptr(rows), R, _lib.ptr(prompts), n_prompts, dim, _lib.ptr(pn), _lib.ptr(sc),
                                         _lib.current_stream()), "revo_op_detect_scores")
    torch.cuda.synchronize()
    want = _range_scores(prompts, rows, dev)
    assert np.array_equal(_u32(sc), want)
    assert float(sc[0, 600]) > 0.99999                   # a planted row scores 1 against its prompt


# ------------------------------------------------------------- region kernel ----
def _run_regions(lib, dev, s, g, cls, thr, nbg, mc, mr):
    B, P, G2 = s.shape
    words = (G2 + cls + 31) // 32
    cap = B * mr
    st = torch.from_numpy(s).to(dev)
    tt = torch.from_numpy(thr).to(dev)
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    out = {"image": i32(cap), "prompt": i32(cap), "boxes": i32(cap, 4), "cells": i32(cap),
           "confidence": torch.full((cap,), float("nan"), device=dev), "bits": i32(cap, words), "labels": i32(B, G2),
           "counts": i32(B)}
    _lib.check(lib.revo_op_detect_regions(
        _lib.ptr(st), B, P, g, cls, _lib.ptr(tt), nbg, mc, mr, _lib.ptr(out["image"]), _lib.ptr(out["prompt"]),
        _lib.ptr(out["boxes"]), _lib.ptr(out["cells"]), _lib.ptr(out["confidence"]), _lib.ptr(out["bits"]),
        _lib.ptr(out["labels"]), _lib.ptr(out["counts"]), _lib.current_stream()), "revo_op_detect_regions")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_regions_equal(got, want, name):
    n = int(want["counts"].sum())
    assert np.array_equal(got["counts"], want["counts"]), name
    assert np.array_equal(got["labels"], want["labels"]), name
    for k in ("image", "prompt", "boxes", "cells"):
        assert np.array_equal(got[k][:n], want[k]), (name, k)
    assert np.array_equal(got["confidence"][:n].view(np.uint32), want["confidence"].view(np.uint32)), name
    assert np.array_equal(got["bits"][:n].view(np.uint32), want["bits"]), name


_CASES = dr.planted_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_region_kernel_against_the_numpy_restatement(lib, dev, case):
    name, s, g, cls, thr, nbg, mc, mr = case
    want = dr.detect_reference(s, g, cls, thr, nbg, mc, mr)
    got = _run_regions(lib, dev, s, g, cls, thr, nbg, mc, mr)
    _assert_regions_equal(got, want, name)
    n = int(want["counts"].sum())
    assert (got["image"][n:] == -7).all() and (got["bits"][n:] == -7).all()      # nothing written past the result
    again = _run_regions(lib, dev, s, g, cls, thr, nbg, mc, mr)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), (name, k)


def test_region_op_refuses_bad_arguments(lib, dev):
    s = torch.zeros((1, 2, 16), device=dev)
    thr = torch.zeros(2, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    call = lambda P=2, g=4, cls=1, nbg=0, mc=1, mr=4, sp=_lib.ptr(s), tp=_lib.ptr(thr), cp=_lib.ptr(cnt): \
        lib.revo_op_detect_regions(sp, 1, P, g, cls, tp, nbg, mc, mr, None, None, None, None, None, None, None, cp,
                                   _lib.current_stream())
    for kw, word in ((dict(P=0), "n_prompts"), (dict(P=65), "n_prompts"), (dict(nbg=2), "n_background"), (dict(nbg=-1), "n_background"),
                     (dict(mc=0), "min_cells"), (dict(mr=0), "max_regions"), (dict(mr=17), "max_regions"), (dict(g=33), "g * g"),
                     (dict(cls=2), "use_cls"), (dict(sp=None), "null"), (dict(tp=None), "null"), (dict(cp=None), "null")):
        assert call(**kw) == -2 and word in lib.revo_last_error().decode(), kw
    torch.cuda.synchronize()
    assert int(cnt[0]) == -7
    assert call() == 0 and int(cnt[0]) == 1              # every output but the counts may be null


# ---------------------------------------------------------------- end to end ----
def _detect_raw(eng, u8, prompts, thr, nbg, mc, mr, with_vectors, with_global=True):
    return eng.detect(u8, prompts, thresholds=thr, n_background=nbg, min_cells=mc, max_regions=mr, with_vectors=with_vectors,
                      with_maps=True, with_global=with_global)


def test_detect_end_to_end(b16, dev):
    eng, cfg = b16, b16.cfg
    B, g, G2, first = 3, cfg.grid, cfg.grid ** 2, 1
    u8 = _images(cfg, B, 21, dev)
    glob, tok = eng.embed_tokens(u8)
    gen = torch.Generator().manual_seed(5)
    planted = [(0, 37), (2, 150)]                        # (image, cell): those cells score 1.0 against their prompt and win
    prompts = torch.cat([torch.stack([tok[b, first + c] for b, c in planted]) * 2.5,      # (not unit: normalised inside)
                         torch.randn((2, cfg.out_dim), generator=gen).to(dev)]).contiguous()
    P = prompts.shape[0]
    # the reference: the restatement applied to embed_tokens plus the range search's scores
    s_bits = _range_scores(prompts, tok[:, first:, :].reshape(B * G2, -1).contiguous(), dev)           # [P, B * G2]
    s = s_bits.view(np.float32).reshape(P, B, G2).transpose(1, 0, 2).copy()
    for p, (b, c) in enumerate(planted):
        assert s[b, p, c] > 0.99999
    thr = np.array([-np.inf, 0.0, -np.inf, -np.inf], dtype=np.float32)
    for nbg, mc, mr in ((1, 1, 50), (0, 2, 7), (1, 1, G2)):
        want = dr.detect_reference(s, g, 1, thr, nbg, mc, mr)
        d = _detect_raw(eng, u8, prompts, thr, nbg, mc, mr, True)
        n = len(d)
        assert n == int(want["counts"].sum()) and n > 0
        assert np.array_equal(_u32(d.scores), s.view(np.uint32)) and np.array_equal(d.labels.cpu().numpy(), want["labels"])
        for k in ("image", "prompt", "boxes", "cells"):
            assert np.array_equal(getattr(d, k).cpu().numpy(), want[k]), k
        assert np.array_equal(_u32(d.confidence), want["confidence"].view(np.uint32))
        assert np.array_equal(_u32(d.bits), want["bits"])
        assert torch.equal(d.global_vectors, glob)
        # the vectors are embed_regions' for the returned bitmaps (device bitmaps, as returned)
        _, reg = eng.embed_regions(u8, d.image.cpu().numpy(), d.bits, with_global=False)
        assert torch.equal(d.vectors, reg)
        # two calls: identical bytes; without vectors: the rest unchanged
        d2 = _detect_raw(eng, u8, prompts, thr, nbg, mc, mr, True)
        d3 = _detect_raw(eng, u8, prompts, thr, nbg, mc, mr, False, with_global=False)
        assert d3.vectors is None and d3.global_vectors is None
        for f in dataclasses.fields(engine.Detections):
            a, b2, c3 = getattr(d, f.name), getattr(d2, f.name), getattr(d3, f.name)
            assert _u32(a).tobytes() == _u32(b2).tobytes(), f.name
            if f.name not in ("vectors", "global_vectors"):
                assert _u32(a).tobytes() == _u32(c3).tobytes(), f.name
    # the planted cells belong to regions of their prompts with confidence 1.0 (prompt 0, image 0; prompt 1, image 2)
    want = dr.detect_reference(s, g, 1, thr, 1, 1, G2)
    for p, (b, c) in enumerate(planted):
        assert want["labels"][b, c] == p
    # un-normalised vectors follow `normalize` (scores do not)
    dn = eng.detect(u8, prompts, thresholds=thr, n_background=1, max_regions=G2, normalize=False)
    _, regn = eng.embed_regions(u8, dn.image.cpu().numpy(), dn.bits, normalize=False, with_global=False)
    assert torch.equal(dn.vectors, regn) and np.array_equal(dn.bits.cpu().numpy().view(np.uint32), want["bits"])


def test_detect_reads_and_their_lifetime(b16, dev):
    eng, cfg, lib = b16, b16.cfg, b16._lib
    u8 = _images(cfg, 2, 22, dev)
    prompts = torch.randn((3, cfg.out_dim), generator=torch.Generator().manual_seed(2)).to(dev)
    thr = (C.c_float * 3)(*([float("-inf")] * 3))
    n = C.c_int64(-1)
    call = lambda with_vec: lib.revo_vit_detect(eng._h, _lib.ptr(u8), 1, 2, _lib.ptr(prompts), 3, thr, 0, 1, 5, None, with_vec, 1,
                                                C.byref(n), _lib.current_stream())
    img = np.full(10, -7, dtype=np.int32)
    vec = torch.full((10, cfg.out_dim), float("nan"), device=dev)
    read = lambda start, cnt, v=None: lib.revo_vit_detect_read(eng._h, start, cnt, C.c_void_p(img.ctypes.data), None, None, None,
                                                                None, None, v, 0)
    eng.embed(u8)
    assert read(0, 0) == -2 and b"no result" in lib.revo_last_error()                 # a forward, no result
    assert lib.revo_vit_detect_maps(eng._h, None, None, 1) == -2
    assert call(0) == 0 and 1 <= n.value <= 10
    assert read(0, n.value) == 0 and sorted(set(img[: n.value])) == [0, 1] and (img[n.value:] == -7).all()
    assert read(1, n.value) == -2 and b"past" in lib.revo_last_error()                 # a range past the end
    assert read(-1, 1) == -2
    assert read(0, 1, _lib.ptr(vec)) == -2 and b"without vectors" in lib.revo_last_error()
    lab = torch.full((2, cfg.grid ** 2), -7, dtype=torch.int32, device=dev)
    assert lib.revo_vit_detect_maps(eng._h, None, _lib.ptr(lab), 1) == 0 and int(lab.min()) >= 0
    assert call(1) == 0
    img[:] = -7
    assert lib.revo_vit_detect_read(eng._h, 0, n.value, None, None, None, None, None, None, _lib.ptr(vec), 1) == 0
    assert torch.isfinite(vec[: n.value]).all() and torch.isnan(vec[n.value:]).all()
    for forward in (lambda: eng.embed(u8), lambda: eng.embed_tokens(u8[:1]),
                    lambda: eng.embed_regions(u8[:1], [0], regions.full_mask(cfg)[None])):
        assert call(0) == 0 and read(0, 1) == 0
        forward()
        assert read(0, 1) == -2 and lib.revo_vit_detect_maps(eng._h, None, _lib.ptr(lab), 1) == -2


# ---------------------------------------------------------------- validation ----
def test_detect_refusals_leave_the_outputs_untouched(b16, dev):
    eng, cfg, lib = b16, b16.cfg, b16._lib
    G2 = cfg.grid ** 2
    u8 = _images(cfg, 2, 23, dev)
    prompts = torch.randn((3, cfg.out_dim), generator=torch.Generator().manual_seed(3)).to(dev)
    glob = torch.full((2, cfg.out_dim), float("nan"), device=dev)
    ok_thr = (C.c_float * 3)(0.0, 0.0, 0.0)
    nan_thr = (C.c_float * 3)(0.0, float("nan"), 0.0)
    n = C.c_int64(-7)

    def call(h=eng._h, im=_lib.ptr(u8), dt=1, B=2, pr=_lib.ptr(prompts), P=3, th=ok_thr, nbg=0, mc=1, mr=5, np_=C.byref(n)):
        return lib.revo_vit_detect(h, im, dt, B, pr, P, th, nbg, mc, mr, _lib.ptr(glob), 1, 1, np_, _lib.current_stream())

    assert call() == 0 and n.value >= 0                  # a result to lose
    held = n.value
    n.value = -7
    glob.fill_(float("nan"))
    for kw, word in ((dict(P=0), "n_prompts"), (dict(P=65), "n_prompts"), (dict(nbg=-1), "n_background"), (dict(nbg=3), "n_background"),
                     (dict(mc=0), "min_cells"), (dict(mr=0), "max_regions"), (dict(mr=G2 + 1), "max_regions"),
                     (dict(th=nan_thr), "thresholds[1]"), (dict(th=None), "thresholds"), (dict(pr=None), "prompts"),
                     (dict(im=None), "images"), (dict(h=None), "handle"), (dict(np_=None), "n_regions"), (dict(B=0), "batch"),
                     (dict(B=4), "batch"), (dict(dt=2), "image_dtype")):
        assert call(**kw) == -2, kw
        assert word in lib.revo_last_error().decode(), (kw, lib.revo_last_error())
    torch.cuda.synchronize()
    assert n.value == -7 and torch.isnan(glob).all()
    # refused before the device is touched: the held result is still there
    img = np.full(max(held, 1), -7, dtype=np.int32)
    assert lib.revo_vit_detect_read(eng._h, 0, held, C.c_void_p(img.ctypes.data), None, None, None, None, None, None, 0) == 0
    # tokens: the region entry point's refusals
    tok = torch.full((2 * cfg.seq, cfg.out_dim), float("nan"), device=dev)
    ft = lambda h=eng._h, im=_lib.ptr(u8), dt=1, B=2, out=_lib.ptr(tok): lib.revo_vit_forward_tokens(
        h, im, dt, B, None, out, 1, _lib.current_stream())
    for kw in (dict(h=None), dict(im=None), dict(out=None), dict(B=0), dict(B=4), dict(dt=3)):
        assert ft(**kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.isnan(tok).all()
    # zero regions is not an error
    inf_thr = (C.c_float * 3)(*([float("inf")] * 3))
    assert call(th=inf_thr) == 0 and n.value == 0
    d = eng.detect(u8, prompts, thresholds=float("inf"), with_maps=True)
    assert len(d) == 0 and d.vectors.shape == (0, cfg.out_dim) and int(d.labels.max()) == -1


# -------------------------------------------------------------------- facade ----
def test_facade_prompt_detector(dev, tmp_path):
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=4, detector="prompt",
                      region_mode="pool", background_prompts=("the road",))
    assert isinstance(r.detector, PromptDetector)
    vocab, merges = tr.synthetic_bpe()
    tcfg = dataclasses.replace(reverso_amd.get_text_config("PE-Tiny-Text-16"), vocab_size=len(vocab), out_dim=r.pe_model.cfg.out_dim)
    tok = ClipTokenizer(merges, context_length=tcfg.context_length, vocab_size=tcfg.vocab_size)
    r.text_model = engine.TextEngine.synthetic(tcfg, seed=5, device=0, tokenizer=tok, randomize_affine=True)
    try:
        cfg = r.pe_model.cfg
        rng = np.random.default_rng(8)
        img = Image.fromarray(rng.integers(0, 256, size=(90, 130, 3), dtype=np.uint8))
        n = r.detect_regions(img, "red car . dog")
        det, last = r.detected_regions, r.detector.last
        assert n == len(det) == len(last) >= 1 and det.class_names == ["red car", "dog"]
        assert det.mask.shape == (n, 90, 130) and set(det.class_id) <= {0, 1}
        assert np.array_equal(det.confidence.view(np.uint32), _u32(last.confidence))
        for i in range(n):
            ys, xs = np.nonzero(det.mask[i])
            assert list(det.xyxy[i]) == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]         # the box encloses the mask, tightly
        # the engine-level call the detector stands for
        u8 = r._frames_u8([img])
        prompts = r.embed_text(["red car", "dog", "the road"])
        d = r.pe_model.detect(u8, prompts, n_background=1, max_regions=16)
        for k in ("image", "prompt", "boxes", "cells", "confidence", "bits"):
            assert torch.equal(getattr(d, k), getattr(last, k)), k
        # pool mode: the stored vectors are the engine's region vectors
        emb, metas = r.extract_embeddings(img)
        assert len(emb) == n and [m["detected_class"] for m in metas] == [det.class_names[c] for c in det.class_id]
        assert torch.equal(torch.stack(list(emb)), d.vectors.cpu())
        # the same instance without a detector: the single full-frame region, as before
        r.detector = None
        assert r.detect_regions(img, "red car . dog") == 1
        assert r.detected_regions.class_names == ["full_image"] and list(r.detected_regions.xyxy[0]) == [0, 0, 130, 90]
        assert r.detected_regions.mask is None
    finally:
        r.text_model.close()
