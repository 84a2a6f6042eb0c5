"""CPU: the k-means entry points' argument checks (they return before the device is touched), the contract in include/revo.h,
the bindings against the header, the host helpers of GalleryStore.themes on numpy data (the seeded rows, the theme
assembly), and the update's summation order restated in numpy against a hand-worked three-chunk example."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "revo.h")


def _fake_handle():
    """a zero-filled stand-in for a handle: no result, no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_kmeans_argument_checks_without_a_device():
    lib = _lib.load()
    n, it, conv = C.c_int64(-5), C.c_int32(-5), C.c_int32(-5)
    cents = C.cast(C.create_string_buffer(64 * 4 * 4), C.c_void_p)
    args = (C.byref(it), C.byref(conv), C.byref(n), None)
    assert lib.revo_gallery_kmeans(None, cents, 4, 1, 0, 10, *args) == -2 and b"null" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_kmeans(fake, None, 4, 1, 0, 10, *args) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans(fake, cents, 4, 1, 0, 10, None, C.byref(conv), C.byref(n), None) == -2
    assert lib.revo_gallery_kmeans(fake, cents, 4, 1, 0, 10, C.byref(it), None, C.byref(n), None) == -2
    assert lib.revo_gallery_kmeans(fake, cents, 4, 1, 0, 10, C.byref(it), C.byref(conv), None, None) == -2
    assert b"null" in lib.revo_last_error()
    for c in (0, -1, 65537, 1 << 30):
        assert lib.revo_gallery_kmeans(fake, cents, c, 1, 0, 10, *args) == -2 and b"[1, 65536]" in lib.revo_last_error()
    for m in (-1, 1001, 1 << 30):
        assert lib.revo_gallery_kmeans(fake, cents, 4, 1, 0, m, *args) == -2 and b"[0, 1000]" in lib.revo_last_error()
    # (the zero-filled handle has no fp32 rows)
    assert lib.revo_gallery_kmeans(fake, cents, 4, 1, 0, 0, *args) == -2 and b"keep_f32" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans(fake, cents, 65536, 0, 0, 1000, *args) == -2 and b"keep_f32" in lib.revo_last_error()
    assert (n.value, it.value, conv.value) == (-5, -5, -5)


def test_kmeans_read_argument_checks_without_a_device():
    lib = _lib.load()
    buf = C.cast(C.create_string_buffer(64 * 8), C.c_void_p)
    assert lib.revo_gallery_kmeans_read(None, 0, 1, buf, buf, 0) == -2 and b"null handle" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans_centroids(None, buf, buf, 0) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_kmeans_read(fake, -1, 1, buf, buf, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans_read(fake, 0, -1, buf, buf, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans_read(fake, 0, 1, buf, buf, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans_read(fake, 0, 0, None, None, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_gallery_kmeans_centroids(fake, buf, buf, 0) == -2 and b"no result" in lib.revo_last_error()


def test_debug_knob_argument_checks():
    exp = _lib.load_exp()
    assert exp.revo_debug_set_kmeans(-1) == -2 and exp.revo_debug_set_kmeans((1 << 28) + 1) == -2
    assert exp.revo_debug_set_kmeans(64) == 0 and exp.revo_debug_set_kmeans(0) == 0
    assert not hasattr(_lib.load(), "revo_debug_set_kmeans")             # the product library has no such switch


def test_header_carries_the_contract():
    text = open(HEADER).read()
    at = text.index("KMEANS.  ")
    doc = text[at:text.index("int32_t revo_gallery_kmeans(", at)]
    for phrase in ("normalises a row", "bit for bit", "label -1 and score -inf", "ties go to the lowest c", "fma chain",
                   "revo_search_topk(k = 1)", "ascending row order", "chunks of 256", "starting from +0.0f", "no fma, no trees",
                   "keeps its previous bits", "zero or not finite", "*converged = 1", "*converged = 0", "*n_iter = updates done",
                   "max_iter = 0 is a pure assignment", "fixed point bit for bit", "identical bytes", "atomics", "workspace size",
                   "number of passes", "labels [size] int32", "sizes [C] int64", "append, clear, remove and update",
                   "1 <= n_centroids <= 65 536", "0 <= max_iter <= 1 000", "keep_f32 = 0", "2^31",
                   "before the device", "not finite, or has zero norm", "SYNCHRONOUS", "slot 3", "slot 6", "slot 7",
                   "NULL independently", "revo_search_set_filter", "not an error"):
        assert phrase in doc, phrase
    assert "revo_debug_set_kmeans(int64_t cap_keys)" in text


_C_TYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _header_signature(name):
    text = open(HEADER).read()
    m = re.search(r"int32_t %s\(([^)]*)\);" % name, text)
    assert m, name
    out = []
    for arg in re.sub(r"/\*.*?\*/", "", m.group(1)).split(","):
        arg = arg.strip()
        if arg.endswith("* n_rows") and arg.startswith("int64_t"):
            out.append(C.POINTER(C.c_int64))
        elif "*" in arg:
            out.append(C.c_void_p)
        else:
            out.append(_C_TYPES[arg.split()[0]])
    return out


def test_bindings_match_the_header():
    for name in ("revo_gallery_kmeans", "revo_gallery_kmeans_read", "revo_gallery_kmeans_centroids"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args == _header_signature(name), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)
    res, args = _lib.EXPERIMENT_SIGNATURES["revo_debug_set_kmeans"]
    assert res is C.c_int32 and args == _header_signature("revo_debug_set_kmeans")


# ---- the host helpers of themes ------------------------------------------------------------------------------------------------
def test_seed_rows_are_seeded_distinct_and_inside_the_mask():
    rng = np.random.default_rng(0)
    mask = rng.random(1000) < 0.4
    a = store.seed_rows(mask, 20, seed=0)
    assert a.dtype == np.int64 and a.shape == (20,) and len(set(a.tolist())) == 20 and mask[a].all()
    assert a.tolist() == sorted(a.tolist())
    assert np.array_equal(a, store.seed_rows(mask, 20, seed=0))
    assert not np.array_equal(a, store.seed_rows(mask, 20, seed=1))
    every = store.seed_rows(mask, int(mask.sum()), seed=3)
    assert np.array_equal(every, np.flatnonzero(mask))                   # as many as there are: all of them
    with pytest.raises(ValueError):
        store.seed_rows(mask, int(mask.sum()) + 1)
    with pytest.raises(ValueError):
        store.seed_rows(mask, 0)


def test_assemble_themes():
    ids = [f"p{r}" for r in range(10)]
    payloads = [{"n": r} for r in range(10)]
    labels = np.array([2, 0, -1, 2, 1, 2, 0, -1, 1, 2])
    scores = np.array([.5, .9, -np.inf, .7, .3, .7, .9, -np.inf, .4, .1], np.float32)
    sizes = np.array([2, 2, 4, 0])
    reps = np.array([1, 8, 3, -1])                                       # best score, then the lowest row
    themes = store.assemble_themes(ids, payloads, labels, sizes, reps, scores)
    assert [t.size for t in themes] == [4, 2, 2]                         # largest first, equal sizes by centroid; empty ones left out
    assert themes[0].ids == ["p0", "p3", "p5", "p9"] and themes[1].ids == ["p1", "p6"] and themes[2].ids == ["p4", "p8"]
    assert [t.representative_id for t in themes] == ["p3", "p1", "p8"]
    assert themes[0].representative_score == float(np.float32(.7)) and themes[0].representative_payload == {"n": 3}
    with pytest.raises(ValueError):
        store.assemble_themes(ids, payloads, labels, np.array([2, 2, 3, 0]), reps, scores)      # sizes that do not add up
    with pytest.raises(ValueError):
        store.assemble_themes(ids, payloads, labels, sizes, np.array([0, 8, 3, -1]), scores)    # a representative of another theme
    assert store.assemble_themes(ids, payloads, np.full(10, -1), np.zeros(4, np.int64), np.full(4, -1), scores) == []


# ---- the update's order -----------------------------------------------------------------------------------------------------------
def _update_sum(rows):
    """the contract's sum of one centroid's members (in row order): chunks of 256, each a sequential fp32 add chain from +0,
    the partials added in chunk order from +0"""
    total = np.zeros(rows.shape[1], np.float32)
    for a in range(0, rows.shape[0], 256):
        part = np.zeros(rows.shape[1], np.float32)
        for r in rows[a:a + 256]:
            part = part + r
        total = total + part
    return total


def test_update_order_on_a_hand_worked_example():
    """513 members in three chunks (256, 256, 1) of one column.  Chunk 0 is 2^24 followed by 255 ones: each 2^24 + 1 rounds
    back to 2^24, the partial is 2^24.  Chunk 1 is 256 ones: exactly 256.  Chunk 2 is the single value 0.5.  In the
    contract's order the sum is fl(fl(2^24 + 256) + 0.5) = 16 777 472 (the 0.5 is lost against 2^24 + 256, whose ulp is 2);
    a single chain over all members would give 2^24 (every one of the 511 ones is lost), the exact sum is 16 777 727.5."""
    col = np.concatenate([[2.0 ** 24], np.ones(255), np.ones(256), [0.5]]).astype(np.float32)[:, None]
    got = _update_sum(col)
    assert got.dtype == np.float32 and float(got[0]) == 16777472.0
    chain = np.float32(0)
    for v in col[:, 0]:
        chain = np.float32(chain + v)
    assert float(chain) == 2.0 ** 24                                     # not the contract's order
    # np.cumsum is the sequential chain (np.sum adds pairwise): the form the GPU test's oracle uses
    parts = [np.cumsum(col[a:a + 256], axis=0, dtype=np.float32)[-1] for a in range(0, 513, 256)]
    assert [float(p[0]) for p in parts] == [2.0 ** 24, 256.0, 0.5]
    assert float(np.float32(np.float32(parts[0][0] + parts[1][0]) + parts[2][0])) == 16777472.0
