"""CPU: the kNN graph's argument checks (they return before the device is touched), its contract in include/revo.h, the
bindings against the header, and the host helpers of GalleryStore.neighbor_graph on numpy data: the seeded sample, the CSR
arrays and their pairs, and the self-and-duplicate rule restated in numpy."""
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


def test_knn_argument_checks_without_a_device():
    lib = _lib.load()
    n = C.c_int64(-5)
    assert lib.revo_gallery_knn(None, 10, 0, 0.0, C.byref(n), None) == -2 and b"null" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_knn(fake, 10, 0, 0.0, None, None) == -2 and b"null" in lib.revo_last_error()
    for k in (0, -1, 65, 1 << 20):
        assert lib.revo_gallery_knn(fake, k, 0, 0.0, C.byref(n), None) == -2 and b"[1, 64]" in lib.revo_last_error()
    assert lib.revo_gallery_knn(fake, 10, 1, float("nan"), C.byref(n), None) == -2 and b"NaN" in lib.revo_last_error()
    # (a NaN that is not a threshold is not looked at; the zero-filled handle has no fp32 rows)
    assert lib.revo_gallery_knn(fake, 10, 0, float("nan"), C.byref(n), None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert lib.revo_gallery_knn(fake, 64, 1, 0.5, C.byref(n), None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert n.value == -5


def test_knn_read_argument_checks_without_a_device():
    lib = _lib.load()
    buf = C.cast(C.create_string_buffer(64 * 8), C.c_void_p)
    assert lib.revo_gallery_knn_read(None, 0, 1, buf, buf, buf, 0) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_knn_read(fake, -1, 1, buf, buf, buf, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_knn_read(fake, 0, -1, buf, buf, buf, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_knn_read(fake, 0, 1, buf, buf, buf, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_gallery_knn_read(fake, 0, 0, None, None, None, 0) == -2 and b"no result" in lib.revo_last_error()


def test_debug_knob_argument_checks():
    exp = _lib.load_exp()
    assert exp.revo_debug_set_knn(-1, 0) == -2
    assert exp.revo_debug_set_knn(0, 4) == -2 and exp.revo_debug_set_knn(0, -1) == -2
    assert exp.revo_debug_set_knn(1000, 3) == 0
    assert exp.revo_debug_set_knn(0, 0) == 0
    assert not hasattr(_lib.load(), "revo_debug_set_knn")                # the product library has no such switch


def test_header_carries_the_contract():
    text = open(HEADER).read()
    at = text.index("KNN.  ")
    doc = text[at:text.index("int32_t revo_gallery_knn(", at)]
    for phrase in ("PAIRS score", "(score desc, index asc)", "never returned", "index-ascending", "-inf / -1", "counts[i]",
                   "nobody's neighbour", "identical bytes", "level estimate", "workspace size", "join passes", "appends",
                   "1 <= k <= 64", "keep_f32 = 0", "2^31", "before the device is touched", "SYNCHRONOUS", "slot 3", "slot 6",
                   "slot 7", "NULL independently", "append, clear, remove and update", "slow", "revo_search_set_filter"):
        assert phrase in doc, phrase
    assert "revo_debug_set_knn(int64_t cap_keys, int32_t level_mode)" in text


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
    for name in ("revo_gallery_knn", "revo_gallery_knn_read"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args == _header_signature(name), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)
    res, args = _lib.EXPERIMENT_SIGNATURES["revo_debug_set_knn"]
    assert res is C.c_int32 and args == _header_signature("revo_debug_set_knn")


# ---- the host helpers of neighbor_graph -----------------------------------------------------------------------------------
def test_sample_mask_is_seeded_and_stays_inside_the_mask():
    rng = np.random.default_rng(0)
    mask = rng.random(1000) < 0.4
    a = store.sample_mask(mask, 100, seed=0)
    assert a.dtype == bool and a.sum() == 100 and not (a & ~mask).any()
    assert np.array_equal(a, store.sample_mask(mask, 100, seed=0))
    assert not np.array_equal(a, store.sample_mask(mask, 100, seed=1))
    assert np.array_equal(store.sample_mask(mask, None), mask) and store.sample_mask(mask, None) is not mask
    assert np.array_equal(store.sample_mask(mask, int(mask.sum()) + 5, seed=3), mask)      # no more than there are
    assert store.sample_mask(mask, 0).sum() == 0
    with pytest.raises(ValueError):
        store.sample_mask(mask, -1)


def _knn_numpy(x, k, mask=None, threshold=None):
    """The contract restated: fp64 scores of the rows, each allowed row's best k allowed OTHER rows by (score desc, index
    asc), identical rows at other indices included, padding -inf / -1."""
    n = x.shape[0]
    mask = np.ones(n, bool) if mask is None else mask
    s = x.astype(np.float64) @ x.astype(np.float64).T
    scores = np.full((n, k), -np.inf, np.float32)
    idx = np.full((n, k), -1, np.int64)
    counts = np.zeros(n, np.int32)
    for i in np.flatnonzero(mask):
        cand = [j for j in np.flatnonzero(mask) if j != i and (threshold is None or s[i, j] >= threshold)]
        cand.sort(key=lambda j: (-s[i, j], j))
        cand = cand[:k]
        counts[i] = len(cand)
        idx[i, :len(cand)] = cand
        scores[i, :len(cand)] = s[i, cand]
    return scores, idx, counts


def test_self_and_duplicate_rule_in_numpy():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 8))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[[3, 7, 11, 20, 21, 22]] = x[3]                                     # six identical rows
    s, idx, cnt = _knn_numpy(x, 4)
    assert (cnt == 4).all() and not (idx == np.arange(40)[:, None]).any()            # never itself
    assert idx[3].tolist() == [7, 11, 20, 21] and idx[22].tolist() == [3, 7, 11, 20]   # the lowest OTHER duplicates
    assert idx[21].tolist() == [3, 7, 11, 20]                            # more than k duplicates below it: still not itself
    mask = np.ones(40, bool)
    mask[[7, 20]] = False
    s, idx, cnt = _knn_numpy(x, 4, mask)
    assert cnt[7] == 0 and cnt[20] == 0 and not np.isin(idx, [7, 20]).any()
    assert idx[3].tolist()[:3] == [11, 21, 22]
    s, idx, cnt = _knn_numpy(x, 4, threshold=0.999)
    assert cnt[3] == 4 and cnt[0] == 0 and idx[0].tolist() == [-1] * 4 and np.isneginf(s[0]).all()


def test_knn_to_graph_and_pairs():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((30, 8))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    mask = rng.random(30) < 0.5
    mask[:3] = True
    ids = [f"p{r}" for r in range(30)]
    scores, idx, counts = _knn_numpy(x, 3, mask, threshold=0.1)
    g = store.knn_to_graph(ids, mask, scores, idx, counts)
    rows = np.flatnonzero(mask)
    assert g.ids == [ids[r] for r in rows]
    assert len(g.offsets_row) == len(g.offsets_col) == len(g.scores) == int(counts.sum())
    assert g.offsets_row.tolist() == sorted(g.offsets_row.tolist())                  # CSR order: by source point
    want = [(ids[i], ids[int(idx[i, c])], float(scores[i, c])) for i in rows for c in range(counts[i])]
    assert g.pairs() == want
    assert all(a != b for a, b, _ in g.pairs())
    # an empty graph, and a neighbour outside the selected rows is refused
    e = store.knn_to_graph(ids, np.zeros(30, bool), scores, idx, counts)
    assert e.ids == [] and e.pairs() == []
    bad = idx.copy()
    bad[rows[0], 0] = int(np.flatnonzero(~mask)[0])
    with pytest.raises(ValueError):
        store.knn_to_graph(ids, mask, scores, bad, counts)
