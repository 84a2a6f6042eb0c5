"""CPU: the argument checks of the search by examples (they return before the device is touched), its binding and export by
both libraries, the register allocation of its kernels (recommend.hip, from hipcc's own resource report: hipcc cross-compiles
for gfx950 without a GPU), and the pure host parts: the numpy statement of score(r) and average_vector_query."""
import ctypes as C
import os
import re
import sys

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill  # noqa: E402
from _recommend_checks import best_score, exhaustive  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_handle():
    """a zero-filled stand-in for a handle: no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_recommend_argument_checks_without_a_device():
    lib = _lib.load()
    ex = C.cast(C.create_string_buffer(4 * 64 * 4), C.c_void_p)
    sc = C.create_string_buffer(b"\x5a" * 64, 64)
    ix = C.create_string_buffer(b"\x5a" * 128, 128)
    ct = C.create_string_buffer(b"\x5a" * 4, 4)
    s, i, c = (C.cast(b, C.c_void_p) for b in (sc, ix, ct))
    fake = _fake_handle()

    def call(g=fake, e=ex, P=2, N=1, k=5, has=0, thr=0.0, s=s, i=i, c=c):
        return lib.revo_search_recommend(g, e, P, N, k, has, thr, 0, s, i, c, None)

    assert call(g=None) == -2 and b"null" in lib.revo_last_error()
    assert call(e=None) == -2 and b"null" in lib.revo_last_error()
    assert call(s=None) == -2 and b"null" in lib.revo_last_error()
    assert call(i=None) == -2 and b"null" in lib.revo_last_error()
    assert call(c=None) == -2 and b"null" in lib.revo_last_error()
    assert call(P=0) == -2 and b"positive" in lib.revo_last_error()
    assert call(N=-1) == -2 and b"negative" in lib.revo_last_error()
    assert call(P=100, N=29) == -2 and b"128" in lib.revo_last_error()
    assert call(P=2 ** 31 - 1, N=2 ** 31 - 1) == -2 and b"128" in lib.revo_last_error()
    assert call(k=0) == -2 and b"1024" in lib.revo_last_error()
    assert call(k=1025) == -2 and b"1024" in lib.revo_last_error()
    assert call(has=1, thr=float("nan")) == -2 and b"NaN" in lib.revo_last_error()
    assert call() == -2 and b"keep_f32" in lib.revo_last_error()
    assert sc.raw == b"\x5a" * 64 and ix.raw == b"\x5a" * 128 and ct.raw == b"\x5a" * 4


def test_binding_and_export():
    assert "revo_search_recommend" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_recommend") and hasattr(_lib.load_exp(), "revo_search_recommend")
    with open(os.path.join(ROOT, "include", "revo.h")) as f:
        header = f.read()
    m = re.search(r"int32_t revo_search_recommend\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["revo_search_recommend"][1])


def test_recommend_kernels_do_not_spill():
    """Every kernel of recommend.hip: no VGPR spills and no scratch (the pass runs the 256 x 256 main loop and then holds
    32 more maxima per lane; a spill inside its tile loop would wait for the next tile's operand DMA)."""
    assert_no_spill("recommend.hip", "recommend_", 7)            # pass (64 / 128 rows x sample / candidates), level, rescore, emit


def test_the_formula_on_hand_computed_cases():
    f = np.float32
    # columns: sp > sn; sp == sn (the -(sn^2) branch); sp < sn; both negative with sp > sn; sn = 0 = sp
    S = np.array([[0.9, 0.5, 0.2, -0.3, 0.0],
                  [0.1, 0.3, 0.1, -0.6, -0.2],
                  [0.4, 0.5, 0.8, -0.5, 0.0],
                  [-0.2, 0.1, 0.3, -0.9, -0.1]], dtype=f)
    got = best_score(S, 2)
    want = np.array([f(0.9), -(f(0.5) * f(0.5)), -(f(0.8) * f(0.8)), f(-0.3), -(f(0.0) * f(0.0))], dtype=f)
    assert got.dtype == f and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.signbit(got[4])                                          # -(0 * 0) = -0
    # no negatives: the maximum over the positives
    assert np.array_equal(best_score(S, 4), S.max(axis=0))
    # one fp32 multiply rounded to nearest: not the square in higher precision
    sn = f(0.3333333432674408)
    assert best_score(np.array([[0.0], [sn]], dtype=f), 1)[0] == -f(sn * sn)
    # the answer: (score desc, row asc), threshold, padding, offset
    s, i, c = exhaustive(np.array([0.5, 0.9, 0.5, -0.1], dtype=f), np.array([True, True, True, False]), 4, None, 10)
    assert c == 3 and i.tolist() == [11, 10, 12, -1] and s[3] == -np.inf and s[:3].tolist() == [f(0.9), f(0.5), f(0.5)]
    s, i, c = exhaustive(np.array([0.5, 0.9, 0.5, -0.1], dtype=f), np.ones(4, dtype=bool), 2, 0.6)
    assert c == 1 and i.tolist() == [1, -1]


def test_average_vector_query():
    rng = np.random.default_rng(0)
    pos = rng.standard_normal((3, 8)).astype(np.float32)
    neg = rng.standard_normal((2, 8)).astype(np.float32)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)   # noqa: E731
    mp, mn = unit(pos).mean(0), unit(neg).mean(0)
    assert np.allclose(store.average_vector_query(pos, neg), mp + (mp - mn), atol=1e-6)
    assert np.allclose(store.average_vector_query(pos, None), mp, atol=1e-6)
    assert np.allclose(store.average_vector_query(pos, neg[:0]), mp, atol=1e-6)
    assert np.allclose(store.average_vector_query(3.0 * pos, 0.5 * neg), mp + (mp - mn), atol=1e-6)   # normalised first
    assert np.allclose(store.average_vector_query(pos[0], None), unit(pos[:1])[0], atol=1e-6)
