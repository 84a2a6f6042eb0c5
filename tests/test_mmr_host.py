"""CPU: the argument checks of the diverse search (revo_search_mmr returns before the device is touched), its binding and
export by both libraries, the register allocation of its kernels (mmr.hip, from hipcc's own resource report: hipcc
cross-compiles for gfx950 without a GPU), and the numpy statement of the greedy selection on hand-made matrices."""
import ctypes as C
import os
import re
import sys

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill  # noqa: E402
from _mmr_checks import greedy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_handle():
    """a zero-filled stand-in for a handle: no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_mmr_argument_checks_without_a_device():
    lib = _lib.load()
    qv = C.cast(C.create_string_buffer(4 * 64 * 4), C.c_void_p)
    sc = C.create_string_buffer(b"\x5a" * 64, 64)
    mv = C.create_string_buffer(b"\x5a" * 64, 64)
    ix = C.create_string_buffer(b"\x5a" * 128, 128)
    ct = C.create_string_buffer(b"\x5a" * 16, 16)
    s, m, i, c = (C.cast(b, C.c_void_p) for b in (sc, mv, ix, ct))
    fake = _fake_handle()

    def call(g=fake, q=qv, n=2, k=5, cand=8, div=0.5, has=0, thr=0.0, s=s, m=m, i=i, c=c):
        return lib.revo_search_mmr(g, q, n, k, cand, div, has, thr, 0, s, m, i, c, None)

    assert call(g=None) == -2 and b"null" in lib.revo_last_error()
    assert call(q=None) == -2 and b"null" in lib.revo_last_error()
    assert call(s=None) == -2 and b"null" in lib.revo_last_error()
    assert call(i=None) == -2 and b"null" in lib.revo_last_error()
    assert call(c=None) == -2 and b"null" in lib.revo_last_error()
    assert call(n=-1) == -2 and b"negative" in lib.revo_last_error()
    assert call(cand=0) == -2 and b"1024" in lib.revo_last_error()
    assert call(cand=1025, k=5) == -2 and b"1024" in lib.revo_last_error()
    assert call(k=0) == -2 and b"candidates" in lib.revo_last_error()
    assert call(k=-3) == -2 and b"candidates" in lib.revo_last_error()
    assert call(k=9, cand=8) == -2 and b"candidates" in lib.revo_last_error()
    assert call(k=1025, cand=1024) == -2 and b"candidates" in lib.revo_last_error()
    assert call(div=float("nan")) == -2 and b"diversity" in lib.revo_last_error()
    assert call(div=-0.01) == -2 and b"diversity" in lib.revo_last_error()
    assert call(div=1.0001) == -2 and b"diversity" in lib.revo_last_error()
    assert call(div=float("inf")) == -2 and b"diversity" in lib.revo_last_error()
    assert call(has=1, thr=float("nan")) == -2 and b"NaN" in lib.revo_last_error()
    # every argument valid, the boundary values included: the handle has no fp32 master rows
    assert call() == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(m=None) == -2 and b"keep_f32" in lib.revo_last_error()          # mmr_values may be NULL
    assert call(q=None, n=0) == -2 and b"keep_f32" in lib.revo_last_error()     # queries may be NULL at n_queries = 0
    assert call(div=0.0, k=1, cand=1) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(div=1.0, k=1024, cand=1024) == -2 and b"keep_f32" in lib.revo_last_error()
    assert sc.raw == b"\x5a" * 64 and mv.raw == b"\x5a" * 64 and ix.raw == b"\x5a" * 128 and ct.raw == b"\x5a" * 16


def test_binding_and_export():
    assert "revo_search_mmr" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_mmr") and hasattr(_lib.load_exp(), "revo_search_mmr")
    with open(os.path.join(ROOT, "include", "revo.h")) as f:
        header = f.read()
    m = re.search(r"int32_t revo_search_mmr\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["revo_search_mmr"][1]) == 14


def test_mmr_kernels_do_not_spill():
    """Every kernel of mmr.hip: no VGPR spills and no scratch (the 8 x 8 form of the similarity kernel holds 64 running
    sums and up to 16 row slices of four floats per lane; a spill would sit inside its fma loop)."""
    assert_no_spill("mmr.hip", "mmr_", 3)            # similarity matrix (4 x 4 and 8 x 8 pairs per wave), selection


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _sym(n, entries, fill=0.0):
    s = np.full((n, n), fill, dtype=np.float32)
    for (i, j), v in entries.items():
        s[i, j] = s[j, i] = np.float32(v)
    np.fill_diagonal(s, np.nan)              # never read for a live candidate: a NaN here must not reach any value
    return s


def test_greedy_on_hand_made_matrices():
    f = np.float32
    rel = np.array([0.9, 0.89, 0.88, 0.5], dtype=f)
    sim = _sym(4, {(0, 1): 0.99, (0, 2): 0.2, (0, 3): 0.1, (1, 2): 0.2, (1, 3): 0.1, (2, 3): 0.1})
    with np.errstate(invalid="ignore"):
        # diversity 0: the plain order, the values are the scores' own bits
        p, v = greedy(rel, sim, 4, 0.0)
        assert p.tolist() == [0, 1, 2, 3] and np.array_equal(_bits(v), _bits(rel))
        # diversity 0.5: the near-copy of the first pick falls behind; every value as three rounded fp32 operations
        p, v = greedy(rel, sim, 3, 0.5)
        assert p.tolist() == [0, 2, 3]
        h = f(0.5)
        want = [h * rel[0], f(h * rel[2]) - f(h * f(0.2)), f(h * rel[3]) - f(h * f(0.1))]
        assert v.dtype == f and np.array_equal(_bits(v), _bits(want))
        # (0.5 * 0.89 - 0.5 * 0.99 = -0.05 is worse than 0.5 * 0.5 - 0.5 * 0.1 = 0.2; it comes last)
        p, v = greedy(rel, sim, 4, 0.5)
        assert p.tolist() == [0, 2, 3, 1] and v[3] == f(f(h * rel[1]) - f(h * f(0.99)))
        # diversity 1: lam = 0, the first pick is position 0 by the tie rule, then the least similar to the picked set
        p, v = greedy(rel, _sym(4, {(0, 1): 0.9, (0, 2): 0.3, (0, 3): 0.5, (1, 2): 0.1, (1, 3): 0.2, (2, 3): 0.8}), 4, 1.0)
        assert p.tolist() == [0, 2, 3, 1]
        assert np.array_equal(_bits(v), _bits([0.0, f(0.0) - f(0.3), f(0.0) - f(0.8), f(0.0) - f(0.9)]))
        # m is the maximum over ALL picked rows, not the last one
        p, _ = greedy(np.array([1.0, 0.9, 0.9, 0.9], dtype=f),
                      _sym(4, {(0, 1): 0.0, (0, 2): 0.8, (0, 3): 0.5, (1, 2): 0.0, (1, 3): 0.6, (2, 3): 0.0}), 4, 0.5)
        assert p.tolist() == [0, 1, 3, 2]
        # ties: equal values -> the lower position, at the first step and later
        p, _ = greedy(np.array([0.7, 0.7, 0.7], dtype=f), _sym(3, {(0, 1): 0.5, (0, 2): 0.5, (1, 2): 0.5}), 3, 0.5)
        assert p.tolist() == [0, 1, 2]
        # -0 = +0: lam * rel = -0 for position 0 (rel = -0) and +0 for position 1; equal values, position 0 wins
        p, v = greedy(np.array([-0.0, 0.0], dtype=f), _sym(2, {(0, 1): 0.0}), 2, 0.5)
        assert p.tolist() == [0, 1] and np.signbit(v[0])
        # ... and neither does -0 at position 1 beat +0 at position 0
        p, _ = greedy(np.array([0.0, -0.0], dtype=f), _sym(2, {(0, 1): 0.0}), 2, 0.5)
        assert p.tolist() == [0, 1]
        # n < k: every candidate once, no more; k = n: a permutation; n = 0
        p, v = greedy(rel, sim, 10, 0.3)
        assert sorted(p.tolist()) == [0, 1, 2, 3] and v.shape == (4,)
        p, _ = greedy(rel, sim, 4, 0.7)
        assert sorted(p.tolist()) == [0, 1, 2, 3] and p[0] == 0
        p, v = greedy(np.zeros(0, dtype=f), np.zeros((0, 0), dtype=f), 3, 0.5)
        assert p.shape == (0,) and v.shape == (0,)
        # lam is one fp32 subtraction from the fp32 diversity (1 - 0.65f is not the fp32 nearest to 0.35)
        p, v = greedy(np.array([0.6], dtype=f), np.zeros((1, 1), dtype=f), 1, 0.65)
        assert v[0] == f(f(1.0) - f(0.65)) * f(0.6) and f(f(1.0) - f(0.65)) != f(0.35)
