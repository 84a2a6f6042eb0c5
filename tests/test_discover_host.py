"""CPU: the argument checks of the discovery / context search (they return before the device is touched), its binding and
export by both libraries, the register allocation of its kernels (discover.hip, from hipcc's own resource report: hipcc
cross-compiles for gfx950 without a GPU), and the numpy statement of score(r) on hand-computed cases, as bit patterns."""
import ctypes as C
import os
import re
import sys

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill  # noqa: E402
from _discover_checks import context_loss, context_score, discovery_score, fs, ranks, sig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32
EPS = f(np.finfo(np.float32).eps)


def _bits(a):
    return np.asarray(a, dtype=f).view(np.uint32)


def _fake_handle():
    """a zero-filled stand-in for a handle: no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_discover_argument_checks_without_a_device():
    lib = _lib.load()
    buf = lambda n: C.cast(C.create_string_buffer(n), C.c_void_p)   # noqa: E731
    tg, ps, ng = buf(64 * 4), buf(4 * 64 * 4), buf(4 * 64 * 4)
    sc = C.create_string_buffer(b"\x5a" * 64, 64)
    ix = C.create_string_buffer(b"\x5a" * 128, 128)
    ct = C.create_string_buffer(b"\x5a" * 4, 4)
    s, i, c = (C.cast(b, C.c_void_p) for b in (sc, ix, ct))
    fake = _fake_handle()

    def call(g=fake, t=tg, p=ps, n=ng, pairs=2, k=5, has=0, thr=0.0, s=s, i=i, c=c):
        return lib.revo_search_discover(g, t, p, n, pairs, k, has, thr, 0, s, i, c, None)

    assert call(g=None) == -2 and b"null" in lib.revo_last_error()
    assert call(s=None) == -2 and b"null" in lib.revo_last_error()
    assert call(i=None) == -2 and b"null" in lib.revo_last_error()
    assert call(c=None) == -2 and b"null" in lib.revo_last_error()
    assert call(p=None) == -2 and b"null positives or negatives" in lib.revo_last_error()
    assert call(n=None) == -2 and b"null positives or negatives" in lib.revo_last_error()
    assert call(t=None, p=None) == -2 and b"null positives or negatives" in lib.revo_last_error()
    # the pair count, per mode
    assert call(pairs=-1) == -2 and b"[0, 63] with a target" in lib.revo_last_error()
    assert call(pairs=64) == -2 and b"[0, 63] with a target" in lib.revo_last_error()
    assert call(pairs=2 ** 31 - 1) == -2 and b"[0, 63] with a target" in lib.revo_last_error()
    assert call(t=None, pairs=0) == -2 and b"[1, 64] without a target" in lib.revo_last_error()
    assert call(t=None, pairs=65) == -2 and b"[1, 64] without a target" in lib.revo_last_error()
    assert call(t=None, pairs=-3) == -2 and b"[1, 64] without a target" in lib.revo_last_error()
    assert call(k=0) == -2 and b"1024" in lib.revo_last_error()
    assert call(k=1025) == -2 and b"1024" in lib.revo_last_error()
    assert call(has=1, thr=float("nan")) == -2 and b"NaN" in lib.revo_last_error()
    # everything in range: the zero-filled handle has no fp32 rows
    assert call() == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(pairs=63) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(pairs=0, p=None, n=None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(t=None, pairs=64) == -2 and b"keep_f32" in lib.revo_last_error()
    assert sc.raw == b"\x5a" * 64 and ix.raw == b"\x5a" * 128 and ct.raw == b"\x5a" * 4


def test_binding_and_export():
    assert "revo_search_discover" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_discover") and hasattr(_lib.load_exp(), "revo_search_discover")
    with open(os.path.join(ROOT, "include", "revo.h")) as fh:
        header = fh.read()
    m = re.search(r"int32_t revo_search_discover\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["revo_search_discover"][1]) == 13


def test_discover_kernels_do_not_spill():
    """Every kernel of discover.hip: no VGPR spills and no scratch (the pass runs the 256 x 256 main loop and then holds 32
    more counts or sums per lane; a spill inside its tile loop would wait for the next tile's operand DMA)."""
    assert_no_spill("discover.hip", "discover_", 9)      # pass (64 / 128 rows x sample / candidates x target / context), rescore


def test_rank_and_discovery_score_on_hand_computed_cases():
    # one pair; columns: sp > sn, sp == sn (rank -1), sp < sn
    SP = np.array([[0.9, 0.5, 0.2]], dtype=f)
    SN = np.array([[0.1, 0.5, 0.8]], dtype=f)
    assert ranks(SP, SN).tolist() == [1, -1, -1]
    st = np.array([0.0, 1.0, -1.0], dtype=f)
    # fs(0) = 0 -> sig 0.5; fs(1) = 0.5 -> sig 0.75; fs(-1) = -0.5 -> sig 0.25: all exact
    assert np.array_equal(_bits(sig(st)), _bits([0.5, 0.75, 0.25]))
    got = discovery_score(st, SP, SN)
    assert got.dtype == f and np.array_equal(_bits(got), _bits([1.5, -0.25, -0.75]))
    # R = +63 and -63: the sum is rounded at the ulp of 64 (2^-18): sig = 0.75 is representable there, sig(0.3) is not
    SP = np.full((63, 2), 0.5, dtype=f)
    SN = np.stack([np.full(63, 0.25, dtype=f), np.full(63, 0.75, dtype=f)], axis=1)
    assert ranks(SP, SN).tolist() == [63, -63]
    assert np.array_equal(_bits(discovery_score(np.array([1.0, 1.0], dtype=f), SP, SN)), _bits([63.75, -62.25]))
    s3 = sig(np.array([0.3], dtype=f))[0]
    got = discovery_score(np.array([0.3, 0.3], dtype=f), SP, SN)
    assert np.array_equal(_bits(got), _bits([f(63) + s3, f(-63) + s3]))
    assert float(got[0]) != 63.0 + float(s3)             # (the sum was rounded: 63 + sig does not fit in 24 bits)
    # zero pairs with a target: R = 0, the score is sig itself
    none = np.zeros((0, 3), dtype=f)
    st = np.array([0.3, -0.7, 0.0], dtype=f)
    assert ranks(none, none).tolist() == [0, 0, 0]
    assert np.array_equal(_bits(discovery_score(st, none, none)), _bits(sig(st)))


def test_sig_is_three_rounded_operations():
    """x = 0.3f: the denominator 1 + x is rounded to fp32 before the division, the quotient before the addition.  The bits
    are those of the three fp32 operations, and they differ from the expression evaluated in fp64 and rounded once."""
    x = f(0.3)
    den = f(f(1) + x)
    q = f(x / den)
    want = f(f(0.5) * f(q + f(1)))
    got = sig(np.array([x], dtype=f))[0]
    assert _bits(got) == _bits(want)
    assert _bits(fs(np.array([x], dtype=f))[0]) == _bits(q)
    # a value where the single rounding of the fp64 expression gives another float
    xs = np.arange(f(0.3).view(np.int32), f(0.3).view(np.int32) + 4096, dtype=np.int32).view(f)
    once = (0.5 * (xs.astype(np.float64) / (1.0 + np.abs(xs.astype(np.float64))) + 1.0)).astype(f)
    differs = np.nonzero(sig(xs).view(np.uint32) != once.view(np.uint32))[0]
    assert differs.shape[0] >= 1
    j = int(differs[0])
    xj = xs[j]
    assert _bits(sig(xs)[j]) == _bits(f(f(0.5) * f(f(xj / f(f(1) + xj)) + f(1)))) != _bits(once[j])


def test_context_loss_on_hand_computed_cases():
    # columns: sp > sn by far; sp == sn; sp < sn; a difference of exactly FLT_EPSILON
    SP = np.array([[0.9, 0.5, 0.25, 0.5 + float(EPS)]], dtype=f)
    SN = np.array([[0.1, 0.5, 0.75, 0.5]], dtype=f)
    assert f(SP[0, 3] - SN[0, 3]) == EPS                 # (0.5 + 2^-23 is a float, the difference is exact)
    L = context_loss(SP, SN)
    m_eps = f(-EPS / f(f(1) + EPS))                      # fs(-eps)
    x2 = f(f(-0.5) - EPS)
    m2 = f(x2 / f(f(1) + np.abs(x2)))
    assert L.dtype == f and np.array_equal(_bits(L[0]), _bits([0.0, m_eps, m2, 0.0]))
    assert not np.signbit(L[0, 0]) and not np.signbit(L[0, 3]) and L[0, 1] < 0     # +0; sp == sn is NOT satisfied
    # the sum: pair order, starting from loss_0
    SP = np.array([[0.5], [0.25], [0.1]], dtype=f)
    SN = np.array([[0.5], [0.75], [0.9]], dtype=f)
    L = context_loss(SP, SN)[:, 0]
    assert _bits(context_score(SP, SN)[0]) == _bits(f(f(L[0] + L[1]) + L[2]))
    # one pair: the loss itself; every pair satisfied: +0
    assert _bits(context_score(SP[:1], SN[:1])[0]) == _bits(m_eps)
    z = context_score(np.full((5, 2), 0.9, dtype=f), np.full((5, 2), 0.1, dtype=f))
    assert np.array_equal(_bits(z), _bits([0.0, 0.0]))
