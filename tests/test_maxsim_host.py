"""CPU: the argument checks of the multi-vector search (they return before the device is touched), its binding and export by
both libraries, the register allocation of its kernels (maxsim.hip, from hipcc's own resource report: hipcc cross-compiles
for gfx950 without a GPU), and the numpy statement of the contract on hand-computed cases, as bit patterns."""
import ctypes as C
import os
import re
import sys

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill  # noqa: E402
from _maxsim_checks import exhaustive, group_parts, ordered_sum  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


def _bits(a):
    return np.asarray(a, dtype=f).view(np.uint32)


def _fake_handle():
    """a zero-filled stand-in for a handle: no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_maxsim_argument_checks_without_a_device():
    lib = _lib.load()
    buf = lambda n: C.cast(C.create_string_buffer(n), C.c_void_p)   # noqa: E731
    qs = buf(64 * 64 * 4)
    sc = C.create_string_buffer(b"\x5a" * 64, 64)
    gi = C.create_string_buffer(b"\x5a" * 64, 64)
    ct = C.create_string_buffer(b"\x5a" * 4, 4)
    ps = C.create_string_buffer(b"\x5a" * 256, 256)
    pr = C.create_string_buffer(b"\x5a" * 512, 512)
    s, gd, c, p1, p2 = (C.cast(b, C.c_void_p) for b in (sc, gi, ct, ps, pr))
    fake = _fake_handle()

    def call(g=fake, q=qs, n=3, k=5, has=0, thr=0.0, s=s, gd=gd, c=c, p1=p1, p2=p2):
        return lib.revo_search_maxsim(g, q, n, k, has, thr, 0, s, gd, c, p1, p2, None)

    assert call(g=None) == -2 and b"null handle" in lib.revo_last_error()
    assert call(q=None) == -2 and b"null queries" in lib.revo_last_error()
    assert call(s=None) == -2 and b"null scores" in lib.revo_last_error()
    assert call(gd=None) == -2 and b"null group_ids" in lib.revo_last_error()
    assert call(c=None) == -2 and b"null counts" in lib.revo_last_error()
    for n in (0, -1, 65, 2 ** 31 - 1):
        assert call(n=n) == -2 and b"n_vectors must be in [1, 64]" in lib.revo_last_error()
    for k in (0, -4, 1025):
        assert call(k=k) == -2 and b"k must be in [1, 1024]" in lib.revo_last_error()
    assert call(has=1, thr=float("nan")) == -2 and b"threshold is NaN" in lib.revo_last_error()
    # everything in range (the part outputs are optional): the zero-filled handle has no fp32 rows
    assert call() == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(n=1, k=1) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(n=64, k=1024, p1=None, p2=None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(has=1, thr=0.5, p1=None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert sc.raw == b"\x5a" * 64 and gi.raw == b"\x5a" * 64 and ct.raw == b"\x5a" * 4
    assert ps.raw == b"\x5a" * 256 and pr.raw == b"\x5a" * 512


def test_binding_and_export():
    assert "revo_search_maxsim" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_maxsim") and hasattr(_lib.load_exp(), "revo_search_maxsim")
    with open(os.path.join(ROOT, "include", "revo.h")) as fh:
        header = fh.read()
    m = re.search(r"int32_t revo_search_maxsim\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["revo_search_maxsim"][1]) == 13
    assert "MAXSIM." in header


def test_maxsim_kernels_do_not_spill():
    """Every kernel of maxsim.hip: no VGPR spills and no scratch (the pass runs the 256 x 256 main loop and then stores up to
    64 accumulators per lane; a spill inside its tile loop would wait for the next tile's operand DMA)."""
    assert_no_spill("maxsim.hip", "maxsim_", 9)      # index (keys, heads, csr), pass, bounds, select, rescore, reduce, emit


def test_a_tie_inside_a_group_goes_to_the_lowest_row():
    S = np.array([[0.5, 0.25, 0.5, 0.5, 0.75],
                  [0.1, 0.30, 0.3, 0.2, 0.90]], dtype=f)
    groups = np.array([7, 7, 7, 3, -1])
    ids, M, R = group_parts(S, groups, np.ones(5, dtype=bool))
    assert ids.tolist() == [3, 7]
    assert R.tolist() == [[3, 3], [0, 1]]                           # vector 0: rows 0 and 2 tie -> 0; vector 1: rows 1, 2 -> 1
    assert np.array_equal(_bits(M), _bits([[0.5, 0.2], [0.5, 0.3]]))
    # the filter removes row 0: the tie is then rows 2 alone; removing every row of group 3 removes the group
    ids, M, R = group_parts(S, groups, np.array([False, True, True, False, True]))
    assert ids.tolist() == [7] and R.tolist() == [[2, 1]]
    s, g, c, ps, pr = exhaustive(S, groups, np.ones(5, dtype=bool), 3, index_offset=100)
    assert c == 2 and g.tolist() == [7, 3, -1] and pr.tolist() == [[100, 101], [103, 103], [-1, -1]]
    assert np.array_equal(_bits(s), _bits([f(0.5) + f(0.3), f(0.5) + f(0.2), -np.inf]))
    assert np.array_equal(_bits(ps[2]), _bits([-np.inf, -np.inf]))
    # threshold on the raw sum; k cuts
    s, g, c, _, _ = exhaustive(S, groups, np.ones(5, dtype=bool), 3, threshold=0.75)
    assert c == 1 and g.tolist() == [7, -1, -1]
    s, g, c, _, _ = exhaustive(S, groups, np.ones(5, dtype=bool), 1)
    assert c == 1 and g.tolist() == [7]


def test_minus_zero_equals_plus_zero():
    # inside a group: -0 in row 0 and +0 in row 1 are equal, the lowest row wins and its own bits (-0) are reported
    S = np.array([[-0.0, 0.0, -1.0]], dtype=f)
    ids, M, R = group_parts(S, np.array([4, 4, 4]), np.ones(3, dtype=bool))
    assert R.tolist() == [[0]] and _bits(M)[0, 0] == 0x80000000
    S = np.array([[0.0, -0.0, -1.0]], dtype=f)
    ids, M, R = group_parts(S, np.array([4, 4, 4]), np.ones(3, dtype=bool))
    assert R.tolist() == [[0]] and _bits(M)[0, 0] == 0x00000000
    # between groups: a score of -0 and one of +0 tie, the lower id comes first whichever holds the minus sign
    for S in (np.array([[-0.0, 0.0]], dtype=f), np.array([[0.0, -0.0]], dtype=f)):
        s, g, c, _, _ = exhaustive(S, np.array([9, 2]), np.ones(2, dtype=bool), 2)
        assert g.tolist() == [2, 9] and np.array_equal(_bits(s), _bits(S[0, ::-1]))


def test_the_order_of_the_additions_is_the_contract():
    """M = (1, 2^-24, 2^-24): from the left, 1 + 2^-24 rounds back to 1 (ties to even), twice; from the right the two small
    terms first make 2^-23, which 1 can hold.  The contract sums from M_0."""
    t = f(2.0 ** -24)
    M = np.array([[1.0, t, t]], dtype=f)
    assert _bits(ordered_sum(M))[0] == _bits(f(1.0))
    assert _bits(ordered_sum(M[:, ::-1]))[0] == _bits(f(1.0) + f(2.0 ** -23)) != _bits(f(1.0))
    S = M.T.copy()                                                   # one row, three vectors
    s, g, c, ps, pr = exhaustive(S, np.array([5]), np.ones(1, dtype=bool), 1)
    assert c == 1 and _bits(s)[0] == _bits(f(1.0)) and np.array_equal(_bits(ps[0]), _bits(M[0]))
    # one vector: the score is M_0 itself; the fp64 statement keeps the small terms
    assert _bits(ordered_sum(M[:, :1]))[0] == _bits(f(1.0))
    assert ordered_sum(M.astype(np.float64))[0] == 1.0 + 2.0 ** -23
