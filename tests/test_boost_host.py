"""CPU: the host side of the boosted search (revers-o_amd/boost.py).  The (M, B) pair of a formula
against a direct fp64 evaluation of the tree for every node type, the refusals, the restated bounds of section 4z against the
exact final score, the correctly rounded host fma the GPU tests are held to, the ABI entry and the kernels' registers."""
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import reverso_amd  # noqa: F401
from reverso_amd import _lib, boost

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boost_checks as bc  # noqa: E402

N = 40


def _payloads(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(N):
        day = int(rng.integers(1, 28))
        out.append({"trust": float(rng.uniform(0.1, 2.0)), "views": int(rng.integers(0, 50)),
                    "taken": f"2024-03-{day:02d}T12:30:00Z", "taken_s": 1.7e9 + 3600.0 * r,
                    "place": {"lat": float(rng.uniform(-80, 80)), "lon": float(rng.uniform(-179, 179))},
                    "meta": {"weight": float(rng.uniform(0.0, 1.0))}})
    return out


_DAY = 86400.0
_FORMULAS = {
    "number": 3.5,
    "score": "$score",
    "key": "trust",
    "nested key": "meta.weight",
    "sum": {"sum": ["$score", "trust", 0.25]},
    "mult": {"mult": ["trust", "$score", 2.0]},
    "neg": {"sum": [{"neg": {"neg": "$score"}}, {"neg": "views"}]},
    "div": {"div": {"left": {"sum": ["$score", 1.0]}, "right": {"sum": ["views", 1]}}},
    "div by zero": {"div": {"left": "$score", "right": "views", "by_zero_default": 7.0}},
    "datetime": {"div": {"left": {"sum": [{"datetime_key": "taken"}, {"neg": {"datetime": "2024-03-01T00:00:00Z"}}]}, "right": _DAY}},
    "datetime seconds": {"mult": [1e-9, {"datetime_key": "taken_s"}]},
    "geo": {"sum": ["$score", {"mult": [1e-7, {"geo_distance": {"origin": {"lat": 52.52, "lon": 13.40}, "to": "place"}}]}]},
    "lin_decay": {"sum": ["$score", {"lin_decay": {"x": "views", "target": 10, "scale": 30, "midpoint": 0.4}}]},
    "exp_decay": {"mult": ["$score", {"exp_decay": {"x": {"datetime_key": "taken"}, "target": {"datetime": "2024-03-14T00:00:00Z"},
                                                     "scale": 5 * _DAY}}]},
    "gauss_decay": {"sum": [{"mult": ["$score", "trust"]},
                            {"gauss_decay": {"x": {"geo_distance": {"origin": {"lat": 0.0, "lon": 0.0}, "to": "place"}},
                                             "scale": 5e6, "midpoint": 0.3}}]},
    "decay defaults": {"exp_decay": {"x": "meta.weight"}},
}


@pytest.mark.parametrize("name", sorted(_FORMULAS))
def test_the_pair_reproduces_a_direct_evaluation(name):
    """M * score + B in fp64 (M, B the fp32 pair) against the tree evaluated directly in fp64 at random scores.  The pair is
    rounded once to fp32 (2^-24 relative each), so with |score| <= 1: |difference| <= 2^-24 (|M| + |B|) and fp64 noise."""
    formula, payloads = _FORMULAS[name], _payloads()
    M, B = boost.compile_formula(formula, payloads)
    assert M.dtype == B.dtype == np.float32 and M.shape == B.shape == (N,)
    rng = np.random.default_rng(1)
    for _ in range(5):
        s = rng.uniform(-1, 1, N)
        for r in range(N):
            want = bc.evaluate(formula, payloads[r], s[r])
            got = float(M[r]) * s[r] + float(B[r])
            tol = 2.0 ** -24 * (abs(float(M[r])) + abs(float(B[r]))) + 1e-12 * (1.0 + abs(want))
            assert abs(got - want) <= tol, (name, r, got, want)


def _reversed(node):
    """the same formula with the operands of every sum and mult in the opposite order"""
    if isinstance(node, dict):
        (op, arg), = node.items()
        if op in ("sum", "mult"):
            return {op: [_reversed(t) for t in reversed(arg)]}
        if op == "neg":
            return {op: _reversed(arg)}
        if op == "div":
            return {op: dict(arg, left=_reversed(arg["left"]), right=_reversed(arg["right"]))}
        if op in ("lin_decay", "exp_decay", "gauss_decay"):
            return {op: {k: (_reversed(v) if k in ("x", "target") else v) for k, v in arg.items()}}
    return node


# what a filter makes of the reviewer-style cases: payload columns multiplied or divided in, written first or last, inside a
# decay's argument and inside a denominator
_FILTERED = dict(_FORMULAS, **{
    "trust first": {"mult": ["trust", "$score"]},
    "decay of a scaled column": {"sum": ["$score", {"exp_decay": {"x": {"mult": ["views", 2.0]}}}]},
    "decay of a scaled distance": {"sum": ["$score", {"exp_decay": {"x": {"mult": [1e-3, {"geo_distance": {
        "origin": {"lat": 10.0, "lon": 20.0}, "to": "place"}}]}, "scale": 5e3}}]},
    "scaled denominator": {"div": {"left": "$score", "right": {"mult": ["trust", 2.0]}}},
    "decay target from a column": {"gauss_decay": {"x": {"datetime_key": "taken_s"}, "target": {"sum": [1.7e9, {"mult": ["views", 60.0]}]},
                                                   "scale": 7200.0}},
})


@pytest.mark.parametrize("order", ["as written", "reversed"])
@pytest.mark.parametrize("name", sorted(_FILTERED))
def test_the_pair_with_a_filter_reproduces_a_direct_evaluation(name, order):
    """The same check with points left out of the search (every third, and the first): the formula compiles as it does without
    a filter, whatever the order of its operands; the searched points get the values of the unfiltered pair, bit for bit, and
    the others NaN.  The points left out carry payloads that would be refused (a missing key, a zero denominator, a negative
    multiplier): they are not looked at."""
    formula = _FILTERED[name] if order == "as written" else _reversed(_FILTERED[name])
    payloads = _payloads()
    allowed = np.arange(N) % 3 != 0
    M0, B0 = boost.compile_formula(formula, payloads)
    for r in np.flatnonzero(~allowed):
        payloads[r] = {"trust": -1.0, "views": -1, "taken_s": 0.0}           # no "taken", "place", "meta"; views + 1 = 0
    M, B = boost.compile_formula(formula, payloads, allowed=allowed)
    assert np.array_equal(M[allowed].view(np.uint32), M0[allowed].view(np.uint32))
    assert np.array_equal(B[allowed].view(np.uint32), B0[allowed].view(np.uint32))
    assert np.isnan(M[~allowed]).all() and np.isnan(B[~allowed]).all()
    rng = np.random.default_rng(2)
    s = rng.uniform(-1, 1, N)
    for r in np.flatnonzero(allowed):
        want = bc.evaluate(_FILTERED[name], payloads[r], s[r])
        got = float(M[r]) * s[r] + float(B[r])
        tol = 2.0 ** -24 * (abs(float(M[r])) + abs(float(B[r]))) + 1e-12 * (1.0 + abs(want))
        assert abs(got - want) <= tol, (name, order, r, got, want)


@pytest.mark.parametrize("formula,what", [
    ({"mult": ["trust", "$score", "$score"]}, "affine"),
    ({"div": {"left": 1.0, "right": {"mult": ["trust", "$score"]}}}, "denominator"),
    ({"exp_decay": {"x": {"mult": ["views", "$score"]}}}, "decay"),
])
def test_refusals_hold_with_a_filter(formula, what):
    allowed = np.arange(N) % 3 != 0
    with pytest.raises(ValueError, match=what):
        boost.compile_formula(formula, _payloads(), allowed=allowed)
    with pytest.raises(ValueError, match=what):
        boost.compile_formula(formula, _payloads(), allowed=np.zeros(N, dtype=bool) | (np.arange(N) == 4))


def test_a_filter_that_selects_nothing():
    M, B = boost.compile_formula({"mult": ["trust", "$score"]}, _payloads(), allowed=np.zeros(N, dtype=bool))
    assert np.isnan(M).all() and np.isnan(B).all() and M.dtype == np.float32


def test_decay_definitions():
    p = [{"x": 3.0}]
    for op, want in (("lin_decay", max(0.0, 1 - (1 - 0.25) * 1.0 / 2.0)), ("exp_decay", math.exp(math.log(0.25) * 1.0 / 2.0)),
                     ("gauss_decay", math.exp(math.log(0.25) * 1.0 / 4.0))):
        M, B = boost.compile_formula({op: {"x": "x", "target": 2.0, "scale": 2.0, "midpoint": 0.25}}, p)
        assert M[0] == 0 and B[0] == np.float32(want), op
    # at d = scale a decay is its midpoint; lin_decay reaches 0 and stays there
    M, B = boost.compile_formula({"lin_decay": {"x": "x", "target": 1003.0, "scale": 10.0}}, p)
    assert B[0] == 0
    for op in ("lin_decay", "exp_decay", "gauss_decay"):
        _, B = boost.compile_formula({op: {"x": "x", "target": 1.0, "scale": 2.0, "midpoint": 0.3}}, p)
        assert abs(float(B[0]) - 0.3) < 1e-7, op


def test_defaults_and_missing_keys():
    payloads = _payloads()
    del payloads[7]["trust"]
    with pytest.raises(ValueError, match="trust"):
        boost.compile_formula({"mult": ["$score", "trust"]}, payloads)
    M, _ = boost.compile_formula({"mult": ["$score", "trust"]}, payloads, defaults={"trust": 0.5})
    assert M[7] == np.float32(0.5) and M[8] == np.float32(payloads[8]["trust"])
    del payloads[9]["taken"]
    with pytest.raises(ValueError, match="taken"):
        boost.compile_formula({"datetime_key": "taken"}, payloads)
    _, B = boost.compile_formula({"datetime_key": "taken"}, payloads, defaults={"taken": "1970-01-02T00:00:00+00:00"})
    assert B[9] == np.float32(86400.0)
    # a point the search does not look at needs no value
    allowed = np.ones(N, dtype=bool)
    allowed[7] = False
    M, B = boost.compile_formula({"mult": ["$score", "trust"]}, payloads, allowed=allowed)
    assert np.isnan(M[7]) and np.isfinite(M[allowed]).all()


@pytest.mark.parametrize("formula,what", [
    ({"mult": ["$score", "$score"]}, "affine"),
    ({"mult": [{"sum": ["$score", 1]}, {"sum": ["trust", "$score"]}]}, "affine"),
    ({"div": {"left": 1.0, "right": "$score"}}, "denominator"),
    ({"div": {"left": "$score", "right": {"sum": ["$score", 2]}}}, "denominator"),
    ({"exp_decay": {"x": "$score"}}, "decay"),
    ({"gauss_decay": {"x": "views", "target": "$score"}}, "decay"),
    ({"div": {"left": "$score", "right": "views"}}, "zero"),
    ({"pow": ["$score", 2]}, "unknown"),
    ({"lin_decay": {"x": "views", "scale": 0}}, "scale"),
])
def test_formulas_that_are_refused(formula, what):
    with pytest.raises(ValueError, match=what):
        boost.compile_formula(formula, _payloads())


def test_a_negative_coefficient_raises_only_on_a_point_that_is_searched():
    payloads = _payloads()
    payloads[5]["trust"] = -0.5
    formula = {"mult": ["$score", "trust"]}
    with pytest.raises(ValueError, match="negative"):
        boost.compile_formula(formula, payloads)
    allowed = np.ones(N, dtype=bool)
    allowed[5] = False
    M, B = boost.compile_formula(formula, payloads, allowed=allowed)
    assert (M[allowed] >= 0).all() and np.isnan(M[5]) and np.isnan(B[5])
    with pytest.raises(ValueError, match="negative"):
        boost.compile_formula({"neg": "$score"}, payloads)
    payloads[6]["views"] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        boost.compile_formula({"sum": ["$score", "views"]}, payloads)
    with pytest.raises(ValueError, match="finite"):
        boost.compile_formula({"mult": ["$score", 1e39]}, payloads)          # finite in fp64, not in fp32


def test_formula_key_tells_formulas_and_defaults_apart():
    a = boost.formula_key({"sum": ["$score", "trust"]})
    assert a == boost.formula_key({"sum": ["$score", "trust"]}) and a != boost.formula_key({"sum": ["$score", "views"]})
    assert a != boost.formula_key({"sum": ["$score", "trust"]}, {"trust": 1.0})


# ---- the host fma the GPU tests are held to ---------------------------------------------------------------------------------
def test_the_host_fma_is_rounded_once():
    f = np.float32
    m, s, b = f(2.0 ** -30), f(2.0 ** -30), f(1.0)                         # 1 + 2^-60: rounds to 1
    assert bc.fma32(m, s, b) == f(1.0)
    # m * s + b = 1 + 2^-24 + 2^-46 + 2^-70 exactly: above the midpoint of 1 and 1 + 2^-23, so fmaf gives 1 + 2^-23.  fp64 arithmetic
    # rounds the product to 53 bits, the sum to 1 + 2^-24 + 2^-46, and -- here still on the right side -- the last rounding
    # decides; the exact route never depends on that
    m, s, b = f(1 + 2.0 ** -23), f(2.0 ** -24 + 2.0 ** -47), f(1.0)
    exact = Fraction(float(m)) * Fraction(float(s)) + Fraction(float(b))
    assert exact > 1 + Fraction(2) ** -24
    assert bc.fma32(m, s, b) == f(1 + 2.0 ** -23)
    # a double rounding that goes wrong: 1 + 2^-24 + 2^-60 is above the tie, fp64 drops the 2^-60 and the tie then goes to even
    m, s, b = f(1 + 2.0 ** -23), f(2.0 ** -24), f(1.0)                     # 1 + 2^-24 + 2^-47
    assert bc.fma32(m, s, b) == f(1 + 2.0 ** -23)
    m, s, b = f(2.0 ** -30), f(2.0 ** -30), f(1 + 2.0 ** -23)              # 1 + 2^-23 + 2^-60
    assert bc.fma32(m, s, b) == f(1 + 2.0 ** -23)
    m, s, b = f(2.0 ** -12 + 2.0 ** -30), f(2.0 ** -12 + 2.0 ** -30), f(1.0)   # 1 + 2^-24 + 2^-41 + 2^-60
    assert bc.fma32(m, s, b) == f(1 + 2.0 ** -23)
    # ties go to even; subnormal results; exact zeros and their sign; infinities
    assert bc.fma32(f(1.0), f(2.0 ** -24), f(1.0)) == f(1.0)
    assert bc.fma32(f(1.0), f(3 * 2.0 ** -24), f(1.0)) == f(1 + 2.0 ** -22)
    assert bc.fma32(f(2.0 ** -100), f(2.0 ** -49), f(0.0)) == f(2.0 ** -149)
    assert bc.fma32(f(2.0 ** -100), f(2.0 ** -50), f(0.0)) == 0 and bc.fma32(f(3 * 2.0 ** -100), f(2.0 ** -50), f(0.0)) == f(2.0 ** -148)
    z = bc.fma32(f(1.0), f(-0.0), f(0.0))
    assert z == 0 and not np.signbit(z)
    assert np.signbit(bc.fma32(f(1.0), f(-0.0), f(-0.0))) and not np.signbit(bc.fma32(f(2.0), f(0.5), f(-1.0)))
    assert bc.fma32(f(3e38), f(2.0), f(0.0)) == f(np.inf) and bc.fma32(f(0.0), f(0.7), f(-2.5)) == f(-2.5)
    # random operands against exact rationals, through an independent route: the two fp32 neighbours of the fp64 value
    rng = np.random.default_rng(3)
    m, s, b = (rng.standard_normal(300).astype(f) for _ in range(3))
    got = bc.fma32(m, s, b)
    for i in range(300):
        exact = Fraction(float(m[i])) * Fraction(float(s[i])) + Fraction(float(b[i]))
        for other in (np.nextafter(got[i], f(-np.inf)), np.nextafter(got[i], f(np.inf))):
            assert abs(Fraction(float(got[i])) - exact) <= abs(Fraction(float(other)) - exact)


# ---- the restated bounds of section 4z ----------------------------------------------------------------------------------------
def _cases(rng, n):
    a = rng.uniform(-1, 1, n).astype(np.float32)
    e = (10.0 ** rng.uniform(-6, -2, n)).astype(np.float32)
    return a, e


@pytest.mark.parametrize("kind", ["random", "m = 0", "subnormal products", "b of magnitude 2^20", "m = 1000"])
def test_the_bounds_contain_the_exact_final_score(kind):
    """For a scan score a, a bound e and ANY fp32 similarity s with |a - s| <= e (in exact arithmetic): lo <= s <= hi, and the
    final score fmaf(m, s, b) lies in [fmaf(m, lo, b), fmaf(m, hi, b)] -- no further widening (steps 1 and 2)."""
    rng = np.random.default_rng(len(kind))
    n = 400
    a, e = _cases(rng, n)
    m = rng.uniform(0, 4, n).astype(np.float32)
    b = rng.uniform(-1, 1, n).astype(np.float32)
    if kind == "m = 0":
        m[:] = 0
    elif kind == "subnormal products":
        m = (2.0 ** rng.uniform(-149, -120, n)).astype(np.float32)
        b = np.where(rng.random(n) < 0.5, 0.0, 2.0 ** -140).astype(np.float32)
    elif kind == "b of magnitude 2^20":
        b = (rng.choice([-1.0, 1.0], n) * 2.0 ** 20 * rng.uniform(1, 2, n)).astype(np.float32)
    elif kind == "m = 1000":
        m[:] = 1000
    lo, hi = bc.similarity_interval(a, e)
    f_lo, f_hi = bc.final_interval(a, e, m, b)
    for i in range(n):
        # the extreme similarities: the fp32 numbers nearest the ends of [a - e, a + e] from inside, and a few between
        lo_x, hi_x = Fraction(float(a[i])) - Fraction(float(e[i])), Fraction(float(a[i])) + Fraction(float(e[i]))
        s_lo, s_hi = bc.round_f32(lo_x), bc.round_f32(hi_x)
        if Fraction(float(s_lo)) < lo_x:
            s_lo = np.nextafter(s_lo, np.float32(np.inf))
        if Fraction(float(s_hi)) > hi_x:
            s_hi = np.nextafter(s_hi, np.float32(-np.inf))
        for s in (s_lo, s_hi, a[i], np.float32(rng.uniform(float(s_lo), float(s_hi)))):
            assert lo[i] <= s <= hi[i], (kind, i)
            f = bc.fma32(m[i], s, b[i])
            assert f_lo[i] <= f <= f_hi[i], (kind, i, f_lo[i], f, f_hi[i])
    if kind == "m = 0":
        assert np.array_equal(f_lo, b) and np.array_equal(f_hi, b)


def test_minimum_similarity_and_level_restated():
    """Steps 3 to 5 on numbers: a row certainly qualifies only with lo >= min_similarity and can qualify only with hi >= it; a
    level from any sample excludes only rows whose upper bound is below the k-th lower bound of the sample."""
    lo, hi = bc.similarity_interval(np.float32(0.5), np.float32(1e-3))
    assert lo < np.float32(0.499) and hi > np.float32(0.501) and lo > np.float32(0.4989) and hi < np.float32(0.5011)
    N, k = 20_037, 10
    rows = bc.sample_rows(N, 4864)
    assert rows.shape == (4864,) and rows[0] == 0 and rows[-1] == 256 * (18 * 79 // 19) + 255 and len(set(rows.tolist())) == 4864
    assert bc.sample_rows(600, 768).max() == 599                              # (a ragged last tile: rows past N do not exist)
    mult = np.ones(N, dtype=np.float32)
    allowed = np.ones(N, dtype=bool)
    flat = np.zeros(N, dtype=np.float32)
    assert bc.rows_the_level_excludes(mult, flat, allowed, rows, k, 1.01) == 0
    rising = (8.0 * (np.arange(N) // 256) / 79).astype(np.float32)
    assert bc.rows_the_level_excludes(mult, rising, allowed, rows, k, 1.01) > N // 2
    assert bc.rows_the_level_excludes(mult, rising, allowed, np.arange(4864), k, 1.01) == 0     # a prefix sees no good row


# ---- the ABI entry and the kernels' registers ---------------------------------------------------------------------------------
def test_the_entry_point_is_declared_bound_and_exported():
    assert "revo_search_boosted" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_boosted") and hasattr(_lib.load_exp(), "revo_search_boosted")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "revo.h")).read()
    m = re.search(r"int32_t revo_search_boosted\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["revo_search_boosted"][1]) == 15


def test_refusals_before_the_device_is_touched():
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_float * 2048)()
    idx = (C.c_int64 * 2048)()
    cnt = (C.c_int32 * 1)()
    assert lib.revo_search_boosted(None, buf, None, None, 5, 0, 0.0, 0, 0.0, 0, buf, buf, idx, cnt, None) == -2
    assert b"null" in lib.revo_last_error()


def test_the_entry_point_under_address_and_ub_sanitizers():
    """tests/native/boost_host_check.cpp: the refusals from a stand-alone program whose host code (the translation units of the C
    ABI) is compiled with -fsanitize=address,undefined; no device is touched."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "revers-o_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "4", "all", "boost_check"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "boost_host_check")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("search_boosted: null arguments", "search_boosted: domains", "search_boosted: valid arguments stop at the master rows"):
        assert case in r.stdout
