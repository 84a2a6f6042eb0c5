"""CPU: Qdrant-style payload filters (filters.py) against a naive per-payload evaluator, the allow-bitmap's bit order and
shard slicing, and the argument checks of revo_search_set_filter (they return before any device call)."""
import ctypes as C
import random

import numpy as np
import pytest

import reverso_amd  # noqa: F401
from reverso_amd import _lib, filters as F

KEYS = ["s", "i", "f", "l", "b"]


def _payloads(n, seed=0):
    rnd = random.Random(seed)
    out = []
    for r in range(n):
        p = {}
        if rnd.random() < 0.9:
            p["s"] = rnd.choice(["a", "b", "c", "d"])
        if rnd.random() < 0.9:
            p["i"] = rnd.randint(0, 9)
        if rnd.random() < 0.9:
            p["f"] = rnd.random()
        if rnd.random() < 0.8:
            p["l"] = [rnd.choice(["a", "b", "c", 1, 2]) for _ in range(rnd.randint(0, 3))]
        if rnd.random() < 0.5:
            p["b"] = rnd.random() < 0.5
        out.append(p)
    return out


def _elem_match(m, v):
    same = lambda a, b: type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))
                                               and not isinstance(a, bool) and not isinstance(b, bool))
    if isinstance(m, F.MatchValue):
        return same(v, m.value) and v == m.value
    if isinstance(m, F.MatchAny):
        return any(same(v, x) and v == x for x in m.any)
    return isinstance(v, (str, int, float)) and not any(same(v, x) and v == x for x in m.except_)


def _naive_cond(c, pid, p):
    if isinstance(c, F.Filter):
        return _naive(c, pid, p)
    if isinstance(c, F.HasIdCondition):
        return pid in c.has_id
    if c.key not in p:
        return False
    vals = p[c.key] if isinstance(p[c.key], list) else [p[c.key]]
    if c.range is not None:
        r = c.range
        ok = lambda v: (isinstance(v, (int, float)) and not isinstance(v, bool) and (r.gt is None or v > r.gt) and
                        (r.gte is None or v >= r.gte) and (r.lt is None or v < r.lt) and (r.lte is None or v <= r.lte))
        return any(ok(v) for v in vals)
    return any(_elem_match(c.match, v) for v in vals)


def _naive(f, pid, p):
    f = F.as_filter(f)
    if f.must and not all(_naive_cond(c, pid, p) for c in f.must):
        return False
    if f.should and not any(_naive_cond(c, pid, p) for c in f.should):
        return False
    if f.must_not and any(_naive_cond(c, pid, p) for c in f.must_not):
        return False
    return True


FC, MV, MA, ME, R = F.FieldCondition, F.MatchValue, F.MatchAny, F.MatchExcept, F.Range
FILTERS = [
    F.Filter(must=[FC("s", match=MV("a"))]),
    F.Filter(must=[FC("i", match=MV(3))]),
    F.Filter(must=[FC("b", match=MV(True))]),
    F.Filter(must=[FC("l", match=MV("b"))]),
    F.Filter(must=[FC("l", match=MV(1))]),
    F.Filter(should=[FC("s", match=MA(["a", "c"])), FC("i", match=MA([1, 2]))]),
    F.Filter(must=[FC("s", match=ME(["a", "b"]))]),
    F.Filter(must=[FC("l", match=ME(["a"]))]),
    F.Filter(must=[FC("f", range=R(gte=0.25, lt=0.5))]),
    F.Filter(must=[FC("i", range=R(gt=2, lte=7))]),
    F.Filter(must_not=[FC("s", match=MV("d")), FC("i", range=R(lt=2))]),
    F.Filter(must=[F.HasIdCondition([3, 17, 4242, 9999])]),
    F.Filter(must=[FC("s", match=MV("a"))], should=[], must_not=None),
    F.Filter(must=[F.Filter(should=[FC("s", match=MV("b")), FC("l", match=MV("c"))])],
             must_not=[F.Filter(must=[FC("i", match=MV(4)), FC("f", range=R(gt=0.5))])]),
    F.Filter(should=[F.Filter(must_not=[FC("s", match=MV("a"))]), FC("missing", match=MV("x"))]),
    F.Filter(must=[FC("missing", range=R(gte=0))]),
    F.Filter(must_not=[FC("missing", match=ME(["x"]))]),
]


def _as_dict(c):
    if isinstance(c, F.Filter):
        return {k: [_as_dict(x) for x in getattr(c, k)] for k in ("must", "should", "must_not") if getattr(c, k) is not None}
    if isinstance(c, F.HasIdCondition):
        return {"has_id": list(c.has_id)}
    if c.range is not None:
        return {"key": c.key, "range": {k: getattr(c.range, k) for k in ("gt", "gte", "lt", "lte") if getattr(c.range, k) is not None}}
    m = c.match
    return {"key": c.key, "match": {"value": m.value} if isinstance(m, F.MatchValue) else
            ({"any": list(m.any)} if isinstance(m, F.MatchAny) else {"except": list(m.except_)})}


@pytest.fixture(scope="module")
def data():
    p = _payloads(10_000)
    ids = list(range(10_000))
    return ids, p, F.PayloadIndex().sync(ids, p)


@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_columnar_evaluation_equals_the_naive_evaluator(data, fi):
    ids, p, idx = data
    f = FILTERS[fi]
    want = np.array([_naive(f, i, x) for i, x in zip(ids, p)])
    assert np.array_equal(idx.evaluate(f), want)
    assert np.array_equal(idx.evaluate(_as_dict(f)), want)            # Qdrant's JSON form
    assert F.filter_key(f) == F.filter_key(_as_dict(f))


def test_index_follows_appends():
    p = _payloads(300, seed=1)
    ids = list(range(300))
    idx = F.PayloadIndex().sync(ids[:100], p[:100])
    f = F.Filter(must=[FC("s", match=MV("a"))])
    assert idx.evaluate(f).shape == (100,)
    idx.sync(ids, p)
    assert np.array_equal(idx.evaluate(f), np.array([_naive(f, i, x) for i, x in zip(ids, p)]))


def test_bitmap_bit_order():
    m = np.zeros(70, bool)
    m[[0, 5, 31, 32, 63, 69]] = True
    w = F.pack_bits(m).view(np.uint32)
    assert w.shape == (3,) and w.dtype == np.uint32
    assert w[0] == (1 | 1 << 5 | 1 << 31) and w[1] == (1 | 1 << 31) and w[2] == 1 << 5
    rnd = np.random.default_rng(0).random(1000) < 0.3
    b = F.pack_bits(rnd).view(np.uint32)
    assert all(bool((b[r >> 5] >> (r & 31)) & 1) == rnd[r] for r in range(1000))


@pytest.mark.parametrize("start,stop", [(0, 1000), (7, 333), (33, 1000), (500, 517), (999, 1000)])
def test_shard_slices_are_repacked_from_their_row_zero(start, stop):
    m = np.random.default_rng(start).random(1000) < 0.5
    b = F.slice_bits(m, start, stop).view(np.uint32)
    assert b.shape == ((stop - start + 31) // 32,)
    assert all(bool((b[r >> 5] >> (r & 31)) & 1) == m[start + r] for r in range(stop - start))
    assert b[-1] >> ((stop - start - 1) & 31) >> 1 == 0                # no bits past the slice


def test_set_filter_argument_checks():
    lib = _lib.load()
    bits = (C.c_uint32 * 4)()
    assert lib.revo_search_set_filter(None, bits, 100, 0, None) != 0
    assert "null" in lib.revo_last_error().decode()
    assert lib.revo_search_set_filter(None, None, 0, 0, None) != 0
    # a negative row count is refused before the handle is looked at any further (no device call)
    fake = C.c_void_p(1)
    assert lib.revo_search_set_filter(fake, bits, -1, 0, None) != 0
    assert "negative" in lib.revo_last_error().decode()
