"""Payload filters for a search restricted to part of the gallery (``GalleryStore.search(..., query_filter=...)``).

The classes mirror Qdrant's ``models.Filter`` / ``FieldCondition`` / ``MatchValue`` / ``MatchAny`` / ``MatchExcept`` /
``Range`` / ``HasIdCondition``, and the same filter in Qdrant's JSON form (a dict) is accepted too, so that scripts written
against ``QdrantClient.search(query_filter=...)`` run unchanged on the ``vector_db`` shim.  Semantics follow Qdrant:

* ``must``: every condition holds; ``should``: at least one holds (an empty or absent ``should`` is ignored);
  ``must_not``: none holds.  Conditions may be nested filters.
* keys are top-level payload keys (no nested paths); a point whose payload lacks the key does not match the condition;
* a list-valued payload matches if any of its elements matches;
* ``MatchValue`` compares within a type: a string with strings, a bool with bools, a number with numbers; ``Range`` applies
  to numbers only (not bools).

Evaluation is columnar: ``PayloadIndex`` keeps, per key, the flattened (point, value) pairs as numpy arrays, built on first
use and extended as points are appended, so a query over 1 M payloads costs a few vectorised compares, not a Python walk
over the payloads.  The result is one bool array over the points; :func:`pack_bits` turns it into the allow-bitmap the
search kernels read (bit ``r & 31`` of word ``r >> 5``)."""
from dataclasses import dataclass, field
from typing import Any, List, Optional, Union

import numpy as np

__all__ = ["Filter", "FieldCondition", "MatchValue", "MatchAny", "MatchExcept", "Range", "HasIdCondition",
           "PayloadIndex", "evaluate", "pack_bits", "slice_bits", "filter_key"]


@dataclass(frozen=True)
class MatchValue:
    value: Any


@dataclass(frozen=True)
class MatchAny:
    any: tuple

    def __init__(self, any):                                  # noqa: A002 (Qdrant's field name)
        object.__setattr__(self, "any", tuple(any))


@dataclass(frozen=True)
class MatchExcept:
    """Matches a value that is NOT one of ``except_`` (Qdrant's ``except``; also accepted as ``**{"except": [...]}``)."""
    except_: tuple

    def __init__(self, except_=None, **kw):
        vals = kw.pop("except", except_)
        if kw or vals is None:
            raise TypeError("MatchExcept(except_=[...])")
        object.__setattr__(self, "except_", tuple(vals))


@dataclass(frozen=True)
class Range:
    gt: Optional[float] = None
    gte: Optional[float] = None
    lt: Optional[float] = None
    lte: Optional[float] = None


@dataclass(frozen=True)
class FieldCondition:
    key: str
    match: Optional[Union[MatchValue, MatchAny, MatchExcept]] = None
    range: Optional[Range] = None

    def __post_init__(self):
        if (self.match is None) == (self.range is None):
            raise ValueError("FieldCondition needs exactly one of match= or range=")


@dataclass(frozen=True)
class HasIdCondition:
    has_id: tuple

    def __init__(self, has_id):
        object.__setattr__(self, "has_id", tuple(has_id))


@dataclass(frozen=True)
class Filter:
    must: Optional[tuple] = None
    should: Optional[tuple] = None
    must_not: Optional[tuple] = None

    def __init__(self, must=None, should=None, must_not=None):
        t = lambda c: None if c is None else tuple(c) if isinstance(c, (list, tuple)) else (c,)
        object.__setattr__(self, "must", t(must))
        object.__setattr__(self, "should", t(should))
        object.__setattr__(self, "must_not", t(must_not))


# ---- the dict (JSON) form -> the classes -------------------------------------------------------------------------------
def _cond_from_dict(d):
    if isinstance(d, (Filter, FieldCondition, HasIdCondition)):
        return d
    if not isinstance(d, dict):
        raise TypeError(f"filter condition must be a dict or a filter class, got {type(d).__name__}")
    if "has_id" in d:
        return HasIdCondition(d["has_id"])
    if "key" in d:
        match = rng = None
        if d.get("match") is not None:
            m = d["match"]
            if isinstance(m, (MatchValue, MatchAny, MatchExcept)):
                match = m
            elif "value" in m:
                match = MatchValue(m["value"])
            elif "any" in m:
                match = MatchAny(m["any"])
            elif "except" in m or "except_" in m:
                match = MatchExcept(m.get("except", m.get("except_")))
            else:
                raise ValueError(f"unsupported match {m!r} (value / any / except)")
        if d.get("range") is not None:
            r = d["range"]
            rng = r if isinstance(r, Range) else Range(**{k: r.get(k) for k in ("gt", "gte", "lt", "lte")})
        return FieldCondition(d["key"], match=match, range=rng)
    if any(k in d for k in ("must", "should", "must_not")):
        return as_filter(d)
    raise ValueError(f"unsupported filter condition {d!r}")


def as_filter(f):
    """A ``Filter`` from a ``Filter`` or its Qdrant JSON form (dict)."""
    if isinstance(f, Filter):
        return Filter([_cond_from_dict(c) for c in f.must] if f.must is not None else None,
                      [_cond_from_dict(c) for c in f.should] if f.should is not None else None,
                      [_cond_from_dict(c) for c in f.must_not] if f.must_not is not None else None)
    if isinstance(f, dict):
        unknown = set(f) - {"must", "should", "must_not"}
        if unknown:
            raise ValueError(f"unsupported filter keys {sorted(unknown)}")
        lst = lambda c: None if c is None else [_cond_from_dict(x) for x in (c if isinstance(c, (list, tuple)) else [c])]
        return Filter(lst(f.get("must")), lst(f.get("should")), lst(f.get("must_not")))
    raise TypeError(f"query_filter must be a Filter or a dict, got {type(f).__name__}")


def filter_key(f):
    """A hashable key of a filter (class or dict form): equal filters give equal keys."""
    return repr(as_filter(f))


# ---- columnar payload index --------------------------------------------------------------------------------------------
_STR, _BOOL, _NUM = 1, 2, 3


def _cat(v):
    if isinstance(v, str):
        return _STR
    if isinstance(v, (bool, np.bool_)):
        return _BOOL
    if isinstance(v, (int, float, np.integer, np.floating)):
        return _NUM
    return 0


class _KeyColumn:
    """Flattened (point, value) pairs of one payload key: rows[e] = point of element e; cat / s / num = its type and
    value (s: the string, num: the number or bool as float)."""

    def __init__(self):
        self._rows, self._cat, self._s, self._num = [], [], [], []
        self.rows = np.zeros(0, np.int64)
        self.cat = np.zeros(0, np.int8)
        self.s = np.zeros(0, object)
        self.num = np.zeros(0, np.float64)
        self._dirty = False
        self.has_list = False         # some point holds a list under this key (group_ids refuses it)
        self.group_rows = []          # (point, value) of the points whose value is a str or an int (not a bool)

    def add(self, row, value):
        if isinstance(value, (list, tuple)):
            self.has_list = True
        elif isinstance(value, str) or (isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))):
            self.group_rows.append((row, value))
        for v in (value if isinstance(value, (list, tuple)) else (value,)):
            c = _cat(v)
            self._rows.append(row)
            self._cat.append(c)
            self._s.append(v if c == _STR else None)
            self._num.append(float(v) if c in (_BOOL, _NUM) else np.nan)
        self._dirty = True

    def arrays(self):
        if self._dirty:
            self.rows = np.concatenate([self.rows, np.asarray(self._rows, np.int64)])
            self.cat = np.concatenate([self.cat, np.asarray(self._cat, np.int8)])
            s = np.empty(len(self._s), object)
            s[:] = self._s
            self.s = np.concatenate([self.s, s])
            self.num = np.concatenate([self.num, np.asarray(self._num, np.float64)])
            self._rows, self._cat, self._s, self._num = [], [], [], []
            self._dirty = False
        return self


class PayloadIndex:
    """Per-key columns over a growing list of payloads (and ids).  ``sync(ids, payloads)`` indexes the points appended
    since the last call; a list that shrank or was replaced is indexed again from scratch."""

    def __init__(self):
        self.cols = {}
        self.n = 0
        self._rows_of = {}          # point id -> its rows (a store may hold an id more than once)
        self._src = None

    def sync(self, ids, payloads):
        if len(ids) != len(payloads):
            raise ValueError("ids and payloads differ in length")
        if self._src is not payloads or len(payloads) < self.n:
            self.cols, self.n, self._src, self._rows_of = {}, 0, payloads, {}
        for r in range(self.n, len(payloads)):
            self._rows_of.setdefault(ids[r], []).append(r)
            p = payloads[r]
            if isinstance(p, dict):
                for k, v in p.items():
                    col = self.cols.get(k)
                    if col is None:
                        col = self.cols[k] = _KeyColumn()
                    col.add(r, v)
        self.n = len(payloads)
        return self

    def group_ids(self, key):
        """Qdrant's ``group_by=key`` as dense ids: (int32 [n] group of every point, -1 = none; the list of values, id i
        being values[i], in order of first appearance).  ``str`` and ``int`` values form groups (``"1"`` and ``1`` are
        different groups); a missing key or any other scalar (bool, float, None, dict) gives -1.  A list value would put
        a point into several groups, which the grouped search does not do: it raises ValueError."""
        out = np.full(self.n, -1, np.int32)
        values = []
        col = self.cols.get(key)
        if col is None:
            return out, values
        if col.has_list:
            raise ValueError(f"group_by over a list-valued key is not supported ({key!r})")
        ids = {}
        for row, v in col.group_rows:
            k = (type(v) is str, v if isinstance(v, str) else int(v))
            g = ids.get(k)
            if g is None:
                g = ids[k] = len(values)
                values.append(v if isinstance(v, str) else int(v))
            out[row] = g
        return out, values

    def _match(self, cond):
        out = np.zeros(self.n, bool)
        col = self.cols.get(cond.key)
        if col is None:
            return out
        c = col.arrays()
        if cond.range is not None:
            r = cond.range
            hit = c.cat == _NUM
            num = c.num
            if r.gt is not None:
                hit &= num > r.gt
            if r.gte is not None:
                hit &= num >= r.gte
            if r.lt is not None:
                hit &= num < r.lt
            if r.lte is not None:
                hit &= num <= r.lte
        else:
            m = cond.match
            vals = (m.value,) if isinstance(m, MatchValue) else (m.any if isinstance(m, MatchAny) else m.except_)
            hit = np.zeros(len(c.rows), bool)
            for v in vals:
                cv = _cat(v)
                if cv == _STR:
                    hit |= (c.cat == _STR) & (c.s == v)
                elif cv in (_BOOL, _NUM):
                    hit |= (c.cat == cv) & (c.num == float(v))
            if isinstance(m, MatchExcept):
                hit = ~hit & (c.cat != 0)
        out[c.rows[hit]] = True
        return out

    def _has_id(self, cond):
        """one dictionary lookup per wanted id (not a walk over the points)"""
        out = np.zeros(self.n, bool)
        rows = [r for i in set(cond.has_id) for r in self._rows_of.get(i, ())]
        if rows:
            out[np.asarray(rows, np.int64)] = True
        return out

    def _cond(self, c):
        if isinstance(c, Filter):
            return self.evaluate(c)
        if isinstance(c, HasIdCondition):
            return self._has_id(c)
        return self._match(c)

    def evaluate(self, f):
        """bool [n]: the points the filter (class or dict form) selects."""
        f = as_filter(f)
        out = np.ones(self.n, bool)
        for c in f.must or ():
            out &= self._cond(c)
        if f.should:
            any_ = np.zeros(self.n, bool)
            for c in f.should:
                any_ |= self._cond(c)
            out &= any_
        for c in f.must_not or ():
            out &= ~self._cond(c)
        return out


def evaluate(f, payloads, ids=None):
    """bool [len(payloads)] for a one-off evaluation (a store keeps a PayloadIndex instead)."""
    return PayloadIndex().sync(list(ids) if ids is not None else list(range(len(payloads))), payloads).evaluate(f)


def pack_bits(mask):
    """bool [n] -> int32 [ceil(n / 32)]: bit r & 31 of word r >> 5 is mask[r] (the search kernels' allow-bitmap)."""
    mask = np.asarray(mask, bool)
    n = mask.shape[0]
    words = (n + 31) // 32
    b = np.packbits(np.concatenate([mask, np.zeros(words * 32 - n, bool)]), bitorder="little")
    return b.view(np.uint32).astype(np.uint32).view(np.int32) if words else np.zeros(0, np.int32)


def slice_bits(mask, start, stop):
    """The allow-bitmap of rows [start, stop) of a global bool mask, re-packed from that range's row 0 (one shard's
    slice; start need not be a multiple of 32)."""
    return pack_bits(np.asarray(mask, bool)[start:stop])
