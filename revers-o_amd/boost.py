"""Score-boosting formulas for :meth:`GalleryStore.search_boosted`, host only.

A formula in the JSON shape of the score-boosting query of the vector database the reference sits on is turned, per stored
point, into the two numbers the device search takes (include/revo.h, BOOSTED): ``final = fma(M[r], $score, B[r])``.  The
tree is evaluated symbolically as a pair (coefficient of ``$score``, constant) in numpy fp64 over all points at once and
rounded once to fp32.  The decay functions stay on the host on purpose: they depend on the payload alone, so they are
evaluated once per (formula, state of the store) and cached there; a device evaluator is out of scope.

Nodes::

    3.5                                   a number
    "$score"                              the similarity of the point
    "key"                                 a payload number (dotted keys walk nested dicts)
    {"datetime_key": "key"}               a payload timestamp (ISO 8601 string, or a number of seconds) as seconds
    {"datetime": "2024-05-01T00:00:00Z"}  a constant timestamp as seconds
    {"sum": [..]}  {"mult": [..]}  {"neg": x}  {"div": {"left": x, "right": y, "by_zero_default": d}}
    {"geo_distance": {"origin": {"lat": .., "lon": ..}, "to": "key"}}      haversine, metres
    {"lin_decay": {"x": .., "target": 0, "scale": 1, "midpoint": 0.5}}     and exp_decay, gauss_decay

``defaults`` maps a payload key to the value of points that lack it; a missing key without a default is a ``ValueError``.

[UPSTREAM-RECALL] The node names, the decay definitions (with ``d = |x - target|``: ``lin_decay = max(0, 1 - (1 - midpoint)
d / scale)``, ``exp_decay = exp(ln(midpoint) d / scale)``, ``gauss_decay = exp(ln(midpoint) d^2 / scale^2)``), their
defaults and the earth radius of ``geo_distance`` are recalled from the database's documentation, not pinned by a fixture.
"""
import datetime as _dt
import json
import math

import numpy as np

EARTH_RADIUS_M = 6371008.8          # [UPSTREAM-RECALL] mean earth radius of the haversine distance
_DECAYS = ("lin_decay", "exp_decay", "gauss_decay")


def formula_key(formula, defaults=None):
    """A hashable key of a formula and its defaults (the store's cache key)."""
    return json.dumps([formula, defaults or {}], sort_keys=True, default=str)


def to_seconds(value):
    """A timestamp as seconds since 1970-01-01 UTC: a number is taken as seconds, a string as ISO 8601 (no zone: UTC)."""
    if isinstance(value, bool):
        raise ValueError(f"not a timestamp: {value!r}")
    if isinstance(value, (int, float, np.integer, np.floating)):
        return float(value)
    if isinstance(value, str):
        text = value.strip()
        if text.endswith(("Z", "z")):
            text = text[:-1] + "+00:00"
        try:
            t = _dt.datetime.fromisoformat(text)
        except ValueError:
            raise ValueError(f"not an ISO 8601 timestamp: {value!r}") from None
        if t.tzinfo is None:
            t = t.replace(tzinfo=_dt.timezone.utc)
        return t.timestamp()
    raise ValueError(f"not a timestamp: {value!r}")


def _lookup(payload, key):
    """(found, value) of a dotted key in a payload dict"""
    cur = payload
    for part in key.split("."):
        if not isinstance(cur, dict) or part not in cur:
            return False, None
        cur = cur[part]
    return True, cur


class _Eval:
    """One evaluation over the points that are searched, and those alone: ``payloads`` are theirs, ``ids`` their rows in the
    store (for the messages).  Every array has one entry per searched point, so no test of the tree (a coefficient that must
    be zero, a denominator that is zero) ever sees a point the search leaves out."""

    def __init__(self, payloads, defaults, ids):
        self.payloads = payloads
        self.defaults = defaults or {}
        self.n = len(payloads)
        self.ids = ids

    def const(self, c):
        return np.zeros(self.n), np.full(self.n, float(c))

    def column(self, key, convert):
        out = np.empty(self.n)
        for r in range(self.n):
            found, v = _lookup(self.payloads[r], key)
            if not found or v is None:
                if key not in self.defaults:
                    raise ValueError(f"boost: point {self.ids[r]} has no payload key {key!r} and the formula gives no default for it")
                v = self.defaults[key]
            out[r] = convert(v)
        return out

    @staticmethod
    def number(v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"boost: payload value {v!r} is not a number")
        return float(v)

    def constant_of(self, node, what):
        """a sub-expression that must not contain $score"""
        a, b = self.pair(node)
        if np.any(a != 0.0):
            raise ValueError(f"boost: {what} must not contain $score (the final score has to be affine in it)")
        return b

    def pair(self, node):
        if isinstance(node, bool):
            raise ValueError(f"boost: unknown expression {node!r}")
        if isinstance(node, (int, float)):
            return self.const(node)
        if isinstance(node, str):
            if node == "$score":
                return np.ones(self.n), np.zeros(self.n)
            return np.zeros(self.n), self.column(node, self.number)
        if not isinstance(node, dict) or len(node) != 1:
            raise ValueError(f"boost: unknown expression {node!r}")
        (op, arg), = node.items()
        if op == "datetime":
            return self.const(to_seconds(arg))
        if op == "datetime_key":
            return np.zeros(self.n), self.column(arg, to_seconds)
        if op == "sum":
            a, b = self.const(0.0)
            for term in arg:
                ta, tb = self.pair(term)
                a, b = a + ta, b + tb
            return a, b
        if op == "mult":
            a, b = self.const(1.0)
            for factor in arg:
                fa, fb = self.pair(factor)
                if np.any(a != 0.0) and np.any(fa != 0.0):
                    raise ValueError("boost: the formula is not affine in $score ($score is multiplied by $score)")
                a, b = a * fb + fa * b, b * fb
            return a, b
        if op == "neg":
            a, b = self.pair(arg)
            return -a, -b
        if op == "div":
            la, lb = self.pair(arg["left"])
            den = self.constant_of(arg["right"], "a denominator")
            zero = den == 0.0
            if np.any(zero) and "by_zero_default" not in arg:
                raise ValueError("boost: division by zero and no by_zero_default")
            safe = np.where(zero, 1.0, den)
            dflt = float(arg.get("by_zero_default", 0.0))
            return np.where(zero, 0.0, la / safe), np.where(zero, dflt, lb / safe)
        if op == "geo_distance":
            lat0, lon0 = math.radians(float(arg["origin"]["lat"])), math.radians(float(arg["origin"]["lon"]))
            lat = np.radians(self.column(arg["to"], lambda v: float(v["lat"])))
            lon = np.radians(self.column(arg["to"], lambda v: float(v["lon"])))
            h = np.sin((lat - lat0) / 2) ** 2 + math.cos(lat0) * np.cos(lat) * np.sin((lon - lon0) / 2) ** 2
            return np.zeros(self.n), 2.0 * EARTH_RADIUS_M * np.arcsin(np.sqrt(np.clip(h, 0.0, 1.0)))
        if op in _DECAYS:
            x = self.constant_of(arg["x"], "a decay argument")
            target = self.constant_of(arg.get("target", 0.0), "a decay target")
            scale, midpoint = float(arg.get("scale", 1.0)), float(arg.get("midpoint", 0.5))
            if not (scale > 0.0 and 0.0 < midpoint < 1.0):
                raise ValueError("boost: a decay needs scale > 0 and 0 < midpoint < 1")
            d = np.abs(x - target)
            if op == "lin_decay":
                v = np.maximum(0.0, 1.0 - (1.0 - midpoint) * d / scale)
            elif op == "exp_decay":
                v = np.exp(math.log(midpoint) * d / scale)
            else:
                v = np.exp(math.log(midpoint) * d * d / (scale * scale))
            return np.zeros(self.n), v
        raise ValueError(f"boost: unknown expression {op!r}")


def compile_formula(formula, payloads, defaults=None, allowed=None):
    """``(M, B)``: fp32 numpy arrays ``[len(payloads)]`` with ``formula == M * $score + B`` on every point.  ``allowed``
    (bool ``[len(payloads)]`` or None: all): the points the search will look at -- only their payload values are read (the
    others get NaN, which the device search does not inspect), and it is a ``ValueError`` if the coefficient of ``$score``
    is negative or not finite, or the constant not finite, on one of them.  A formula that is not affine in ``$score``, a
    denominator or decay argument that contains it, and a missing key without a default raise ``ValueError`` too."""
    if allowed is not None:
        allowed = np.asarray(allowed, dtype=bool)
        if allowed.shape != (len(payloads),):
            raise ValueError(f"boost: allowed must be bool [{len(payloads)}]")
    ids = np.arange(len(payloads)) if allowed is None else np.flatnonzero(allowed)
    with np.errstate(all="ignore"):
        a, b = _Eval([payloads[r] for r in ids.tolist()], defaults, ids.tolist()).pair(formula)
        m, c = a.astype(np.float32), b.astype(np.float32)
    bad = ~(np.isfinite(m) & (m >= 0) & np.isfinite(c))
    if np.any(bad):
        raise ValueError(f"boost: on {int(bad.sum())} of the points searched the coefficient of $score is negative or not finite, "
                         "or the constant is not finite (the boosted score must not decrease with the similarity)")
    m32 = np.full(len(payloads), np.nan, dtype=np.float32)
    b32 = np.full(len(payloads), np.nan, dtype=np.float32)
    m32[ids], b32[ids] = m, c
    return m32, b32
