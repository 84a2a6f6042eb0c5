"""Helpers of the boosted-search tests (include/revo.h, BOOSTED): a correctly rounded fp32 fused
multiply-add on the host, the exhaustive answer built from the plain search's score bits of every row, a Python restatement
of the bounds of section 4z, the strided sample's rows, and an independent fp64 evaluator of boost.py's formulas."""
import datetime
import math
from fractions import Fraction

import numpy as np

F32_MAX = Fraction(float(np.finfo(np.float32).max))
F32_OVER = F32_MAX + Fraction(2) ** 103          # half an ulp above the largest fp32: rounds to infinity from here on


def round_f32(x):
    """The fp32 nearest to the rational x, ties to even, rounded ONCE (subnormals included; +0 for an exact 0)."""
    if x == 0:
        return np.float32(0.0)
    ax = abs(x)
    if ax >= F32_OVER:
        return np.float32(math.copysign(math.inf, x))
    e = ax.numerator.bit_length() - ax.denominator.bit_length()          # 2^(e-1) <= ax < 2^(e+1)
    if Fraction(2) ** e > ax:
        e -= 1                                                            # 2^e <= ax < 2^(e+1)
    q = Fraction(2) ** (max(e, -126) - 23)                                # the spacing of fp32 numbers there
    n = round(ax / q)                                                     # Python rounds a Fraction half to even
    v = float(n) * float(q)                                               # exact: n < 2^25, q a power of two
    return np.float32(math.copysign(v, x))                                # exact in fp32 (n = 2^24 is the next binade's first)


def fma32(m, s, b):
    """fmaf(m, s, b) for fp32 arrays (or scalars): the exact rational m * s + b rounded once to fp32.  Never m * s + b in
    floating point: fp64 rounds the sum to 53 bits first, and the second rounding to 24 can then go the other way."""
    m, s, b = np.broadcast_arrays(np.asarray(m, np.float32), np.asarray(s, np.float32), np.asarray(b, np.float32))
    out = np.empty(m.shape, dtype=np.float32)
    fm, fs, fb, fo = m.ravel(), s.ravel(), b.ravel(), out.reshape(-1)
    for i in range(fm.shape[0]):
        mi, si, bi = float(fm[i]), float(fs[i]), float(fb[i])
        if not (math.isfinite(mi) and math.isfinite(si) and math.isfinite(bi)):
            fo[i] = np.float32(mi * si + bi)                              # infinities and NaN: no rounding involved
            continue
        x = Fraction(mi) * Fraction(si) + Fraction(bi)
        if x == 0:
            # an exact zero: -0 only when the product and the addend are both negative zeros
            neg = math.copysign(1.0, mi) * math.copysign(1.0, si) < 0 and math.copysign(1.0, bi) < 0 and mi * si == 0 and bi == 0
            fo[i] = np.float32(-0.0 if neg else 0.0)
        else:
            fo[i] = round_f32(x)
    return out


def final_scores(s, mult, bias):
    """final(r) of the contract from the similarities s: s itself when both arrays are None, else fmaf(m, s, b)."""
    if mult is None and bias is None:
        return s.copy()
    n = s.shape[0]
    return fma32(np.ones(n, np.float32) if mult is None else mult, s, np.zeros(n, np.float32) if bias is None else bias)


def exhaustive(s, allowed, final, k, threshold=None, min_similarity=None, index_offset=0):
    """The contract's answer from every row's similarity s and final score: the allowed rows with s >= min_similarity and
    final >= threshold, the best k by (final desc, row asc), padded with -inf / -inf / -1 -> (scores, sims, indices, count)."""
    keep = np.asarray(allowed, dtype=bool).copy()
    if min_similarity is not None:
        keep &= s >= np.float32(min_similarity)
    if threshold is not None:
        keep &= final >= np.float32(threshold)
    rows = np.nonzero(keep)[0]
    order = np.lexsort((rows, -final[rows].astype(np.float64)))[:k]
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_m = np.full(k, -np.inf, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:order.shape[0]] = final[rows[order]]
    out_m[:order.shape[0]] = s[rows[order]]
    out_i[:order.shape[0]] = rows[order] + index_offset
    return out_s, out_m, out_i, int(order.shape[0])


# ---- the bounds of DESIGN.md section 4z, restated --------------------------------------------------------------------------
_C = np.float32(4e-7)
_ONE = np.float32(1.0)


def score_down(x, ref):
    x, ref = np.float32(x), np.float32(ref)
    return np.float32(x - np.float32(_C * np.float32(_ONE + np.abs(ref))))


def score_up(x, ref):
    x, ref = np.float32(x), np.float32(ref)
    return np.float32(x + np.float32(_C * np.float32(_ONE + np.abs(ref))))


def similarity_interval(a, e):
    """[lo, hi] of section 4z step 1 from the bf16 scan score a and the rounding bound e, every operation in fp32"""
    a, e = np.float32(a), np.float32(e)
    d, u = np.float32(a - e), np.float32(a + e)
    return score_down(d, d), score_up(u, u)


def final_interval(a, e, m, b):
    """[fmaf(m, lo, b), fmaf(m, hi, b)] of step 2"""
    lo, hi = similarity_interval(a, e)
    return fma32(m, lo, b), fma32(m, hi, b)


def sample_rows(N, n_sample):
    """The rows of the strided sample (step "Sample placement"): tile i of the n_sample / 256 sample tiles is gallery tile
    floor(i T / S), T = ceil(N / 256); rows past N do not exist."""
    T, S = (N + 255) // 256, n_sample // 256
    rows = np.concatenate([np.arange(256) + 256 * (i * T // S) for i in range(S)])
    return rows[rows < N]


def rows_the_level_excludes(mult, bias, allowed, sample, k, s_abs):
    """How many allowed rows a level from `sample` certainly excludes when all that is known of the similarities is
    |lo|, |hi| <= s_abs: tau is at least the k-th largest of fmaf(m, -s_abs, b) over the allowed sample rows (steps 2 and 4),
    and a row with fmaf(m, +s_abs, b) < tau is no candidate (step 5)."""
    sample = sample[allowed[sample]]
    if sample.shape[0] < k:
        return 0
    lows = fma32(mult[sample], np.float32(-s_abs), bias[sample])
    tau = np.sort(lows)[::-1][k - 1]
    ups = fma32(mult, np.float32(s_abs), bias)
    return int((allowed & (ups < tau)).sum())


# ---- an independent fp64 evaluator of a formula at given scores ---------------------------------------------------------------
def _seconds(v):
    if isinstance(v, (int, float)):
        return float(v)
    t = datetime.datetime.fromisoformat(v.replace("Z", "+00:00"))
    if t.tzinfo is None:
        t = t.replace(tzinfo=datetime.timezone.utc)
    return (t - datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)).total_seconds()


def _get(payload, key, defaults):
    cur = payload
    for part in key.split("."):
        if not isinstance(cur, dict) or part not in cur:
            return defaults[key]
        cur = cur[part]
    return cur


def evaluate(node, payload, score, defaults=None):
    """The value of a formula for ONE point at one score, plain recursive fp64 (no symbolic split)."""
    defaults = defaults or {}
    ev = lambda n: evaluate(n, payload, score, defaults)
    if isinstance(node, (int, float)):
        return float(node)
    if isinstance(node, str):
        return float(score) if node == "$score" else float(_get(payload, node, defaults))
    (op, arg), = node.items()
    if op == "datetime":
        return _seconds(arg)
    if op == "datetime_key":
        return _seconds(_get(payload, arg, defaults))
    if op == "sum":
        return sum(ev(t) for t in arg)
    if op == "mult":
        return math.prod(ev(t) for t in arg)
    if op == "neg":
        return -ev(arg)
    if op == "div":
        den = ev(arg["right"])
        return float(arg["by_zero_default"]) if den == 0 else ev(arg["left"]) / den
    if op == "geo_distance":
        to = _get(payload, arg["to"], defaults)
        p0, l0 = math.radians(arg["origin"]["lat"]), math.radians(arg["origin"]["lon"])
        p1, l1 = math.radians(to["lat"]), math.radians(to["lon"])
        h = math.sin((p1 - p0) / 2) ** 2 + math.cos(p0) * math.cos(p1) * math.sin((l1 - l0) / 2) ** 2
        return 2 * 6371008.8 * math.asin(math.sqrt(h))
    d = abs(ev(arg["x"]) - ev(arg.get("target", 0.0)))
    scale, mid = float(arg.get("scale", 1.0)), float(arg.get("midpoint", 0.5))
    if op == "lin_decay":
        return max(0.0, 1.0 - (1.0 - mid) * d / scale)
    if op == "exp_decay":
        return math.exp(math.log(mid) * d / scale)
    if op == "gauss_decay":
        return math.exp(math.log(mid) * d * d / (scale * scale))
    raise AssertionError(op)
