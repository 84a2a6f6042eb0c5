"""The FUSION contract of include/revo.h in numpy, from the lists alone: fp32 scalar operations for RRF, Python float (fp64)
loops for DBSF.  `fuse` is the statement itself, one fused search at a time; `fuse_many` computes the same thing with array
operations (each still one IEEE operation per element) for the large GPU cases, and a CPU test holds it to `fuse`.

The `variant` argument of `fuse` names a plausible WRONG reading of the contract (tests/test_fusion_host.py shows that each
one differs from the contract on a hand-made fixture):
  "lists_desc"  the fused sum taken over the lists in descending order
  "fma"         the variance accumulated with a fused multiply-add
  "renumber"    ranks re-numbered after the per-list threshold cut
  "row_desc"    ties between equal fused scores go to the higher row"""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
RRF, DBSF = 0, 1


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def list_members(scores, count, t):
    """[(r, s)]: the kept entries of one list with their 1-based positions in the uncut list"""
    return [(p + 1, f32(scores[p])) for p in range(int(count)) if not (f32(scores[p]) < f32(t))]


def dbsf_stats(values, fma=False):
    """(mu, sd) of the members' scores in position order, Python floats, every operation rounded on its own"""
    n = len(values)
    S = float(values[0])
    for s in values[1:]:
        S = S + float(s)
    mu = S / n
    V = None
    for s in values:
        d = float(s) - mu
        if V is None:
            V = d * d
        else:
            V = _fma(d, d, V) if fma else V + d * d
    return mu, math.sqrt(V / n)


def contributions(members, w, method, rrf_k, variant=None):
    """[c] fp32, one per member"""
    w = f32(w)
    if method == RRF:
        out = []
        for n_th, (r, _) in enumerate(members):
            rr = n_th + 1 if variant == "renumber" else r
            out.append(f32(w / f32(f32(rrf_k) + f32(rr))))
        return out
    if not members:
        return []
    mu, sd = dbsf_stats([s for _, s in members], fma=variant == "fma")
    out = []
    for _, s in members:
        if not (sd > 0.0):
            v = f32(0.5)
        else:
            lo = mu - 3.0 * sd
            v = f32((float(s) - lo) / (6.0 * sd))
        out.append(f32(w * v))
    return out


def fuse(scores, indices, counts, k, method, rrf_k=60.0, weights=None, list_thresholds=None, threshold=None, variant=None):
    """One fused search: scores fp32 [m, C], indices int64 [m, C], counts [m].  Returns (F fp32 [k], rows int64 [k], count,
    ranks int32 [k, m]) with the contract's padding."""
    scores = np.asarray(scores, dtype=f32)
    indices = np.asarray(indices, dtype=np.int64)
    m, C = scores.shape
    weights = [1.0] * m if weights is None else weights
    list_thresholds = [-np.inf] * m if list_thresholds is None else list_thresholds
    F, ranks = {}, {}
    order = range(m - 1, -1, -1) if variant == "lists_desc" else range(m)
    with np.errstate(all="ignore"):
        for j in order:
            members = list_members(scores[j], min(int(counts[j]), C), list_thresholds[j])
            cs = contributions(members, weights[j], method, rrf_k, variant)
            for n_th, ((r, _), c) in enumerate(zip(members, cs)):
                row = int(indices[j, r - 1])
                F[row] = f32(F[row] + c) if row in F else c
                ranks.setdefault(row, {}).setdefault(j, n_th + 1 if variant == "renumber" else r)
    sign = -1 if variant == "row_desc" else 1
    cand = sorted(F, key=lambda row: (-float(F[row]), sign * row))      # -0.0 == 0.0 to Python's comparison
    if threshold is not None:
        cand = [row for row in cand if not (F[row] < f32(threshold))]
    cand = cand[:k]
    out_f = np.full(k, -np.inf, dtype=f32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_r = np.zeros((k, m), dtype=np.int32)
    for e, row in enumerate(cand):
        out_f[e], out_i[e] = F[row], row
        for j, r in ranks[row].items():
            out_r[e, j] = r
    return out_f, out_i, len(cand), out_r


def _fuse_one_fast(scores, indices, counts, k, method, rrf_k, weights, list_thresholds, threshold):
    m, C = scores.shape
    keep = [np.flatnonzero(~(scores[j, :min(int(counts[j]), C)] < f32(list_thresholds[j]))) for j in range(m)]
    rows_all = np.unique(np.concatenate([indices[j, keep[j]] for j in range(m)])) if m else np.zeros(0, np.int64)
    F = np.zeros(rows_all.shape[0], dtype=f32)
    present = np.zeros(rows_all.shape[0], dtype=bool)
    ranks = np.zeros((rows_all.shape[0], m), dtype=np.int32)
    with np.errstate(all="ignore"):
        for j in range(m):
            pos = keep[j]
            if pos.shape[0] == 0:
                continue
            s = scores[j, pos]
            w = f32(weights[j])
            if method == RRF:
                c = (w / (f32(rrf_k) + (pos + 1).astype(f32))).astype(f32)
            else:
                mu, sd = dbsf_stats(s.tolist())
                if not (sd > 0.0):
                    c = np.full(pos.shape[0], w * f32(0.5), dtype=f32)
                else:
                    lo = mu - 3.0 * sd
                    c = w * ((s.astype(np.float64) - lo) / (6.0 * sd)).astype(f32)
            at = np.searchsorted(rows_all, indices[j, pos])
            if np.unique(at).shape[0] == at.shape[0]:
                F[at] = np.where(present[at], F[at] + c, c)
                present[at] = True
                ranks[at, j] = pos + 1
            else:                                   # a row twice in one list: once per occurrence, in position order
                for a, cc, p in zip(at.tolist(), c, pos.tolist()):
                    F[a] = f32(F[a] + cc) if present[a] else cc
                    present[a] = True
                    if ranks[a, j] == 0:
                        ranks[a, j] = p + 1
    order = np.lexsort((rows_all, -(F + f32(0.0)).astype(np.float64)))   # (F + 0: -0 becomes +0)
    if threshold is not None:
        order = order[~(F[order] < f32(threshold))]
    order = order[:k]
    n = order.shape[0]
    out_f = np.full(k, -np.inf, dtype=f32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_r = np.zeros((k, m), dtype=np.int32)
    out_f[:n], out_i[:n], out_r[:n] = F[order], rows_all[order], ranks[order]
    return out_f, out_i, n, out_r


def fuse_many(scores, indices, counts, k, method, rrf_k=60.0, weights=None, list_thresholds=None, threshold=None):
    """n fused searches: scores [n, m, C], indices [n, m, C], counts [n, m] -> (F [n, k], rows [n, k], counts [n],
    ranks [n, k, m]); the result of `fuse` on each"""
    scores = np.asarray(scores, dtype=f32)
    indices = np.asarray(indices, dtype=np.int64)
    n, m, _ = scores.shape
    weights = [1.0] * m if weights is None else weights
    list_thresholds = [-np.inf] * m if list_thresholds is None else list_thresholds
    out = [_fuse_one_fast(scores[i], indices[i], counts[i], k, method, rrf_k, weights, list_thresholds, threshold)
           for i in range(n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.stack([o[3] for o in out]))


def bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)
