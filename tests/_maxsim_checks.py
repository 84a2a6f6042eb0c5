"""Helpers of the multi-vector search tests: the numpy statement of the contract (include/revo.h, MAXSIM) from a score matrix
S [n, rows], the rows' group ids and an allow mask, in S's own precision (float32: the contract's bits; float64: the oracle)."""
import numpy as np


def group_parts(S, groups, allowed):
    """(ids [G] ascending, M [G, n], rows [G, n]) over the groups that have an allowed row: M[g, i] = the largest S[i, r]
    over the group's allowed rows (compared as numbers: -0 equals +0), rows[g, i] = the LOWEST row that attains it, and M
    holds that row's own bits."""
    S = np.asarray(S)
    groups = np.asarray(groups)
    ok = np.asarray(allowed, dtype=bool) & (groups >= 0)
    rows = np.nonzero(ok)[0]
    n = S.shape[0]
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, n), dtype=S.dtype), np.zeros((0, n), dtype=np.int64)
    order = rows[np.argsort(groups[rows], kind="stable")]            # by group, rows ascending inside a group
    g = groups[order].astype(np.int64)
    heads = np.nonzero(np.r_[True, g[1:] != g[:-1]])[0]
    ids = g[heads]
    seg = np.repeat(np.arange(heads.shape[0]), np.diff(np.r_[heads, g.shape[0]]))
    M = np.empty((ids.shape[0], n), dtype=S.dtype)
    R = np.empty((ids.shape[0], n), dtype=np.int64)
    for i in range(n):
        s = S[i, order]
        mx = np.maximum.reduceat(s, heads)
        first = np.full(ids.shape[0], order.shape[0], dtype=np.int64)
        at = np.nonzero(s == mx[seg])[0]                             # (== : -0 equals +0)
        np.minimum.at(first, seg[at], at)
        M[:, i] = s[first]
        R[:, i] = order[first]
    return ids, M, R


def ordered_sum(M):
    """(((M_0 + M_1) + M_2) + ...) + M_{n-1} per group, every addition rounded in M's precision"""
    acc = M[:, 0].copy()
    for i in range(1, M.shape[1]):
        acc = (acc + M[:, i]).astype(M.dtype)
    return acc


def exhaustive(S, groups, allowed, k, threshold=None, index_offset=0, parts=None):
    """the contract's answer: (scores [k], group_ids [k], count, part_scores [k, n], part_rows [k, n]), the best k groups by
    (score desc, group id asc) with -0 ordered as +0, threshold cut, padded with -inf / -1 / -inf / -1.  parts: the result of
    group_parts(S, groups, allowed), computed once and shared between calls that differ in k, threshold or offset."""
    S = np.asarray(S)
    n = S.shape[0]
    ids, M, R = parts if parts is not None else group_parts(S, groups, allowed)
    score = ordered_sum(M) if ids.shape[0] else np.zeros(0, dtype=S.dtype)
    keep = np.ones(ids.shape[0], dtype=bool) if threshold is None else score >= S.dtype.type(threshold)
    ids, M, R, score = ids[keep], M[keep], R[keep], score[keep]
    order = np.lexsort((ids, -(score.astype(np.float64) + 0.0)))[:k]
    m = order.shape[0]
    out_s = np.full(k, -np.inf, dtype=S.dtype)
    out_g = np.full(k, -1, dtype=np.int32)
    out_ps = np.full((k, n), -np.inf, dtype=S.dtype)
    out_pr = np.full((k, n), -1, dtype=np.int64)
    out_s[:m], out_g[:m], out_ps[:m], out_pr[:m] = score[order], ids[order], M[order], R[order] + index_offset
    return out_s, out_g, int(m), out_ps, out_pr
