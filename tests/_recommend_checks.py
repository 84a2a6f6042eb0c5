"""Helpers of the search-by-examples tests: the numpy statement of score(r) (include/revo.h, RECOMMEND) and the exhaustive
answer built from a per-example score matrix."""
import numpy as np


def best_score(S, P):
    """score(r) from the fp32 (or fp64) score matrix S [P + N, rows], positives first: sp if sp > sn else -(sn * sn), each
    operation in S's own precision (numpy rounds an fp32 product to nearest and fuses nothing)."""
    sp = S[:P].max(axis=0)
    if S.shape[0] == P:
        return sp
    sn = S[P:].max(axis=0)
    return np.where(sp > sn, sp, -(sn * sn)).astype(S.dtype)


def exhaustive(score, allowed, k, threshold=None, index_offset=0):
    """the contract's answer: the best k allowed rows by (score desc, row asc), threshold cut, padded with -inf / -1"""
    rows = np.nonzero(allowed)[0]
    s = score[rows]
    if threshold is not None:
        keep = s >= np.float32(threshold)
        rows, s = rows[keep], s[keep]
    order = np.lexsort((rows, -s.astype(np.float64)))[:k]
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:order.shape[0]] = s[order]
    out_i[:order.shape[0]] = rows[order] + index_offset
    return out_s, out_i, int(order.shape[0])
