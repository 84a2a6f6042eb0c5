"""Helpers of the discovery / context search tests: the numpy statement of score(r) (include/revo.h, DISCOVER).  Every
operation is one operation of the arrays' own precision (float32 in the contract; numpy rounds to nearest and fuses
nothing), in the order the header writes them."""
import numpy as np

from _recommend_checks import exhaustive  # noqa: F401  (the answer built from a score row is the same)


def fs(x):
    """x / (1 + |x|): an addition and a division"""
    one = x.dtype.type(1)
    return x / (one + np.abs(x))


def sig(st):
    """0.5 * (fs(st) + 1)"""
    t = st.dtype.type
    return t(0.5) * (fs(st) + t(1))


def ranks(SP, SN):
    """R [rows] (int64, exact) from the score matrices [pairs, rows] of the positives and the negatives"""
    if SP.shape[0] == 0:
        return np.zeros(SP.shape[1], dtype=np.int64)
    return np.where(SP > SN, 1, -1).sum(axis=0).astype(np.int64)


def discovery_score(st, SP, SN):
    """(float)R + sig(st)"""
    return (ranks(SP, SN).astype(st.dtype) + sig(st)).astype(st.dtype)


def context_loss(SP, SN):
    """loss_i [pairs, rows] = fs(min((sp_i - sn_i) - eps, 0)), eps = FLT_EPSILON in every precision"""
    t = SP.dtype.type
    return fs(np.minimum((SP - SN) - t(np.finfo(np.float32).eps), t(0)))


def context_score(SP, SN):
    """loss_0 + loss_1 + ... added in pair order starting from loss_0"""
    L = context_loss(SP, SN)
    acc = L[0].copy()
    for i in range(1, L.shape[0]):
        acc = acc + L[i]
    return acc.astype(SP.dtype)


def score(st, SP, SN):
    """the contract's score row: discovery with a target's scores st, context with st = None"""
    return context_score(SP, SN) if st is None else discovery_score(st, SP, SN)
