"""Helpers of the diverse-search tests: the numpy fp32 statement of the greedy MMR selection (include/revo.h, MMR)."""
import numpy as np


def greedy(rel, sim, k, diversity):
    """The selection of the contract over n candidates: ``rel`` fp32 [n] (the candidates' scores, best first), ``sim`` fp32
    [n, n] (symmetric; the diagonal is never read).  Returns ``(picks, values)``: the candidate positions in pick order
    (``min(k, n)`` of them) and the fp32 value each was picked with.  Every operation is one numpy fp32 operation (numpy
    rounds each to nearest and fuses nothing): lam = 1 - diversity, v = lam * rel - diversity * m, m = the largest sim to a
    picked candidate.  Values compare as numbers (-0 = +0); among equal values the lower position wins (np.argmax returns
    the first maximum)."""
    f = np.float32
    rel = np.asarray(rel, dtype=f)
    sim = np.asarray(sim, dtype=f)
    n = rel.shape[0]
    diversity = f(diversity)
    lam = f(f(1.0) - diversity)
    lr = (lam * rel).astype(f)
    m = np.full(n, -np.inf, dtype=f)
    alive = np.ones(n, dtype=bool)
    picks, values = [], []
    for step in range(min(int(k), n)):
        v = lr if step == 0 else (lr - (diversity * m).astype(f)).astype(f)
        assert v.dtype == f
        masked = np.where(alive, v, f(-np.inf))
        # (an alive candidate whose value is -inf must still be picked before a dead one)
        p = int(np.argmax(masked)) if masked.max() > -np.inf else int(np.nonzero(alive)[0][0])
        picks.append(p)
        values.append(v[p])
        alive[p] = False
        m = np.maximum(m, sim[p]).astype(f)
    return np.array(picks, dtype=np.int64), np.array(values, dtype=f)
