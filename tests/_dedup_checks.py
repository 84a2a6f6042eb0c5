"""Shared by the tests of the deduplicating append (revo_gallery_append_unique, include/revo.h DEDUP): the video-like input
generator and the numpy statement of the greedy selection -- rows decided in order, a row is dropped when a gallery row or an
earlier KEPT batch row scores >= t against it, and its representative is the lowest such row (first seen wins)."""
import numpy as np


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def video_like(N, n, D, seed):
    """(gallery [N, D], batch [n, D]) fp32.  The gallery: random directions with planted clusters of perturbed copies.  The
    batch, in runs of 3 to 39 frames: static shots (perturbed copies of one centre, sigma 0.05 .. 0.5), slow pans (each frame the
    previous one plus noise: chains), exact repeats (every second one rescaled), near and exact copies of gallery rows (fresh
    content instead when the gallery is empty), and fresh content."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((N, D)).astype(np.float32)
    for _ in range(N // 40):
        ctr = _unit(rng.standard_normal(D))
        for r in rng.choice(N, size=int(rng.integers(2, 6)), replace=False):
            g[r] = ctr + rng.uniform(0.22, 0.45) * rng.standard_normal(D) / np.sqrt(D)
    b = []
    while len(b) < n:
        kind = int(rng.integers(5))
        L = int(rng.integers(3, 40))
        if kind == 0:
            ctr = _unit(rng.standard_normal(D))
            s = rng.uniform(0.05, 0.5)
            b += [ctr + s * rng.standard_normal(D) / np.sqrt(D) for _ in range(L)]
        elif kind == 1:
            x = _unit(rng.standard_normal(D))
            s = rng.uniform(0.1, 0.25)
            for _ in range(L):
                b.append(x.copy())
                x = _unit(x + s * rng.standard_normal(D) / np.sqrt(D))
        elif kind == 2:
            x = rng.standard_normal(D)
            b += [x * rng.uniform(0.5, 3) if i % 2 else x.copy() for i in range(L)]
        elif kind == 3 and N > 0:
            for _ in range(L):
                r = int(rng.integers(N))
                s = 0 if rng.integers(2) else rng.uniform(0.05, 0.5)
                b.append(g[r] + s * np.linalg.norm(g[r]) * rng.standard_normal(D) / np.sqrt(D))
        else:
            b += [rng.standard_normal(D) for _ in range(L)]
    return g, np.asarray(b[:n], dtype=np.float32)


def greedy_lists(N, n, neighbours):
    """neighbours[j]: iterable of (row, score) over the rows `row` < N + j (gallery rows 0 .. N - 1, batch row i as N + i) whose
    score against batch row j is >= t.  Returns (kept bool [n], rep int64 [n], rep_score [n]): rep = the representative in that
    numbering, -1 for a kept row; rep_score = the score given with it (dtype of the scores; -inf for a kept row)."""
    kept = np.zeros(n, dtype=bool)
    rep = np.full(n, -1, dtype=np.int64)
    rep_score = [-np.inf] * n
    for j in range(n):
        best = None
        for row, score in neighbours[j]:
            row = int(row)
            assert 0 <= row < N + j
            if row >= N and not kept[row - N]:
                continue                                   # a dropped row never suppresses a later one
            if best is None or row < best[0]:
                best = (row, score)
        if best is None:
            kept[j] = True
        else:
            rep[j], rep_score[j] = best
    return kept, rep, np.asarray(rep_score)


def greedy_dense(S, N, t):
    """the same over a dense score matrix S [N + n, N + n] (gallery rows first); only S[N + j, : N + j] is read"""
    n = S.shape[0] - N
    lists = []
    for j in range(n):
        row = S[N + j, :N + j]
        hit = np.flatnonzero(row >= t)
        lists.append([(int(r), row[r]) for r in hit])
    return greedy_lists(N, n, lists)


def greedy_pairs(N, n, pairs, scores):
    """the same from an edge list: pairs [m, 2] (i < j) with their scores, every pair of the N + n rows that reaches t"""
    lists = [[] for _ in range(n)]
    for (i, j), s in zip(np.asarray(pairs).tolist(), np.asarray(scores)):
        assert i < j
        if j >= N:
            lists[j - N].append((i, s))
    return greedy_lists(N, n, lists)


def final_rows(N, kept, rep):
    """rows [n] int64 as the call reports them: a kept row's new index N + (kept rows before it), a dropped row's
    representative's final index"""
    new = N + np.cumsum(kept) - kept                       # (for kept rows)
    out = np.where(kept, new, 0).astype(np.int64)
    for j in np.flatnonzero(~kept):
        out[j] = rep[j] if rep[j] < N else new[rep[j] - N]
    return out


def teeth(S, N, t, kept, rep):
    """(rows kept although an earlier DROPPED batch row scores >= t against them, dropped rows whose representative is not
    their best-scoring member of D_j) -- what tells first-seen leader selection from its two plausible mistakes"""
    n = S.shape[0] - N
    naive = notbest = 0
    for j in range(n):
        row = S[N + j]
        if kept[j]:
            naive += bool(np.any(row[N:N + j] >= t))
        else:
            d = np.concatenate([np.flatnonzero(row[:N] >= t), N + np.flatnonzero((row[N:N + j] >= t) & kept[:j])])
            notbest += bool(row[d].max() > row[rep[j]])
    return naive, notbest
