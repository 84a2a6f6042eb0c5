"""Hybrid queries (revo_search_fusion, revo_topk_fuse; include/revo.h FUSION; Gallery.search_fusion, engine.fuse_topk): the
fuse op against the numpy statement of the contract (tests/_fusion_checks.py) bit for bit over the sort sizes and list shapes;
the search against the composition of calls that existed before it plus the op; the identities of the contract; and a fixture
in which fusing matters."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fusion_checks import DBSF, RRF, bits, fuse_many  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32 = np.float32
INF = float("inf")
METHODS = {RRF: "rrf", DBSF: "dbsf"}
# m * C = 1, 1024, 2, 64, 63, 66, 64, 8192, 8192, 7000: at, below and above the sort sizes 64 .. 8192
MC = ((1, 1), (1, 1024), (2, 1), (2, 32), (3, 21), (3, 22), (64, 1), (64, 128), (8, 1024), (7, 1000))
KS = (1, 10, 1024)
RRF_KS = (0.0, 2.0, 60.0)
TOP = (1 << 47) - 1


def _weights(m, kind):
    if kind == 0:
        return None
    w = [float(f32(0.25 + 0.37 * ((j * 7) % 5))) for j in range(m)]
    if kind == 2:
        w[m // 2] = 0.0
    return w


def _desc_scores(rng, shape):
    """random scores, descending along the last axis (a sorted list), with a few exact ties"""
    s = np.sort(rng.uniform(0.05, 0.95, size=shape).astype(f32), axis=-1)[..., ::-1].copy()
    if shape[-1] >= 4:
        s[..., 2] = s[..., 1]
    return s


# ---- list shapes: (scores [n, m, C], rows [n, m, C], counts [n, m], list_thresholds or None)
def _identical(rng, n, m, C):
    s = np.repeat(_desc_scores(rng, (n, 1, C)), m, axis=1)
    rows = np.repeat(np.stack([rng.permutation(4 * C)[:C] for _ in range(n)])[:, None], m, axis=1)
    return s, rows, np.full((n, m), C), None


def _disjoint(rng, n, m, C):
    rows = (np.arange(m)[:, None] * C + np.stack([rng.permutation(C) for _ in range(m)]))[None].repeat(n, axis=0)
    return _desc_scores(rng, (n, m, C)), rows, np.full((n, m), C), None


def _half(rng, n, m, C):
    step = max(1, C // 2)
    rows = (np.arange(m)[:, None] * step + np.stack([rng.permutation(C) for _ in range(m)]))[None].repeat(n, axis=0)
    return _desc_scores(rng, (n, m, C)), rows, np.full((n, m), C), None


def _one_in_all(rng, n, m, C):
    s, rows, counts, _ = _disjoint(rng, n, m, C)
    rows = rows + 1                                      # row 0 is free: it goes into every list, at a position of its own
    for j in range(m):
        rows[:, j, (j * 5) % C] = 0
    return s, rows, counts, None


def _mixed_counts(rng, n, m, C):
    s, rows, _, _ = _half(rng, n, m, C)
    counts = np.array([[(0, 1, C)[(i + j) % 3] for j in range(m)] for i in range(n)])
    return s, rows, counts, None


def _unsorted_thr(rng, n, m, C):
    s = rng.uniform(-0.3, 0.9, size=(n, m, C)).astype(f32)
    rows = np.stack([np.stack([rng.permutation(max(2, 2 * C))[:C] for _ in range(m)]) for _ in range(n)])
    thr = [(-INF, 0.2, 0.5, INF)[j % 4] if m > 1 else 0.2 for j in range(m)]
    return s, rows, np.full((n, m), C), thr


def _high_idx(rng, n, m, C):
    s, rows, counts, _ = _half(rng, n, m, C)
    return s, rows + (TOP - int(rows.max())), counts, None


def _few_rows(rng, n, m, C):
    rows = rng.integers(0, 3, size=(n, m, C))            # three distinct rows, repeated inside the lists
    return _desc_scores(rng, (n, m, C)), rows, np.full((n, m), C), None


def _nine_one(rng, n, m, C):
    """DBSF noise: nine equal scores and one exactly 3 sd below the mean in real arithmetic (v = rounding noise alone)"""
    s, rows, counts, _ = _half(rng, n, m, C)
    a = rng.uniform(0.3, 0.9, size=(n, m)).astype(f32)
    s[:, :, :9] = a[:, :, None]
    s[:, :, 9] = (a - rng.uniform(0.05, 0.25, size=(n, m)).astype(f32))
    return s, rows, np.full((n, m), 10), None


def _straddle(rng, n, m, C):
    """Runs laid across the boundaries of the sorted key array: rows 0 .. 62 in one list each, row 63 in every list (its run
    starts at key position 63, the last lane of a wave), single rows up to key position 1022, then a row of every list
    starting at 1023 (where m * C reaches that far)."""
    total = m * C
    lists = [[] for _ in range(m)]
    state = {"row": 0, "at": 0, "j": 0}

    def singles(until):
        while state["at"] < until:
            for _ in range(m):
                j = state["j"] = (state["j"] + 1) % m
                if len(lists[j]) < C:
                    break
            else:
                return
            lists[j].append(state["row"])
            state["row"] += 1
            state["at"] += 1

    def shared():
        if all(len(l) < C for l in lists):
            for l in lists:
                l.append(state["row"])
            state["row"] += 1
            state["at"] += m

    if m > 1 and total >= 63 + m:
        singles(63)
        shared()
        if total >= 1023 + m:
            singles(1023)
            shared()
    singles(total)
    counts = np.array([len(l) for l in lists])
    rows = np.zeros((m, C), dtype=np.int64)
    for j, l in enumerate(lists):
        rows[j, :len(l)] = rng.permutation(np.array(l, dtype=np.int64)) if l else []
    return _desc_scores(rng, (n, m, C)), rows[None].repeat(n, axis=0), counts[None].repeat(n, axis=0), None


SHAPES = (_identical, _disjoint, _half, _one_in_all, _mixed_counts, _unsorted_thr, _high_idx, _straddle, _few_rows, _nine_one)


def _run_op(s, rows, counts, k, method, rrf_k, weights, thr, fused_thr):
    got = engine.fuse_topk(torch.from_numpy(s).to(DEV), torch.from_numpy(rows.astype(np.int64)).to(DEV),
                           torch.from_numpy(counts.astype(np.int32)).to(DEV), k=k, method=METHODS[method], rrf_k=rrf_k,
                           weights=weights, list_thresholds=thr, score_threshold=fused_thr)
    return tuple(t.cpu().numpy() for t in got)


def _assert_op(got, want, what):
    gs, gi, gc, gr = got
    ws, wi, wc, wr = want
    assert np.array_equal(gc, wc), (what, gc[:8], wc[:8])
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:4])
    bad = np.argwhere(bits(gs) != bits(ws))
    assert bad.shape[0] == 0, (what, bad[:4], gs[tuple(bad[0])], ws[tuple(bad[0])])
    assert np.array_equal(gr, wr), (what, np.argwhere(gr != wr)[:4])


@pytest.mark.parametrize("method", (RRF, DBSF), ids=("rrf", "dbsf"))
@pytest.mark.parametrize("mc", MC, ids=lambda mc: f"m{mc[0]}xC{mc[1]}")
def test_fuse_op_equals_the_statement(mc, method):
    """Every list shape at one (m, C): k, n, rrf_k and the weights rotate with the shape so that each value meets each sort
    size; n = 130 where a fused search is small, 3 or 1 where it holds thousands of members."""
    m, C = mc
    rng = np.random.default_rng(1000 * m + C + method)
    big = m * C > 1024
    for si, shape in enumerate(SHAPES):
        if shape is _nine_one and C < 10:
            continue
        n = (1, 3)[si % 2] if big else (130, 3, 1)[si % 3]
        k = KS[(si + m) % 3]
        rrf_k = RRF_KS[(si + C) % 3]
        weights = _weights(m, (si + m + C) % 3)
        s, rows, counts, thr = shape(rng, n, m, C)
        fused_thr = None if si % 4 else (0.004 if method == RRF else 0.3)
        want = fuse_many(s, rows, counts, k, method, rrf_k=rrf_k, weights=weights, list_thresholds=thr, threshold=fused_thr)
        got = _run_op(s, rows, counts, k, method, rrf_k, weights, thr, fused_thr)
        _assert_op(got, want, (shape.__name__, n, k, rrf_k, weights is not None))


@pytest.mark.parametrize("mc,k", (((2, 32), 10), ((3, 22), 1024), ((64, 128), 10)), ids=("m2xC32", "m3xC22", "m64xC128"))
def test_fuse_op_many_searches(mc, k):
    """n = 130 at a small, an odd and the largest sort size: a workgroup per fused search, none reads its neighbour's lists"""
    m, C = mc
    rng = np.random.default_rng(7 + m)
    s, rows, counts, _ = _half(rng, 130, m, C)
    rows = np.stack([rows[i] + 3 * i for i in range(130)])
    counts = rng.integers(0, C + 1, size=(130, m))
    for method in (RRF, DBSF):
        want = fuse_many(s, rows, counts, k, method, rrf_k=2.0, weights=_weights(m, 1))
        _assert_op(_run_op(s, rows, counts, k, method, 2.0, _weights(m, 1), None, None), want, (m, C, method))


def test_fuse_op_corner_values():
    """-0 and +0 tie and keep their sign; a weight-0 list's rows are candidates with F = 0; a count above C counts as C; a row
    twice in one list; all lists empty; two calls give identical bytes."""
    s = np.array([[[0.9] * 10 + [0.1, 0.0]]], dtype=f32)
    rows = np.array([[list(range(5, 15)) + [2, 99]]])
    got = _run_op(s, rows, np.array([[11]]), 12, DBSF, 60.0, [0.0], None, None)
    assert got[1][0].tolist() == [2] + list(range(5, 15)) + [-1] and got[2][0] == 11
    assert np.signbit(got[0][0][:11]).tolist() == [True] + [False] * 10 and np.isneginf(got[0][0][11])
    _assert_op(got, fuse_many(s, rows, np.array([[11]]), 12, DBSF, weights=[0.0]), "neg zero")
    got = _run_op(s, rows, np.array([[4000]]), 12, RRF, 60.0, None, None, None)       # a count above C
    _assert_op(got, fuse_many(s, rows, np.array([[12]]), 12, RRF), "count above C")
    dup = np.array([[[4, 4, 2, 4]], [[1, 1, 1, 1]]])
    sd = np.array([[[0.9, 0.8, 0.7, 0.6]], [[0.5, 0.5, 0.5, 0.5]]], dtype=f32)
    for method in (RRF, DBSF):
        _assert_op(_run_op(sd, dup, np.full((2, 1), 4), 3, method, 0.0, None, None, None),
                   fuse_many(sd, dup, np.full((2, 1), 4), 3, method, rrf_k=0.0), ("duplicates", method))
    got = _run_op(sd, dup, np.zeros((2, 1)), 3, RRF, 60.0, None, None, None)
    assert got[2].tolist() == [0, 0] and (got[1] == -1).all() and np.isneginf(got[0]).all() and (got[3] == 0).all()
    rng = np.random.default_rng(3)
    s, rows, counts, thr = _unsorted_thr(rng, 3, 8, 1024)
    a = _run_op(s, rows, counts, 1024, DBSF, 60.0, _weights(8, 2), thr, 0.2)
    b = _run_op(s, rows, counts, 1024, DBSF, 60.0, _weights(8, 2), thr, 0.2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # no ranks asked for: the same three outputs
    c = engine.fuse_topk(torch.from_numpy(s).to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(counts.astype(np.int32)).to(DEV),
                         k=1024, method="dbsf", weights=_weights(8, 2), list_thresholds=thr, score_threshold=0.2, with_ranks=False)
    assert len(c) == 3 and all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(c, a[:3]))


# ---- the search -----------------------------------------------------------------------------------------------------------
def _planted(N, D, seed):
    """tests/test_gpu_mmr.py::_planted: random directions and clusters of perturbed copies of a few of them"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(f32)
    if N < 2:
        return x
    rows = rng.permutation(N)
    at = 0
    for _ in range(max(1, N // 40)):
        size = int(rng.integers(2, 7))
        if at + size > N:
            break
        members = rows[at:at + size]
        at += size
        c = rng.standard_normal(D).astype(f32)
        c /= np.linalg.norm(c)
        for r in members:
            x[r] = c + rng.uniform(0.22, 0.45) * rng.standard_normal(D).astype(f32) / np.sqrt(D)
    return x


def _gallery(x):
    G = engine.Gallery(x.shape[1], max(1, x.shape[0]), device=0)
    if x.shape[0]:
        G.add(torch.from_numpy(x).to(DEV))
    return G


def _queries(x, n, m, seed):
    """[n, m, D]: perturbed gallery rows; list 1 of a search looks at the same row as list 0 from further away (overlap)"""
    rng = np.random.default_rng(seed)
    D = x.shape[1]
    pick = rng.integers(0, x.shape[0], (n, m))
    pick[:, 1:2] = pick[:, 0:1]
    q = x[pick] / np.linalg.norm(x[pick], axis=-1, keepdims=True)
    q = q + rng.uniform(0.05, 0.6, size=(n, m, 1)).astype(f32) * rng.standard_normal((n, m, D)).astype(f32) / np.sqrt(D)
    return torch.from_numpy(q.astype(f32)).to(DEV)


def _composition(G, q, k, C, method, rrf_k=60.0, weights=None, thr=None, fused_thr=None, allow=None, index_offset=0):
    """the contract's answer from Gallery.search per list and the fuse op: (scores, indices, counts, ranks, lists)"""
    n, m, _ = q.shape
    ls, li, lc = G.search(q.reshape(n * m, -1), k=C, allow=allow)
    ls, li, lc = ls.reshape(n, m, C), li.reshape(n, m, C), lc.reshape(n, m)
    s, i, c, r = engine.fuse_topk(ls, li, lc, k=k, method=method, rrf_k=rrf_k, weights=weights, list_thresholds=thr,
                                  score_threshold=fused_thr)
    i = torch.where(i >= 0, i + index_offset, i)
    return (s, i, c, r), (ls, li, lc)


def _assert_same(got, want, what):
    for name, g, w in zip(("scores", "indices", "counts", "ranks"), got, want):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (what, name)


@pytest.mark.parametrize("D", (64, 1024))
@pytest.mark.parametrize("R", (1, 255, 257, 20_037))
def test_search_equals_search_per_list_plus_the_op(R, D):
    x = _planted(R, D, seed=R + D)
    G = _gallery(x)
    n, m = 3, 3
    q = _queries(x, n, m, seed=R)
    allow = torch.from_numpy(np.random.default_rng(R).random(R) < 0.6).to(DEV) if R > 1 else None
    cases = [dict(k=10, C=100, method="rrf"), dict(k=10, C=100, method="dbsf", weights=[1.0, 0.5, 2.0]),
             dict(k=1024, C=50, method="dbsf", allow=allow, thr=[-INF, 0.05, 0.3]),
             dict(k=5, C=21, method="rrf", rrf_k=2.0, allow=allow, index_offset=(1 << 40) + 3, fused_thr=0.3),
             dict(k=64, C=1024, method="dbsf", fused_thr=0.45, index_offset=7, weights=[0.0, 1.0, 1.0])]
    for case in cases:
        kw = dict(case)
        k, C, method = kw.pop("k"), kw.pop("C"), kw.pop("method")
        want, (ls, li, lc) = _composition(G, q, k, C, method, **kw)
        got = G.search_fusion(q, k=k, limit=C, method=method, rrf_k=kw.get("rrf_k", 60.0), weights=kw.get("weights"),
                              list_thresholds=kw.get("thr"), score_threshold=kw.get("fused_thr"),
                              index_offset=kw.get("index_offset", 0), allow=kw.get("allow"), with_list_scores=True)
        _assert_same(got[:4], want, (R, D, case))
        # list_scores: the inner search's bits where the row is a member of the list (cut by its threshold or not) ...
        s, i, c, ranks, lsc = (t.cpu().numpy() for t in got)
        ls, li, lc = ls.cpu().numpy(), li.cpu().numpy(), lc.cpu().numpy()
        full = None
        if R <= 257:      # ... and Gallery.search(k = rows)'s bits everywhere (every allowed row is in that result)
            fs, fi, fc = (t.cpu().numpy() for t in G.search(q.reshape(n * m, -1), k=R, allow=kw.get("allow")))
            full = [{int(r): sc for r, sc in zip(fi[a, :fc[a]], fs[a, :fc[a]])} for a in range(n * m)]
        off = kw.get("index_offset", 0)
        for a in range(n):
            assert np.isneginf(lsc[a, c[a]:]).all() and (ranks[a, c[a]:] == 0).all()
            for e in range(int(c[a])):
                row = int(i[a, e]) - off
                for j in range(m):
                    at = np.flatnonzero(li[a, j, :lc[a, j]] == row)
                    if at.size:
                        assert bits(lsc[a, e, j]) == bits(ls[a, j, at[0]]), (R, D, case, a, e, j)
                        cut = kw.get("thr") is not None and ls[a, j, at[0]] < f32(kw["thr"][j])
                        assert ranks[a, e, j] == (0 if cut else at[0] + 1)
                    else:
                        assert ranks[a, e, j] == 0
                    if full is not None:
                        assert bits(lsc[a, e, j]) == bits(full[a * m + j][row]), (R, D, case, a, e, j)
    G.close()


def test_more_lists_than_one_chunk_of_the_inner_search():
    """n * m = 1040 queries: the inner large-k search runs them in chunks of 1024 and reuses its normalised query rows, the
    list_scores kernel needs all of them"""
    x = _planted(4000, 64, seed=5)
    G = _gallery(x)
    q = _queries(x, 130, 8, seed=6)
    want, (ls, li, lc) = _composition(G, q, 10, 20, "rrf")
    got = G.search_fusion(q, k=10, limit=20, with_list_scores=True)
    _assert_same(got[:4], want, "1040 lists")
    s, i, c, ranks, lsc = (t.cpu().numpy() for t in got)
    ls, r = ls.cpu().numpy(), ranks.astype(np.int64)
    member = r > 0
    inner = ls[np.arange(130)[:, None, None], np.arange(8)[None, None, :], np.maximum(r - 1, 0)]     # [a, e, j] = ls[a, j, r - 1]
    assert member.any() and np.array_equal(bits(lsc)[member], bits(inner)[member])
    G.close()


def test_identities():
    x = _planted(20_037, 1024, seed=21)
    G = _gallery(x)
    q = _queries(x, 3, 2, seed=22)
    one = q[:, :1].contiguous()
    ps, pi, pc = G.search(one[:, 0], k=100)
    # m = 1, RRF: the list's first k rows in order, for every weight > 0 and rrf_k <= 60
    for rrf_k, w in ((0.0, 1.0), (60.0, 0.25), (2.0, 3.0)):
        s, i, c, r = G.search_fusion(one, k=10, limit=100, rrf_k=rrf_k, weights=[w])
        assert torch.equal(i, pi[:, :10]) and bool((c == 10).all()) and torch.equal(r[:, :, 0].cpu(), torch.arange(1, 11).expand(3, 10).int())
        want = (f32(w) / (f32(rrf_k) + np.arange(1, 11).astype(f32))).astype(f32)
        assert np.array_equal(bits(s.cpu().numpy()), bits(np.tile(want, (3, 1))))
    # the same query twice with equal weights: the single list's order
    twice = torch.cat([one, one], dim=1)
    for method in ("rrf", "dbsf"):
        s, i, c, r = G.search_fusion(twice, k=100, limit=100, method=method)
        assert torch.equal(i, pi) and torch.equal(r[:, :, 0], r[:, :, 1])
    # two calls: identical bytes
    a = G.search_fusion(q, k=50, limit=1024, method="dbsf", with_list_scores=True)
    b = G.search_fusion(q, k=50, limit=1024, method="dbsf", with_list_scores=True)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    # [m, dim] is one fused search; outputs that were not asked for are not returned
    s1 = G.search_fusion(q[0], k=50, limit=1024, method="dbsf", with_ranks=False)
    assert len(s1) == 3 and torch.equal(s1[0][0], a[0][0]) and torch.equal(s1[1][0], a[1][0])
    G.close()


def test_errors_empty_gallery_stats_and_results_that_survive():
    from reverso_amd import _lib
    D = 1024
    x = _planted(20_037, D, seed=51)
    q = _queries(x, 3, 2, seed=52)
    G0 = engine.Gallery(D, 300, device=0, keep_f32=False)
    G0.add(torch.from_numpy(x[:300]).to(DEV))
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.search_fusion(q, k=5)
    G0.close()

    def all_padding(out):
        s, i, c, r, ls = out
        return (bool((c == 0).all()) and bool((i == -1).all()) and bool((r == 0).all()) and bool(torch.isinf(s).all())
                and bool((s < 0).all()) and bool(torch.isinf(ls).all()) and bool((ls < 0).all()))

    E = engine.Gallery(D, 16, device=0)
    assert all_padding(E.search_fusion(q, k=7, limit=20, with_list_scores=True))
    E.close()
    G = _gallery(x)
    for kw, word in (({"k": 0}, "k must"), ({"limit": 1025}, "1024"), ({"limit": 0}, "1024"), ({"rrf_k": -1.0}, "rrf_k"),
                     ({"weights": [1.0, -1.0]}, "weight"), ({"list_thresholds": [0.0, float("nan")]}, "list threshold"),
                     ({"score_threshold": float("nan")}, "NaN")):
        with pytest.raises(RuntimeError, match=word):
            G.search_fusion(q, **kw)
    with pytest.raises(ValueError, match="method"):
        G.search_fusion(q, method="sum")
    with pytest.raises(ValueError, match="one entry per list"):
        G.search_fusion(q, weights=[1.0])
    with pytest.raises(RuntimeError, match="8192"):
        G.search_fusion(torch.zeros(1, 9, D, device=DEV), limit=1024)
    # nothing allowed
    assert all_padding(G.search_fusion(q, k=7, limit=20, allow=torch.zeros(len(G), dtype=torch.bool, device=DEV),
                                       with_list_scores=True))
    # the stats are the inner large-k search's; a pairs and a range result held by the handle are still readable
    pairs, ps = G.pairs(0.93)
    off, ridx, rsc = G.search_range(q[:2, 0], 0.5)
    G.search_fusion(q, k=50, limit=1024, method="dbsf", with_list_scores=True)
    st = G.search_stats()
    G.search(q.reshape(6, D), k=1024)
    assert st == G.search_stats() and st["collected_rows"] >= 6 * 1024
    p2, ps2 = torch.empty_like(pairs), torch.empty_like(ps)
    _lib.check(G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert pairs.shape[0] > 0 and torch.equal(p2, pairs) and torch.equal(ps2, ps)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(G._lib.revo_search_range_read(G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)
    G.close()


def test_fusion_finds_what_neither_raw_combination_finds():
    """Two query directions u (an image: cosines of 0.8 to 0.9) and v (words: the same evidence in a low band, cosines below
    0.3).  Rows near u only, rows near v only, and five near both -- further from u than the u-only rows are.  The both-rows
    lead under RRF and DBSF; the search of normalize(u + v), the averaged vector, ranks a u-only row first, and so does the
    sum of the two raw scores."""
    D, N = 1024, 6000
    rng = np.random.default_rng(77)
    u, v = np.linalg.qr(rng.standard_normal((D, 2)))[0].T.astype(f32)
    x = rng.standard_normal((N, D)).astype(f32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)          # the other rows: cosines of about +-0.03 with u and v

    def row(cu, cv, r):
        noise = x[r] - (x[r] @ u) * u - (x[r] @ v) * v
        return cu * u + cv * v + np.sqrt(1.0 - cu * cu - cv * cv) * noise / np.linalg.norm(noise)

    u_only, v_only, both = np.arange(100, 140), np.arange(200, 240), np.arange(300, 305)
    for t, r in enumerate(u_only):
        x[r] = row(0.90 - 0.002 * t, 0.0, r)
    for t, r in enumerate(v_only):
        x[r] = row(0.0, 0.30 - 0.002 * t, r)
    for t, r in enumerate(both):
        x[r] = row(0.62 - 0.002 * t, 0.26 - 0.002 * t, r)
    G = _gallery(x)
    q = torch.from_numpy(np.stack([u, v])[None]).to(DEV)
    for method in ("rrf", "dbsf"):
        s, i, c, r = G.search_fusion(q, k=5, limit=100, method=method)
        assert sorted(i[0].tolist()) == both.tolist(), (method, i)
        assert bool((r[0] > 0).all())
    mean = torch.from_numpy(((u + v) / np.linalg.norm(u + v))[None]).to(DEV)
    _, mi, _ = G.search(mean, k=5)
    assert int(mi[0, 0]) in u_only.tolist()
    s, i, c, r, ls = G.search_fusion(q, k=50, limit=100, with_list_scores=True)
    raw = ls[0, :int(c[0])].sum(-1)
    assert int(i[0, int(raw.argmax())]) in u_only.tolist()
    G.close()
