"""Search by examples (revo_search_recommend, include/revo.h RECOMMEND; Gallery.recommend, GalleryStore.recommend,
SimpleReverso.search_by_examples): bit for bit against a composition of the range search (every example's score of every
row, the one fp32 chain) with the formula in numpy, the identities of the contract, an fp64 oracle of the fp32 rows, planted
rows that only the rounding bound keeps, filters, thresholds, ties, errors, the stats, the store and the facade."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _recommend_checks import best_score, exhaustive  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KS = (1, 10, 50, 51, 1024)


def _delta(D):
    """the fp32 chain's band: 3e-7 at D = 1024 (test_gpu_search.py), scaled with D, never below that"""
    return 3e-7 * max(1.0, D / 1024)


def _planted(N, D, seed, n_clusters=None):
    """tests/test_gpu_range_search.py::_planted: random directions and clusters of perturbed copies of a few of them"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    if N < 2:
        return x
    n_clusters = n_clusters if n_clusters is not None else max(1, N // 40)
    rows = rng.permutation(N)
    at = 0
    for _ in range(n_clusters):
        size = int(rng.integers(2, 7))
        if at + size > N:
            break
        members = rows[at:at + size]
        at += size
        c = rng.standard_normal(D).astype(np.float32)
        c /= np.linalg.norm(c)
        for r in members:
            sigma = rng.uniform(0.22, 0.45)
            x[r] = c + sigma * rng.standard_normal(D).astype(np.float32) / np.sqrt(D)
    return x


def _gallery(x, keep_f32=True):
    G = engine.Gallery(x.shape[1], max(1, x.shape[0]), device=0, keep_f32=keep_f32)
    if x.shape[0]:
        G.add(torch.from_numpy(x).to(DEV))
    return G


def _normalised(q):
    """the fp32 example rows the library scores (the same normalisation kernel as an append)"""
    T = engine.Gallery(q.shape[1], q.shape[0], device=0)
    T.add(q)
    r = T.read()
    T.close()
    return r


def _examples(x, n, seed):
    """n examples: perturbed gallery rows"""
    rng = np.random.default_rng(seed)
    src = x[rng.integers(0, x.shape[0], n)]
    q = src / np.linalg.norm(src, axis=1, keepdims=True)
    q = q + 0.2 * rng.standard_normal(q.shape).astype(np.float32) / np.sqrt(x.shape[1])
    return torch.from_numpy(q.astype(np.float32)).to(DEV)


def _chain_scores(G, ex, allow=None):
    """S [examples, rows] fp32: every example's score of every row from the range search (parent-commit code, the one
    chain); rows the filter does not allow stay at -inf"""
    off, idx, sc = G.search_range(ex, -2.0, allow=allow)
    E, N = ex.shape[0], len(G)
    S = torch.full((E, N), -np.inf, dtype=torch.float32, device=DEV)
    cnt = (off[1:] - off[:-1]).to(torch.int64)
    qe = torch.repeat_interleave(torch.arange(E, device=DEV), cnt)
    S[qe, idx] = sc
    return S.cpu().numpy()


def _allowed(G, allow):
    return np.ones(len(G), dtype=bool) if allow is None else allow.cpu().numpy()


def _assert_equals(got, want, what=""):
    s, i, c = got
    ws, wi, wc = want
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert int(c) == wc, (what, int(c), wc)
    assert np.array_equal(i, wi), (what, np.nonzero(i != wi)[0][:10], i[:12], wi[:12])
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (what, np.nonzero(s != ws)[0][:10])


def _check_composition(G, pos, neg, ks=KS, allow=None, threshold=None, index_offset=0):
    """check 1: the call against the formula over the range search's scores; no tolerance.  Returns the fp32 score row."""
    ex = pos if neg is None else torch.cat([pos, neg])
    score = best_score(_chain_scores(G, ex, allow), pos.shape[0])
    for k in ks:
        got = G.recommend(pos, neg, k=k, score_threshold=threshold, index_offset=index_offset, allow=allow)
        _assert_equals(got, exhaustive(score, _allowed(G, allow), k, threshold, index_offset), f"k={k}")
    return score


def _stats_are_the_recommend_search(G, passes=1):
    st = G.search_stats()
    assert st["join_passes"] == passes, st
    assert st["uncertified"] == st["bruteforced"] == st["checked"] == st["from_segments"] == 0, st
    assert st["grouped_fallback"] == st["large_k_fallback"] == 0, st
    return st["collected_rows"]


# ---- 1. bit for bit against the composition --------------------------------------------------------------------------------
_PN = [(1, 0), (1, 1), (4, 2), (64, 0), (63, 1), (64, 64), (100, 28)]
_CASES = [(P, N, 20_037, [64, 768, 1024, 1280][i % 4]) for i, (P, N) in enumerate(_PN)]
_CASES += [(4, 2, 20_037, D) for D in (64, 768, 1280)] + [(100, 28, 20_037, 64), (1, 0, 20_037, 1280)]
_CASES += [(P, N, R, 1024) for R in (1, 255, 256, 257) for (P, N) in ((4, 2), (100, 28))]


@pytest.mark.parametrize("P,N,R,D", _CASES)
def test_equals_the_composition_bit_for_bit(P, N, R, D):
    x = _planted(R, D, seed=R + D + P + N)
    G = _gallery(x)
    ex = _examples(x, P + N, seed=P * 131 + N)
    pos, neg = ex[:P], (ex[P:] if N else None)
    score = _check_composition(G, pos, neg)
    n = _stats_are_the_recommend_search(G)
    assert n >= min(R, 1024)
    # the level does its work: a k = 10 request re-scores a small part of a large gallery
    if R > 20_000:
        G.recommend(pos, neg, k=10)
        assert _stats_are_the_recommend_search(G) < R // 4
    # two calls: identical bytes
    a = G.recommend(pos, neg, k=51)
    b = G.recommend(pos, neg, k=51)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and int(a[2]) == int(b[2])
    assert score.shape == (R,)
    G.close()


# ---- 2. the identities of the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 1024])
def test_one_positive_is_the_plain_search(D):
    x = _planted(20_037, D, seed=5 + D)
    G = _gallery(x)
    ex = _examples(x, 3, seed=7)
    for e in range(3):
        for k in KS + (300,):
            s, i, c = G.search(ex[e:e + 1], k=k)
            _assert_equals(G.recommend(ex[e:e + 1], None, k=k), (s[0].cpu().numpy(), i[0].cpu().numpy(), int(c[0])), f"k={k}")
    G.close()


def test_no_negatives_is_the_merge_of_the_single_searches():
    x = _planted(20_037, 768, seed=11)
    G = _gallery(x)
    P = 6
    ex = _examples(x, P, seed=12)
    for k in (10, 1024):
        best = {}
        for e in range(P):
            s, i, c = G.search(ex[e:e + 1], k=k)
            for sv, iv in zip(s[0, :int(c[0])].cpu().numpy(), i[0, :int(c[0])].cpu().numpy()):
                best[int(iv)] = max(best.get(int(iv), -np.inf), float(sv))
        rows = np.array(sorted(best), dtype=np.int64)
        sc = np.array([best[int(r)] for r in rows], dtype=np.float32)
        order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
        s, i, c = G.recommend(ex, None, k=k)
        assert int(c) == k
        assert np.array_equal(i.cpu().numpy(), rows[order])
        assert np.array_equal(s.cpu().numpy().view(np.uint32), sc[order].view(np.uint32))
    G.close()


# ---- 3. the fp64 oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,D", [(4, 2, 64), (32, 32, 768), (1, 1, 1024), (100, 28, 1280), (5, 0, 1024)])
def test_matches_the_fp64_oracle(P, N, D):
    """Independent of the library's chain: fp64 scores of the fp32 rows.  Rows with |sp - sn| <= 2 delta sit on the jump of the
    formula and are left out; at most 0.1 % of the rows may (20 of 20 037; the count is printed, and asserted against that
    cap; observed with these generators: 0, 1, 0, 0, 0 rows over the five cases)."""
    R = 20_037
    x = _planted(R, D, seed=D + P)
    G = _gallery(x)
    ex = _examples(x, P + N, seed=P + 17 * N)
    rows = G.read().to(torch.float64)
    S = (_normalised(ex).to(torch.float64) @ rows.T).cpu().numpy()
    score = best_score(S, P)
    delta = _delta(D)
    jump = np.zeros(R, dtype=bool) if N == 0 else np.abs(S[:P].max(0) - S[P:].max(0)) <= 2 * delta
    print("rows on the jump:", int(jump.sum()))
    assert jump.sum() <= 0.001 * R
    for k in KS:
        s, i, c = G.recommend(ex[:P], ex[P:] if N else None, k=k)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        assert int(c) == k and len(set(i.tolist())) == k
        kth = np.sort(score)[::-1][k - 1]
        got = np.zeros(R, dtype=bool)
        got[i] = True
        must = (score >= kth + 2 * delta) & ~jump
        assert not (must & ~got).any(), np.nonzero(must & ~got)[0][:10]
        assert not (got & ~jump & (score < kth - 2 * delta)).any()
        ok = ~jump[i]
        assert np.abs(s[ok].astype(np.float64) - score[i][ok]).max() <= 1e-6
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all()
    G.close()


# ---- 4. rows that only the bound keeps ---------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def test_a_row_whose_bf16_scores_say_the_other_branch():
    """One positive p and one negative n; 1 500 rows near unit(p + n) score about 0.7 against both, sp - sn spread around 0 at
    the scale of the bf16 rounding.  About half of them have sp > sn (score sp: the top of the answer), the others -(sn^2).
    Among the first kind there are rows whose bf16 scan scores (emulated here: bf16-rounded rows and examples, summed in
    fp64) say a < b: only the widening by e keeps them on branch A."""
    R, D, M = 20_037, 1024, 1500
    rng = np.random.default_rng(41)
    x = _planted(R, D, seed=41)
    p = rng.standard_normal(D).astype(np.float32)
    n = rng.standard_normal(D).astype(np.float32)
    p /= np.linalg.norm(p)
    n /= np.linalg.norm(n)
    where = rng.permutation(R)[:M]
    x[where] = (p + n)[None, :] + 4e-4 * rng.standard_normal((M, D)).astype(np.float32)
    G = _gallery(x)
    ex = torch.from_numpy(np.stack([p, n])).to(DEV)
    rows, exn = G.read(), _normalised(ex)
    S64 = (exn.to(torch.float64) @ rows.to(torch.float64).T).cpu().numpy()
    Sb = (_bf16(exn) @ _bf16(rows).T).cpu().numpy()
    margin = 2e-6                                   # far above the fp32 chain's and the MFMA accumulation's rounding
    flipped = np.nonzero((S64[0] - S64[1] > margin) & (Sb[0] - Sb[1] < -margin))[0]
    flipped = flipped[np.isin(flipped, where)]      # (of the rows near unit(p + n): those belong in the top-k)
    assert flipped.shape[0] >= 1, "the construction lost its rows"
    score = _check_composition(G, ex[:1], ex[1:], ks=(1024,))
    s, i, c = G.recommend(ex[:1], ex[1:], k=1024)
    got = set(i.cpu().numpy().tolist())
    top = set(np.nonzero(score > 0.5)[0].tolist())
    assert len(top) <= 1024 and top <= got
    assert set(flipped.tolist()) <= got
    G.close()


def test_a_row_below_the_level_in_bf16():
    """One positive; 1 500 rows in the sample (the first rows) score within 1e-4 of each other, k = 700: by the bf16 scores
    alone (emulated as above) hundreds of rows of the fp32 top-k rank below the k-th bf16 score of the sample -- the level
    without the widening by e would drop them."""
    R, D, M, k = 20_037, 1024, 1500, 700
    rng = np.random.default_rng(43)
    x = _planted(R, D, seed=43)
    p = rng.standard_normal(D).astype(np.float32)
    p /= np.linalg.norm(p)
    # unit rows s p + sqrt(1 - s^2) u, u a unit vector orthogonal to p, s = 0.8 + 1e-4 z
    u = rng.standard_normal((M, D))
    u -= (u @ p.astype(np.float64))[:, None] * p[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sc = 0.8 + 1e-4 * rng.standard_normal(M)
    x[:M] = (sc[:, None] * p[None, :] + np.sqrt(1.0 - sc * sc)[:, None] * u).astype(np.float32)
    G = _gallery(x)
    ex = torch.from_numpy(p[None]).to(DEV)
    rows, exn = G.read(), _normalised(ex)
    s64 = (exn.to(torch.float64) @ rows.to(torch.float64).T).cpu().numpy()[0]
    sb = (_bf16(exn) @ _bf16(rows).T).cpu().numpy()[0]
    kth64 = np.sort(s64)[::-1][k - 1]
    level_b = np.sort(sb[:4864])[::-1][k - 1]        # the k-th bf16 score of the sample rows
    below = np.nonzero((s64 > kth64 + 2e-6) & (sb < level_b - 2e-6))[0]
    assert below.shape[0] >= 1, "the construction lost its rows"
    _check_composition(G, ex, None, ks=(k,))
    s, i, c = G.recommend(ex, None, k=k)
    assert set(below.tolist()) <= set(i.cpu().numpy().tolist())
    G.close()


# ---- 5. filters, thresholds, offsets, ties, errors, stats -------------------------------------------------------------
def test_filters():
    R, D = 20_037, 768
    x = _planted(R, D, seed=51)
    G = _gallery(x)
    ex = _examples(x, 6, seed=52)
    pos, neg = ex[:4], ex[4:]
    rng = np.random.default_rng(53)
    everything = torch.ones(R, dtype=torch.bool, device=DEV)
    half = torch.from_numpy(rng.random(R) < 0.5).to(DEV)
    few = torch.zeros(R, dtype=torch.bool, device=DEV)
    few[torch.from_numpy(rng.permutation(R)[:2]).to(DEV)] = True                 # 0.01 %
    tail = torch.zeros(R, dtype=torch.bool, device=DEV)
    tail[R - 700:] = True                                                        # allowed rows only beyond the sample
    for allow in (everything, half, few, tail):
        _check_composition(G, pos, neg, allow=allow)                             # (k > allowed rows: few, tail at k = 1024)
        assert _stats_are_the_recommend_search(G) <= int(allow.sum())
    none = torch.zeros(R, dtype=torch.bool, device=DEV)
    s, i, c = G.recommend(pos, neg, k=10, allow=none)
    assert int(c) == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    assert _stats_are_the_recommend_search(G, passes=0) == 0
    # the filter is gone afterwards
    _check_composition(G, pos, neg, ks=(10,))
    G.close()


def test_thresholds_and_index_offset():
    R, D = 20_037, 1024
    x = _planted(R, D, seed=61)
    G = _gallery(x)
    ex = _examples(x, 6, seed=62)
    pos, neg = ex[:4], ex[4:]
    score = _check_composition(G, pos, neg, ks=(10,))
    # between the negative range (-(sn^2) <= 0) and the positive one, inside each, above everything
    for t in (-1e-3, float(np.sort(score)[-30]), float(np.sort(score)[40]), 0.0, 1.5):
        _check_composition(G, pos, neg, ks=(10, 1024), threshold=t)
    s, i, c = G.recommend(pos, neg, k=10, score_threshold=1.5)
    assert int(c) == 0 and bool((i == -1).all())
    _check_composition(G, pos, neg, ks=(10, 51), index_offset=1_000_000_007)
    _check_composition(G, pos, neg, ks=(10,), index_offset=5, threshold=0.1)
    G.close()


def test_ties_duplicates_and_an_example_that_is_a_row():
    R, D = 20_037, 1024
    rng = np.random.default_rng(171)
    x = _planted(R, D, seed=71)
    v = rng.standard_normal(D).astype(np.float32)
    x[3000:5000] = v                                                             # 2 000 identical rows
    G = _gallery(x)
    vt = torch.from_numpy(v[None]).to(DEV)
    other = _examples(x, 3, seed=72)
    # the identical rows tie: row order decides, whatever k cuts through them
    _check_composition(G, vt, None, ks=(1, 50, 1024))
    _check_composition(G, torch.cat([vt, other[:1]]), other[1:], ks=(10, 1024))
    s, i, c = G.recommend(vt, None, k=1024)
    assert np.array_equal(i.cpu().numpy(), np.arange(3000, 4024))
    # duplicate examples change nothing
    a = G.recommend(other[:2], other[2:], k=51)
    b = G.recommend(torch.cat([other[:2], other[:2], other[:1]]), torch.cat([other[2:], other[2:]]), k=51)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # an example that IS a gallery row: that row first, with its self-score bits
    row = G.read(777, 1)
    s, i, c = G.recommend(row, None, k=5)
    s1, i1, _ = G.search(row, k=5)
    assert int(i[0]) == 777 and torch.equal(s.view(torch.int32), s1[0].view(torch.int32)) and torch.equal(i, i1[0])
    # the same vector on both sides: sp == sn takes the -(sn^2) branch for every row
    s, i, c = G.recommend(other[:1], other[:1], k=10)
    assert bool((s <= 0).all())
    _check_composition(G, other[:1], other[:1], ks=(10,))
    G.close()


def test_errors_empty_gallery_and_results_that_survive():
    D = 1024
    x = _planted(20_037, D, seed=81)
    ex = _examples(x, 4, seed=82)
    G0 = _gallery(x[:300], keep_f32=False)
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.recommend(ex[:2], ex[2:], k=5)
    G0.close()
    E = engine.Gallery(D, 16, device=0)
    s, i, c = E.recommend(ex[:2], ex[2:], k=7)
    assert int(c) == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all())
    assert _stats_are_the_recommend_search(E, passes=0) == 0
    E.close()
    G = _gallery(x)
    with pytest.raises(RuntimeError, match="128"):
        G.recommend(_examples(x, 100, 1), _examples(x, 29, 2), k=5)
    with pytest.raises(RuntimeError, match="1024"):
        G.recommend(ex[:1], None, k=1025)
    pairs, ps = G.pairs(0.93)
    off, ridx, rsc = G.search_range(ex[:2], 0.5)
    G.recommend(ex[:2], ex[2:], k=1024)
    import ctypes as C
    from reverso_amd import _lib
    p2 = torch.empty_like(pairs)
    ps2 = torch.empty_like(ps)
    _lib.check(G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert torch.equal(p2, pairs) and torch.equal(ps2, ps)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(G._lib.revo_search_range_read(G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)
    assert C.sizeof(C.c_void_p) == 8
    G.close()


# ---- 6. store and facade ---------------------------------------------------------------------------------------------------
def _store(N, D, seed):
    from reverso_amd import store
    x = _planted(N, D, seed=seed, n_clusters=N // 10)
    payloads = [{"image_source": f"img{r}.jpg", "filename": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1]} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    return st, x


def test_store_recommend():
    from reverso_amd import filters, store
    N, D = 5000, 256
    st, x = _store(N, D, seed=91)
    vec = _examples(x, 3, seed=92)
    # ids and vectors mixed: the vectors of ids come from the fp32 master rows, the points given by id are left out
    pos, neg = ["p17", vec[0].cpu().numpy(), "p400"], [vec[1], "p33"]
    hits = st.recommend(pos, neg, limit=20)
    allow = torch.ones(N, dtype=torch.bool, device=DEV)
    allow[[17, 400, 33]] = False
    pv = torch.stack([st.gallery.read(17, 1)[0], vec[0], st.gallery.read(400, 1)[0]])
    nv = torch.stack([vec[1], st.gallery.read(33, 1)[0]])
    s, i, c = st.gallery.recommend(pv, nv, k=20, allow=allow)
    assert int(c) == 20 and [(h.id, h.score) for h in hits] == [(f"p{j}", sc) for j, sc in zip(i.tolist(), s.tolist())]
    assert all(isinstance(h, store.ScoredPoint) and h.payload is st.payloads[int(h.id[1:])] for h in hits)
    assert not {"p17", "p400", "p33"} & {h.id for h in hits}
    # without the exclusion the examples' own rows lead
    s2, i2, _ = st.gallery.recommend(pv, nv, k=20)
    assert {17, 400} <= set(i2.tolist()[:3])
    # query_filter combined with the exclusion
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    fh = st.recommend(pos, neg, limit=20, query_filter=flt, score_threshold=-0.5)
    allow2 = allow & torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    s, i, c = st.gallery.recommend(pv, nv, k=20, allow=allow2, score_threshold=-0.5)
    assert [(h.id, h.score) for h in fh] == [(f"p{j}", sc) for j, sc in zip(i.tolist()[:int(c)], s.tolist()[:int(c)])]
    assert all(int(h.id[1:]) % 2 == 1 for h in fh) and len(fh) == 20
    # one example, not in a list
    one = st.recommend("p17", limit=3)
    assert len(one) == 3 and "p17" not in {h.id for h in one}
    # average_vector: the plain search of the host-computed vector
    av = st.recommend(pos, neg, limit=10, strategy="average_vector")
    q = store.average_vector_query(pv.cpu().numpy(), nv.cpu().numpy())
    s, i, c = st.gallery.search(torch.from_numpy(q)[None].to(DEV), k=10, allow=allow)
    assert [(h.id, h.score) for h in av] == [(f"p{j}", sc) for j, sc in zip(i[0].tolist(), s[0].tolist())]
    with pytest.raises(KeyError, match="nope"):
        st.recommend(["p17", "nope"], limit=3)
    with pytest.raises(ValueError, match="strategy"):
        st.recommend(["p17"], limit=3, strategy="other")
    with pytest.raises(ValueError, match="positive"):
        st.recommend([], ["p17"], limit=3)


def test_search_by_examples_on_a_database(tmp_path):
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, items = r.search_by_examples(["p7"])
    assert text.startswith("❌") and "No database loaded" in text and items == []
    st, x = _store(3000, 64, seed=93)
    r.vector_db = st
    r.current_database = "recommend"
    text, items = r.search_by_examples([])
    assert text.startswith("❌") and items == []
    v = torch.from_numpy(x[11] / np.linalg.norm(x[11]))
    text, items = r.search_by_examples(["p7", v], negative=["p8"], max_results=6)
    want = st.recommend(["p7", v], ["p8"], limit=6)
    assert [(it["id"], it["score"]) for it in items] == [(h.id, h.score) for h in want] and len(items) == 6
    assert all(set(it) == {"filename", "image_source", "bbox", "id", "score"} for it in items)
    assert "p7" not in {it["id"] for it in items} and "p8" not in {it["id"] for it in items}
    assert text.startswith("🎯 Found 6 regions like the 2 positive and unlike the 1 negative examples")
    assert items[0]["id"] == "p11" and f"1. {items[0]['filename']}  score {items[0]['score']:.3f}" in text
    flt = {"must": [{"key": "detected_class", "match": {"value": "person"}}]}
    _, fitems = r.search_by_examples(["p7"], max_results=5, query_filter=flt)
    assert [it["id"] for it in fitems] == [h.id for h in st.recommend(["p7"], limit=5, query_filter=flt)]
    assert all(int(it["id"][1:]) % 2 == 1 for it in fitems)
    text, items = r.search_by_examples(["p7"], similarity_threshold=1.5)
    assert items == [] and "No regions found" in text and "1.5" in text
    text, items = r.search_by_examples(["no-such-id"])
    assert text.startswith("❌") and "no-such-id" in text and items == []


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    x = _planted(20_037, 1024, seed=71)
    G = _gallery(x)
    ex = _examples(x, 6, seed=72)
    for k in (10, 51):
        _assert_offset_moves_the_indices_only(lambda off: G.recommend(ex[:4], ex[4:], k=k, index_offset=off), {1})
    G.close()
