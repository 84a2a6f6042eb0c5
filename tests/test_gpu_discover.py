"""Discovery and context search (revo_search_discover, include/revo.h DISCOVER; Gallery.discover, GalleryStore.discover,
SimpleReverso.search_by_context): bit for bit against a composition of the range search (every example's score of every row,
the one fp32 chain) with the formulas in numpy float32, the identities of the contract, planted rows that only the rounding
bound keeps, an fp64 oracle of the fp32 rows, filters, thresholds, ties, errors, the stats, the store and the facade."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _discover_checks as dc  # noqa: E402
from _recommend_checks import exhaustive  # noqa: E402
from test_gpu_recommend import (_allowed, _assert_equals, _bf16, _chain_scores, _delta, _examples, _gallery,  # noqa: E402
                                _normalised, _planted, _stats_are_the_recommend_search, _store)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KS = (1, 10, 50, 51, 1024)
f = np.float32
FS_EPS = dc.fs(np.array([-np.finfo(f).eps], dtype=f))[0]          # fs(-FLT_EPSILON): the loss of a pair with sp == sn


def _split(ex, n, has_target):
    """(target, positives, negatives) of an example block laid out target | positives | negatives"""
    t = ex[0] if has_target else None
    o = 1 if has_target else 0
    return t, ex[o:o + n], ex[o + n:o + 2 * n]


def _score_rows(G, ex, n, has_target, allow=None):
    """the contract's fp32 score of every row, from the range search's chain scores of every example"""
    S = _chain_scores(G, ex, allow)
    o = 1 if has_target else 0
    with np.errstate(invalid="ignore"):                 # (rows the filter does not allow are -inf: never looked at)
        return dc.score(S[0] if has_target else None, S[o:o + n], S[o + n:o + 2 * n])


def _check_composition(G, ex, n, has_target, ks=KS, allow=None, threshold=None, index_offset=0):
    """check 1: the call against the formulas over the range search's scores; no tolerance.  Returns the fp32 score row."""
    score = _score_rows(G, ex, n, has_target, allow)
    t, pos, neg = _split(ex, n, has_target)
    for k in ks:
        got = G.discover(t, pos, neg, k=k, score_threshold=threshold, index_offset=index_offset, allow=allow)
        _assert_equals(got, exhaustive(score, _allowed(G, allow), k, threshold, index_offset), f"k={k}")
    return score


# ---- 1. bit for bit against the composition --------------------------------------------------------------------------------
_MODES = [(n, True) for n in (0, 1, 2, 5, 31, 32, 33, 63)] + [(n, False) for n in (1, 2, 5, 32, 33, 64)]
_CASES = [(n, t, 20_037, [1024, 64, 768, 1280][i % 4]) for i, (n, t) in enumerate(_MODES)]
_CASES += [(n, t, R, 1024) for R in (1, 255, 256, 257) for (n, t) in ((2, True), (33, True), (5, False), (64, False))]


@pytest.mark.parametrize("n,has_target,R,D", _CASES)
def test_equals_the_composition_bit_for_bit(n, has_target, R, D):
    x = _planted(R, D, seed=R + D + 3 * n + int(has_target))
    G = _gallery(x)
    ex = _examples(x, 2 * n + int(has_target), seed=n * 131 + int(has_target))
    score = _check_composition(G, ex, n, has_target)
    assert _stats_are_the_recommend_search(G) >= min(R, 1024)
    assert score.shape == (R,)
    # two calls: identical bytes
    t, pos, neg = _split(ex, n, has_target)
    a = G.discover(t, pos, neg, k=51)
    b = G.discover(t, pos, neg, k=51)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and int(a[2]) == int(b[2])
    G.close()


def test_the_level_does_its_work():
    """a k = 10 discovery re-scores a small part of a large gallery (the stratum of the best R and what the bound cannot
    tell from it)"""
    R, D = 20_037, 1024
    x = _planted(R, D, seed=7)
    G = _gallery(x)
    ex = _examples(x, 1 + 2 * 5, seed=8)
    t, pos, neg = _split(ex, 5, True)
    G.discover(t, pos, neg, k=10)
    assert _stats_are_the_recommend_search(G) < R // 4
    G.close()


# ---- 2. the identities of the contract ---------------------------------------------------------------------------------
def test_a_pair_of_one_vector_and_swapped_pairs():
    R, D = 20_037, 768
    x = _planted(R, D, seed=21)
    G = _gallery(x)
    ex = _examples(x, 1 + 2 * 4, seed=22)
    t, pos, neg = _split(ex, 4, True)
    rng = np.random.default_rng(23)
    half = torch.from_numpy(rng.random(R) < 0.5).to(DEV)
    v = ex[1:2]
    # no target, positive == negative: every allowed row scores fs(-FLT_EPSILON); the first k allowed rows by index
    for allow in (None, half):
        for k in (1, 10, 1024):
            s, i, c = G.discover(None, v, v, k=k, allow=allow)
            rows = np.nonzero(_allowed(G, allow))[0][:k]
            assert int(c) == k and np.array_equal(i.cpu().numpy(), rows)
            assert (s.cpu().numpy().view(np.uint32) == FS_EPS.view(np.uint32)).all()
    # with a target it shifts every score's R by -1
    base = _score_rows(G, ex, 4, True)
    more = _score_rows(G, torch.cat([ex[:1], pos, v, neg, v]), 5, True)
    st = _chain_scores(G, ex[:1])[0]
    SP, SN = _chain_scores(G, pos), _chain_scores(G, neg)
    assert np.array_equal(more.view(np.uint32), ((dc.ranks(SP, SN) - 1).astype(f) + dc.sig(st)).view(np.uint32))
    _check_composition(G, torch.cat([ex[:1], pos, v, neg, v]), 5, True, ks=(10, 1024))
    # swapping the two sides of every pair negates R for every row with sp_i != sn_i for all i
    decided = (SP != SN).all(axis=0)
    assert decided.sum() > R // 2
    assert np.array_equal(dc.ranks(SN, SP)[decided], -dc.ranks(SP, SN)[decided])
    swapped = _check_composition(G, torch.cat([ex[:1], neg, pos]), 4, True, ks=(10, 1024))
    assert np.array_equal((swapped - dc.sig(st))[decided].round(), -(base - dc.sig(st))[decided].round())
    G.close()


def test_zero_pairs_with_a_target_is_the_order_of_sig():
    """the rows of exhaustive(sig).  (Not search_topk_large's rows: sig sends most neighbouring scores to one float -- ties
    then go by row index -- and is not monotone to the last bit, so the two orders legitimately differ among near-equal
    target scores.)"""
    R, D = 20_037, 1024
    x = _planted(R, D, seed=31)
    G = _gallery(x)
    t = _examples(x, 1, seed=32)
    sigs = dc.sig(_chain_scores(G, t)[0])
    for k in KS:
        _assert_equals(G.discover(t[0], None, None, k=k), exhaustive(sigs, np.ones(R, dtype=bool), k), f"k={k}")
    G.close()


# ---- 3. rows that only the widening keeps ------------------------------------------------------------------------------
def test_a_pair_whose_bf16_scores_say_the_other_side():
    """One pair (p, n) and the target unit(p + n); 1 500 rows near the target score about 0.7 against both p and n, sp - sn
    spread around 0 at the scale of the bf16 rounding.  About half have sp > sn (R = +1: the top of the answer).  Among
    them are rows whose bf16 scan scores (emulated: bf16-rounded rows and examples, summed in fp64) say a < b: only the
    widening by 2 e keeps the pair open for them."""
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
    ex = torch.from_numpy(np.stack([p + n, p, n])).to(DEV)
    rows, exn = G.read(), _normalised(ex)
    S64 = (exn.to(torch.float64) @ rows.to(torch.float64).T).cpu().numpy()
    Sb = (_bf16(exn) @ _bf16(rows).T).cpu().numpy()
    margin = 2e-6                                   # far above the fp32 chain's and the MFMA accumulation's rounding
    flipped = np.nonzero((S64[1] - S64[2] > margin) & (Sb[1] - Sb[2] < -margin))[0]
    flipped = flipped[np.isin(flipped, where)]      # (of the rows near the target: those belong in the top-k)
    assert flipped.shape[0] >= 1, "the construction lost its rows"
    score = _check_composition(G, ex, 1, True, ks=(1024,))
    s, i, c = G.discover(ex[0], ex[1:2], ex[2:3], k=1024)
    got = set(i.cpu().numpy().tolist())
    top = set(np.nonzero(score > 1.7)[0].tolist())  # R = +1 and sig near its top, 0.75: the planted rows on the positive side
    assert len(top) <= 1024 and top <= got and set(flipped.tolist()) <= top
    # the same rows satisfy the pair in the context search: score +0, the head of the answer
    cs = _check_composition(G, ex[1:], 1, False, ks=(1024,))
    assert (cs[flipped] == 0).all()
    G.close()


def test_a_row_below_the_level_in_bf16():
    """No pairs, a target; 1 500 rows in the sample (the first rows) score within 1e-4 of each other, k = 700: by the bf16
    scores alone (emulated as above) rows of the fp32 top-k rank below the k-th bf16 score of the sample -- the level without
    the widening by e would drop them.  (2e-6 in the target score is 3e-7 in sig: five of its ulps.)"""
    R, D, M, k = 20_037, 1024, 1500, 700
    rng = np.random.default_rng(43)
    x = _planted(R, D, seed=43)
    p = rng.standard_normal(D).astype(np.float32)
    p /= np.linalg.norm(p)
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
    _check_composition(G, ex, 0, True, ks=(k,))
    s, i, c = G.discover(ex[0], None, None, k=k)
    assert set(below.tolist()) <= set(i.cpu().numpy().tolist())
    G.close()


# ---- 4. the fp64 oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,has_target,D", [(2, True, 64), (8, True, 1024), (63, True, 768), (4, False, 1024), (64, False, 1280)])
def test_matches_the_fp64_oracle(n, has_target, D):
    """Independent of the library's chain: the formulas in fp64 over fp64 scores of the fp32 rows.  delta is the near_tie band
    of test_gpu_search.py (3e-7 at D = 1024, scaled with D): what an fp32 chain score may differ from the fp64 one.  In the
    discovery search a pair with |sp - sn| <= 2 delta may take either rank: a row with such a pair is excused (the context
    loss is continuous: nothing to excuse).  An fp32 score may differ from the fp64 one by
        tol(v) = ops * (2 delta + 3.5e-7) + ops * 2^-24 * |v| + ulp32(|v|)
    with ops the operations that depend on a score (one sig for the discovery search, one loss per pair for the context
    search): 2 delta for the two chain scores behind a difference (the target's single score moves sig by less, its slope
    is below 1), 3.5e-7 for the fp32 roundings inside one sig / loss, 2^-24 |v| per addition of the
    context sum, and one ulp of the fp32 result (3.8e-6 at |R| = 63).  Two rows whose fp64 scores are within tol(k-th
    score) of the k-th may swap across the cut; returned score values are held to tol(their own value).  The excused share
    of the compared results is printed and may not exceed 1 %."""
    R = 20_037
    x = _planted(R, D, seed=D + n)
    G = _gallery(x)
    ex = _examples(x, 2 * n + int(has_target), seed=n + 17)
    t, pos, neg = _split(ex, n, has_target)
    rows = G.read().to(torch.float64)
    S = (_normalised(ex).to(torch.float64) @ rows.T).cpu().numpy()
    o = int(has_target)
    SP, SN = S[o:o + n], S[o + n:o + 2 * n]
    score = dc.score(S[0] if has_target else None, SP, SN)
    assert score.dtype == np.float64
    delta = _delta(D)
    jump = (np.abs(SP - SN) <= 2 * delta).any(axis=0) if has_target else np.zeros(R, dtype=bool)
    ops = 1 if has_target else n

    def tol(v):
        return ops * (2 * delta + 3.5e-7) + ops * 2.0 ** -24 * np.abs(v) + np.spacing(np.abs(v).astype(f)).astype(np.float64)

    excused = compared = 0
    for k in KS:
        s, i, c = G.discover(t, pos, neg, k=k)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        assert int(c) == k and len(set(i.tolist())) == k
        kth = np.sort(score)[::-1][k - 1]
        band = float(tol(kth))
        got = np.zeros(R, dtype=bool)
        got[i] = True
        must = (score >= kth + band) & ~jump
        assert not (must & ~got).any(), np.nonzero(must & ~got)[0][:10]
        assert not (got & ~jump & (score < kth - band)).any()
        ok = ~jump[i]
        assert (np.abs(s[ok].astype(np.float64) - score[i][ok]) <= tol(score[i][ok])).all()
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all()
        compared += k
        excused += int(jump[i].sum())
    print(f"excused rows (a pair inside the band): {excused} of {compared} compared results")
    assert excused <= 0.01 * compared
    G.close()


# ---- 5. filters, thresholds, offsets, ties, errors, stats -------------------------------------------------------------
@pytest.mark.parametrize("n,has_target", [(4, True), (3, False)])
def test_filters(n, has_target):
    R, D = 20_037, 768
    x = _planted(R, D, seed=51)
    G = _gallery(x)
    ex = _examples(x, 2 * n + int(has_target), seed=52)
    t, pos, neg = _split(ex, n, has_target)
    rng = np.random.default_rng(53)
    half = torch.from_numpy(rng.random(R) < 0.5).to(DEV)
    one = torch.zeros(R, dtype=torch.bool, device=DEV)
    one[12_345] = True
    tail = torch.zeros(R, dtype=torch.bool, device=DEV)
    tail[R - 700:] = True                                                        # allowed rows only beyond the sample
    for allow in (half, one, tail):
        _check_composition(G, ex, n, has_target, allow=allow)
        assert _stats_are_the_recommend_search(G) <= int(allow.sum())
    none = torch.zeros(R, dtype=torch.bool, device=DEV)
    s, i, c = G.discover(t, pos, neg, k=10, allow=none)
    assert int(c) == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    assert _stats_are_the_recommend_search(G, passes=0) == 0
    _check_composition(G, ex, n, has_target, ks=(10,))                           # the filter is gone afterwards
    G.close()


def test_thresholds_and_index_offset():
    R, D = 20_037, 1024
    x = _planted(R, D, seed=61)
    G = _gallery(x)
    ex = _examples(x, 1 + 2 * 4, seed=62)
    score = _check_composition(G, ex, 4, True, ks=(10,))
    # above every score, between two strata of R, inside a stratum, -inf
    inside = float(np.sort(score)[-30])
    for thr in (5.5, 2.0, inside, 0.5 + float(np.floor(inside)), -np.inf):
        _check_composition(G, ex, 4, True, ks=(10, 1024), threshold=thr)
    t, pos, neg = _split(ex, 4, True)
    s, i, c = G.discover(t, pos, neg, k=10, score_threshold=5.5)
    assert int(c) == 0 and bool((i == -1).all())
    _check_composition(G, ex, 4, True, ks=(10, 51), index_offset=1_000_000_007)
    # context: 0 keeps exactly the rows that satisfy every pair; inside the negative range; -inf
    cs = _check_composition(G, ex[1:], 4, False, ks=(10,))
    for thr in (0.0, float(np.sort(cs)[-3000]), 1e-9, -np.inf):
        _check_composition(G, ex[1:], 4, False, ks=(10, 1024), threshold=thr)
    s, i, c = G.discover(None, pos, neg, k=1024, score_threshold=0.0)
    assert int(c) == min(1024, int((cs == 0).sum())) and bool((s[:int(c)] == 0).all())
    _check_composition(G, ex[1:], 4, False, ks=(10,), index_offset=5, threshold=-0.1)
    G.close()


def test_exact_duplicate_rows_go_by_index():
    R, D = 20_037, 1024
    rng = np.random.default_rng(171)
    x = _planted(R, D, seed=71)
    v = rng.standard_normal(D).astype(np.float32)
    x[3000:5000] = v                                                             # 2 000 identical rows
    G = _gallery(x)
    other = _examples(x, 2, seed=72)
    vt = torch.from_numpy(v[None]).to(DEV)
    # target = the duplicated vector, one pair it satisfies: the duplicates lead, in row order, whatever k cuts through them
    ex = torch.cat([vt, vt, other[:1]])
    _check_composition(G, ex, 1, True, ks=(1, 50, 1024))
    s, i, c = G.discover(vt[0], vt, other[:1], k=1024)
    assert np.array_equal(i.cpu().numpy(), np.arange(3000, 4024))
    _check_composition(G, torch.cat([vt, other[:1]]), 1, False, ks=(50, 1024))
    G.close()


def test_errors_empty_gallery_and_results_that_survive():
    D = 1024
    x = _planted(20_037, D, seed=81)
    ex = _examples(x, 5, seed=82)
    t, pos, neg = _split(ex, 2, True)
    G0 = _gallery(x[:300], keep_f32=False)
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.discover(t, pos, neg, k=5)
    G0.close()
    E = engine.Gallery(D, 16, device=0)
    for tt in (t, None):
        s, i, c = E.discover(tt, pos, neg, k=7)
        assert int(c) == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all())
        assert _stats_are_the_recommend_search(E, passes=0) == 0
    E.close()
    G = _gallery(x)
    many = _examples(x, 128, 1)
    with pytest.raises(RuntimeError, match="63"):
        G.discover(t, many[:64], many[64:], k=5)
    with pytest.raises(RuntimeError, match="64"):
        G.discover(None, None, None, k=5)
    with pytest.raises(RuntimeError, match="1024"):
        G.discover(t, pos, neg, k=1025)
    with pytest.raises(ValueError, match="same number"):
        G.discover(t, pos, neg[:1], k=5)
    pairs, ps = G.pairs(0.93)
    off, ridx, rsc = G.search_range(ex[:2], 0.5)
    G.discover(t, pos, neg, k=1024)
    G.discover(None, pos, neg, k=1024)
    from reverso_amd import _lib
    p2 = torch.empty_like(pairs)
    ps2 = torch.empty_like(ps)
    _lib.check(G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert torch.equal(p2, pairs) and torch.equal(ps2, ps)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(G._lib.revo_search_range_read(G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)
    G.close()


# ---- 6. store and facade ---------------------------------------------------------------------------------------------------
def test_store_discover():
    from reverso_amd import filters, store
    N, D = 5000, 256
    st, x = _store(N, D, seed=91)
    vec = _examples(x, 3, seed=92)
    context = [("p17", vec[0].cpu().numpy()), (vec[1], "p33")]
    hits = st.discover("p400", context, limit=20)
    allow = torch.ones(N, dtype=torch.bool, device=DEV)
    allow[[17, 33, 400]] = False
    row = lambda r: st.gallery.read(r, 1)[0]   # noqa: E731
    pv, nv = torch.stack([row(17), vec[1]]), torch.stack([vec[0], row(33)])
    s, i, c = st.gallery.discover(row(400), pv, nv, k=20, allow=allow)
    assert int(c) == 20 and [(h.id, h.score) for h in hits] == [(f"p{j}", sc) for j, sc in zip(i.tolist(), s.tolist())]
    assert all(isinstance(h, store.ScoredPoint) and h.payload is st.payloads[int(h.id[1:])] for h in hits)
    assert not {"p17", "p400", "p33"} & {h.id for h in hits}
    # a vector target, a filter and a threshold
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    fh = st.discover(vec[2], context, limit=20, query_filter=flt, score_threshold=0.5)
    allow2 = torch.ones(N, dtype=torch.bool, device=DEV)
    allow2[[17, 33]] = False
    allow2 &= torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    s, i, c = st.gallery.discover(vec[2], pv, nv, k=20, allow=allow2, score_threshold=0.5)
    assert [(h.id, h.score) for h in fh] == [(f"p{j}", sc) for j, sc in zip(i.tolist()[:int(c)], s.tolist()[:int(c)])]
    assert all(int(h.id[1:]) % 2 == 1 for h in fh) and len(fh) >= 1
    # target=None: the context search
    ch = st.discover(None, context, limit=20)
    allow3 = torch.ones(N, dtype=torch.bool, device=DEV)
    allow3[[17, 33]] = False
    s, i, c = st.gallery.discover(None, pv, nv, k=20, allow=allow3)
    assert [(h.id, h.score) for h in ch] == [(f"p{j}", sc) for j, sc in zip(i.tolist()[:int(c)], s.tolist()[:int(c)])]
    assert len(ch) == 20 and all(h.score <= 0 for h in ch) and not {"p17", "p33"} & {h.id for h in ch}
    # no pairs with a target; a bare pair is not a list of pairs
    with pytest.raises(ValueError, match="pair"):
        st.discover("p400", ("p17", "p33"), limit=3)
    only = st.discover("p400", limit=3)
    assert len(only) == 3 and "p400" not in {h.id for h in only} and all(0 < h.score < 1 for h in only)
    with pytest.raises(KeyError, match="nope"):
        st.discover("p400", [("p17", "nope")], limit=3)
    with pytest.raises(KeyError, match="nope"):
        st.discover("nope", [("p17", "p33")], limit=3)
    with pytest.raises(ValueError, match="target or at least one"):
        st.discover(None, [], limit=3)
    with pytest.raises(ValueError, match="pair"):
        st.discover("p400", [("p17", "p33", "p34")], limit=3)


def test_search_by_context_on_a_database(tmp_path):
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, items = r.search_by_context("p7", [("p8", "p9")])
    assert text.startswith("❌") and "No database loaded" in text and items == []
    st, x = _store(3000, 64, seed=93)
    r.vector_db = st
    r.current_database = "discover"
    text, items = r.search_by_context(None, [])
    assert text.startswith("❌") and items == []
    v = torch.from_numpy(x[11] / np.linalg.norm(x[11]))
    text, items = r.search_by_context(v, [("p7", "p8"), (v, "p9")], max_results=6)
    want = st.discover(v, [("p7", "p8"), (v, "p9")], limit=6)
    assert [(it["id"], it["score"]) for it in items] == [(h.id, h.score) for h in want] and len(items) == 6
    assert all(set(it) == {"filename", "image_source", "bbox", "id", "score"} for it in items)
    assert not {"p7", "p8", "p9"} & {it["id"] for it in items}
    assert text.startswith("🎯 Found 6 regions for the target under 2 context pairs")
    assert f"1. {items[0]['filename']}  score {items[0]['score']:.3f}" in text
    flt = {"must": [{"key": "detected_class", "match": {"value": "person"}}]}
    _, fitems = r.search_by_context("p7", [("p8", "p9")], max_results=5, query_filter=flt)
    assert [it["id"] for it in fitems] == [h.id for h in st.discover("p7", [("p8", "p9")], limit=5, query_filter=flt)]
    assert all(int(it["id"][1:]) % 2 == 1 for it in fitems)
    text, items = r.search_by_context(None, [("p8", "p9")], max_results=4)
    assert [it["id"] for it in items] == [h.id for h in st.discover(None, [("p8", "p9")], limit=4)]
    assert text.startswith("🎯 Found 4 regions for the context under 1 context pairs")
    text, items = r.search_by_context("p7", [("p8", "p9")], similarity_threshold=5.0)
    assert items == [] and "No regions found" in text and "5.0" in text
    text, items = r.search_by_context("no-such-id", [("p8", "p9")])
    assert text.startswith("❌") and "no-such-id" in text and items == []


@pytest.mark.parametrize("has_target", [True, False])
def test_index_offset_at_and_above_2_31(has_target):
    from _search_checks import _assert_offset_moves_the_indices_only
    x = _planted(20_037, 1024, seed=61)
    G = _gallery(x)
    t, pos, neg = _split(_examples(x, 1 + 2 * 4, seed=62), 4, True)
    for k in (10, 51):
        _assert_offset_moves_the_indices_only(
            lambda off: G.discover(t if has_target else None, pos, neg, k=k, index_offset=off), {1})
    G.close()
