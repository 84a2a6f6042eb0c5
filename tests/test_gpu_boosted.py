"""Boosted search (revo_search_boosted, include/revo.h BOOSTED; Gallery.search_boosted,
GalleryStore.search_boosted, SimpleReverso.search_similar_boosted): byte for byte against an exhaustive reference built from
the plain search's score bits of every row (the range search's, the one fp32 chain), the two cuts and a correctly rounded
host fma (tests/_boost_checks.py).  Two gallery sizes: 3 000 rows (below the small-gallery size: no sample, tau is -inf or
the threshold) and 20 037 rows (a strided sample of 19 tiles, a ragged last gallery tile)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boost_checks as bc  # noqa: E402
from test_gpu_recommend import _bf16, _examples, _normalised, _planted  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL, LARGE = 3_000, 20_037
SAMPLE = 4_864            # the sample of 20 037 rows, whatever k: a quarter of the gallery in whole tiles (test_gpu_recommend.py has it too)
WIDTHS = (64, 320, 768, 1024, 1280)       # test_gpu_recommend.py's, and 320: five K-tiles, an odd count above one


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


class _Case:
    """A gallery, one query, and the plain search's score of every row (computed once, never changed)."""

    def __init__(self, x, q):
        self.x = x
        self.N, self.D = x.shape
        self.G = engine.Gallery(self.D, max(1, self.N), device=0)
        self.G.add(torch.from_numpy(x).to(DEV))
        self.q = q
        off, idx, sc = self.G.search_range(q[None], -2.0)
        s = torch.full((self.N,), -np.inf, dtype=torch.float32, device=DEV)
        s[idx] = sc
        self.s = s.cpu().numpy()
        assert np.isfinite(self.s).all()
        self.s.setflags(write=False)

    def check(self, mult, bias, k, threshold=None, min_similarity=None, allow=None, index_offset=0, final=None):
        """the call against the exhaustive reference, byte for byte; returns the call's result on the host"""
        allowed = np.ones(self.N, dtype=bool) if allow is None else allow
        final = bc.final_scores(self.s, mult, bias) if final is None else final
        want = bc.exhaustive(self.s, allowed, final, k, threshold, min_similarity, index_offset)
        got = self.G.search_boosted(self.q, _dev(mult), _dev(bias), k=k, score_threshold=threshold, min_similarity=min_similarity,
                                    index_offset=index_offset, allow=_dev(allow))
        s, m, i, c = (t.cpu().numpy() for t in got)
        what = (self.N, self.D, k, threshold, min_similarity)
        assert int(c) == want[3], (what, int(c), want[3])
        assert np.array_equal(i, want[2]), (what, np.nonzero(i != want[2])[0][:10], i[:8], want[2][:8])
        assert np.array_equal(s.view(np.uint32), want[0].view(np.uint32)), (what, np.nonzero(s != want[0])[0][:10])
        assert np.array_equal(m.view(np.uint32), want[1].view(np.uint32)), (what, np.nonzero(m != want[1])[0][:10])
        return s, m, i, int(c)

    def candidates(self, passes=1):
        st = self.G.search_stats()
        assert st["join_passes"] == passes, st
        assert st["uncertified"] == st["bruteforced"] == st["checked"] == st["from_segments"] == 0, st
        assert st["grouped_fallback"] == st["large_k_fallback"] == 0, st
        return st["collected_rows"]


@functools.lru_cache(maxsize=None)
def _case(N, D):
    x = _planted(N, D, seed=N + D)
    return _Case(x, _examples(x, 1, seed=D)[0])


@functools.lru_cache(maxsize=None)
def _boosts(N, seed=0):
    """random m in [0, 4] and b in [-1, 1], and their final scores per (N, D) computed when first asked for"""
    rng = np.random.default_rng(1000 + N + seed)
    m, b = rng.uniform(0, 4, N).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32)
    m.setflags(write=False)
    b.setflags(write=False)
    return m, b


@functools.lru_cache(maxsize=None)
def _final(N, D):
    return bc.final_scores(_case(N, D).s, *_boosts(N))


SHAPES = [(SMALL, D) for D in WIDTHS] + [(LARGE, D) for D in WIDTHS]


# ---- 1. the equivalences with the plain search -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", SHAPES)
def test_both_arrays_null_is_the_plain_search(N, D):
    c = _case(N, D)
    for k in (1, 10, 50, 51, 1024):
        s, i, n = c.G.search(c.q[None], k=k)
        bs, bm, bi, bn = c.G.search_boosted(c.q, k=k)
        assert int(bn) == int(n[0]) and torch.equal(bi, i[0])
        assert torch.equal(bs.view(torch.int32), s[0].view(torch.int32)) and torch.equal(bm.view(torch.int32), s[0].view(torch.int32))
    # two calls: identical bytes
    a, b = c.G.search_boosted(c.q, k=300), c.G.search_boosted(c.q, k=300)
    assert all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(a, b))


@pytest.mark.parametrize("N,D", [(SMALL, 64), (LARGE, 320), (LARGE, 1024)])
def test_ones_and_zeros_are_the_plain_search_up_to_the_sign_of_zero(N, D):
    c = _case(N, D)
    one, zero = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    for k in (10, 1024):
        s, i, n = c.G.search(c.q[None], k=k)
        for m, b in ((one, zero), (one, None), (None, zero)):
            bs, bm, bi, bn = c.G.search_boosted(c.q, m, b, k=k)
            assert int(bn) == int(n[0]) and torch.equal(bi, i[0])
            assert torch.equal((bs + 0.0).view(torch.int32), (s[0] + 0.0).view(torch.int32))       # (x + 0.0: -0 -> +0)
            assert torch.equal(bm.view(torch.int32), s[0].view(torch.int32))


# ---- 2. the exhaustive reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", SHAPES)
def test_equals_the_exhaustive_reference(N, D):
    c = _case(N, D)
    m, b = _boosts(N)
    final = _final(N, D)
    for k in (1, 10, 1024):
        c.check(m, b, k, final=final)
    assert c.candidates() >= min(N, 1024)
    # k exceeds the number of qualifying rows: the similarity cut leaves about 40 rows, then the threshold fewer still
    cut = float(np.sort(c.s)[-40])
    _, _, _, n = c.check(m, b, 1024, min_similarity=cut, final=final)
    assert n == 40
    _, _, _, n = c.check(m, b, 1024, min_similarity=cut, threshold=float(np.median(final[c.s >= np.float32(cut)])), final=final)
    assert 15 <= n <= 25
    # one array only
    c.check(m, None, 10)
    c.check(None, b, 10)
    if N == LARGE:
        # the level does its work: a k = 10 request re-scores a small part of the gallery
        c.check(m, b, 10, final=final)
        assert c.candidates() < N // 4


# ---- 3. planted rows that only the widening keeps ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _near_ties():
    """test_gpu_recommend.py::test_a_row_below_the_level_in_bf16's rows: 1 500 unit rows scoring 0.8 + 1e-4 z against p, placed
    on rows of the strided sample; their bf16 scan scores (emulated: bf16-rounded rows and query, summed in fp64) scatter by
    about 1e-3, ten times the spread of the fp32 scores."""
    R, D, M = LARGE, 1024, 1500
    rng = np.random.default_rng(43)
    x = _planted(R, D, seed=43)
    p = rng.standard_normal(D).astype(np.float32)
    p /= np.linalg.norm(p)
    u = rng.standard_normal((M, D))
    u -= (u @ p.astype(np.float64))[:, None] * p[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sc = 0.8 + 1e-4 * rng.standard_normal(M)
    sample = bc.sample_rows(R, SAMPLE)
    where = np.sort(rng.permutation(sample)[:M])
    x[where] = (sc[:, None] * p[None, :] + np.sqrt(1.0 - sc * sc)[:, None] * u).astype(np.float32)
    c = _Case(x, torch.from_numpy(p).to(DEV))
    rows, qn = c.G.read(), _normalised(c.q[None])
    s64 = (qn.to(torch.float64) @ rows.to(torch.float64).T).cpu().numpy()[0]
    sb = (_bf16(qn) @ _bf16(rows).T).cpu().numpy()[0]
    return c, s64, sb, sample, where


@pytest.mark.parametrize("mult", [2.0, 1000.0])
def test_a_row_below_the_level_in_bf16(mult):
    """m the same on every row, so the order is the similarity's; k = 700 cuts through the near-ties.  By the bf16 scores alone
    (final score m * sb + b in fp64) rows of the fp32 top-k rank below the k-th bf16 final score of the sample: a level without
    the widening (m e at m = 1000) would drop them.  Checked here before the GPU is asked."""
    c, s64, sb, sample, _ = _near_ties()
    k, bias = 700, 0.25
    f64, fb = mult * s64 + bias, mult * sb + bias
    kth = np.sort(f64)[::-1][k - 1]
    level_b = np.sort(fb[sample])[::-1][k - 1]
    margin = 2e-6 * mult                             # far above the fp32 chain's and the MFMA accumulation's rounding, times m
    below = np.nonzero((f64 > kth + margin) & (fb < level_b - margin))[0]
    assert below.shape[0] >= 1, "the construction lost its rows"
    m = np.full(c.N, mult, dtype=np.float32)
    b = np.full(c.N, bias, dtype=np.float32)
    _, _, i, n = c.check(m, b, k)
    assert n == k and set(below.tolist()) <= set(i.tolist())


def test_rows_on_either_side_of_the_minimum_similarity_in_bf16():
    """min_similarity in the middle of the near-ties: rows whose fp32 similarity reaches it while their bf16 score does not must
    come back, and the mirror rows (bf16 above, fp32 below) must not."""
    c, s64, sb, _, where = _near_ties()
    cut = 0.8
    inside = np.nonzero((s64 >= cut + 2e-6) & (sb < cut - 2e-6))[0]
    mirror = np.nonzero((s64 < cut - 2e-6) & (sb > cut + 2e-6))[0]
    assert inside.shape[0] >= 1 and mirror.shape[0] >= 1, "the construction lost its rows"
    assert np.isin(inside, where).all() and np.isin(mirror, where).all()
    m, b = _boosts(c.N, seed=3)
    for k in (10, 1024):
        _, _, i, n = c.check(m, b, k, min_similarity=cut)
    assert n < 1024                                  # about half of the 1 500 qualify: the answer holds every one of them
    got = set(i[:n].tolist())
    assert set(inside.tolist()) <= got and not (set(mirror.tolist()) & got)


# ---- 4. special row values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [SMALL, LARGE])
def test_zero_multipliers_equal_finals_and_duplicate_rows(N):
    D = 768
    rng = np.random.default_rng(7 + N)
    x = _planted(N, D, seed=7 + N).copy()
    v = rng.standard_normal(D).astype(np.float32)
    x[1500:1900] = v                                  # 400 identical rows
    c = _Case(x, _examples(x, 1, seed=8)[0])
    m, b = (a.copy() for a in _boosts(N, seed=4))
    # m = 0: the final score is b whatever the similarity -- 300 rows with distinct biases above every other final score
    zero = rng.permutation(N)[:300]
    m[zero] = 0.0
    b[zero] = (6.0 + rng.permutation(300) / 300.0).astype(np.float32)
    s, sim, i, n = c.check(m, b, 300)
    assert set(i.tolist()) == set(zero.tolist()) and np.array_equal(s, b[i]) and np.array_equal(sim, c.s[i])
    # a block of equal final scores comes back in row order, wherever k cuts it
    b[zero] = np.float32(-3.0)
    block = np.arange(600, 1400)
    m[block] = 0.0
    b[block] = np.float32(9.0)
    for k in (1, 10, 1024):
        s, sim, i, n = c.check(m, b, k)
        assert np.array_equal(i[:min(k, 800)], block[:k]) and (s[:min(k, 800)] == 9.0).all()
    # duplicate rows with one multiplier and bias: equal similarities, equal finals, row order
    m[1500:1900], b[1500:1900] = np.float32(3.0), np.float32(20.0)
    s, sim, i, n = c.check(m, b, 500)
    assert np.array_equal(i[:400], np.arange(1500, 1900)) and len(set(sim[:400].tolist())) == 1
    c.G.close()


# ---- 5. good rows outside any prefix -----------------------------------------------------------------------------------------
def test_good_rows_in_the_last_tile_and_a_bias_that_grows_with_the_row():
    """The bias grows by 8 / 79 per 256-row tile (timestamps grow with the row index) and the rows like the query are the 69 rows
    of the ragged last tile.  A sample of the first rows would see no good row: tau would stay below every upper bound.  The
    strided sample's last tile is gallery tile 74 of 79: with nothing known of the similarities but |s| <= 1.01 (unit rows, and
    e far below 0.01), tau >= b(tile 74) - 1.01, which rows with b + 1.01 < tau cannot reach: tiles 0 .. 54, more than half of
    the gallery (_boost_checks.rows_the_level_excludes; asserted here on the CPU first)."""
    N, D, k = LARGE, 1024, 10
    rng = np.random.default_rng(77)
    x = _planted(N, D, seed=77).copy()
    p = rng.standard_normal(D).astype(np.float32)
    p /= np.linalg.norm(p)
    last = np.arange(N // 256 * 256, N)
    x[last] = p[None, :] + 0.3 * rng.standard_normal((last.shape[0], D)).astype(np.float32) / np.sqrt(D)
    c = _Case(x, torch.from_numpy(p).to(DEV))
    assert np.abs(c.s).max() <= 1.001
    m = np.ones(N, dtype=np.float32)
    b = (8.0 * (np.arange(N) // 256) / 79).astype(np.float32)
    everything = np.ones(N, dtype=bool)
    excluded = bc.rows_the_level_excludes(m, b, everything, bc.sample_rows(N, SAMPLE), k, 1.01)
    assert excluded > N // 2, excluded
    assert bc.rows_the_level_excludes(m, b, everything, np.arange(SAMPLE), k, 1.01) == 0
    s, sim, i, n = c.check(m, b, k)
    assert n == k and (i >= last[0]).all() and (sim > 0.9).all()
    assert c.candidates() < N // 2
    c.G.close()


# ---- 6. options and errors ---------------------------------------------------------------------------------------------------
def test_filters():
    N, D = LARGE, 768
    c = _case(N, D)
    m, b = _boosts(N)
    final = _final(N, D)
    rng = np.random.default_rng(53)
    half = rng.random(N) < 0.5
    few = np.zeros(N, dtype=bool)
    few[rng.permutation(N)[:2]] = True
    tail = np.zeros(N, dtype=bool)
    tail[N - 700:] = True                               # allowed rows only in the last tiles
    for allow in (np.ones(N, dtype=bool), half, few, tail):
        for k in (10, 1024):
            c.check(m, b, k, allow=allow, final=final)
        assert c.candidates() <= int(allow.sum())
    s, sim, i, n = c.check(m, b, 10, allow=np.zeros(N, dtype=bool), final=final)
    assert n == 0 and (i == -1).all() and np.isneginf(s).all() and np.isneginf(sim).all()
    assert c.candidates(passes=0) == 0
    c.check(m, b, 10, final=final)                      # the filter is gone afterwards
    cs = _case(SMALL, 320)
    ms, bs_ = _boosts(SMALL)
    cs.check(ms, bs_, 1024, allow=rng.random(SMALL) < 0.3, final=_final(SMALL, 320))


@pytest.mark.parametrize("N,D", [(SMALL, 1280), (LARGE, 1024)])
def test_both_thresholds(N, D):
    c = _case(N, D)
    m, b = _boosts(N)
    final = _final(N, D)
    fs, ss = np.sort(final), np.sort(c.s)
    for t in (float(fs[-30]), float(fs[N // 2]), -10.0, 10.0):
        for k in (10, 1024):
            c.check(m, b, k, threshold=t, final=final)
    for cut in (float(ss[-30]), float(ss[N // 2]), -2.0, 2.0):
        for k in (10, 1024):
            c.check(m, b, k, min_similarity=cut, final=final)
    _, _, i, n = c.check(m, b, 1024, threshold=float(fs[-300]), min_similarity=float(ss[-300]), final=final)
    assert 0 < n < 300
    _, _, i, n = c.check(m, b, 10, threshold=10.0, final=final)
    assert n == 0 and (i == -1).all()
    # exactly AT a row's values: >= keeps it
    r = int(np.argsort(final)[-5])
    _, _, i, n = c.check(m, b, 10, threshold=float(final[r]), min_similarity=float(c.s[r]), final=final)
    assert r in i[:n].tolist()


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    c = _case(LARGE, 1024)
    m, b = (_dev(a) for a in _boosts(LARGE))
    for k in (10, 51):
        _assert_offset_moves_the_indices_only(lambda off: c.G.search_boosted(c.q, m, b, k=k, index_offset=off), {2})
    c.check(*_boosts(LARGE), 10, index_offset=1_000_000_007, threshold=0.5, final=_final(LARGE, 1024))


@pytest.mark.parametrize("N", [SMALL, LARGE])
def test_values_outside_the_domain(N):
    c = _case(N, 768)
    m0, b0 = _boosts(N)
    final = _final(N, 768)
    rows = [5, N // 2, N - 1]
    for which, value in (("m", np.nan), ("m", -1e-3), ("m", np.inf), ("m", -np.inf), ("b", np.nan), ("b", np.inf), ("b", -np.inf)):
        m, b = m0.copy(), b0.copy()
        (m if which == "m" else b)[rows] = value
        with pytest.raises(RuntimeError, match="3 allowed rows"):
            c.G.search_boosted(c.q, _dev(m), _dev(b), k=10)
        # on rows the filter does not allow they are not looked at: the answer is that of the clean arrays
        allow = np.ones(N, dtype=bool)
        allow[rows] = False
        want = bc.exhaustive(c.s, allow, final, 10)
        s, sim, i, n = (t.cpu().numpy() for t in c.G.search_boosted(c.q, _dev(m), _dev(b), k=10, allow=_dev(allow)))
        assert int(n) == want[3] and np.array_equal(i, want[2]) and np.array_equal(s.view(np.uint32), want[0].view(np.uint32))
    # -0 is a multiplier >= 0, and a row that is far from the answer is inspected like any other
    m = m0.copy()
    m[7] = -0.0
    c.check(m, b0, 10)
    c.check(m0, b0, 10, final=final)                    # and the handle answers as before


def test_errors_an_empty_gallery_and_results_that_survive():
    D = 1024
    c = _case(LARGE, D)
    m, b = (_dev(a) for a in _boosts(LARGE))
    G0 = engine.Gallery(D, 300, device=0, keep_f32=False)
    G0.add(torch.from_numpy(c.x[:300]).to(DEV))
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.search_boosted(c.q, k=5)
    G0.close()
    E = engine.Gallery(D, 16, device=0)
    s, sim, i, n = E.search_boosted(c.q, None, None, k=7, score_threshold=0.1)
    assert int(n) == 0 and bool((i == -1).all()) and bool(torch.isneginf(s).all()) and bool(torch.isneginf(sim).all())
    st = E.search_stats()
    assert st["join_passes"] == 0 and st["collected_rows"] == 0
    E.close()
    with pytest.raises(RuntimeError, match="1024"):
        c.G.search_boosted(c.q, m, b, k=1025)
    with pytest.raises(RuntimeError, match="NaN"):
        c.G.search_boosted(c.q, m, b, k=5, min_similarity=float("nan"))
    with pytest.raises(RuntimeError, match="NaN"):
        c.G.search_boosted(c.q, m, b, k=5, score_threshold=float("nan"))
    with pytest.raises(ValueError, match="one entry per gallery row"):
        c.G.search_boosted(c.q, m[:-1], b, k=5)
    with pytest.raises(ValueError, match="one vector"):
        c.G.search_boosted(torch.stack([c.q, c.q]), m, b, k=5)
    pairs, ps = c.G.pairs(0.93)
    off, ridx, rsc = c.G.search_range(c.q[None], 0.5)
    c.G.search_boosted(c.q, m, b, k=1024)
    from reverso_amd import _lib
    p2, ps2 = torch.empty_like(pairs), torch.empty_like(ps)
    _lib.check(c.G._lib.revo_gallery_pairs_read(c.G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert torch.equal(p2, pairs) and torch.equal(ps2, ps)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(c.G._lib.revo_search_range_read(c.G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)


# ---- 7. store and facade -----------------------------------------------------------------------------------------------------
_DAY = 86400.0
_T0 = 1_700_000_000.0


def _store(N, D, seed):
    from reverso_amd import store
    x = _planted(N, D, seed=seed, n_clusters=N // 10)
    payloads = [{"image_source": f"img{r}.jpg", "filename": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1], "taken": _T0 + 600.0 * r, "trust": 0.5 + (r % 7) / 4.0} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    return st, x


def _date_decay(target_row, scale_days=2.0):
    """similarity times trust, plus a Gaussian preference for points taken near a date"""
    return {"sum": [{"mult": ["$score", "trust"]},
                    {"gauss_decay": {"x": {"datetime_key": "taken"}, "target": {"datetime": _T0 + 600.0 * target_row},
                                     "scale": scale_days * _DAY}}]}


def test_store_search_boosted():
    from reverso_amd import boost, filters, store
    N, D = 5000, 256
    st, x = _store(N, D, seed=91)
    q = _examples(x, 1, seed=92)[0]
    formula = _date_decay(4000)
    hits = st.search_boosted(q.cpu().numpy(), 20, formula)
    M, B = boost.compile_formula(formula, st.payloads)
    s, sim, i, c = st.gallery.search_boosted(q, _dev(M), _dev(B), k=20)
    assert int(c) == 20 and [(h.id, h.score, h.similarity) for h in hits] == \
        [(f"p{j}", a, b) for j, a, b in zip(i.tolist(), s.tolist(), sim.tolist())]
    assert all(isinstance(h, store.BoostedPoint) and isinstance(h, store.ScoredPoint) and h.payload is st.payloads[int(h.id[1:])]
               for h in hits)
    # the date matters: the hits lie around row 4000, which the plain search's do not
    assert np.median([int(h.id[1:]) for h in hits]) > 3000
    assert sorted(int(h.id[1:]) for h in st.search(q.cpu().numpy(), 20)) != sorted(int(h.id[1:]) for h in hits)
    # the device arrays are cached per (formula, filter, state of the store) ...
    cached = st._boost_cache
    assert st.search_boosted(q.cpu().numpy(), 20, formula) == hits and st._boost_cache is cached
    # ... and every change of the points drops them: set_payload moves a point's date and trust, delete removes the best hit
    best = hits[0].id
    st.set_payload([best], dict(st.payloads[int(best[1:])], taken=_T0, trust=0.0))
    assert st._boost_cache is None
    again = st.search_boosted(q.cpu().numpy(), 20, formula)
    assert best not in {h.id for h in again} and again[0].id == hits[1].id
    st.delete([again[0].id])
    assert st._boost_cache is None
    third = st.search_boosted(q.cpu().numpy(), 20, formula)
    assert again[0].id not in {h.id for h in third} and len(st) == N - 1
    M, B = boost.compile_formula(formula, st.payloads)
    s, sim, i, c = st.gallery.search_boosted(q, _dev(M), _dev(B), k=20)
    assert [(h.id, h.score) for h in third] == [(st.ids[j], a) for j, a in zip(i.tolist(), s.tolist())]
    st.upsert(torch.from_numpy(x[:1]), ["new"], [dict(st.payloads[0], taken=_T0 + 600.0 * 4000, trust=3.0)])
    assert st._boost_cache is None and len(st.search_boosted(q.cpu().numpy(), 5, formula)) == 5
    # a filter, both cuts; a negative coefficient on a point the filter leaves out is no error, on one it selects it is
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    st.set_payload(["p10"], dict(st.payloads[st.ids.index("p10")], trust=-1.0))
    fh = st.search_boosted(q.cpu().numpy(), 20, formula, score_threshold=0.2, min_similarity=-0.05, query_filter=flt)
    assert fh and all(h.payload["detected_class"] == "person" and h.score >= 0.2 and h.similarity >= -0.05 for h in fh)
    with pytest.raises(ValueError, match="negative"):
        st.search_boosted(q.cpu().numpy(), 20, formula)
    with pytest.raises(ValueError, match="affine"):
        st.search_boosted(q.cpu().numpy(), 20, {"mult": ["$score", "$score"]}, query_filter=flt)
    with pytest.raises(ValueError, match="no payload key"):
        st.search_boosted(q.cpu().numpy(), 20, {"sum": ["$score", "missing"]}, query_filter=flt)
    assert len(st.search_boosted(q.cpu().numpy(), 3, {"sum": ["$score", "missing"]}, query_filter=flt, defaults={"missing": 1.0})) == 3
    st.close()


def test_store_search_boosted_with_a_filter_in_any_operand_order():
    """A filter with payload columns multiplied and divided in, the column written first, inside a decay's argument and in a
    denominator: the formula compiles as it does without the filter, and the hits are those of the device search over the
    unfiltered pair with the filter's rows allowed."""
    from reverso_amd import boost
    N, D = 3000, 64
    st, x = _store(N, D, seed=95)
    q = _examples(x, 1, seed=96)[0]
    hours = {"div": {"left": {"sum": [{"datetime_key": "taken"}, {"neg": {"datetime": _T0 + 600.0 * 2000}}]}, "right": {"mult": [60.0, 60.0]}}}
    formula = {"sum": [{"mult": ["trust", "$score"]}, {"div": {"left": "$score", "right": {"mult": ["trust", 4.0]}}},
                       {"mult": [0.5, {"exp_decay": {"x": {"mult": [hours, 2.0]}, "scale": 48.0}}]}]}
    flt = {"must": [{"key": "detected_class", "match": {"value": "person"}}]}
    hits = st.search_boosted(q.cpu().numpy(), 25, formula, query_filter=flt, min_similarity=-0.2)
    M, B = boost.compile_formula(formula, st.payloads)
    allow = torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    s, sim, i, c = st.gallery.search_boosted(q, _dev(M), _dev(B), k=25, min_similarity=-0.2, allow=allow)
    assert int(c) == 25 and [(h.id, h.score, h.similarity) for h in hits] == \
        [(f"p{j}", a, b) for j, a, b in zip(i.tolist(), s.tolist(), sim.tolist())]
    assert all(h.payload["detected_class"] == "person" for h in hits)
    assert np.median([int(h.id[1:]) for h in hits]) > 1000                      # the decay around row 2000 matters
    st.close()


def test_search_similar_boosted_on_a_database(tmp_path):
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, items = r.search_similar_boosted("$score")
    assert text.startswith("❌") and items == []
    st, x = _store(3000, 64, seed=93)
    r.vector_db = st
    r.current_database = "boosted"
    v = torch.from_numpy(x[11] / np.linalg.norm(x[11]))
    r.region_embeddings = [v]
    formula = _date_decay(2500, scale_days=1.0)
    text, items = r.search_similar_boosted(formula, similarity_threshold=None, max_results=6)
    want = st.search_boosted(v, 6, formula)
    assert [(it["id"], it["score"], it["similarity"]) for it in items] == [(h.id, h.score, h.similarity) for h in want] and len(items) == 6
    assert all(set(it) == {"filename", "image_source", "bbox", "id", "score", "similarity"} for it in items)
    assert text.startswith("🎯 Found 6 similar regions (boosted)") and f"1. {items[0]['filename']}  score {items[0]['score']:.3f}" in text
    # similarity_threshold is the cut on the similarity, not on the boosted score
    text, items = r.search_similar_boosted(formula, similarity_threshold=0.7, max_results=5)
    assert items and all(it["similarity"] >= 0.7 for it in items) and "p11" in {it["id"] for it in items}
    assert [it["id"] for it in items] == [h.id for h in st.search_boosted(v, 5, formula, min_similarity=0.7)]
    flt = {"must": [{"key": "detected_class", "match": {"value": "car"}}]}
    _, fitems = r.search_similar_boosted(formula, similarity_threshold=None, max_results=5, query_filter=flt)
    assert [it["id"] for it in fitems] == [h.id for h in st.search_boosted(v, 5, formula, query_filter=flt)]
    assert all(int(it["id"][1:]) % 2 == 0 for it in fitems)
    text, items = r.search_similar_boosted(formula, similarity_threshold=1.5)
    assert items == [] and "No similar regions found" in text and "1.5" in text
    text, items = r.search_similar_boosted({"mult": ["$score", "$score"]})
    assert text.startswith("❌") and "affine" in text and items == []
    st.close()
