"""Diverse search (revo_search_mmr, include/revo.h MMR; Gallery.search_mmr, GalleryStore.search_mmr,
SimpleReverso.search_similar_diverse): bit for bit against a composition of calls that existed before it (the candidates of
Gallery.search at k = C, the similarities of Gallery.pairs restricted to those candidates, the greedy selection in numpy
fp32), the identities of the contract, fixtures in which diversity matters, a float64 replay of every pick, errors, the
stats, the store and the facade."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _mmr_checks import greedy  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DIMS = (64, 768, 1024, 1280)
ROWS = (1, 255, 256, 257, 20_037)
KC = ((1, 1), (10, 100), (50, 50), (50, 1024), (1024, 1024))
DIVERSITIES = (0.0, 0.3, 0.5, 1.0)
QUERIES = (1, 3, 64, 130)


def _delta(D):
    """the fp32 chain's band: 3e-7 at D = 1024 (test_gpu_search.py), scaled with D, never below that"""
    return 3e-7 * max(1.0, D / 1024)


def _planted(N, D, seed, n_clusters=None):
    """tests/test_gpu_recommend.py::_planted: random directions and clusters of perturbed copies of a few of them"""
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
    """the fp32 query rows the library scores (the same normalisation kernel as an append)"""
    T = engine.Gallery(q.shape[1], q.shape[0], device=0)
    T.add(q)
    out = T.read(0, q.shape[0])
    T.close()
    return out


def _queries(x, n, seed):
    """perturbed gallery rows (a planted gallery: many of them next to a cluster of near-copies)"""
    rng = np.random.default_rng(seed)
    D = x.shape[1]
    pick = rng.integers(0, x.shape[0], n)
    q = x[pick] / np.linalg.norm(x[pick], axis=1, keepdims=True)
    q = q + 0.05 * rng.standard_normal((n, D)).astype(np.float32) / np.sqrt(D)
    return torch.from_numpy(q.astype(np.float32)).to(DEV)


def _candidate_sims(G, rows):
    """fp32 [n, n]: the scores Gallery.pairs reports for every pair of the given rows (distinct), in the rows' order"""
    n = rows.shape[0]
    sim = np.zeros((n, n), dtype=np.float32)
    if n < 2:
        return sim
    mask = torch.zeros(len(G), dtype=torch.bool, device=DEV)
    mask[torch.from_numpy(rows).to(DEV)] = True
    pairs, ps = G.pairs(-2.0, allow=mask)
    assert pairs.shape[0] == n * (n - 1) // 2, (pairs.shape, n)
    pos = np.full(len(G), -1, dtype=np.int64)
    pos[rows] = np.arange(n)
    pairs, ps = pairs.cpu().numpy(), ps.cpu().numpy()
    a, b = pos[pairs[:, 0]], pos[pairs[:, 1]]
    sim[a, b] = ps
    sim[b, a] = ps
    return sim


def _composition(G, q, k, C, diversity, threshold=None, allow=None, index_offset=0):
    """the contract's answer from calls that existed before the feature: (scores, values, indices, counts) numpy"""
    cs, ci, cc = G.search(q, k=C, score_threshold=threshold, allow=allow)
    cs, ci, cc = cs.cpu().numpy(), ci.cpu().numpy(), cc.cpu().numpy()
    Q = q.shape[0]
    S = np.full((Q, k), -np.inf, dtype=np.float32)
    V = np.full((Q, k), -np.inf, dtype=np.float32)
    I = np.full((Q, k), -1, dtype=np.int64)
    cnt = np.zeros(Q, dtype=np.int32)
    for r in range(Q):
        n = int(cc[r])
        rows, rel = ci[r, :n], cs[r, :n]
        picks, values = greedy(rel, _candidate_sims(G, rows), k, diversity)
        m = picks.shape[0]
        S[r, :m], V[r, :m], I[r, :m], cnt[r] = rel[picks], values, rows[picks] + index_offset, m
    return S, V, I, cnt


def _assert_equals(got, want, what=""):
    gs, gv, gi, gc = (t.cpu().numpy() for t in got)
    ws, wv, wi, wc = want
    assert np.array_equal(gc, wc), (what, gc, wc)
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5])
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), what
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (what, np.argwhere(gv.view(np.uint32) != wv.view(np.uint32))[:5])


def _check(G, q, k, C, diversity, **kw):
    want = _composition(G, q, k, C, diversity, **kw)
    got = G.search_mmr(q, k=k, candidates=C, diversity=diversity, score_threshold=kw.get("threshold"),
                       index_offset=kw.get("index_offset", 0), allow=kw.get("allow"))
    _assert_equals(got, want, (k, C, diversity, q.shape[0], kw.keys()))
    return got


# ---- 1. bit for bit against the composition ----------------------------------------------------------------------------------
# every dimension against every gallery size; (k, C), diversity and the query count rotate through their values
_SIZES = [(D, R, KC[(a + b) % 5], DIVERSITIES[(a + 2 * b) % 4], QUERIES[(a + b) % 3])
          for a, D in enumerate(DIMS) for b, R in enumerate(ROWS)]


@pytest.mark.parametrize("D,R,kc,diversity,nq", _SIZES)
def test_equals_the_composition_bit_for_bit(D, R, kc, diversity, nq):
    x = _planted(R, D, seed=100 + D + R)
    G = _gallery(x)
    _check(G, _queries(x, nq, seed=7), kc[0], kc[1], diversity)
    G.close()


@pytest.mark.parametrize("kc", KC)
@pytest.mark.parametrize("diversity", DIVERSITIES)
def test_every_k_c_and_diversity(kc, diversity):
    x = _planted(20_037, 1024, seed=11)
    G = _gallery(x)
    _check(G, _queries(x, 3, seed=12), kc[0], kc[1], diversity)
    G.close()


@pytest.mark.parametrize("nq,kc", [(64, (50, 1024)), (130, (50, 1024)), (130, (10, 100)), (65, (1024, 1024))])
def test_query_counts_across_the_chunk_size(nq, kc):
    """C = 1024: 64 queries fill the similarity workspace exactly, 65 and 130 cross it"""
    x = _planted(20_037, 1024, seed=13)
    G = _gallery(x)
    _check(G, _queries(x, nq, seed=14), kc[0], kc[1], 0.5)
    G.close()


def test_filter_threshold_and_index_offset():
    D = 1024
    x = _planted(20_037, D, seed=15)
    G = _gallery(x)
    q = _queries(x, 5, seed=16)
    allow = torch.from_numpy(np.random.default_rng(17).random(x.shape[0]) < 0.4).to(DEV)
    got = _check(G, q, 10, 100, 0.5, allow=allow)
    idx = got[2].cpu().numpy()
    assert bool(allow.cpu().numpy()[idx[idx >= 0]].all())
    _check(G, q, 50, 1024, 0.3, allow=allow, index_offset=1_000_000_007)
    # a threshold that cuts the candidate lists below k (a cluster's few near-copies pass it, nothing else)
    got = _check(G, q, 10, 100, 0.5, threshold=0.8)
    cnt = got[3].cpu().numpy()
    assert (cnt < 10).all() and (cnt > 0).any(), cnt
    assert bool(torch.isinf(got[0][0, int(cnt[0]):]).all()) and bool((got[2][0, int(cnt[0]):] == -1).all())
    _check(G, q, 50, 1024, 1.0, threshold=0.8, allow=allow, index_offset=-5)
    _check(G, q, 10, 100, 0.5, threshold=1.5)                   # nothing passes
    G.close()


# ---- 2. identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,C", [(10, 100), (50, 50), (100, 1024), (1024, 1024)])
def test_diversity_zero_is_the_plain_search(k, C):
    x = _planted(20_037, 1024, seed=21)
    G = _gallery(x)
    q = _queries(x, 4, seed=22)
    s, v, i, c = G.search_mmr(q, k=k, candidates=C, diversity=0.0)
    ps, pi, pc = G.search(q, k=k)
    assert torch.equal(i, pi) and torch.equal(c, pc) and torch.equal(s.view(torch.int32), ps.view(torch.int32))
    assert torch.equal(v.view(torch.int32), ps.view(torch.int32))
    G.close()


def test_permutation_batch_repeat_and_null_values():
    import ctypes as C
    from reverso_amd import _lib
    x = _planted(20_037, 768, seed=23)
    G = _gallery(x)
    q = _queries(x, 6, seed=24)
    # k = C: a permutation of the candidates, the first pick the best candidate
    s, v, i, c = G.search_mmr(q, k=200, candidates=200, diversity=0.6)
    ps, pi, pc = G.search(q, k=200)
    assert torch.equal(i.sort(dim=1).values, pi.sort(dim=1).values) and torch.equal(c, pc) and torch.equal(i[:, 0], pi[:, 0])
    assert not torch.equal(i, pi)
    # batch == one query at a time; two calls: the same bytes
    for r in range(q.shape[0]):
        one = G.search_mmr(q[r:r + 1], k=200, candidates=200, diversity=0.6)
        assert all(torch.equal(a[0].view(torch.int32) if a.dtype == torch.float32 else a[0],
                               b[r].view(torch.int32) if b.dtype == torch.float32 else b[r]) for a, b in zip(one, (s, v, i, c)))
    again = G.search_mmr(q, k=200, candidates=200, diversity=0.6)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(again, (s, v, i, c)))
    # mmr_values = NULL changes nothing else
    s2, i2, c2 = torch.empty_like(s), torch.empty_like(i), torch.empty_like(c)
    qn = q.contiguous()
    _lib.check(G._lib.revo_search_mmr(G._h, _lib.ptr(qn), q.shape[0], 200, 200, 0.6, 0, 0.0, 0, _lib.ptr(s2), None, _lib.ptr(i2),
                                      _lib.ptr(c2), _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(s2.view(torch.int32), s.view(torch.int32)) and torch.equal(i2, i) and torch.equal(c2, c)
    assert C.sizeof(C.c_void_p) == 8
    G.close()


# ---- 3. teeth ----------------------------------------------------------------------------------------------------------------
def test_diversity_removes_near_copies():
    D = 1024
    x = _planted(20_037, D, seed=31)
    G = _gallery(x)
    # queries next to rows that have a near-copy: the first row of 32 of the gallery's pairs scoring >= 0.9
    near = np.unique(G.pairs(0.9)[0][:, 0].cpu().numpy())[:32]
    assert near.shape[0] == 32
    rng = np.random.default_rng(32)
    qh = x[near] / np.linalg.norm(x[near], axis=1, keepdims=True) + 0.05 * rng.standard_normal((32, D)).astype(np.float32) / np.sqrt(D)
    q = torch.from_numpy(qh.astype(np.float32)).to(DEV)
    rows = G.read().cpu().numpy().astype(np.float64)

    def close_pairs(idx):
        n = 0
        for r in range(idx.shape[0]):
            g = rows[idx[r][idx[r] >= 0]]
            n += int((np.triu(g @ g.T, 1) >= 0.9).sum())
        return n
    _, pi, _ = G.search(q, k=10)
    _, _, mi, _ = G.search_mmr(q, k=10, candidates=100, diversity=0.5)
    pi, mi = pi.cpu().numpy(), mi.cpu().numpy()
    plain, diverse = close_pairs(pi), close_pairs(mi)
    print("pairs with sim >= 0.9 in the top-10: plain", plain, "diversity 0.5", diverse)
    assert (pi != mi).any(axis=1).any()
    assert plain > 0 and diverse < plain
    G.close()


def test_an_exact_duplicate_is_picked_last_at_diversity_one():
    D = 256
    x = _planted(3000, D, seed=33)
    x = np.concatenate([x, x[40:41], x[40:41]])                 # rows 3000 and 3001: copies of row 40
    G = _gallery(x)
    q = torch.from_numpy(x[40:41].copy()).to(DEV)
    C = 60
    s, v, i, c = G.search_mmr(q, k=C, candidates=C, diversity=1.0)
    i, v = i[0].cpu().numpy(), v[0].cpu().numpy()
    copies = {40, 3000, 3001}
    assert int(c[0]) == C and copies <= set(i.tolist()) and int(i[0]) == 40
    sim = _candidate_sims(G, np.sort(i))
    order = {r: n for n, r in enumerate(np.sort(i).tolist())}
    for step in range(1, C):
        if int(i[step]) in copies:
            # a copy of a picked row (m = sim to its twin, the largest a pair can have here) goes only when every candidate
            # still left is as similar to the picked set as that
            twin = sim[order[40], order[3000]]
            left = [max(sim[order[int(a)], order[int(b)]] for b in i[:step]) for a in i[step:]]
            assert min(left) >= twin, (step, min(left), twin)
    G.close()


# ---- 4. float64 replay of every pick -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,C,diversity", [(64, 50, 50, 0.5), (768, 10, 100, 0.3), (1024, 50, 1024, 0.5), (1280, 100, 100, 1.0),
                                             (1024, 1024, 1024, 0.7), (1024, 10, 100, 0.0)])
def test_every_pick_is_a_float64_maximum_within_the_rounding(D, k, C, diversity):
    """Greedy MMR is discontinuous, so the pick sequence is not compared with a float64 greedy run.  The library's own picks
    are replayed in float64 over the gallery's fp32 rows: at every step the picked row's float64 value is within
    2 (delta + 3 * 2^-24) of the float64 maximum over the candidates not yet picked.  delta bounds the fp32 chain's error of
    a score (|lam| + |diversity| = 1 keeps the propagated error at delta), the three roundings add 3 * 2^-24 on values of
    magnitude <= 1.  Every step of every query; nothing is excluded."""
    x = _planted(20_037, D, seed=41 + D)
    G = _gallery(x)
    q = _queries(x, 4, seed=42)
    s, v, i, c = G.search_mmr(q, k=k, candidates=C, diversity=diversity)
    _, ci, cc = G.search(q, k=C)
    rows = G.read().cpu().numpy().astype(np.float64)
    qn = _normalised(q).cpu().numpy().astype(np.float64)
    d32 = np.float32(diversity)
    lam, div = float(np.float32(1.0) - d32), float(d32)
    bound = 2.0 * (_delta(D) + 3.0 * 2.0 ** -24)
    worst = 0.0
    for r in range(q.shape[0]):
        cand = ci[r, :int(cc[r])].cpu().numpy()
        picks = i[r, :int(c[r])].cpu().numpy()
        assert int(c[r]) == min(k, cand.shape[0]) and set(picks.tolist()) <= set(cand.tolist())
        g = rows[cand]
        rel, sim = g @ qn[r], g @ g.T
        where = {int(row): n for n, row in enumerate(cand.tolist())}
        alive = np.ones(cand.shape[0], dtype=bool)
        m = np.full(cand.shape[0], -np.inf)
        for step, row in enumerate(picks.tolist()):
            val = lam * rel if step == 0 else lam * rel - div * m
            p = where[row]
            assert alive[p]
            gap = float(val[alive].max() - val[p])
            worst = max(worst, gap)
            assert gap <= bound, (r, step, gap, bound)
            assert abs(float(v[r, step]) - float(val[p])) <= bound, (r, step)
            alive[p] = False
            m = np.maximum(m, sim[p])
    print(f"D={D} k={k} C={C} diversity={diversity}: largest float64 gap {worst:.3e}, bound {bound:.3e}")
    G.close()


# ---- 5. errors, empty results, stats, results that survive ---------------------------------------------------------------------
def test_errors_empty_gallery_stats_and_results_that_survive():
    from reverso_amd import _lib
    D = 1024
    x = _planted(20_037, D, seed=51)
    q = _queries(x, 3, seed=52)
    G0 = _gallery(x[:300], keep_f32=False)
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.search_mmr(q, k=5)
    G0.close()
    E = engine.Gallery(D, 16, device=0)
    s, v, i, c = E.search_mmr(q, k=7, candidates=20)
    assert bool((c == 0).all()) and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool(torch.isinf(v).all())
    assert bool((s < 0).all()) and bool((v < 0).all())
    E.close()
    G = engine.Gallery(D, x.shape[0] + 1, device=0)
    G.add(torch.from_numpy(x).to(DEV))
    for kw, word in (({"k": 0}, "candidates"), ({"k": 11, "candidates": 10}, "candidates"), ({"candidates": 1025}, "1024"),
                     ({"diversity": 1.5}, "diversity"), ({"diversity": float("nan")}, "diversity"),
                     ({"score_threshold": float("nan")}, "NaN")):
        with pytest.raises(RuntimeError, match=word):
            G.search_mmr(q, **kw)
    # a filter set for another gallery size
    bits = G.allow_bits(torch.ones(len(G), dtype=torch.bool, device=DEV))
    _lib.check(G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), len(G), 1, _lib.current_stream()))
    G.add(torch.from_numpy(x[:1]).to(DEV))
    with pytest.raises(RuntimeError, match="filter"):
        G.search_mmr(q, k=5)
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    # nothing allowed
    s, v, i, c = G.search_mmr(q, k=7, candidates=20, allow=torch.zeros(len(G), dtype=torch.bool, device=DEV))
    assert bool((c == 0).all()) and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool(torch.isinf(v).all())
    # the stats are the inner large-k search's
    pairs, ps = G.pairs(0.93)
    off, ridx, rsc = G.search_range(q[:2], 0.5)
    G.search_mmr(q, k=50, candidates=1024, diversity=0.5)
    st = G.search_stats()
    G.search(q, k=1024)
    assert st == G.search_stats() and st["collected_rows"] >= 3 * 1024
    assert all(st[key] == 0 for key in ("uncertified", "bruteforced", "checked", "from_segments", "grouped_fallback", "join_passes"))
    # a pairs and a range result held by the handle are still readable
    p2, ps2 = torch.empty_like(pairs), torch.empty_like(ps)
    _lib.check(G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert torch.equal(p2, pairs) and torch.equal(ps2, ps)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(G._lib.revo_search_range_read(G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)
    G.close()


# ---- 6. store and facade -------------------------------------------------------------------------------------------------------
def _store(N, D, seed):
    from reverso_amd import store
    x = _planted(N, D, seed=seed, n_clusters=N // 10)
    payloads = [{"image_source": f"img{r}.jpg", "filename": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1]} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    return st, x


def test_store_search_mmr():
    from reverso_amd import filters, store
    N, D = 5000, 256
    st, x = _store(N, D, seed=61)
    qv = x[11] / np.linalg.norm(x[11])
    hits = st.search_mmr(qv, limit=8, diversity=0.5)
    s, v, i, c = st.gallery.search_mmr(torch.from_numpy(qv)[None].to(DEV), k=8, candidates=100, diversity=0.5)
    assert int(c[0]) == 8 and [(h.id, h.score) for h in hits] == [(f"p{j}", sc) for j, sc in zip(i[0].tolist(), s[0].tolist())]
    assert all(isinstance(h, store.ScoredPoint) and h.payload is st.payloads[int(h.id[1:])] for h in hits) and hits[0].id == "p11"
    # diversity 0: the plain search
    assert [(h.id, h.score) for h in st.search_mmr(qv, limit=8, diversity=0.0)] == [(h.id, h.score) for h in st.search(qv, 8)]
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    fh = st.search_mmr(qv, limit=8, diversity=0.7, candidates_limit=40, score_threshold=-0.5, query_filter=flt)
    allow = torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    s, v, i, c = st.gallery.search_mmr(torch.from_numpy(qv)[None].to(DEV), k=8, candidates=40, diversity=0.7, score_threshold=-0.5,
                                       allow=allow)
    assert [(h.id, h.score) for h in fh] == [(f"p{j}", sc) for j, sc in zip(i[0].tolist(), s[0].tolist())] and len(fh) == 8
    assert all(int(h.id[1:]) % 2 == 1 for h in fh)
    assert st.search_mmr(qv, limit=8, score_threshold=1.5) == []


def test_search_similar_diverse_on_a_database(tmp_path):
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, items = r.search_similar_diverse()
    assert text.startswith("❌") and "No query embeddings" in text and items == []
    st, x = _store(3000, 64, seed=63)
    r.region_embeddings = [torch.from_numpy(x[11] / np.linalg.norm(x[11]))]
    text, items = r.search_similar_diverse()
    assert text.startswith("❌") and "No database loaded" in text and items == []
    r.vector_db = st
    r.current_database = "diverse"
    text, items = r.search_similar_diverse(similarity_threshold=-1.0, max_results=6, diversity=0.5)
    want = st.search_mmr(r.region_embeddings[0], limit=6, diversity=0.5, score_threshold=-1.0)
    assert [(it["id"], it["score"]) for it in items] == [(h.id, h.score) for h in want] and len(items) == 6
    assert all(set(it) == {"filename", "image_source", "bbox", "id", "score"} for it in items)
    assert items[0]["id"] == "p11" and text.startswith("🎯 Found 6 similar regions (diversity 0.5)")
    assert f"1. {items[0]['filename']}  score {items[0]['score']:.3f}" in text
    flt = {"must": [{"key": "detected_class", "match": {"value": "person"}}]}
    _, fitems = r.search_similar_diverse(similarity_threshold=-1.0, max_results=5, query_filter=flt)
    assert [it["id"] for it in fitems] == [h.id for h in st.search_mmr(r.region_embeddings[0], 5, score_threshold=-1.0,
                                                                       query_filter=flt)]
    assert all(int(it["id"][1:]) % 2 == 1 for it in fitems)
    text, items = r.search_similar_diverse(similarity_threshold=1.5)
    assert items == [] and "No similar regions found above threshold 1.5" in text


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    x = _planted(20_037, 1024, seed=15)
    G = _gallery(x)
    q = _queries(x, 5, seed=16)
    for k, C in ((10, 100), (50, 1024)):
        _assert_offset_moves_the_indices_only(
            lambda off: G.search_mmr(q, k=k, candidates=C, diversity=0.3, index_offset=off), {2})
    G.close()
