"""Range search (revo_search_range, include/revo.h RANGE; Gallery.search_range, GalleryStore.search_range /
search_range_batch, SimpleReverso.search_all_similar) against an fp64 oracle of the fp32 rows, bit for bit against the
large-k search, with a planted row that only the rounding bound keeps, under filters, on 2 000 identical rows (the
workspace regrow), on edge cases and errors, through the store and the facade, and against the near-duplicate pairs."""
import ctypes as C

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _delta(D):
    """the fp32 chain's band: 3e-7 at D = 1024 (test_gpu_search.py), scaled with D, never below that"""
    return 3e-7 * max(1.0, D / 1024)


def _planted(N, D, seed, n_clusters=None):
    """N rows: random directions, and clusters of perturbed copies of a few of them (scores from about 0.8 to 0.95)."""
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


def _gallery(x, keep_f32=True, extra=0):
    G = engine.Gallery(x.shape[1], max(1, x.shape[0] + extra), device=0, keep_f32=keep_f32)
    if x.shape[0]:
        G.add(torch.from_numpy(x).to(DEV))
    return G


def _normalised(q):
    """the fp32 query rows the library scores (the same normalisation kernel as an append)"""
    T = engine.Gallery(q.shape[1], q.shape[0], device=0)
    T.add(q)
    r = T.read()
    T.close()
    return r


def _queries(x, Q, seed):
    """Q queries: perturbed gallery rows (hits in the planted clusters) and random directions"""
    rng = np.random.default_rng(seed)
    src = x[rng.integers(0, x.shape[0], Q)] if x.shape[0] else rng.standard_normal((Q, x.shape[1])).astype(np.float32)
    q = src / np.linalg.norm(src, axis=1, keepdims=True)
    q = q + 0.2 * rng.standard_normal(q.shape).astype(np.float32) / np.sqrt(x.shape[1])
    q[::3] = rng.standard_normal(q[::3].shape).astype(np.float32)
    return torch.from_numpy(q.astype(np.float32)).to(DEV)


def _entries_query(off):
    """the query id of every result entry"""
    cnt = (off[1:] - off[:-1]).to(torch.int64)
    return torch.repeat_interleave(torch.arange(cnt.shape[0], device=off.device), cnt)


def _check_against_oracle(off, idx, sc, qrows, rows, t, delta, allow=None, index_offset=0):
    """sets against the fp64 scores of the fp32 rows (every row >= t + delta returned, none < t - delta), each score to 1e-6,
    the order (score desc, index asc) and the CSR layout.  Returns the fp64 score matrix."""
    Q, N = qrows.shape[0], rows.shape[0]
    assert off.shape == (Q + 1,) and int(off[0]) == 0 and int(off[-1]) == idx.shape[0] == sc.shape[0]
    assert bool((off[1:] >= off[:-1]).all())
    S = qrows.to(torch.float64) @ rows.to(torch.float64).T
    ok = torch.ones(N, dtype=torch.bool, device=DEV) if allow is None else allow.to(DEV)
    qe = _entries_query(off)
    r = idx - index_offset
    assert bool(((r >= 0) & (r < N)).all())
    got = torch.zeros((Q, N), dtype=torch.bool, device=DEV)
    got[qe, r] = True
    assert int(got.sum()) == idx.shape[0]                                    # no row twice for a query
    must = (S >= t + delta) & ok[None, :]
    may = (S >= t - delta) & ok[None, :]
    assert not bool((must & ~got).any()), torch.nonzero(must & ~got)[:10].tolist()
    assert not bool((got & ~may).any()), torch.nonzero(got & ~may)[:10].tolist()
    if idx.shape[0]:
        assert float((sc.to(torch.float64) - S[qe, r]).abs().max()) <= 1e-6
        same = qe[1:] == qe[:-1]
        ordered = (sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (r[:-1] < r[1:]))
        assert bool((ordered | ~same).all())
    return S


def _stats_are_the_range_search(G, n):
    st = G.search_stats()
    assert st["join_passes"] in (1, 2) and st["collected_rows"] >= n      # (2: the workspace grew for thousands of hits)
    assert st["uncertified"] == st["bruteforced"] == st["checked"] == st["from_segments"] == 0
    assert st["grouped_fallback"] == st["large_k_fallback"] == 0


# ---- 1. exactness against the fp64 oracle ---------------------------------------------------------------------------------
_DS = [64, 768, 1024, 1280]
_CASES = [(Q, 20_037, _DS[i % 4]) for i, Q in enumerate([1, 64, 65, 128, 129, 192, 193, 256, 257, 1500])]
_CASES += [(65, N, 1024) for N in (1, 255, 256, 257)] + [(129, 20_037, 64)]


@pytest.mark.parametrize("Q,N,D", _CASES)
def test_matches_the_fp64_oracle(Q, N, D):
    x = _planted(N, D, seed=N + D + Q)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    q = _queries(x, Q, seed=Q)
    qrows = _normalised(q)
    # no hits, a few (the planted clusters), thousands per query (random directions at D = 64: ~20 % of the rows)
    for t in (1.0 + 4 * delta, 0.7, 0.1 if D == 64 else 0.02):
        off, idx, sc = G.search_range(q, t)
        S = _check_against_oracle(off, idx, sc, qrows, rows, t, delta)
        _stats_are_the_range_search(G, idx.shape[0])
        if t > 1.0:
            assert idx.shape[0] == 0
        elif t < 0.5 and N > 1000:
            assert idx.shape[0] >= 200 * Q
    G.close()


def test_two_phases_of_query_tiles_match_the_fp64_oracle():
    """2304 queries are 9 query tiles: the join's launch is a pinned phase of 8 and a last phase of 1 (scan_plan.h; the phase
    table is tests/test_scan_plan.py's test_the_two_phase_launch_of_the_small_gpu_cases).  At 0.7 a perturbed query keeps its own row and its cluster mates, about
    2100 entries in all (fp64 on the CPU: 1884 in the first eight query tiles, 241 in the ninth): hits in both phases."""
    Q, N, D = 2304, 1024, 64
    x = _planted(N, D, seed=N + D + Q)
    G = _gallery(x)
    q = _queries(x, Q, seed=Q)
    off, idx, sc = G.search_range(q, 0.7)
    _check_against_oracle(off, idx, sc, _normalised(q), G.read(), 0.7, _delta(D))
    _stats_are_the_range_search(G, idx.shape[0])
    assert int(off[2048]) >= 100 and int(off[Q]) - int(off[2048]) >= 10, (int(off[2048]), int(off[Q]))
    G.close()


# ---- 2. bit for bit against the large-k search ---------------------------------------------------------------------------
def test_equals_the_large_k_search_bit_for_bit():
    N, D = 20_037, 1024
    rng = np.random.default_rng(21)
    x = _planted(N, D, seed=21)
    v = rng.standard_normal(D).astype(np.float32)
    x[100:1600] = v                                                          # 1 500 identical rows
    c = rng.standard_normal(D).astype(np.float32)
    c /= np.linalg.norm(c)
    x[5000:8000] = c + 0.08 * rng.standard_normal((3000, D)).astype(np.float32) / np.sqrt(D)   # a tight cluster of 3 000
    G = _gallery(x)
    q = _queries(x, 300, seed=22)
    q[0] = torch.from_numpy(v).to(DEV)
    q[1] = torch.from_numpy(c).to(DEV)
    q[2] = torch.from_numpy(x[6000]).to(DEV)
    t = 0.9
    off, idx, sc = G.search_range(q, t)
    s, i, cnt = G.search(q, k=1024, score_threshold=t)
    c_q = (off[1:] - off[:-1]).cpu()
    assert int(c_q[0]) == 1500 and int(c_q[1]) > 1024 and int(c_q[2]) > 1024           # beyond what any top-k returns
    assert torch.equal(cnt.cpu().to(torch.int64), torch.clamp(c_q, max=1024))
    offc, idxc, scc = off.cpu(), idx.cpu(), sc.cpu()
    for r in range(q.shape[0]):
        n = int(cnt[r])
        a = int(offc[r])
        assert torch.equal(idxc[a:a + n], i[r, :n].cpu()), r
        assert torch.equal(scc[a:a + n].view(torch.int32), s[r, :n].cpu().view(torch.int32)), r
    _check_against_oracle(off, idx, sc, _normalised(q), G.read(), t, _delta(D))
    G.close()


# ---- 3. the rounding bound is applied -------------------------------------------------------------------------------------
def test_a_row_only_the_rounding_bound_keeps_is_returned():
    N, D = 8192, 1024
    x = _planted(N, D, seed=23)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    # queries: the fp32 copies of planted rows; the bf16 score of a partner below t, its fp32 score well above
    X = rows.to(torch.float64)
    S = X @ X.T
    S.fill_diagonal_(0)
    i, j = torch.nonzero(S >= 0.75, as_tuple=True)
    Xb = rows.to(torch.bfloat16).to(torch.float64)
    gap = (X[i] * X[j]).sum(1) - (Xb[i] * Xb[j]).sum(1)
    k = int(torch.argmax(gap))
    assert float(gap[k]) > 4 * delta, "the planted pairs have no bf16 score below their fp32 score"
    qi, qj = int(i[k]), int(j[k])
    qrow = rows[qi:qi + 1].clone()
    qn = _normalised(qrow)                                                             # the bits the library scores
    s64 = float((qn[0].to(torch.float64) * X[qj]).sum())
    sb = float((qn[0].to(torch.bfloat16).to(torch.float64) * Xb[qj]).sum())
    assert s64 - sb > 4 * delta
    t = s64 - (s64 - sb) / 2
    assert s64 >= t + delta and sb < t
    off, idx, sc = G.search_range(qrow, t)
    assert qj in idx.cpu().tolist()                                                    # a bf16 threshold would miss it
    _check_against_oracle(off, idx, sc, qn, rows, t, delta)
    G.close()


# ---- 4. filters and index_offset -----------------------------------------------------------------------------------------
def test_filters_and_index_offset():
    N, D = 20_037, 64
    x = _planted(N, D, seed=24, n_clusters=2000)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    q = _queries(x, 200, seed=25)
    qrows = _normalised(q)
    t = 0.6
    allow = torch.from_numpy(np.random.default_rng(26).random(N) < 0.6).to(DEV)
    off, idx, sc = G.search_range(q, t, allow=allow)
    _check_against_oracle(off, idx, sc, qrows, rows, t, delta, allow=allow)
    assert idx.shape[0] > 100 and bool(allow[idx].all())
    o0, i0, s0 = G.search_range(q, t, allow=torch.zeros(N, dtype=torch.bool, device=DEV))     # nothing allowed
    assert i0.shape[0] == 0 and bool((o0 == 0).all()) and o0.shape == (201,)
    full, fi, fs = G.search_range(q, t)                                                         # the filter was cleared
    assert fi.shape[0] > idx.shape[0]
    _check_against_oracle(full, fi, fs, qrows, rows, t, delta)
    o2, i2, s2 = G.search_range(q, t, index_offset=1_000_000_007)
    assert torch.equal(o2, full) and torch.equal(i2, fi + 1_000_000_007)
    assert torch.equal(s2.view(torch.int32), fs.view(torch.int32))
    G.close()


# ---- 5. identical rows: more candidates than the first workspace holds; determinism ---------------------------------------
def test_two_thousand_identical_rows_regrow():
    D, n = 64, 2000
    v = np.random.default_rng(27).standard_normal(D).astype(np.float32)
    G = _gallery(np.repeat(v[None], n, 0))
    q = torch.from_numpy(v[None]).to(DEV)
    off, idx, sc = G.search_range(q, 0.99)
    st = G.search_stats()
    assert st["join_passes"] == 2 and st["collected_rows"] == n
    assert off.tolist() == [0, n]
    assert torch.equal(idx.cpu(), torch.arange(n))                                    # ties: index ascending
    s = sc.cpu().numpy()
    assert (s == s[0]).all() and abs(float(s[0]) - 1.0) <= 1e-6
    o2, i2, s2 = G.search_range(q, 0.99)                                              # bit-identical, one pass now
    assert torch.equal(o2, off) and torch.equal(i2, idx) and torch.equal(s2.view(torch.int32), sc.view(torch.int32))
    assert G.search_stats()["join_passes"] == 1
    G.close()


def test_two_calls_give_identical_bytes():
    N, D = 20_037, 768
    x = _planted(N, D, seed=28)
    G = _gallery(x)
    q = _queries(x, 1500, seed=29)
    a = G.search_range(q, 0.05)
    b = G.search_range(q, 0.05)
    assert a[1].shape[0] > 100_000
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    G.close()


# ---- 6. result lifetime, edge cases, errors -------------------------------------------------------------------------------
def _raw_read(G, start, n, offsets=None):
    idx = torch.full((max(n, 1),), -7, dtype=torch.int64, device=DEV)
    sc = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=DEV)
    rc = G._lib.revo_search_range_read(G._h, _lib.ptr(offsets) if offsets is not None else None, start, n, _lib.ptr(idx),
                                       _lib.ptr(sc), 1)
    return rc, idx[:n], sc[:n]


def _raw_range(G, q, t, n_queries=None):
    n = C.c_int64(-5)
    rc = G._lib.revo_search_range(G._h, _lib.ptr(q) if q is not None else None, q.shape[0] if n_queries is None else n_queries,
                                  float(t), 0, C.byref(n), _lib.current_stream())
    return rc, n.value


def test_result_lifetime():
    N, D = 4096, 256
    x = _planted(N, D, seed=30, n_clusters=300)
    G = _gallery(x, extra=5)
    q = _queries(x, 40, seed=31)
    off, idx, sc = G.search_range(q, 0.1)
    n = idx.shape[0]
    assert n > 100
    pairs, pscores = G.pairs(0.8)                                                     # a pairs result ...
    G.search(q, k=10)                                                                 # ... and top-k searches leave it valid
    G.search(q, k=100)
    offs = torch.full((41,), -7, dtype=torch.int64, device=DEV)
    rc, i1, s1 = _raw_read(G, 0, n, offs)
    assert rc == 0 and torch.equal(offs, off) and torch.equal(i1, idx) and torch.equal(s1.view(torch.int32), sc.view(torch.int32))
    G.search_range(q[:3], 0.5)                                                        # a range search leaves the pairs valid
    p = torch.empty((pairs.shape[0], 2), dtype=torch.int64, device=DEV)
    s = torch.empty((pairs.shape[0],), dtype=torch.float32, device=DEV)
    assert G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p), _lib.ptr(s), 1) == 0
    assert torch.equal(p, pairs)
    off, idx, _ = G.search_range(q, 0.1)
    pages = [_raw_read(G, a, min(97, n - a)) for a in range(0, n, 97)]               # pages == one read
    assert all(rc == 0 for rc, _, _ in pages) and torch.equal(torch.cat([i for _, i, _ in pages]), idx)
    rc, _, _ = _raw_read(G, n - 3, 4)                                                 # past the result
    assert rc == -2 and b"past the result" in G._lib.revo_last_error()
    assert _raw_read(G, n, 0)[0] == 0
    G.add(torch.from_numpy(x[:5]).to(DEV))                                            # rows changed: no result
    rc, _, _ = _raw_read(G, 0, 1)
    assert rc == -2 and b"no result" in G._lib.revo_last_error()
    assert _raw_read(G, 0, 0)[0] == -2
    G.search_range(q, 0.1)
    G.clear()
    assert _raw_read(G, 0, 0)[0] == -2 and b"no result" in G._lib.revo_last_error()
    G.close()


def test_edge_cases_and_errors():
    N, D = 3000, 128
    x = _planted(N, D, seed=32)
    G = _gallery(x)
    q = _queries(x, 10, seed=33)
    off, idx, sc = G.search_range(q[:0], 0.5)                                         # no queries
    assert off.tolist() == [0] and idx.shape == (0,) and sc.shape == (0,)
    assert G.search_stats()["join_passes"] == 0
    rc, n = _raw_range(G, q, float("nan"))
    assert rc == -2 and b"NaN" in G._lib.revo_last_error() and n == -5
    rc, n = _raw_range(G, q, 0.5, n_queries=-1)
    assert rc == -2 and b"negative" in G._lib.revo_last_error()
    with pytest.raises(_lib.RevoError):
        G.search_range(q, float("nan"))
    bits = G.allow_bits(torch.ones(N, dtype=torch.bool, device=DEV))                  # a stale filter
    G.close()
    S = _gallery(x, extra=10)
    assert S._lib.revo_search_set_filter(S._h, _lib.ptr(bits), N, 1, _lib.current_stream()) == 0
    S.add(torch.from_numpy(x[:10]).to(DEV))
    rc, _ = _raw_range(S, q, 0.5)
    assert rc == -2 and b"set it again" in S._lib.revo_last_error()
    S._lib.revo_search_set_filter(S._h, None, 0, 0, None)
    S.close()
    K = _gallery(x[:300], keep_f32=False)                                             # no fp32 master rows
    rc, _ = _raw_range(K, q, 0.5)
    assert rc == -2 and b"keep_f32" in K._lib.revo_last_error()
    K.close()
    E = engine.Gallery(D, 10, device=0)                                               # empty gallery
    off, idx, _ = E.search_range(q, -1.0)
    assert off.tolist() == [0] * 11 and idx.shape == (0,)
    E.close()


def test_too_many_candidates_is_refused():
    D, N, Q = 64, (1 << 18) + 1000, 1024          # 1 024 x 263 144 = 269 459 456 candidates > 2^28 at a threshold of -1
    rng = np.random.default_rng(34)
    G = _gallery(rng.standard_normal((N, D)).astype(np.float32))
    q = torch.from_numpy(rng.standard_normal((Q, D)).astype(np.float32)).to(DEV)
    rc, _ = _raw_range(G, q, -1.0)
    assert rc == -2 and b"269459456 candidates exceed" in G._lib.revo_last_error()
    assert _raw_read(G, 0, 0)[0] == -2                                               # no result
    off, idx, _ = G.search_range(q[:2], 0.6)                                          # the handle still works
    assert off.shape == (3,)
    G.close()


# ---- 7. store and facade ---------------------------------------------------------------------------------------------------
def _store(N, D, seed):
    x = _planted(N, D, seed=seed, n_clusters=N // 10)
    payloads = [{"image_source": f"img{r}.jpg", "filename": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1]} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    return st, x


def test_store_search_range_equals_the_engine():
    st, x = _store(5000, 256, seed=35)
    q = _queries(x, 12, seed=36)
    t = 0.5
    off, idx, sc = st.gallery.search_range(q, t)
    off, idx, sc = off.tolist(), idx.tolist(), sc.tolist()
    batch = st.search_range_batch(q.cpu().numpy(), t)
    assert len(batch) == 12
    for r, hits in enumerate(batch):
        want = list(zip(idx[off[r]:off[r + 1]], sc[off[r]:off[r + 1]]))
        assert [(h.id, h.score) for h in hits] == [(f"p{j}", s) for j, s in want]
        assert all(isinstance(h, store.ScoredPoint) and h.payload is st.payloads[int(h.id[1:])] for h in hits)
    assert sum(len(h) for h in batch) > 12
    one = st.search_range(q[4].cpu(), t)
    assert [(h.id, h.score) for h in one] == [(h.id, h.score) for h in batch[4]]
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    allow = torch.from_numpy(np.arange(5000) % 2 == 0).to(DEV)
    off, idx, sc = st.gallery.search_range(q, t, allow=allow)
    off, idx, sc = off.tolist(), idx.tolist(), sc.tolist()
    fb = st.search_range_batch(q, t, query_filter=flt)
    for r, hits in enumerate(fb):
        assert [(h.id, h.score) for h in hits] == [(f"p{j}", s) for j, s in zip(idx[off[r]:off[r + 1]], sc[off[r]:off[r + 1]])]
        assert all(int(h.id[1:]) % 2 == 0 for h in hits)
    # the first hits are the top-k search's
    top = st.search(q[4].cpu(), limit=5, score_threshold=t)
    assert [(h.id, h.score) for h in top] == [(h.id, h.score) for h in one[:5]]
    assert st.search_range_batch(q[:0], t) == []


def test_search_all_similar_on_a_database(tmp_path):
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    r.region_embeddings = None
    text, items = r.search_all_similar()
    assert text.startswith("❌") and items == []
    st, x = _store(3000, 64, seed=37)
    r.vector_db = st
    r.current_database = "range"
    q = torch.from_numpy(x[7] / np.linalg.norm(x[7])).to(DEV)
    r.region_embeddings = [q]
    t = 0.3
    text, items = r.search_all_similar(similarity_threshold=t)
    want = st.search_range(q, t)
    assert len(items) == len(want) > 1
    assert [(it["id"], it["score"]) for it in items] == [(h.id, h.score) for h in want]
    assert items[0]["id"] == "p7" and all(set(it) == {"filename", "image_source", "bbox", "id", "score"} for it in items)
    assert items[3]["bbox"] == st.payloads[int(items[3]["id"][1:])]["bbox"]
    assert text.startswith(f"🎯 Found {len(items)} similar regions")
    flt = {"must": [{"key": "detected_class", "match": {"value": "person"}}]}
    _, fitems = r.search_all_similar(similarity_threshold=t, query_filter=flt)
    assert [it["id"] for it in fitems] == [h.id for h in st.search_range(q, t, query_filter=flt)]
    assert all(int(it["id"][1:]) % 2 == 1 for it in fitems)
    text, items = r.search_all_similar(similarity_threshold=1.5)
    assert items == [] and "No similar regions" in text


# ---- 8. against the near-duplicate pairs -----------------------------------------------------------------------------------
def test_rows_as_queries_recover_the_pairs():
    N, D = 4096, 256
    x = _planted(N, D, seed=38, n_clusters=300)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    t = 0.85
    pairs, _ = G.pairs(t)
    p = pairs.cpu().numpy()
    assert p.shape[0] > 50
    off, idx, sc = G.search_range(rows, t)
    S = rows.to(torch.float64) @ rows.to(torch.float64).T
    Sc = S.cpu().numpy()
    off, idx = off.cpu().numpy(), idx.cpu().numpy()
    partners = {i: set() for i in range(N)}
    for a, b in p.tolist():
        partners[a].add(b)
        partners[b].add(a)
    for i in range(N):
        def far(j):
            return abs(Sc[i, j] - t) > 2 * delta
        found = set(idx[off[i]:off[i + 1]].tolist()) - {i}
        assert {j for j in partners[i] if far(j)} == {j for j in found if far(j)}, i
    G.close()


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    N, D = 20_037, 64
    x = _planted(N, D, seed=24, n_clusters=2000)
    G = _gallery(x)
    q = _queries(x, 200, seed=25)
    _assert_offset_moves_the_indices_only(lambda off: G.search_range(q, 0.6, index_offset=off), {1})
    G.close()
