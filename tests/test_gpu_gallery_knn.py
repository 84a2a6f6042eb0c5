"""Exact kNN graph of one gallery (revo_gallery_knn, include/revo.h KNN; Gallery.knn, GalleryStore.neighbor_graph,
SimpleReverso.similarity_graph): bit for bit against the lists built from revo_gallery_pairs' own scores, against an fp64
oracle with the level estimate live, on a block of identical rows, with every path of the call (level modes, a workspace
that loses keys) held to the same bytes, on edge cases, against the pairs' score bits, and through the store and the facade."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store

from test_gpu_gallery_pairs import _delta, _gallery, _planted

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEG = float("-inf")


_OPEN = []                                                               # the galleries of the shared cases


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_cases():
    """behind the module's last test: the shared galleries and references go, and their memory goes back to the device"""
    yield
    for G in _OPEN:
        G.close()
    _OPEN.clear()
    _case.cache_clear()
    _big.cache_clear()
    torch.cuda.empty_cache()


def _same(a, b, what=""):
    for x, y, name in zip(a, b, ("scores", "indices", "counts")):
        if x.dtype == torch.float32:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name)
        else:
            assert torch.equal(x, y), (what, name)


def _lists_from_pairs(G, N, allow=None):
    """[N, N] fp32 on the device: entry (i, j) = the PAIRS score of rows i and j, -inf on the diagonal and wherever a row is
    not allowed -- from Gallery.pairs(-2.0), which returns every pair of allowed rows -- and each row's columns ordered by
    (score desc, index asc): (sorted scores, sorted indices)."""
    pairs, scores = G.pairs(-2.0, allow=allow)
    n_ok = N if allow is None else int(allow.sum())
    assert pairs.shape[0] == n_ok * (n_ok - 1) // 2
    S = torch.full((N, N), NEG, dtype=torch.float32, device=DEV)
    S[pairs[:, 0], pairs[:, 1]] = scores
    S[pairs[:, 1], pairs[:, 0]] = scores
    return torch.sort(S, dim=1, descending=True, stable=True)            # stable: equal scores stay index-ascending


def _expected(sorted_s, sorted_i, k, threshold=None):
    N = sorted_s.shape[0]
    s = torch.full((N, k), NEG, dtype=torch.float32, device=DEV)
    i = torch.full((N, k), -1, dtype=torch.int64, device=DEV)
    kk = min(k, N)
    s[:, :kk], i[:, :kk] = sorted_s[:, :kk], sorted_i[:, :kk]
    ok = s > NEG if threshold is None else (s > NEG) & (s >= threshold)
    s = torch.where(ok, s, torch.full_like(s, NEG))
    i = torch.where(ok, i, torch.full_like(i, -1))
    return s, i, ok.sum(1).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(D):
    """N = 1 500 (6 row tiles, the last of 220 rows; 21 tile pairs) planted rows at width D, with the reference lists of the
    whole gallery and of a random half of it.  Computed once, never changed."""
    N = 1500
    x = _planted(N, D, seed=100 + D)
    G = _gallery(x)
    _OPEN.append(G)
    allow = torch.from_numpy(np.random.default_rng(D).random(N) < 0.5).to(DEV)
    return x, allow, _lists_from_pairs(G, N), _lists_from_pairs(G, N, allow), G


# ---- 1. bit-exact against lists built from the pairs' own scores ------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 192, 1024])
def test_equals_the_lists_built_from_pairs(D):
    x, allow, full, half, G = _case(D)
    N = x.shape[0]
    for k in (1, 10, 64):
        _same(G.knn(k), _expected(*full, k), f"k={k}")
        got = G.knn(k, score_threshold=0.85)
        _same(got, _expected(*full, k, 0.85), f"k={k} threshold")
        assert 0 < int((got[2] > 0).sum()) < N                            # the threshold cuts some lists and not others
        got = G.knn(k, allow=allow)
        _same(got, _expected(*half, k), f"k={k} filter")
        assert (got[2][~allow] == 0).all() and (got[2][allow] == min(k, int(allow.sum()) - 1)).all()
        listed = got[1][got[1] >= 0]
        assert allow[listed].all()                                       # a disallowed row is nobody's neighbour
        assert (got[1][~allow] == -1).all() and torch.isneginf(got[0][~allow]).all()
    st = G.search_stats()
    assert st["join_passes"] == 1 and st["large_k_fallback"] == 0
    assert st["uncertified"] == 0 and st["bruteforced"] == 0 and st["checked"] == 0 and st["from_segments"] == 0


# ---- 2. the fp64 oracle, with the level estimate live -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    N, D = 20_000, 256
    G = _gallery(_planted(N, D, seed=21))
    _OPEN.append(G)
    return G, G.read()


def test_matches_the_fp64_oracle_with_estimated_levels():
    G, rows = _big()
    N, D = rows.shape
    k = 10
    delta = _delta(D)
    s, idx, cnt = G.knn(k)
    st = G.search_stats()
    print("knn stats at N = 20000:", st)
    assert (cnt == k).all() and (idx >= 0).all()
    assert not (idx == torch.arange(N, device=DEV)[:, None]).any()
    assert (s[:, :-1] >= s[:, 1:]).all()
    X = rows.to(torch.float64)
    for a in range(0, N, 4096):
        b = min(N, a + 4096)
        S = X[a:b] @ X.T
        S[torch.arange(b - a, device=DEV), torch.arange(a, b, device=DEV)] = NEG
        kth = torch.topk(S, k, dim=1).values[:, -1:]
        got = torch.zeros_like(S, dtype=torch.bool)
        got.scatter_(1, idx[a:b], True)
        assert int(got.sum()) == (b - a) * k                             # k distinct rows each
        assert not ((S >= kth + delta) & ~got).any()                     # every row clearly inside is there
        assert not (got & (S < kth - delta)).any()                       # nothing clearly outside is
        assert (torch.gather(S, 1, idx[a:b]) - s[a:b].to(torch.float64)).abs().max() <= delta
    # the fast path is what was tested: at least 90 % of the rows were certified without the fallback
    assert st["join_passes"] == 1 and st["large_k_fallback"] <= N // 10, st
    _same(G.knn(k), (s, idx, cnt), "second call")                        # two calls: identical bytes


# ---- 3. ties -------------------------------------------------------------------------------------------------------------
def test_a_block_of_identical_rows():
    N, D, k = 1500, 64, 10
    x = _planted(N, D, seed=31)
    lo, hi = 400, 700
    x[lo:hi] = x[lo]
    G = _gallery(x)
    s, idx, cnt = G.knn(k)
    assert (cnt == k).all()
    block = np.arange(lo, hi)
    for i in (lo, lo + 1, lo + 5, lo + 10, lo + 11, lo + 150, hi - 1):
        want = [j for j in block.tolist() if j != i][:k]                  # the 10 lowest OTHER block rows: never itself
        assert idx[i].tolist() == want, i
    sb = s[lo:hi].view(torch.int32)
    assert (sb == sb[0, 0]).all() and abs(float(s[lo, 0]) - 1.0) <= 1e-6
    assert not (idx == torch.arange(N, device=DEV)[:, None]).any()
    G.close()


# ---- 4. every path gives the same bytes ------------------------------------------------------------------------------------
def test_every_path_gives_the_same_bytes():
    x, allow, full, half, _ = _case(192)
    N = x.shape[0]
    lib = _lib.load_exp()
    G = engine.Gallery(x.shape[1], N, device=0, experiments=True)
    G.add(torch.from_numpy(x).to(DEV))
    try:
        for k, thr, alw, small in ((10, None, None, 1000), (64, None, allow, 1000), (10, 0.85, None, 10)):
            assert lib.revo_debug_set_knn(0, 0) == 0
            base = G.knn(k, score_threshold=thr, allow=alw)
            _same(base, _expected(*(full if alw is None else half), k, thr), "default")
            st = G.search_stats()
            assert st["large_k_fallback"] == 0 and st["join_passes"] == 1 and st["collected_rows"] > 0
            n_ok = N if alw is None else int(alw.sum())
            for mode in (1, 2, 3):
                assert lib.revo_debug_set_knn(0, mode) == 0
                _same(G.knn(k, score_threshold=thr, allow=alw), base, f"level_mode {mode}")
                st = G.search_stats()
                assert st["join_passes"] == 1
                if mode == 2:                                            # nothing is a candidate: every allowed row falls back
                    assert st["collected_rows"] == 0 and st["large_k_fallback"] == n_ok
            assert lib.revo_debug_set_knn(small, 0) == 0                 # room for a few of the candidate keys: keys are lost
            _same(G.knn(k, score_threshold=thr, allow=alw), base, "small workspace")
            st = G.search_stats()
            assert st["large_k_fallback"] > 0 and st["join_passes"] == 1 and st["collected_rows"] == small
            assert st["uncertified"] == 0 and st["bruteforced"] == 0 and st["checked"] == 0
    finally:
        assert lib.revo_debug_set_knn(0, 0) == 0
    G.close()


def test_every_path_gives_the_same_bytes_with_estimated_levels():
    """N = 20 000: the levels come from the sample pass, so a raised level (mode 3) leaves some rows short and others not"""
    _, rows = _big()
    N = rows.shape[0]
    lib = _lib.load_exp()
    G = engine.Gallery(rows.shape[1], N, device=0, experiments=True)
    G.add(rows, normalize=False)
    try:
        for k in (1, 10):
            assert lib.revo_debug_set_knn(0, 0) == 0
            base = G.knn(k)
            fb0 = G.search_stats()["large_k_fallback"]
            assert fb0 <= N // 10
            assert lib.revo_debug_set_knn(0, 3) == 0
            _same(G.knn(k), base, f"k={k} level_mode 3")
            fb3 = G.search_stats()["large_k_fallback"]
            print(f"k={k}: fallback rows {fb0} by the estimate, {fb3} with the level raised")
            assert fb3 > fb0 and (k != 1 or fb3 < N)
            assert lib.revo_debug_set_knn(0, 1) == 0
            if k == 1:
                _same(G.knn(k), base, "level_mode 1")                    # 2e8 pairs: keys are lost, rows fall back
                assert G.search_stats()["large_k_fallback"] > 0
            assert lib.revo_debug_set_knn(100_000, 0) == 0
            _same(G.knn(k), base, f"k={k} small workspace")
            st = G.search_stats()
            assert st["large_k_fallback"] > fb0 and st["join_passes"] == 1
    finally:
        assert lib.revo_debug_set_knn(0, 0) == 0
    G.close()


def test_a_large_block_of_identical_rows_takes_the_fallback_alone():
    """3 000 identical rows among 20 000: each has 2 999 equal partners, more than any workspace sized for k neighbours holds.
    The counting pass sends the block's rows (and few others) to the fallback; the result is that of the exhaustive path."""
    _, rows = _big()
    N, k = rows.shape[0], 10
    lo, hi = 5000, 8000
    x = rows.clone()
    x[lo:hi] = x[lo]
    lib = _lib.load_exp()
    G = engine.Gallery(rows.shape[1], N, device=0, experiments=True)
    G.add(x, normalize=False)
    try:
        assert lib.revo_debug_set_knn(0, 0) == 0
        base = G.knn(k)
        st = G.search_stats()
        print("dense block:", st)
        assert hi - lo <= st["large_k_fallback"] <= hi - lo + N // 10 and st["collected_rows"] < 100 * N
        s, idx, cnt = base
        for i in (lo, lo + 3, lo + 10, lo + 11, hi - 1):
            assert idx[i].tolist() == [j for j in range(lo, lo + k + 1) if j != i][:k], i
        assert (s[lo:hi].view(torch.int32) == s[lo, 0].view(torch.int32)).all()
        assert lib.revo_debug_set_knn(0, 2) == 0                         # every row by the exhaustive fallback
        _same(G.knn(k), base, "level_mode 2")
        assert G.search_stats()["large_k_fallback"] == N
    finally:
        assert lib.revo_debug_set_knn(0, 0) == 0
    G.close()


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------------
def _raw(G, k, has_thr=0, thr=0.0):
    n = C.c_int64(-5)
    return G._lib.revo_gallery_knn(G._h, k, has_thr, thr, C.byref(n), _lib.current_stream()), n.value


def _raw_read(G, start, n, k):
    idx = torch.full((max(n, 1), k), -7, dtype=torch.int64, device=DEV)
    s = torch.full((max(n, 1), k), -7.0, dtype=torch.float32, device=DEV)
    c = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    rc = G._lib.revo_gallery_knn_read(G._h, start, n, _lib.ptr(idx), _lib.ptr(s), _lib.ptr(c), 1)
    return rc, (s[:n], idx[:n], c[:n])


@pytest.mark.parametrize("N", [0, 1, 2, 255, 256, 257, 513])
def test_small_galleries_and_padding(N):
    D, k = 64, 64 if N == 257 else 5
    x = _planted(N, D, seed=40 + N) if N else np.zeros((0, D), np.float32)
    G = _gallery(x, extra=4)
    s, idx, cnt = G.knn(k)
    assert s.shape == (N, k) and idx.shape == (N, k) and cnt.shape == (N,)
    st = G.search_stats()
    assert st["join_passes"] == (1 if N else 0) and st["large_k_fallback"] == 0
    if N >= 2:
        _same((s, idx, cnt), _expected(*_lists_from_pairs(G, N), k), f"N={N}")
    assert (cnt == min(k, max(N - 1, 0))).all()                          # k larger than the number of other rows: padding
    pad = torch.arange(k, device=DEV)[None, :] >= cnt[:, None]
    assert (idx[pad] == -1).all() and torch.isneginf(s[pad]).all() and (idx[~pad] >= 0).all()
    if N == 257:
        s2, idx2, cnt2 = G.knn(300 // 5, score_threshold=0.85)
        _same((s2, idx2, cnt2), _expected(*_lists_from_pairs(G, N), 60, 0.85), "threshold")
        one = torch.zeros(N, dtype=torch.bool, device=DEV)
        one[100] = True
        s1, idx1, cnt1 = G.knn(5, allow=one)                             # a filter that allows one row: it has no neighbour
        assert (cnt1 == 0).all() and (idx1 == -1).all() and torch.isneginf(s1).all()
        none = torch.zeros(N, dtype=torch.bool, device=DEV)
        assert (G.knn(5, allow=none)[2] == 0).all()
    G.close()


def test_more_tile_pairs_than_workgroups():
    """N = 5 889: 23 row tiles, 276 tile pairs for the one workgroup per CU, so a workgroup's range of the join's walk
    (csrc/tile_walk.h) crosses a row of the triangle.  Fewer rows than the level's sample: every pair is a candidate."""
    N, D, k = 5889, 64, 10
    G = _gallery(_planted(N, D, seed=77))
    want = _expected(*_lists_from_pairs(G, N), k)
    _same(G.knn(k), want, "N=5889")
    st = G.search_stats()
    assert st["large_k_fallback"] == 0
    G.close()


def test_refusals_and_result_lifetime():
    N, D = 600, 64
    x = _planted(N, D, seed=50)
    K = _gallery(x[:300], keep_f32=False)
    assert _raw(K, 5) == (-2, -5) and b"keep_f32" in K._lib.revo_last_error()
    with pytest.raises(_lib.RevoError):
        K.knn(5)
    K.close()
    G = _gallery(x, extra=5)
    assert _raw_read(G, 0, 1, 5)[0] == -2 and b"no result" in G._lib.revo_last_error()       # before any call
    for k in (0, 65):
        assert _raw(G, k) == (-2, -5) and b"[1, 64]" in G._lib.revo_last_error()
    assert _raw(G, 5, 1, float("nan")) == (-2, -5) and b"NaN" in G._lib.revo_last_error()
    assert G._lib.revo_gallery_knn(G._h, 5, 0, 0.0, None, _lib.current_stream()) == -2
    assert _raw(G, 5) == (0, N)
    rc, got = _raw_read(G, 0, N, 5)
    assert rc == 0
    _same(got, G.knn(5), "raw read")
    rc, part = _raw_read(G, 97, 100, 5)                                  # a page, and each pointer alone
    assert rc == 0
    _same(part, tuple(t[97:197] for t in got), "page")
    only = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    assert G._lib.revo_gallery_knn_read(G._h, 0, N, None, None, _lib.ptr(only), 1) == 0 and torch.equal(only, got[2])
    assert G._lib.revo_gallery_knn_read(G._h, 0, N, None, None, None, 1) == 0
    assert _raw_read(G, N - 3, 4, 5)[0] == -2 and b"past the result" in G._lib.revo_last_error()
    assert _raw_read(G, N, 0, 5)[0] == 0
    # a pairs result survives a knn call, and a knn result a pairs call
    p1, s1 = G.pairs(0.8)
    assert p1.shape[0] > 10
    knn1 = G.knn(7, score_threshold=0.5)
    pr = torch.empty_like(p1)
    sr = torch.empty_like(s1)
    assert G._lib.revo_gallery_pairs_read(G._h, 0, p1.shape[0], _lib.ptr(pr), _lib.ptr(sr), 1) == 0
    assert torch.equal(pr, p1) and torch.equal(sr.view(torch.int32), s1.view(torch.int32))
    G.pairs(0.9)
    G.clusters(0.9)
    G.search_range(G.read(0, 3), 0.9)
    rc, again = _raw_read(G, 0, N, 7)
    assert rc == 0
    _same(again, knn1, "after pairs, clusters and a range search")
    G.add(torch.from_numpy(x[:5]).to(DEV))                               # rows changed: no result
    assert _raw_read(G, 0, 1, 7)[0] == -2 and b"no result" in G._lib.revo_last_error()
    G.knn(3)
    keep = torch.ones(N + 5, dtype=torch.bool, device=DEV)
    keep[0] = False
    G.remove(~keep)
    assert _raw_read(G, 0, 1, 3)[0] == -2
    G.knn(3)
    G.clear()
    assert _raw_read(G, 0, 0, 3)[0] == -2
    G.close()


def test_stale_filter_is_refused():
    x = _planted(3000, 64, seed=51)
    G = _gallery(x, extra=10)
    bits = G.allow_bits(torch.ones(3000, dtype=torch.bool, device=DEV))
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), 3000, 1, _lib.current_stream()) == 0
    G.add(torch.from_numpy(x[:10]).to(DEV))
    assert _raw(G, 5) == (-2, -5) and b"set it again" in G._lib.revo_last_error()
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    G.close()


# ---- 6. symmetry with pairs -------------------------------------------------------------------------------------------------
def test_scores_are_the_pairs_bits():
    G, rows = _big()
    k, t = 10, 0.8
    s, idx, cnt = G.knn(k)
    pairs, ps = G.pairs(t)
    assert pairs.shape[0] > 500
    seen = 0
    for a, b in ((0, 1), (1, 0)):                                        # (i, j) in i's list, and in j's
        hit = idx[pairs[:, a]] == pairs[:, b][:, None]
        listed = hit.any(1)
        seen += int(listed.sum())
        got = s[pairs[:, a]][hit]
        assert torch.equal(got.view(torch.int32), ps[listed].view(torch.int32))
    assert seen > 500


# ---- 7. store and facade ---------------------------------------------------------------------------------------------------
def test_store_neighbor_graph():
    N, D = 3000, 128
    vec = _planted(N, D, seed=60)
    payloads = [{"image_source": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2]} for r in range(N)]
    ids = [f"p{r}" for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(vec), ids, payloads)
    s, idx, cnt = st.gallery.knn(3)
    g = st.neighbor_graph(limit=3)
    assert g.ids == ids and len(g.scores) == 3 * N
    assert g.offsets_row.tolist() == np.repeat(np.arange(N), 3).tolist()
    assert g.offsets_col.tolist() == idx.cpu().numpy().reshape(-1).tolist()
    assert g.scores.tobytes() == s.cpu().numpy().reshape(-1).tobytes()
    assert g.pairs()[0] == ("p0", f"p{int(idx[0, 0])}", float(s[0, 0]))
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    f = st.neighbor_graph(limit=3, query_filter=flt)
    assert f.ids == ids[0::2] and len(f.scores) == 3 * len(f.ids)
    even = torch.zeros(N, dtype=torch.bool, device=DEV)
    even[0::2] = True
    se, ie, _ = st.gallery.knn(3, allow=even)
    assert (f.offsets_col * 2).tolist() == ie[0::2].cpu().numpy().reshape(-1).tolist()
    assert f.scores.tobytes() == se[0::2].cpu().numpy().reshape(-1).tobytes()
    cut = st.neighbor_graph(limit=3, score_threshold=0.8)
    assert 0 < len(cut.scores) < 3 * N and (cut.scores >= 0.8).all() and cut.ids == ids
    a = st.neighbor_graph(limit=3, sample=100, seed=0)
    b = st.neighbor_graph(limit=3, sample=100, seed=0)
    assert len(a.ids) == 100 and a.ids == b.ids and a.pairs() == b.pairs()                     # deterministic
    assert len(a.scores) == 300 and int(a.offsets_col.max()) < 100 and int(a.offsets_col.min()) >= 0
    assert {x for p in a.pairs() for x in p[:2]} <= set(a.ids)            # every neighbour is inside the sample
    assert st.neighbor_graph(limit=3, sample=100, seed=1).ids != a.ids
    both = st.neighbor_graph(limit=2, query_filter=flt, sample=50, seed=2)
    assert len(both.ids) == 50 and all(int(i[1:]) % 2 == 0 for i in both.ids)


def test_similarity_graph_on_a_database(tmp_path):
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, graph = r.similarity_graph()
    assert text.startswith("❌") and graph == []
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(61)
    for n in range(6):
        arr = (rng.integers(0, 256, (3,)) + rng.integers(0, 80, (96, 120, 3))) % 256
        Image.fromarray(arr.astype(np.uint8)).save(str(folder / f"img_{n}.jpg"), quality=90)
    assert "✅" in r.create_database(str(folder), "graph", use_direct_pe=True)
    db = r.vector_db
    text, graph = r.similarity_graph(max_neighbors=2)
    assert text.startswith("🎯") and len(graph) == len(db)
    s, idx, cnt = db.gallery.knn(2)
    names = [p["filename"] for p in db.payloads]
    assert [e["filename"] for e in graph] == names and all(n.endswith(".jpg") for n in names)
    for row, e in enumerate(graph):
        assert set(e) == {"filename", "image_source", "bbox", "id", "neighbors"}
        assert [m["filename"] for m in e["neighbors"]] == [names[j] for j in idx[row, :int(cnt[row])].tolist()]
        assert [m["score"] for m in e["neighbors"]] == s[row, :int(cnt[row])].tolist()
        assert e["filename"] in text
    text, graph = r.similarity_graph(max_neighbors=2, similarity_threshold=1.5)
    assert all(e["neighbors"] == [] for e in graph)
    text, graph = r.similarity_graph(max_neighbors=500)                  # the facade never raises to the UI
    assert text.startswith("❌") and graph == []
