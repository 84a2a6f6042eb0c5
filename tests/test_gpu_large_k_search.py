"""The large-k search (revo_search_topk_large, include/revo.h LARGE K; Gallery.search with 51 <= k <= 1024) against the fp64
oracle, against the k <= 50 search bit for bit, against its own exhaustive fallback bit for bit, under filters, on edge cases,
on ties that overflow the band, and through the store and the facade."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store
from oracle import search as osearch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _search_checks import _check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEAR_TIE = 3e-7
CAP = 8192                       # LARGE_CAP, kernels.h: band rows per query


def _rows(N, D, seed):
    return np.random.default_rng(seed).standard_normal((N, D), dtype=np.float32)


def _queries(gal, Q, seed):
    """Q queries: half near gallery rows, half random directions."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((Q, gal.shape[1]), dtype=np.float32)
    near = rng.integers(0, gal.shape[0], Q // 2)
    q[: Q // 2] = gal[near] * 4 + q[: Q // 2] * 0.5
    return q


def _gallery(gal, keep_f32=True, experiments=False):
    G = engine.Gallery(gal.shape[1], max(1, gal.shape[0]), device=0, keep_f32=keep_f32, experiments=experiments)
    if gal.shape[0]:
        G.add(torch.from_numpy(gal).to(DEV))
    return G


def _call(G, q, k, thr=None, offset=0, fn="revo_search_topk_large"):
    """The C entry point itself (the engine sends k <= 50 to revo_search_topk): (status, (scores, indices, counts))."""
    q = q.to(DEV).contiguous()
    Q = q.shape[0]
    s = torch.empty((max(Q, 1), k), dtype=torch.float32, device=DEV)      # (non-null outputs even for Q = 0)
    i = torch.empty((max(Q, 1), k), dtype=torch.int64, device=DEV)
    c = torch.empty((max(Q, 1),), dtype=torch.int32, device=DEV)
    rc = getattr(G._lib, fn)(G._h, _lib.ptr(q) if Q else None, Q, k, int(thr is not None), float(thr or 0.0), offset,
                             _lib.ptr(s), _lib.ptr(i), _lib.ptr(c), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, (s, i, c)


def _large(G, q, k, thr=None, offset=0):
    rc, out = _call(G, q, k, thr, offset)
    assert rc == 0, G._lib.revo_last_error()
    return out


def _eq(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _oracle(gal, qr, k, thr=None, offset=0, allow=None):
    rs, ri, rc = osearch.search(gal, qr, k, thr, allow=allow)
    return rs, np.where(ri >= 0, ri + offset, -1), rc


# ---- 1. against the fp64 oracle -----------------------------------------------------------------------------------------
CASES = [  # N, D, Q, k, threshold, index_offset
    (5_000, 64, 7, 1024, None, 0),             # small gallery (no sample), k a fifth of the rows
    (12_345, 1536, 64, 257, 0.05, 0),
    (16_384, 64, 1, 51, None, 0),              # the first size with a sample, aligned
    (70_001, 1024, 200, 100, None, 1_000),
    (70_001, 1024, 300, 1000, 0.08, 0),
    (70_144, 1024, 7, 64, 0.1, 7),
    (250_000, 1024, 64, 1024, None, 0),
    (250_000, 64, 1, 1000, None, 0),
    (20_000, 64, 1_100, 100, None, 0),         # more than one chunk of 1024 queries
]


@pytest.mark.parametrize("N,D,Q,k,thr,off", CASES)
def test_matches_the_fp64_oracle(N, D, Q, k, thr, off):
    gal = _rows(N, D, N + D)
    qr = _queries(gal, Q, Q + k)
    G = _gallery(gal)
    out = G.search(torch.from_numpy(qr).to(DEV), k, thr, index_offset=off)
    _check(out, _oracle(gal, qr, k, thr, off), atol=1e-5, near_tie=NEAR_TIE)
    st = G.search_stats()
    assert st["large_k_fallback"] == 0 and st["collected_rows"] >= min(k, N) * (Q if thr is None else 0)
    G.close()


def test_one_million_rows_few_queries():
    N, D, Q = 1_000_000, 1024, 4
    g = torch.Generator(device=DEV).manual_seed(11)
    G = engine.Gallery(D, N, device=0)
    for s0 in range(0, N, 125_000):
        G.add(torch.randn(125_000, D, device=DEV, generator=g))
    q = torch.randn(Q, D, device=DEV, generator=g)
    q[:2] = G.read(5, 2) * 4 + 0.5 * q[:2]
    qn = q.cpu().numpy()
    chunks = ((s0, G.read(s0, 125_000).cpu().numpy()) for s0 in range(0, N, 125_000))
    rs, ri, rc = osearch.search_chunked(chunks, qn, 1024)
    for k, thr in ((1024, None), (100, None), (300, 0.06)):
        r = (rs[:, :k].copy(), ri[:, :k].copy())
        if thr is not None:
            keep = r[0] >= np.float32(thr)
            r[0][~keep], r[1][~keep] = -np.inf, -1
        want = (r[0], r[1], (r[1] >= 0).sum(1).astype(np.int32))
        _check(G.search(q, k, thr), want, atol=1e-5, near_tie=6e-7)
        st = G.search_stats()
        assert st["large_k_fallback"] == 0
        print(f"k={k} thr={thr}: band rows per query {st['collected_rows'] / Q:.0f}")
    G.close()


# ---- 2. bit for bit against the other GPU paths ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,Q", [(70_001, 1024, 64), (9_000, 256, 130), (40_000, 64, 300)])
def test_prefix_equals_the_k50_search(N, D, Q):
    gal = _rows(N, D, 3)
    q = torch.from_numpy(_queries(gal, Q, 4)).to(DEV)
    G = _gallery(gal)
    for thr in (None, 0.1):
        s50, i50, c50 = G.search(q, 50, thr)
        for k in (51, 100, 1000):
            s, i, c = G.search(q, k, thr)
            assert torch.equal(s[:, :50], s50) and torch.equal(i[:, :50], i50)
            assert torch.equal(torch.clamp(c, max=50), c50)
    for k in (1, 10, 25, 26, 50):
        _eq(_large(G, q, k), G.search(q, k))
        _eq(_large(G, q, k, 0.1, 5), G.search(q, k, 0.1, index_offset=5))
    G.close()


@pytest.mark.parametrize("N,D,Q,k", [(70_001, 1024, 20, 300), (3_000, 64, 150, 1024), (20_000, 256, 257, 64)])
def test_band_path_equals_the_exhaustive_fallback(N, D, Q, k):
    gal = _rows(N, D, 5)
    q = torch.from_numpy(_queries(gal, Q, 6)).to(DEV)
    G = _gallery(gal, experiments=True)
    for thr in (None, 0.05):
        band = G.search(q, k, thr)
        assert G.search_stats()["large_k_fallback"] == 0
        G.set_search_mode("bruteforce")
        _eq(G.search(q, k, thr), band)
        assert G.search_stats()["large_k_fallback"] == Q
        G.set_search_mode("certified")
    # and the k <= 50 search leaves the slot at 0
    G.search(q, 10)
    assert G.search_stats()["large_k_fallback"] == 0
    G.close()


# ---- 3. filters -------------------------------------------------------------------------------------------------------
def _mixed_mask(N, seed):
    """Each 64-row block: all allowed, none, random 50 %, only bit 0, only bit 63, only bits 31 and 32."""
    rng = np.random.default_rng(seed)
    blocks = (N + 63) // 64
    kind = rng.integers(0, 6, blocks)
    kind[rng.permutation(blocks)[:6]] = np.arange(6)
    m = np.zeros((blocks, 64), dtype=bool)
    m[kind == 0] = True
    rnd = rng.random((blocks, 64)) < 0.5
    m[kind == 2] = rnd[kind == 2]
    m[kind == 3, 0] = True
    m[kind == 4, 63] = True
    m[kind == 5, 31] = True
    m[kind == 5, 32] = True
    return m.reshape(-1)[:N].copy()


@pytest.mark.parametrize("N", [9_001, 70_001])
@pytest.mark.parametrize("shape", ["all", "none", "random", "mixed", "single", "few"])
def test_filtered_equals_the_oracle_and_the_sub_gallery(N, shape):
    D, Q, k = 256, 66, 200
    gal = _rows(N, D, 7)
    qr = _queries(gal, Q, 8)
    rng = np.random.default_rng(9)
    m = {"all": np.ones(N, bool), "none": np.zeros(N, bool), "random": rng.random(N) < 0.3,
         "mixed": _mixed_mask(N, 10), "single": np.arange(N) == N // 2,
         "few": np.isin(np.arange(N), rng.permutation(N)[:k // 2])}[shape]   # fewer than k allowed rows
    G = _gallery(gal)
    q = torch.from_numpy(qr).to(DEV)
    for thr in (None, 0.1):
        out = G.search(q, k, thr, allow=torch.from_numpy(m).to(DEV))
        _check(out, _oracle(gal, qr, k, thr, allow=m), atol=1e-5, near_tie=NEAR_TIE)
        allowed = np.flatnonzero(m)
        if allowed.size:
            # the allowed rows as stored (normalize=False: identical fp32 and bf16 rows), searched without a filter
            a = torch.from_numpy(allowed).to(DEV)
            S = engine.Gallery(D, int(allowed.size), device=0)
            S.add(G.read(0, N)[a], normalize=False)
            ss, si, sc = S.search(q, k, thr)
            si = torch.where(si >= 0, a[si.clamp(min=0)], si)
            _eq(out, (ss, si, sc))
            S.close()
        else:
            assert (out[2] == 0).all() and (out[1] == -1).all()
    G.close()


def test_stale_filter_is_refused():
    gal = _rows(20_000, 64, 11)
    G = engine.Gallery(64, 20_010, device=0)
    G.add(torch.from_numpy(gal).to(DEV))
    m = torch.ones(20_000, dtype=torch.bool, device=DEV)
    bits = G.allow_bits(m)
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), 20_000, 1, _lib.current_stream()) == 0
    G.add(torch.from_numpy(gal[:10]).to(DEV))
    rc, _ = _call(G, torch.from_numpy(gal[:3]), 100)
    assert rc == -2 and b"set it again" in G._lib.revo_last_error()
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    G.close()


# ---- 4. edge cases ----------------------------------------------------------------------------------------------------
def test_k_at_least_the_gallery_and_empty_cases():
    gal = _rows(300, 128, 12)
    qr = _queries(gal, 5, 13)
    G = _gallery(gal)
    for k in (300, 301, 1024):
        _check(G.search(torch.from_numpy(qr).to(DEV), k), _oracle(gal, qr, k), atol=1e-5, near_tie=NEAR_TIE)
    s, i, c = G.search(torch.from_numpy(qr).to(DEV), 1024)
    assert (c == 300).all() and (i[:, 300:] == -1).all() and torch.isinf(s[:, 300:]).all()
    rc, _ = _call(G, torch.empty((0, 128)), 100)                          # Q = 0
    assert rc == 0
    G.close()
    E = engine.Gallery(128, 10, device=0)                                  # empty gallery
    s, i, c = E.search(torch.from_numpy(qr).to(DEV), 500)
    assert (c == 0).all() and (i == -1).all() and torch.isinf(s).all()
    E.close()
    N = _gallery(gal, keep_f32=False)                                     # no fp32 master rows: refused
    rc, _ = _call(N, torch.from_numpy(qr), 100)
    assert rc == -2 and b"keep_f32" in N._lib.revo_last_error()
    with pytest.raises(_lib.RevoError):
        N.search(torch.from_numpy(qr).to(DEV), 100)
    N.close()


# ---- 5. ties that overflow the band -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_rand", [8_000, 60_000])
def test_exact_duplicates_straddling_the_kth_place(N_rand):
    D, k = 64, 200
    rng = np.random.default_rng(14)
    base = rng.standard_normal(D).astype(np.float32)
    gal = rng.standard_normal((N_rand, D)).astype(np.float32)
    closer = base[None] + 0.05 * rng.standard_normal((k // 2, D)).astype(np.float32)     # fewer than k rows above the copies
    copies = np.repeat((base + 0.3 * rng.standard_normal(D).astype(np.float32))[None], CAP + 1000, 0)
    gal = np.concatenate([gal, closer, copies])
    gal = gal[rng.permutation(gal.shape[0])]
    qr = np.stack([base, base + 0.01 * rng.standard_normal(D).astype(np.float32)])
    G = _gallery(gal)
    s, i, c = G.search(torch.from_numpy(qr).to(DEV), k)
    assert G.search_stats()["large_k_fallback"] >= 1
    _check((s, i, c), _oracle(gal, qr, k), atol=1e-5, near_tie=NEAR_TIE)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    for q in range(2):
        for j in range(1, k):                                              # equal scores: indices ascending
            if s[q, j] == s[q, j - 1]:
                assert i[q, j] > i[q, j - 1]
        assert (s[q] == s[q, k - 1]).sum() > 50                            # the copies do take the tail
    G.close()


# ---- 6. store and facade ----------------------------------------------------------------------------------------------
def test_store_limit_200_with_a_query_filter():
    N, D = 30_000, 256
    rng = np.random.default_rng(15)
    vec = rng.standard_normal((N, D)).astype(np.float32)
    payloads = [{"image_source": f"img{r % 50}.jpg", "detected_class": ["car", "person", "dog"][r % 3]} for r in range(N)]
    ids = [f"p{r}" for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(vec), ids, payloads)
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    m = st.filter_mask(flt)
    for t in range(3):
        q = vec[rng.integers(N)] + 0.3 * rng.standard_normal(D).astype(np.float32)
        for f, allow in ((None, None), (flt, m)):
            got = st.search(q, 200, query_filter=f)
            assert len(got) == 200
            rs, ri, rc = osearch.search(vec, q[None], 200, allow=allow)
            want = (torch.from_numpy(np.array([[h.score for h in got]], np.float32)),
                    torch.from_numpy(np.array([[int(h.id[1:]) for h in got]], np.int64)),
                    torch.tensor([len(got)], dtype=torch.int32))
            _check(want, (rs, ri, rc), atol=1e-5, near_tie=NEAR_TIE)
            if f is not None:
                assert all(h.payload["detected_class"] == "car" for h in got)


def test_search_similar_100_results(tmp_path):
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(16)
    paths = []
    for n in range(4):
        arr = (rng.integers(0, 256, (3,)) + rng.integers(0, 40, (96, 120, 3))) % 256
        p = str(folder / f"img_{n}.jpg")
        Image.fromarray(arr.astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    assert "✅" in r.create_database(str(folder), "big", use_direct_pe=True)
    db = r.vector_db
    D = db.gallery.dim
    extra = rng.standard_normal((150, D)).astype(np.float32)
    db.upsert(torch.from_numpy(extra), [f"x{j}" for j in range(150)],
              [{"filename": f"extra_{j}.jpg", "image_source": ""} for j in range(150)])
    r.process_image_direct_pe(paths[1])
    text, items = r.search_similar(similarity_threshold=-1.0, max_results=100)
    assert len(items) == 100 and items[0]["filename"] == "img_1.jpg"
    assert text.startswith("🎯 Found 100 similar regions")
    # the oracle's order over every stored row
    rows = db.gallery.read(0, len(db)).cpu().numpy()
    q = torch.as_tensor(r.region_embeddings[0]).reshape(1, -1).float().cpu().numpy()
    rs, ri, rc = osearch.search(rows, q, 100)
    names = [db.payloads[j]["filename"] for j in ri[0]]
    got = [it["filename"] for it in items]
    gs = np.array([it["score"] for it in items], np.float64)
    assert sorted(got) == sorted(names)
    assert np.abs(gs - rs[0].astype(np.float64)).max() <= 1e-3
    for j in np.flatnonzero(np.array(got) != np.array(names)):             # only neighbours within fp32 resolution swap
        jj = names.index(got[j])
        assert abs(jj - j) == 1 and abs(rs[0][jj] - rs[0][j]) <= NEAR_TIE


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    gal = _rows(20_037, 1024, seed=81)
    G = _gallery(gal)
    q = torch.from_numpy(_queries(gal, 5, seed=82)).to(DEV)
    for k in (51, 1024):
        _assert_offset_moves_the_indices_only(lambda off: G.search(q, k, index_offset=off), {1})
    G.close()
