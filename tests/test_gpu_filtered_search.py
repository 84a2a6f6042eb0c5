"""Filtered search (revo_search_set_filter / Gallery.search(allow=...)): the result equals the unfiltered search of a
gallery holding only the allowed rows -- bit for bit, indices mapped back -- on every scan form, in the certificate's
fallbacks and through the store's Qdrant-style query_filter."""
import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store
from oracle import search as osearch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _gallery(N, D=1024, seed=0, experiments=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = engine.Gallery(D, N, device=0, experiments=experiments)
    for s0 in range(0, N, 1 << 18):
        n = min(1 << 18, N - s0)
        G.add(torch.randn(n, D, device=DEV, generator=g))
    return G


def _queries(G, Q, seed=1):
    """Q queries: half near gallery rows (realistic high-scoring hits), half random directions."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    head = G.read(0, min(len(G), 65536))
    rows = torch.randint(0, head.shape[0], (Q,), device=DEV, generator=g)
    q = torch.randn(Q, G.dim, device=DEV, generator=g)
    q[: Q // 2] = head[rows[: Q // 2]] * 4 + q[: Q // 2] * 0.5
    return q


def _sub(G, allowed, experiments=False):
    """A gallery of the allowed rows only (the fp32 rows as stored, added with normalize=False: identical fp32 and bf16
    rows, so the two searches see the same scores)."""
    S = engine.Gallery(G.dim, max(int(allowed.numel()), 1), device=0, experiments=experiments)
    full = G.read(0, len(G))
    for s0 in range(0, int(allowed.numel()), 1 << 18):
        S.add(full[allowed[s0: s0 + (1 << 18)]], normalize=False)
    del full
    return S


def _mapped(out, allowed):
    """a sub-gallery's result with its indices mapped back to the full gallery's rows"""
    s, i, c = out
    assert int(i.max()) < int(allowed.numel())               # (checked on the host: never an out-of-range gather)
    m = torch.where(i >= 0, allowed[i.clamp(min=0)], i)
    return s, m, c


def _eq(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y), (x, y)


def _mask(N, kind, frac, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "random":
        m = torch.rand(N, device=DEV, generator=g) < frac
    elif kind == "runs":
        m = torch.zeros(N, dtype=torch.bool, device=DEV)
        run = max(1, int(1000 * frac))
        starts = torch.randint(0, N, (max(1, int(N * frac / run)),), device=DEV, generator=g)
        for s in starts.tolist():
            m[s: s + run] = True
    else:                                                     # stripes: every other row
        m = torch.arange(N, device=DEV) % 2 == 0
    if not m.any():
        m[N // 2] = True
    return m


# ---- 1. an all-ones filter is no filter ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 100_000])
def test_all_ones_filter_equals_no_filter(N):
    G = _gallery(N, seed=N)
    ones = torch.ones(N, dtype=torch.bool, device=DEV)
    for Q in ((1, 64) if N == 4096 else (1, 64, 129, 256, 1000)):
        q = _queries(G, Q, seed=Q)
        for k in (1, 10, 26, 50):
            for thr in (None, 0.05):
                _eq(G.search(q, k=k, score_threshold=thr, allow=ones), G.search(q, k=k, score_threshold=thr))


# ---- 2. filtered = unfiltered search of the sub-gallery --------------------------------------------------------------
@pytest.mark.parametrize("N,masks", [
    (100_000, [("random", 0.5), ("random", 0.1), ("random", 0.01), ("random", 0.0001), ("runs", 0.1), ("stripes", 0.5)]),
    (1_000_000, [("random", 0.5), ("random", 0.01), ("runs", 0.1), ("stripes", 0.5)]),
])
def test_filtered_equals_search_of_the_sub_gallery(N, masks):
    G = _gallery(N, seed=7)
    for kind, frac in masks:
        m = _mask(N, kind, frac)
        allowed = torch.nonzero(m).flatten()
        S = _sub(G, allowed)
        for Q in (1, 64, 300):
            q = _queries(G, Q, seed=Q + 3)
            for k in (10, 50):
                got = G.search(q, k=k, allow=m)
                want = _mapped(S.search(q, k=k), allowed)
                _eq(got, want)
                # the packed form of the same mask
                _eq(G.search(q, k=k, allow=G.allow_bits(m)), want)
        if N == 100_000:
            q = _queries(G, 8, seed=11)
            rs, ri, rc = osearch.search(S.read().cpu().numpy(), q.cpu().numpy(), 10, None)
            s, i, c = S.search(q, k=10)
            ii = i.cpu().numpy()
            assert np.array_equal(c.cpu().numpy(), rc)
            fin = np.isfinite(rs)
            assert np.array_equal(np.isfinite(s.cpu().numpy()), fin)
            assert np.abs(s.cpu().numpy()[fin] - rs[fin]).max(initial=0.0) <= 1e-5
            for r in range(ii.shape[0]):                       # near_tie: adjacent swaps inside fp32 rounding only
                for j in np.where(ii[r] != ri[r])[0]:
                    jj = int(np.where(ri[r] == ii[r][j])[0][0])
                    assert abs(jj - j) == 1 and abs(rs[r][jj] - rs[r][j]) <= 3e-7
        del S


# ---- 3. edge cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 100_000])
def test_zero_and_few_allowed_rows(N):
    G = _gallery(N, seed=3)
    q = _queries(G, 5)
    none = torch.zeros(N, dtype=torch.bool, device=DEV)
    s, i, c = G.search(q, k=10, allow=none)
    assert (c == 0).all() and (i == -1).all() and torch.isinf(s).all() and (s < 0).all()
    for n_allowed in (3, 20, 40):                              # fewer than k; fewer than ksel (32 / 64)
        m = torch.zeros(N, dtype=torch.bool, device=DEV)
        m[torch.randperm(N, device=DEV)[:n_allowed]] = True
        allowed = torch.nonzero(m).flatten()
        for k in (10, 50):
            got = G.search(q, k=k, allow=m)
            _eq(got, _mapped(_sub(G, allowed).search(q, k=k), allowed))
            assert (got[2] == min(k, n_allowed)).all()


def test_allowed_rows_only_inside_or_only_outside_the_prepass():
    N = 300_000
    G = _gallery(N, seed=4)
    for Q in (1, 64):
        n_pre = G.search_plan(Q)["prepass_rows"]
        q = _queries(G, Q)
        for m in (torch.arange(N, device=DEV) < n_pre, torch.arange(N, device=DEV) >= n_pre,
                  torch.arange(N, device=DEV) < 40, (torch.arange(N, device=DEV) >= n_pre) & (torch.arange(N, device=DEV) < n_pre + 300)):
            allowed = torch.nonzero(m).flatten()
            S = _sub(G, allowed)
            for k in (10, 50):
                _eq(G.search(q, k=k, allow=m), _mapped(S.search(q, k=k), allowed))


def test_disallowed_near_duplicates_never_seed_a_bound():
    """The query's best 200 unfiltered rows (near-duplicates, spread over the pre-pass and the scan) are all disallowed:
    had any of them seeded or raised an admission bound, the allowed rows' results would be cut short."""
    N, D = 200_000, 1024
    G0 = _gallery(N, D, seed=9)
    rows = G0.read(0, N)
    q = torch.randn(4, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    pos = torch.randperm(N, device=DEV)[:200]
    for j in range(4):                                        # 50 near-duplicates of each query
        rows[pos[j * 50:(j + 1) * 50]] = q[j] + 0.01 * torch.randn(50, D, device=DEV)
    G = engine.Gallery(D, N, device=0)
    G.add(rows)
    _, top, _ = G.search(q, k=50)
    m = torch.ones(N, dtype=torch.bool, device=DEV)
    m[pos] = False
    m[top.flatten()] = False
    allowed = torch.nonzero(m).flatten()
    for k in (10, 50):
        _eq(G.search(q, k=k, allow=m), _mapped(_sub(G, allowed).search(q, k=k), allowed))


def test_stale_filter_raises():
    G = engine.Gallery(1024, 20_100, device=0)
    G.add(torch.randn(20_000, 1024, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    m = torch.ones(20_000, dtype=torch.bool, device=DEV)
    bits = G.allow_bits(m)
    _lib.check(G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), len(G), 1, _lib.current_stream()), "set_filter")
    G.add(torch.randn(10, G.dim, device=DEV))
    q = _queries(G, 2)
    s = torch.empty((2, 5), dtype=torch.float32, device=DEV)
    i = torch.empty((2, 5), dtype=torch.int64, device=DEV)
    c = torch.empty((2,), dtype=torch.int32, device=DEV)
    rc = G._lib.revo_search_topk(G._h, _lib.ptr(q), 2, 5, 0, 0.0, 0, _lib.ptr(s), _lib.ptr(i), _lib.ptr(c),
                                 _lib.current_stream())
    assert rc != 0 and "filter" in _lib.load().revo_last_error().decode()
    _lib.check(G._lib.revo_search_set_filter(G._h, None, 0, 0, None), "set_filter")
    G.search(q, k=5)                                          # cleared: searches run again
    with pytest.raises(ValueError):                          # a mask of the old length is refused by the binding
        G.search(q, k=5, allow=m)


# ---- 4. the certificate's fallbacks under a filter -----------------------------------------------------------------
def test_fallback_modes_under_a_filter():
    N, D = 100_000, 1024
    g = torch.Generator(device=DEV).manual_seed(21)
    rows = torch.randn(N, D, device=DEV, generator=g)
    base = torch.randn(D, device=DEV, generator=g)
    rows[: 3000] = base + 0.02 * torch.randn(3000, D, device=DEV, generator=g)   # a near-duplicate cluster: certificates fail
    G = engine.Gallery(D, N, device=0, experiments=True)
    G.add(rows)
    q = torch.cat([(base + 0.02 * torch.randn(4, D, device=DEV, generator=g)), torch.randn(4, D, device=DEV, generator=g)])
    m = _mask(N, "random", 0.5)
    want = G.search(q, k=10, allow=m)
    # certified mode: the cluster's queries did fail their certificate, so the filtered fallback produced part of `want`
    assert G.search_stats()["uncertified"] >= 1, G.search_stats()
    for mode in ("collect", "bruteforce"):
        G.set_search_mode(mode)
        _eq(G.search(q, k=10, allow=m), want)
    G.set_search_mode("certified")
    allowed = torch.nonzero(m).flatten()
    _eq(want, _mapped(_sub(G, allowed).search(q, k=10), allowed))


# ---- 6. store ---------------------------------------------------------------------------------------------------------
def test_store_query_filter_equals_store_of_matching_points():
    N, D = 30_000, 256
    rng = np.random.default_rng(0)
    vec = rng.standard_normal((N, D)).astype(np.float32)
    payloads = [{"image_source": f"img{r % 50}.jpg", "detected_class": ["car", "person", "dog"][r % 3],
                 "confidence": float(rng.random())} for r in range(N)]
    ids = [f"p{r}" for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(vec), ids, payloads)
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car")),
                               filters.FieldCondition("confidence", range=filters.Range(gte=0.3))],
                         must_not=[filters.FieldCondition("image_source", match=filters.MatchValue("img3.jpg"))])
    sel = np.nonzero(st.filter_mask(flt))[0]
    sub = store.GalleryStore(D, device=0, capacity=len(sel))
    sub.upsert(torch.from_numpy(vec[sel]), [ids[j] for j in sel], [payloads[j] for j in sel])
    for t in range(5):
        q = vec[rng.integers(N)] + 0.3 * rng.standard_normal(D).astype(np.float32)
        for thr in (None, 0.1):
            got = st.search(q, 10, score_threshold=thr, query_filter=flt)
            want = sub.search(q, 10, score_threshold=thr)
            assert [(h.id, h.score) for h in got] == [(h.id, h.score) for h in want]
            assert all(h.payload["detected_class"] == "car" and h.payload["image_source"] != "img3.jpg" for h in got)
            # the dict form gives the same hits; no filter gives today's result
            d = {"must": [{"key": "detected_class", "match": {"value": "car"}}, {"key": "confidence", "range": {"gte": 0.3}}],
                 "must_not": [{"key": "image_source", "match": {"value": "img3.jpg"}}]}
            assert [(h.id, h.score) for h in st.search(q, 10, score_threshold=thr, query_filter=d)] == \
                [(h.id, h.score) for h in got]
    # kept current on upsert: new points are searchable under the same filter
    st.upsert(torch.from_numpy(vec[:1] * 1.0), ["new"], [{"detected_class": "car", "confidence": 0.9, "image_source": "x"}])
    hits = st.search(vec[0], 1, query_filter=flt)
    assert hits[0].id in ("new", "p0")


# ---- 5. sharded (one process) ---------------------------------------------------------------------------------------
def test_local_shards_filtered_equal_the_unfiltered_search_of_the_sub_gallery():
    from reverso_amd import sharded
    N, D = 1_000_000, 1024
    G = _gallery(N, D, seed=17)
    full = G.read(0, N)
    m = _mask(N, "random", 0.1)
    allowed = torch.nonzero(m).flatten()
    S = _sub(G, allowed)
    q = _queries(G, 64, seed=5)
    for P in (2, 8):
        bounds = [N * p // P for p in range(P + 1)]
        shards = []
        for p in range(P):
            h = engine.Gallery(D, bounds[p + 1] - bounds[p], device=0)
            h.add(full[bounds[p]:bounds[p + 1]], normalize=False)
            shards.append(h)
        ls = sharded.LocalShards.from_galleries(shards)
        est_before = ls.estimating
        for k in (10, 50):
            s, i, c = ls.search(q, k, allow=m)
            _eq((s, i, c), _mapped(S.search(q, k=k), allowed))
        assert ls.estimating == est_before                    # a filtered search never switches the estimate off
        s, i, c = ls.search(q, 10)                            # the next unfiltered search: still the whole gallery's result
        _eq((s, i, c), G.search(q, k=10))
        ls.close()
        del shards


def _rank_worker(rank, world, port, tmp, N, k):
    """One rank of a two-rank ShardedSearch on one GPU (gloo, as tests/test_gpu_sharded.py): the rank's shard, the rank's
    slice of one global mask; results saved for the parent to compare with the single-process filtered search."""
    import os
    import sys
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import reverso_amd  # noqa: F401
    from reverso_amd import engine as eng_, sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gal, q, mask = _rank_data(N)
    lo, hi = N * rank // world, N * (rank + 1) // world
    G = eng_.Gallery(gal.shape[1], hi - lo, device=0)
    G.add(gal[lo:hi].to(DEV))
    ss = sharded.ShardedSearch.from_gallery(G)
    est0 = ss._estimating
    local = mask[lo:hi].to(DEV)
    out = {}
    for kk, thr in ((k, None), (50, None), (k, 0.02)):
        s, i, c = ss.search(q.to(DEV), kk, thr, allow=local)
        out[f"{kk}_{thr}"] = (s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy())
    # pipelined: the second search is enqueued before the first one's result is asked for (the first one's uncertified
    # queries -- the tie group -- are re-done by a repair search, which must carry the same filter)
    p1 = ss.search_async(q.to(DEV), k, None, allow=local)
    p2 = ss.search_async(q.to(DEV), 50, None, allow=local)
    for tag, p in ((f"{k}_None", p1), ("50_None", p2)):
        got = p.result()
        for a, b in zip(got, out[tag]):
            assert np.array_equal(a.cpu().numpy(), b), tag
    assert ss._estimating == est0                            # filtered searches never switch the estimate off
    s, i, c = ss.search(q.to(DEV), k)                         # unfiltered again
    out["unf"] = (s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy())
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **{f"{t}_{n}": v for t, (a, b, c) in out.items()
                                                     for n, v in (("s", a), ("i", b), ("c", c))})
    dist.barrier()
    dist.destroy_process_group()


def _rank_data(N, D=256):
    g = torch.Generator().manual_seed(31)
    gal = torch.randn(N, D, generator=g)
    gal[100:160] = gal[100]                                   # a tie group wider than the candidate lists
    q = torch.cat([torch.randn(15, D, generator=g), gal[100:101]])
    mask = torch.rand(N, generator=g) < 0.3
    mask[100:160] = True
    return gal, q, mask


def test_two_ranks_filtered_equal_the_single_process_filtered_search(tmp_path):
    import os
    import torch.multiprocessing as mp
    N, k, world = 60_001, 10, 2
    port = 29700 + (os.getpid() % 2000)
    mp.spawn(_rank_worker, args=(world, port, str(tmp_path), N, k), nprocs=world, join=True)
    gal, q, mask = _rank_data(N)
    G = engine.Gallery(gal.shape[1], N, device=0)
    G.add(gal.to(DEV))
    for kk, thr in ((k, None), (50, None), (k, 0.02)):
        s, i, c = (t.cpu().numpy() for t in G.search(q.to(DEV), kk, thr, allow=mask.to(DEV)))
        assert mask[torch.from_numpy(i[i >= 0])].all()
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), f"rank{rank}.npz"))
            for n, v in (("s", s), ("i", i), ("c", c)):
                assert np.array_equal(got[f"{kk}_{thr}_{n}"], v), (rank, kk, thr, n)
    s, i, c = (t.cpu().numpy() for t in G.search(q.to(DEV), k))
    for rank in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{rank}.npz"))
        assert np.array_equal(got["unf_i"], i) and np.array_equal(got["unf_s"], s)


# ---- the façade -------------------------------------------------------------------------------------------------------
def test_search_similar_query_filter_excludes_the_query_image(tmp_path):
    import os
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(3)
    paths = []
    for n in range(8):
        arr = (rng.integers(0, 256, (3,)) + rng.integers(0, 40, (96, 120, 3))) % 256
        p = str(folder / f"img_{n}.jpg")
        Image.fromarray(arr.astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    assert "✅" in r.create_database(str(folder), "flt", use_direct_pe=True)
    r.process_image_direct_pe(paths[2])
    text0, items0 = r.search_similar(similarity_threshold=-1.0, max_results=5)
    # (threshold -1: every cosine passes, so the lists are full and the comparisons below are of whole lists)
    assert items0[0]["filename"] == "img_2.jpg"                          # unfiltered: the query's own image first
    # the default is today's call: same text, same hits
    text1, items1 = r.search_similar(-1.0, 5, query_filter=None)
    assert text1 == text0 and [(i["filename"], i["score"]) for i in items1] == [(i["filename"], i["score"]) for i in items0]
    _, items6 = r.search_similar(-1.0, 6)
    assert items6[0]["filename"] == "img_2.jpg"
    src = r.vector_db.payloads[[p["filename"] for p in r.vector_db.payloads].index("img_2.jpg")]["image_source"]
    for flt in (filters.Filter(must_not=[filters.FieldCondition("image_source", match=filters.MatchValue(src))]),
                {"must_not": [{"key": "image_source", "match": {"value": src}}]}):
        text, items = r.search_similar(-1.0, 5, query_filter=flt)
        assert len(items) == 5 and all(i["filename"] != "img_2.jpg" for i in items)
        # exactly the unfiltered top 6 without the query's own image (one embedding per image in direct mode)
        assert [(i["filename"], i["score"]) for i in items] == [(i["filename"], i["score"]) for i in items6[1:]]
