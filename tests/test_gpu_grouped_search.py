"""Grouped search (revo_search_groups / Gallery.search_groups / GalleryStore.search_groups / search_similar(group_by=)):
the best groups of rows, each by its best row, with each group's best rows -- exactly the grouping of an exhaustive fp32
scoring of the allowed rows.  Checked against the ungrouped search (singleton groups), the fp64 oracle on region-like
galleries, the grouped fallback forced in the experiment library, and the search of the allowed rows alone."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, store
from oracle import search as osearch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _search_checks import _check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEAR_TIE = 3e-7


def _random_gallery(N, D=1024, seed=0, experiments=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = engine.Gallery(D, N, device=0, experiments=experiments)
    for s0 in range(0, N, 1 << 17):
        G.add(torch.randn(min(1 << 17, N - s0), D, device=DEV, generator=g))
    return G


def _region_rows(N, D=1024, mode="global", seed=0):
    """Rows of a region-mode database: groups ("images") of 1-80 rows, every row of a group identical ("global": the
    image's embedding for each region) or close to the group's base ("crop"), and about 10 % ungrouped rows (-1), in
    blocks at random places.  Returns (fp32 rows [N, D] on the device, int32 groups [N] on the device)."""
    rng = np.random.default_rng(seed)
    sizes, kinds, n = [], [], 0
    while n < N:
        if rng.random() < 0.1:
            s, k = int(rng.integers(1, 40)), -1
        else:
            s, k = int(rng.integers(1, 81)), 1
        s = min(s, N - n)
        sizes.append(s)
        kinds.append(k)
        n += s
    groups = np.empty(N, np.int32)
    owner = np.empty(N, np.int64)                              # which block each row belongs to
    gid, r = 0, 0
    for b, (s, k) in enumerate(zip(sizes, kinds)):
        groups[r: r + s] = gid if k > 0 else -1
        gid += k > 0
        owner[r: r + s] = b
        r += s
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    base = torch.randn(len(sizes), D, device=DEV, generator=g)
    rows = base[torch.from_numpy(owner).to(DEV)]
    if mode == "crop":
        rows = rows + 0.15 * torch.randn(N, D, device=DEV, generator=g)
    ungrouped = torch.from_numpy(groups < 0).to(DEV)
    rows[ungrouped] = torch.randn(int(ungrouped.sum()), D, device=DEV, generator=g)
    return rows, torch.from_numpy(groups).to(DEV)


def _gallery_of(rows, experiments=False):
    G = engine.Gallery(rows.shape[1], rows.shape[0], device=0, experiments=experiments)
    for s0 in range(0, rows.shape[0], 1 << 17):
        G.add(rows[s0: s0 + (1 << 17)])
    return G


def _queries_near(rows, groups, Q, seed=2, big_first=0):
    """Q queries: `big_first` of them at rows of the largest groups (their top 50 is one group: the fallback), then half
    of the rest near random rows, the others random directions."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(Q, rows.shape[1], device=DEV, generator=g)
    if big_first:
        gr = groups.cpu().numpy()
        cnt = np.bincount(gr[gr >= 0])
        big = np.argsort(-cnt, kind="stable")[:big_first]
        first = np.array([int(np.flatnonzero(gr == b)[0]) for b in big])
        q[:big_first] = rows[torch.from_numpy(first).to(DEV)] * 4 + 0.05 * q[:big_first]
    rest = Q - big_first
    pick = torch.randint(0, rows.shape[0], (rest // 2,), device=DEV, generator=g)
    q[big_first: big_first + rest // 2] = rows[pick] * 4 + 0.5 * q[big_first: big_first + rest // 2]
    return q


def _oracle_groups(gal, groups, queries, L, S, thr=None, allow=None, sc=None):
    """Grouping of an exhaustive fp64-accumulated scoring: (scores [Q, L, S], indices, hit_counts [Q, L],
    group_ids [Q, L], group_counts [Q]) in the layout of Gallery.search_groups.  sc: that scoring [Q, N], fp64 sums
    rounded once to fp32, where the caller has it already (gal and queries are then not read)."""
    if sc is None:
        sc = osearch.cosine_scores(gal, osearch.normalize_rows(queries))     # [Q, N] fp32
    Q = sc.shape[0]
    out = (np.full((Q, L, S), -np.inf, np.float32), np.full((Q, L, S), -1, np.int64), np.zeros((Q, L), np.int32),
           np.full((Q, L), -1, np.int32), np.zeros(Q, np.int32))
    base = groups >= 0
    if allow is not None:
        base &= allow
    for q in range(Q):
        row = sc[q]
        ok = base & (row >= np.float32(thr)) if thr is not None else base
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -row[cand].astype(np.float64)))]
        gs = groups[order]
        _, first = np.unique(gs, return_index=True)
        chosen = gs[np.sort(first)][:L]
        for r, gid in enumerate(chosen):
            hits = order[gs == gid][:S]
            out[0][q, r, : len(hits)] = row[hits]
            out[1][q, r, : len(hits)] = hits
            out[2][q, r] = len(hits)
            out[3][q, r] = gid
        out[4][q] = len(chosen)
    return out


def _check_oracle(got, ref):
    """Equal to the oracle, up to swaps of neighbours whose fp64 scores are within the fp32 chain's rounding band."""
    s, i, hc, gid, gc = got
    Q, L, S = s.shape
    _check((s.reshape(Q, L * S), i.reshape(Q, L * S), gc), (ref[0].reshape(Q, L * S), ref[1].reshape(Q, L * S), ref[4]),
           near_tie=NEAR_TIE)
    exact = (i.cpu().numpy() == ref[1]).all((1, 2))
    assert np.array_equal(hc.cpu().numpy()[exact], ref[2][exact])
    assert np.array_equal(gid.cpu().numpy()[exact], ref[3][exact])
    assert exact.mean() > 0.9


def _eq(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y), (x, y)


# ---- 1. singleton groups: the grouped search IS the ungrouped one --------------------------------------------------------
@pytest.mark.parametrize("N,Q", [(4096, 64), (100_000, 1), (100_000, 64), (100_000, 300), (100_000, 1000)])
def test_singleton_groups_equal_the_ungrouped_search(N, Q):
    G = _random_gallery(N, seed=N + Q)
    g = torch.Generator(device=DEV).manual_seed(Q)
    q = torch.randn(Q, G.dim, device=DEV, generator=g)
    head = G.read(0, min(N, 4096))
    q[: Q // 2] = head[torch.randint(0, head.shape[0], (Q // 2,), device=DEV, generator=g)] * 4 + q[: Q // 2] * 0.5
    single = torch.arange(N, dtype=torch.int32, device=DEV)
    mask = torch.rand(N, device=DEV, generator=g) < 0.3
    for L in (1, 10, 25, 50):
        for thr in (None, 0.1):
            for allow in (None, mask):
                s, i, c = G.search(q, k=L, score_threshold=thr, allow=allow)
                gs, gi, hc, gid, gc = G.search_groups(q, single, limit=L, group_size=1, score_threshold=thr, allow=allow)
                assert G.search_stats()["grouped_fallback"] == 0
                assert torch.equal(gs[:, :, 0], s) and torch.equal(gi[:, :, 0], i) and torch.equal(gc, c), (L, thr)
                filled = torch.arange(L, device=DEV)[None] < c[:, None]
                assert torch.equal(hc, filled.to(torch.int32))
                assert torch.equal(gid, torch.where(filled, i, -1).to(torch.int32))
    # index_offset moves the row indices only
    s, i, c = G.search(q, k=10, index_offset=1000)
    gs, gi, hc, gid, gc = G.search_groups(q, single, limit=10, index_offset=1000)
    assert torch.equal(gi[:, :, 0], i) and torch.equal(gs[:, :, 0], s)
    assert torch.equal(gid, torch.where(i >= 0, i - 1000, -1).to(torch.int32))


# ---- 2. region-like galleries against the fp64 oracle ------------------------------------------------------------------
@pytest.fixture(scope="module", params=["global", "crop"])
def regions(request):
    rows, groups = _region_rows(100_000, mode=request.param, seed=11)
    G = _gallery_of(rows)
    gal = G.read(0, len(G)).cpu().numpy()                      # the rows as stored (normalised fp32)
    yield request.param, rows, groups, G, gal
    G.close()


@pytest.mark.parametrize("L,S,thr", [(5, 1, None), (10, 3, None), (3, 16, None), (50, 1, None), (8, 6, 0.2), (2, 25, None)])
def test_region_galleries_equal_the_oracle(regions, L, S, thr):
    mode, rows, groups, G, gal = regions
    q = _queries_near(rows, groups, 48, seed=L * 100 + S, big_first=6)
    got = G.search_groups(q, groups, limit=L, group_size=S, score_threshold=thr)
    ref = _oracle_groups(gal, groups.cpu().numpy(), q.cpu().numpy(), L, S, thr)
    _check_oracle(got, ref)
    if mode == "global" and L * S > 1:
        # a query at a group of more than 50 identical rows: its top 50 holds one group
        assert G.search_stats()["grouped_fallback"] >= 1
    gc = got[4].cpu().numpy()
    gid = got[3].cpu().numpy()
    for qq in range(gid.shape[0]):                              # distinct groups, padded with -1
        assert len(set(gid[qq, : gc[qq]].tolist())) == gc[qq] and (gid[qq, gc[qq]:] == -1).all()


@pytest.mark.parametrize("regions", ["global"], indirect=True)
def test_fallback_many_queries_filter_and_group_size(regions):
    """More than 64 queries that all take the fallback in one call, pass B (group_size > 1), and a filter."""
    mode, rows, groups, G, gal = regions
    g = torch.Generator(device=DEV).manual_seed(3)
    mask = torch.rand(len(G), device=DEV, generator=g) < 0.7
    q = _queries_near(rows, groups, 130, seed=5, big_first=130)
    gr = groups.cpu().numpy()
    for L, S, allow in ((5, 1, None), (4, 8, None), (5, 3, mask), (1, 50, mask)):
        got = G.search_groups(q, groups, limit=L, group_size=S, allow=allow)
        st = G.search_stats()
        if L > 1:                                               # (one group of >= 50 allowed rows decides a limit-1 query)
            assert st["grouped_fallback"] > 64, (L, S, st)
        ref = _oracle_groups(gal, gr, q.cpu().numpy(), L, S, allow=None if allow is None else mask.cpu().numpy())
        _check_oracle(got, ref)


# ---- 3. the grouped fallback gives the fast path's bits ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["global", "crop"])
def test_forced_fallback_equals_fast_path(mode):
    rows, groups = _region_rows(60_000, mode=mode, seed=21)
    P = _gallery_of(rows)
    X = _gallery_of(rows, experiments=True)
    X.set_search_mode("bruteforce")
    q = _queries_near(rows, groups, 96, seed=7, big_first=4)
    g = torch.Generator(device=DEV).manual_seed(8)
    mask = torch.rand(len(P), device=DEV, generator=g) < 0.5
    single = torch.arange(len(P), dtype=torch.int32, device=DEV)
    for L, S, thr, allow in ((5, 1, None, None), (10, 3, None, None), (2, 25, None, mask), (50, 1, 0.15, None),
                             (6, 4, 0.1, mask), (10, 1, None, "single"), (50, 1, 0.1, "single")):
        grp = single if allow == "single" else groups
        allow = None if allow == "single" else allow
        a = P.search_groups(q, grp, limit=L, group_size=S, score_threshold=thr, allow=allow, index_offset=7)
        b = X.search_groups(q, grp, limit=L, group_size=S, score_threshold=thr, allow=allow, index_offset=7)
        assert X.search_stats()["grouped_fallback"] == q.shape[0]
        if grp is single:                                       # (the product library certified every query here)
            assert P.search_stats()["grouped_fallback"] == 0
        _eq(a, b)


# ---- 4. filter = the grouped search of the allowed rows alone -------------------------------------------------------------
def test_filter_equals_the_sub_gallery():
    rows, groups = _region_rows(80_000, mode="crop", seed=31)
    G = _gallery_of(rows)
    g = torch.Generator(device=DEV).manual_seed(9)
    q = _queries_near(rows, groups, 64, seed=9, big_first=2)
    full = G.read(0, len(G))
    for frac in (0.5, 0.05):
        mask = torch.rand(len(G), device=DEV, generator=g) < frac
        allowed = torch.nonzero(mask).flatten()
        S = engine.Gallery(G.dim, int(allowed.numel()), device=0)
        S.add(full[allowed], normalize=False)
        for L, Sz in ((5, 1), (10, 4), (3, 16)):
            a = G.search_groups(q, groups, limit=L, group_size=Sz, allow=mask)
            s, i, hc, gid, gc = S.search_groups(q, groups[allowed].contiguous(), limit=L, group_size=Sz)
            assert int(i.max()) < int(allowed.numel())
            i = torch.where(i >= 0, allowed[i.clamp(min=0)], i)
            _eq(a, (s, i, hc, gid, gc))
        S.close()


# ---- 5. edges and errors --------------------------------------------------------------------------------------------------
def test_no_groups_and_stale_groups():
    G = engine.Gallery(1024, 20_010, device=0)                 # (room for the rows appended below)
    G.add(torch.randn(20_000, 1024, device=DEV))
    q = torch.randn(5, G.dim, device=DEV)
    none = torch.full((len(G),), -1, dtype=torch.int32, device=DEV)
    s, i, hc, gid, gc = G.search_groups(q, none, limit=4, group_size=2)
    assert (gc == 0).all() and (hc == 0).all() and (gid == -1).all() and (i == -1).all() and torch.isinf(s).all()
    # group ids set for 20 000 rows, then rows appended: the search fails instead of reading past them
    lib = G._lib
    ids = torch.zeros(len(G), dtype=torch.int32, device=DEV)
    _lib.check(lib.revo_search_set_groups(G._h, _lib.ptr(ids), len(G), 1, None))
    G.add(torch.randn(10, G.dim, device=DEV))
    out = [torch.empty((5, 4, 2), dtype=torch.float32, device=DEV), torch.empty((5, 4, 2), dtype=torch.int64, device=DEV),
           torch.empty((5, 4), dtype=torch.int32, device=DEV), torch.empty((5, 4), dtype=torch.int32, device=DEV),
           torch.empty((5,), dtype=torch.int32, device=DEV)]
    rc = lib.revo_search_groups(G._h, _lib.ptr(q), 5, 4, 2, 0, 0.0, 0, *[_lib.ptr(t) for t in out], None)
    assert rc == -2 and b"set them again after appending" in lib.revo_last_error()
    lib.revo_search_set_groups(G._h, None, 0, 0, None)
    rc = lib.revo_search_groups(G._h, _lib.ptr(q), 5, 4, 2, 0, 0.0, 0, *[_lib.ptr(t) for t in out], None)
    assert rc == -2 and b"no group ids set" in lib.revo_last_error()
    with pytest.raises(ValueError):
        G.search_groups(q, torch.zeros(len(G) - 1, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.RevoError):
        G.search_groups(q, torch.zeros(len(G), dtype=torch.int32, device=DEV), limit=10, group_size=6)
    # no fp32 master rows: no exact grouping
    H = engine.Gallery(G.dim, 100, device=0, keep_f32=False)
    H.add(torch.randn(100, G.dim, device=DEV))
    with pytest.raises(_lib.RevoError, match="keep_f32"):
        H.search_groups(q, torch.zeros(100, dtype=torch.int32, device=DEV))
    # an empty gallery returns empty groups
    E = engine.Gallery(G.dim, 10, device=0)
    s, i, hc, gid, gc = E.search_groups(q, torch.zeros(0, dtype=torch.int32, device=DEV), limit=3)
    assert (gc == 0).all() and (gid == -1).all() and (i == -1).all()


# ---- 6. store and façade --------------------------------------------------------------------------------------------------
def test_store_search_groups_matches_the_oracle():
    rows, groups = _region_rows(30_000, D=512, mode="crop", seed=41)
    gr = groups.cpu().numpy()
    st = store.GalleryStore(512, device=0, capacity=len(gr))
    payloads = [({"image_source": f"/img/{int(x)}.jpg", "kind": int(x) % 3} if x >= 0 else {"kind": 5}) for x in gr]
    st.upsert(rows, [f"id{r}" for r in range(len(gr))], payloads)
    gal = st.gallery.read(0, len(st)).cpu().numpy()
    flt = {"must_not": [{"key": "kind", "match": {"value": 1}}]}
    allow = np.array([p["kind"] != 1 for p in payloads])
    q = _queries_near(rows, groups, 6, seed=12, big_first=2)
    for qq in range(q.shape[0]):
        for f, a in ((None, None), (flt, allow)):
            res = st.search_groups(q[qq].cpu().numpy(), group_by="image_source", limit=4, group_size=3, query_filter=f)
            ref = _oracle_groups(gal, gr, q[qq: qq + 1].cpu().numpy(), 4, 3, allow=a)
            assert len(res.groups) == ref[4][0]
            for r, grp in enumerate(res.groups):
                assert grp.id == f"/img/{ref[3][0, r]}.jpg"
                assert [h.id for h in grp.hits] == [f"id{j}" for j in ref[1][0, r, : ref[2][0, r]]]
                assert np.allclose([h.score for h in grp.hits], ref[0][0, r, : ref[2][0, r]], atol=1e-3)
                assert all(h.payload["image_source"] == grp.id for h in grp.hits)
    # a point with a list value under the key: refused, not grouped differently from Qdrant
    st.upsert(rows[:1], ["listed"], [{"image_source": ["/img/0.jpg", "/img/1.jpg"]}])
    with pytest.raises(ValueError, match="list-valued"):
        st.search_groups(q[0].cpu().numpy(), group_by="image_source", limit=2)
    st.close()


def test_search_similar_group_by_image_source(tmp_path, dev):
    from PIL import Image
    from reverso_amd.core_system import Regions, SimpleReverso
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(3)
    for n in range(12):
        Image.fromarray(rng.integers(0, 256, (90 + 4 * n, 110, 3), dtype=np.uint8)).save(folder / f"img_{n:02d}.png")

    def detector(pil, prompt):
        w, h = pil.size
        return Regions([[0, 0, w // 2, h // 2], [w // 4, h // 4, w - 1, h - 1], [w // 3, 0, w - 1, h // 2]],
                       confidence=[0.9, 0.8, 0.7], class_id=[0, 1, 0], class_names=["person", "car"])

    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=4, detector=detector,
                      region_mode="global")
    msg = r.create_database(str(folder), "regions", text_prompt="person . car")
    assert "✅" in msg and len(r.vector_db) == 36
    r.detect_regions(str(folder / "img_00.png"), "person . car")
    r.extract_embeddings(str(folder / "img_00.png"))
    _, plain = r.search_similar(-1.0, 5)
    names = [it["filename"] for it in plain]
    assert len(set(names)) < len(names)                         # three identical rows per image: repeats
    text, grouped = r.search_similar(-1.0, 5, group_by="image_source")
    gnames = [it["filename"] for it in grouped]
    assert len(gnames) == 5 and len(set(gnames)) == 5 and "Found 5 similar regions" in text
    # each image by its best score: the first five distinct images of the ungrouped ranking
    _, wide = r.search_similar(-1.0, 36)
    first, seen = [], set()
    for it in wide:
        if it["filename"] not in seen:
            seen.add(it["filename"])
            first.append(it)
    assert gnames == [it["filename"] for it in first[:5]]
    assert [it["score"] for it in grouped] == [it["score"] for it in first[:5]]
    # the default call is unchanged
    _, again = r.search_similar(-1.0, 5)
    assert [it["filename"] for it in again] == names


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    N = 20_037
    G = _random_gallery(N, seed=5)
    g = torch.Generator(device=DEV).manual_seed(6)
    q = torch.randn(9, G.dim, device=DEV, generator=g)
    groups = torch.randint(0, N // 3, (N,), device=DEV, generator=g).to(torch.int32)
    _assert_offset_moves_the_indices_only(
        lambda off: G.search_groups(q, groups, limit=10, group_size=3, index_offset=off), {1})
    G.close()
