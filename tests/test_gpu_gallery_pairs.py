"""Near-duplicate pairs of one gallery (revo_gallery_pairs, include/revo.h PAIRS; Gallery.pairs, GalleryStore.duplicate_pairs /
duplicate_groups, SimpleReverso.find_duplicates) against an fp64 oracle of the fp32 master rows, against the search, under
filters, on 2 000 identical rows (the workspace regrow), on edge cases, and through the store and the facade."""
import ctypes as C
import shutil

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
    """N rows: random directions, and clusters of perturbed copies of a few of them (pair scores from about 0.8 to 0.95)."""
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


def _oracle(rows, t, delta, allow=None):
    """fp64 scores of the fp32 master rows: (must, may, score), `must` the pairs i < j at or above t + delta, `may` those at
    or above t - delta (as sets of (i, j)), `score` {pair: fp64 score} over `may`.  Row blocks on the device."""
    X = rows.to(torch.float64)
    N = X.shape[0]
    ok = torch.ones(N, dtype=torch.bool, device=X.device) if allow is None else allow.to(X.device)
    must, may, score = set(), set(), {}
    for a in range(0, N, 4096):
        S = X[a:a + 4096] @ X.T
        i = torch.arange(a, min(N, a + 4096), device=X.device)[:, None]
        j = torch.arange(N, device=X.device)[None, :]
        valid = (j > i) & ok[i] & ok[j]
        hit = torch.nonzero(valid & (S >= t - delta))
        vals = S[hit[:, 0], hit[:, 1]].cpu().numpy()
        for (r, c), v in zip(hit.cpu().numpy().tolist(), vals.tolist()):
            p = (r + a, c)
            may.add(p)
            score[p] = v
            if v >= t + delta:
                must.add(p)
    return must, may, score


def _check_against_oracle(pairs, scores, must, may, score, delta):
    p = pairs.cpu().numpy()
    s = scores.cpu().numpy().astype(np.float64)
    got = [tuple(r) for r in p.tolist()]
    assert len(set(got)) == len(got)
    assert all(i < j for i, j in got)                                   # never (i, i), never (j, i)
    assert got == sorted(got)                                            # (i asc, j asc)
    missing = must - set(got)
    assert not missing, sorted(missing)[:10]
    extra = set(got) - may
    assert not extra, sorted(extra)[:10]
    for q, v in zip(got, s.tolist()):
        assert abs(v - score[q]) <= delta, (q, v, score[q])


def _teeth_threshold(rows, x_pairs, delta):
    """A threshold with a planted pair at fp32 >= t + delta whose bf16-rounded score is below t: (t, pair)."""
    X = rows.to(torch.float64)
    Xb = rows.to(torch.bfloat16).to(torch.float64)
    i = torch.tensor([a for a, _ in x_pairs], device=rows.device)
    j = torch.tensor([b for _, b in x_pairs], device=rows.device)
    s64 = (X[i] * X[j]).sum(1)
    sb = (Xb[i] * Xb[j]).sum(1)
    gap = s64 - sb
    k = int(torch.argmax(gap))
    assert float(gap[k]) > 4 * delta, "the planted pairs have no bf16 score below their fp32 score"
    t = float(s64[k] - gap[k] / 2)
    return t, (int(i[k]), int(j[k])), float(s64[k]), float(sb[k])


def _cluster_pairs(rows, lo=0.75):
    """pairs (i < j) of the planted clusters (fp64 score above lo), at most 4096"""
    X = rows.to(torch.float64)
    out = []
    for a in range(0, X.shape[0], 4096):
        S = X[a:a + 4096] @ X.T
        i = torch.arange(a, min(X.shape[0], a + 4096), device=X.device)[:, None]
        j = torch.arange(X.shape[0], device=X.device)[None, :]
        hit = torch.nonzero((j > i) & (S >= lo))
        out += [(r + a, c) for r, c in hit.cpu().numpy().tolist()]
    return out[:4096]


# ---- 1. exactness against the fp64 oracle, with teeth --------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 4096, 20_037])
@pytest.mark.parametrize("D", [64, 1024, 1536])
def test_matches_the_fp64_oracle(N, D):
    _matches_the_fp64_oracle(N, D)


@pytest.mark.parametrize("N", [256, 257, 513, 5889])
def test_matches_the_fp64_oracle_where_the_tile_walk_turns(N):
    """The join's walk over the tile pairs (csrc/tile_walk.h) at the sizes where it can go wrong, next to N = 1 and 255 above:
    one full tile, a second tile of one row (a partial last tile, and tj wraps into the next ti), three tiles, and T = 23 row
    tiles = 276 tile pairs, more than the one workgroup per CU of this part, so that a workgroup's range crosses a row of
    the triangle."""
    _matches_the_fp64_oracle(N, 64)


def _matches_the_fp64_oracle(N, D):
    x = _planted(N, D, seed=N + D)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    if N < 2:
        pairs, scores = G.pairs(0.9)
        assert pairs.shape == (0, 2) and scores.shape == (0,)
        pairs, scores = G.pairs(-1.0)                                    # no pair at all, whatever the threshold
        assert pairs.shape == (0, 2)
        G.close()
        return
    planted = _cluster_pairs(rows)
    assert planted
    t, tooth, s64, sb = _teeth_threshold(rows, planted, delta)
    assert s64 >= t + delta and sb < t                                   # fp32 reaches t, the bf16 score does not
    pairs, scores = G.pairs(t)
    must, may, score = _oracle(rows, t, delta)
    assert tooth in must
    _check_against_oracle(pairs, scores, must, may, score, delta)
    assert tooth in {tuple(r) for r in pairs.cpu().numpy().tolist()}    # a join that thresholded bf16 scores misses it
    st = G.search_stats()
    assert st["join_passes"] == 1 and st["collected_rows"] >= pairs.shape[0]
    assert st["uncertified"] == 0 and st["large_k_fallback"] == 0
    G.close()


# ---- 2. consistency with the search ------------------------------------------------------------------------------------
def test_partners_equal_the_search_of_each_row():
    N, D = 20_037, 1024
    x = _planted(N, D, seed=5)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    t = 0.85
    pairs, scores = G.pairs(t)
    p = pairs.cpu().numpy()
    _, _, score = _oracle(rows, t, delta)
    assert p.shape[0] > 50
    rng = np.random.default_rng(6)
    sample = sorted(set(rng.choice(p[:, 0], 20).tolist()) | set(rng.choice(p[:, 1], 20).tolist()))
    s, idx, cnt = G.search(rows[sample], k=1024, score_threshold=t)
    for q, i in enumerate(sample):
        def far(j):
            v = score.get((min(i, j), max(i, j)))
            return v is None or abs(v - t) > 2 * delta
        got = {int(b) for a, b in p.tolist() if a == i} | {int(a) for a, b in p.tolist() if b == i}
        found = {int(j) for j in idx[q, :int(cnt[q])].tolist()} - {i}
        assert {j for j in got if far(j)} == {j for j in found if far(j)}, i
    G.close()


# ---- 3. filters ----------------------------------------------------------------------------------------------------------
def test_filtered_pairs_equal_the_oracle_of_the_allowed_rows():
    N, D = 20_037, 64
    x = _planted(N, D, seed=7, n_clusters=2000)
    G = _gallery(x)
    rows = G.read()
    delta = _delta(D)
    allow = torch.from_numpy(np.random.default_rng(8).random(N) < 0.6).to(DEV)
    t = 0.85
    pairs, scores = G.pairs(t, allow=allow)
    must, may, score = _oracle(rows, t, delta, allow=allow)
    assert len(must) > 100
    _check_against_oracle(pairs, scores, must, may, score, delta)
    a = allow.cpu().numpy()
    assert a[pairs[:, 0].cpu().numpy()].all() and a[pairs[:, 1].cpu().numpy()].all()
    full, _ = G.pairs(t)                                                 # the filter was cleared again
    assert full.shape[0] > pairs.shape[0]
    G.close()


def test_stale_filter_is_refused():
    x = _planted(3000, 64, seed=9)
    G = _gallery(x, extra=10)
    bits = G.allow_bits(torch.ones(3000, dtype=torch.bool, device=DEV))
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), 3000, 1, _lib.current_stream()) == 0
    G.add(torch.from_numpy(x[:10]).to(DEV))
    n = C.c_int64(-5)
    assert G._lib.revo_gallery_pairs(G._h, 0.9, C.byref(n), _lib.current_stream()) == -2
    assert b"set it again" in G._lib.revo_last_error()
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    G.close()


# ---- 4. identical rows: more candidates than the first workspace holds ------------------------------------------------
def test_two_thousand_identical_rows():
    D, n = 64, 2000
    v = np.random.default_rng(10).standard_normal(D).astype(np.float32)
    G = _gallery(np.repeat(v[None], n, 0))
    pairs, scores = G.pairs(0.99)
    assert pairs.shape == (n * (n - 1) // 2, 2) == (1_999_000, 2)
    st = G.search_stats()
    assert st["join_passes"] == 2 and st["collected_rows"] == 1_999_000
    assert st["uncertified"] == 0 and st["bruteforced"] == 0 and st["checked"] == 0
    s = scores.cpu().numpy()
    assert (s == s[0]).all() and abs(float(s[0]) - 1.0) <= 1e-6
    i, j = torch.triu_indices(n, n, 1)
    assert torch.equal(pairs.cpu(), torch.stack([i, j], 1))
    # a search afterwards reports 0 join passes
    G.search(G.read(0, 1), k=5)
    assert G.search_stats()["join_passes"] == 0
    G.close()


# ---- 5. edge cases -------------------------------------------------------------------------------------------------------
def _raw_read(G, start, n, on_device=True):
    pairs = torch.full((max(n, 1), 2), -7, dtype=torch.int64, device=DEV if on_device else "cpu")
    scores = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=DEV if on_device else "cpu")
    rc = G._lib.revo_gallery_pairs_read(G._h, start, n, _lib.ptr(pairs) if on_device else pairs.data_ptr(),
                                        _lib.ptr(scores) if on_device else scores.data_ptr(), int(on_device))
    return rc, pairs[:n], scores[:n]


def test_edge_cases():
    N, D = 4096, 256
    x = _planted(N, D, seed=11, n_clusters=300)
    G = _gallery(x, extra=5)
    delta = _delta(D)
    p0, s0 = G.pairs(1.0 + 2 * delta)
    assert p0.shape == (0, 2)
    t = 0.8
    p1, s1 = G.pairs(t)
    p2, s2 = G.pairs(t)
    assert p1.shape[0] > 100
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))     # bit-identical
    n = p1.shape[0]
    pages = [_raw_read(G, a, min(97, n - a)) for a in range(0, n, 97)]                        # pages == one read
    assert all(rc == 0 for rc, _, _ in pages)
    assert torch.equal(torch.cat([p for _, p, _ in pages]), p1)
    assert torch.equal(torch.cat([s for _, _, s in pages]).view(torch.int32), s1.view(torch.int32))
    rc, ph, sh = _raw_read(G, 5, 20, on_device=False)                                         # host destination
    assert rc == 0 and torch.equal(ph, p1[5:25].cpu()) and torch.equal(sh, s1[5:25].cpu())
    rc, _, _ = _raw_read(G, n - 3, 4)                                                         # past the result
    assert rc == -2 and b"past the result" in G._lib.revo_last_error()
    assert _raw_read(G, n, 0)[0] == 0
    G.add(torch.from_numpy(x[:5]).to(DEV))                                                    # rows changed: no result
    rc, _, _ = _raw_read(G, 0, 1)
    assert rc == -2 and b"no result" in G._lib.revo_last_error()
    G.close()
    K = _gallery(x[:300], keep_f32=False)                                                     # no fp32 master rows
    n = C.c_int64(-5)
    assert K._lib.revo_gallery_pairs(K._h, 0.9, C.byref(n), _lib.current_stream()) == -2
    assert b"keep_f32" in K._lib.revo_last_error()
    with pytest.raises(_lib.RevoError):
        K.pairs(0.9)
    K.close()
    E = engine.Gallery(D, 10, device=0)                                                      # empty gallery
    p, s = E.pairs(0.5)
    assert p.shape == (0, 2)
    E.clear()
    assert _raw_read(E, 0, 1)[0] == -2
    E.close()


def test_too_many_candidates_is_refused():
    D, n = 64, 24_000                    # 287 988 000 identical pairs > 2^28 candidates
    v = np.random.default_rng(12).standard_normal(D).astype(np.float32)
    G = _gallery(np.repeat(v[None], n, 0))
    c = C.c_int64(-5)
    assert G._lib.revo_gallery_pairs(G._h, 0.5, C.byref(c), _lib.current_stream()) == -2
    assert b"287988000 candidate pairs exceed" in G._lib.revo_last_error()
    G.close()


# ---- 6. store and facade ------------------------------------------------------------------------------------------------
def _oracle_groups(rows, t, delta):
    must, may, score = _oracle(rows, t, delta)
    assert not {p for p in may if abs(score[p] - t) <= delta}, "a pair inside the band: choose another threshold"
    return store.connected_groups(np.array(sorted(must), dtype=np.int64).reshape(-1, 2), rows.shape[0])


def test_store_duplicate_groups_recover_the_planted_clusters():
    N, D = 6000, 256
    rng = np.random.default_rng(13)
    vec = rng.standard_normal((N, D)).astype(np.float32)
    clusters = []
    perm = rng.permutation(N)
    for c in range(40):
        members = sorted(perm[c * 5:c * 5 + int(rng.integers(2, 6))].tolist())
        base = vec[members[0]] / np.linalg.norm(vec[members[0]])
        for r in members:
            vec[r] = base + 0.1 * rng.standard_normal(D).astype(np.float32) / np.sqrt(D)
        clusters.append(members)
    payloads = [{"image_source": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2]} for r in range(N)]
    ids = [f"p{r}" for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(vec), ids, payloads)
    groups = st.duplicate_groups(0.95)
    assert groups == [[f"p{r}" for r in m] for m in sorted(clusters)]
    dp = st.duplicate_pairs(0.95)
    assert len(dp) == sum(len(m) * (len(m) - 1) // 2 for m in clusters)
    assert all(isinstance(p, store.DuplicatePair) and p.score >= 0.95 for p in dp)
    assert [(int(p.id_a[1:]), int(p.id_b[1:])) for p in dp] == sorted((int(p.id_a[1:]), int(p.id_b[1:])) for p in dp)
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    want = [[f"p{r}" for r in m if r % 2 == 0] for m in sorted(clusters)]
    want = sorted([g for g in want if len(g) >= 2], key=lambda g: int(g[0][1:]))
    assert st.duplicate_groups(0.95, query_filter=flt) == want
    assert st.duplicate_groups(0.95) == groups


def test_find_duplicates_on_a_database(tmp_path):
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, groups = r.find_duplicates()
    assert text.startswith("❌") and groups == []
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(14)
    for n in range(6):
        arr = (rng.integers(0, 256, (3,)) + rng.integers(0, 80, (96, 120, 3))) % 256
        Image.fromarray(arr.astype(np.uint8)).save(str(folder / f"img_{n}.jpg"), quality=90)
    shutil.copy(folder / "img_1.jpg", folder / "repost_1.jpg")            # the same file twice
    shutil.copy(folder / "img_4.jpg", folder / "repost_4.jpg")
    assert "✅" in r.create_database(str(folder), "dups", use_direct_pe=True)
    db = r.vector_db
    rows = db.gallery.read(0, len(db))
    t = 0.95
    want = [[db.payloads[i]["filename"] for i in g] for g in _oracle_groups(rows, t, _delta(rows.shape[1]))]
    text, groups = r.find_duplicates(similarity_threshold=t)
    got = [[m["filename"] for m in g] for g in groups]
    assert got == want
    for a, b in (("img_1.jpg", "repost_1.jpg"), ("img_4.jpg", "repost_4.jpg")):
        assert any(a in g and b in g for g in got)
    assert all(set(m) == {"filename", "image_source", "bbox", "id"} for g in groups for m in g)
    assert text.startswith(f"🎯 Found {len(groups)} groups") and "repost_1.jpg" in text
    text, groups = r.find_duplicates(similarity_threshold=1.5)
    assert groups == [] and "No near-duplicates" in text
