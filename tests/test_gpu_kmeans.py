"""Exact spherical k-means over one gallery (revo_gallery_kmeans, include/revo.h KMEANS; Gallery.kmeans, GalleryStore.themes,
SimpleReverso.summarize_database).  All comparisons are on bytes unless said otherwise.  Oracles:
  assignment  a second Gallery holding the returned centroids (add(normalize=False)) and search(first.read(), k=1): its
              indices and scores are the labels and scores, byte for byte;
  fp64        the fp64 argmax in torch agrees on every row whose fp64 top-two gap exceeds 3e-7 (_search_checks.py's band);
  update      a numpy float32 loop in the contract's order (np.cumsum per chunk of 256 members, the partials added in chunk
              order), normalised by appending the sums to a scratch Gallery with normalize=True and reading them back."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TIE = 3e-7                                                               # _search_checks.py: the fp32 chain's band


def _gallery(x, normalize=True, experiments=False, extra=0):
    G = engine.Gallery(x.shape[1], max(1, x.shape[0] + extra), device=0, experiments=experiments)
    if x.shape[0]:
        G.add(x.to(DEV), normalize=normalize)
    return G


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what=""):
    """two results of Gallery.kmeans: the same bytes"""
    names = ("centroids", "labels", "scores", "sizes")
    for x, y, name in zip(a[:4], b[:4], names):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, name)
    assert a[4:] == b[4:], (what, a[4:], b[4:])


def _normalised(c):
    """rows as an append with normalize=True writes them"""
    S = _gallery(c)
    out = S.read()
    S.close()
    return out


def _check_assignment(G, res, allow=None, what=""):
    """labels / scores against the search oracle, then the fp64 argmax outside the band; sizes against the labels"""
    cents, labels, scores, sizes = res[:4]
    n_c = cents.shape[0]
    rows = G.read()
    O = _gallery(cents, normalize=False)
    s, i, c = O.search(rows, k=1)
    O.close()
    want_l, want_s = i[:, 0].to(torch.int32), s[:, 0].clone()
    if allow is not None:
        want_l[~allow] = -1
        want_s[~allow] = float("-inf")
    assert torch.equal(labels, want_l), (what, "labels", int((labels != want_l).sum()))
    assert torch.equal(_bits(scores), _bits(want_s)), (what, "scores")
    R = rows.to(torch.float64)
    S = (R / R.norm(dim=1, keepdim=True)) @ cents.to(torch.float64).T   # the row as a query: unit length
    top = torch.topk(S, min(2, n_c), dim=1).values
    clear = torch.ones(rows.shape[0], dtype=torch.bool, device=DEV) if n_c == 1 else (top[:, 0] - top[:, 1]) > TIE
    if allow is not None:
        clear &= allow
    assert torch.equal(labels[clear].to(torch.int64), S.argmax(1)[clear]), (what, "fp64 argmax")
    lab = labels.to(torch.int64)
    assert torch.equal(sizes, torch.bincount(lab[lab >= 0], minlength=n_c)), (what, "sizes")


def _update_oracle(rows, labels, prev):
    """the contract's update in numpy float32: (new centroids [C, D] as a device tensor)"""
    rows, labels, prev_np = rows.cpu().numpy(), labels.cpu().numpy(), prev.cpu().numpy()
    n_c, D = prev_np.shape
    sums = np.zeros((n_c, D), np.float32)
    keep = np.zeros(n_c, bool)
    for c in range(n_c):
        members = np.flatnonzero(labels == c)
        total = np.zeros(D, np.float32)
        for a in range(0, members.size, 256):
            total = total + np.cumsum(rows[members[a:a + 256]], axis=0, dtype=np.float32)[-1]
        assert total.dtype == np.float32
        sums[c] = total
        sq = float(np.sum(total.astype(np.float64) ** 2))
        keep[c] = members.size == 0 or sq == 0.0 or not np.isfinite(sq)
    out = _normalised(torch.from_numpy(sums)).cpu().numpy()
    out[keep] = prev_np[keep]
    return torch.from_numpy(out).to(DEV)


def _rows(N, D, seed):
    return torch.randn(N, D, generator=torch.Generator().manual_seed(seed))


# ---- 1. ragged shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_ragged_shapes(N):
    D = 64
    G = _gallery(_rows(N, D, 10 + N))
    for n_c in (1, 2, 255, 257, 600):
        res = G.kmeans(_rows(n_c, D, 1000 + n_c).to(DEV), max_iter=0)
        assert res[4] == 0 and res[5] is False and res[1].shape == (N,) and res[0].shape == (n_c, D)
        _check_assignment(G, res, what=f"N={N} C={n_c}")
        assert int(res[3].sum()) == N
    G.close()


# ---- 2. widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 192, 1024, 2112])
def test_widths(D):
    G = _gallery(_rows(300, D, 20 + D))
    res = G.kmeans(_rows(5, D, 30 + D).to(DEV), max_iter=2)
    _check_assignment(G, res, what=f"D={D}")
    one = G.kmeans(_rows(5, D, 30 + D).to(DEV), max_iter=1)              # the update at this width, against numpy
    zero = G.kmeans(_rows(5, D, 30 + D).to(DEV), max_iter=0)
    assert torch.equal(_bits(one[0]), _bits(_update_oracle(G.read(), zero[1], zero[0])))
    G.close()


# ---- 3. bf16 disagrees with fp32 -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _between_two_centroids(D=64, N=2048, n_c=5):
    """rows between two centroids: row = normalise(c_a + c_b + 1e-3 noise), a != b.  Returns (rows, centroids) on the host,
    the centroids of unit length (used with normalize=False: bit for bit)."""
    torch.manual_seed(7)
    cents = torch.nn.functional.normalize(torch.randn(n_c, D), dim=1)
    a = torch.randint(0, n_c, (N,))
    b = (a + torch.randint(1, n_c, (N,))) % n_c
    rows = torch.nn.functional.normalize(cents[a] + cents[b] + 1e-3 * torch.randn(N, D), dim=1)
    return rows, cents


def _bf16_disagreements(rows, cents):
    """rows whose argmax over bf16-rounded operands (accumulated in fp64) differs from the fp64 argmax by a gap above 1e-6"""
    S = rows.to(torch.float64) @ cents.to(torch.float64).T
    Sb = rows.to(torch.bfloat16).to(torch.float64) @ cents.to(torch.bfloat16).to(torch.float64).T
    top = torch.topk(S, 2, dim=1).values
    return int(((S.argmax(1) != Sb.argmax(1)) & ((top[:, 0] - top[:, 1]) > 1e-6)).sum())


def test_bf16_disagrees_with_fp32():
    rows, cents = _between_two_centroids()
    G = _gallery(rows)
    n_bad = _bf16_disagreements(G.read().cpu(), cents)
    print("rows where the bf16 argmax is wrong:", n_bad)
    assert n_bad >= 32
    res = G.kmeans(cents.to(DEV), max_iter=0, normalize=False)
    assert torch.equal(_bits(res[0]), _bits(cents.to(DEV)))             # normalize=False: used as given
    st = G.search_stats()
    print("stats:", st)
    _check_assignment(G, res, what="teeth")
    assert st["large_k_fallback"] > 0 and st["collected_rows"] > 0 and st["join_passes"] == 1
    G.close()


def test_rows_stored_at_any_length():
    """rows appended with normalize=False at lengths 0.2 .. 5: the score is the search's (the row as a normalised query), the
    rounding bound is per row -- the labels and scores are still the search oracle's bytes, on the teeth fixture too"""
    rows, cents = _between_two_centroids()
    scale = 0.2 + 4.8 * torch.rand(rows.shape[0], 1, generator=torch.Generator().manual_seed(31))
    G = _gallery(rows * scale, normalize=False)
    res = G.kmeans(cents.to(DEV), max_iter=1, normalize=False)
    _check_assignment(G, res, what="any length")
    assert G.search_stats()["large_k_fallback"] > 0
    zero = G.kmeans(cents.to(DEV), max_iter=0, normalize=False)          # the update sums the rows AS STORED
    assert torch.equal(_bits(res[0]), _bits(_update_oracle(G.read(), zero[1], zero[0])))
    G.close()


# ---- 4. exact ties ---------------------------------------------------------------------------------------------------------
def test_exact_ties():
    D, N = 64, 300
    x = _rows(N, D, 40)
    c = _rows(5, D, 41)
    c[3] = c[1]
    x[:5] = c                                                            # rows identical to a centroid
    G = _gallery(x)
    res = G.kmeans(c.to(DEV), max_iter=0)
    _check_assignment(G, res, what="ties")
    assert not (res[1] == 3).any() and int(res[3][3]) == 0 and (res[1] == 1).any()
    assert res[1][:3].tolist() == [0, 1, 2] and int(res[1][3]) == 1 and int(res[1][4]) == 4
    G.close()
    # all rows identical: one cluster of N, the others keep their bits
    same = x[7:8].repeat(N, 1)
    G = _gallery(same)
    start = _normalised(c)
    res = G.kmeans(c.to(DEV), max_iter=3)
    _check_assignment(G, res, what="identical rows")
    win = int(res[1][0])
    assert (res[1] == win).all() and int(res[3][win]) == N and int(res[3].sum()) == N
    others = [i for i in range(5) if i != win]
    assert torch.equal(_bits(res[0][others]), _bits(start[others]))
    assert res[5] is True
    G.close()


# ---- 5. update chunks ------------------------------------------------------------------------------------------------------
def test_update_chunks():
    D = 64
    counts = [1, 255, 256, 257, 513]
    gen = torch.Generator().manual_seed(50)
    centres = torch.eye(D)[:5]
    owner = torch.cat([torch.full((n,), i) for i, n in enumerate(counts)])[torch.randperm(sum(counts), generator=gen)]
    x = centres[owner] + 0.05 * torch.randn(owner.shape[0], D, generator=gen)
    G = _gallery(x)
    init = (centres + 0.01 * torch.randn(5, D, generator=gen)).to(DEV)
    zero = G.kmeans(init, max_iter=0)
    assert zero[3].tolist() == counts and torch.equal(zero[1].cpu().to(torch.int64), owner)
    one = G.kmeans(init, max_iter=1)
    assert one[4] == 1
    assert torch.equal(_bits(one[0]), _bits(_update_oracle(G.read(), zero[1], zero[0])))
    _check_assignment(G, one, what="chunks")
    G.close()
    # one cluster holding every row: four chunks
    x = centres[:1] + 0.05 * torch.randn(1000, D, generator=gen)
    G = _gallery(x)
    init = torch.stack([centres[0], -centres[0]]).to(DEV)
    zero = G.kmeans(init, max_iter=0)
    assert zero[3].tolist() == [1000, 0]
    one = G.kmeans(init, max_iter=1)
    assert torch.equal(_bits(one[0]), _bits(_update_oracle(G.read(), zero[1], zero[0])))
    assert torch.equal(_bits(one[0][1]), _bits(zero[0][1]))              # the empty cluster keeps its bits
    G.close()


# ---- 6. keep-previous ---------------------------------------------------------------------------------------------------------
def test_keep_previous():
    D = 64
    v = _rows(1, D, 60)
    G = _gallery(torch.cat([v, -v]))
    c = _rows(1, D, 61).to(DEV)
    res = G.kmeans(c, max_iter=1)
    assert res[4] == 1 and res[3].tolist() == [2]
    assert torch.equal(_bits(res[0]), _bits(_normalised(c)))             # the sum is exactly zero: the centroid stays
    more = G.kmeans(c, max_iter=5)
    assert more[4] == 1 and more[5] is True and torch.equal(_bits(more[0]), _bits(res[0]))
    G.close()


# ---- 7. filter ---------------------------------------------------------------------------------------------------------------
def test_filter():
    D, N = 64, 700
    x = _rows(N, D, 70)
    c = _rows(6, D, 71).to(DEV)
    G = _gallery(x)
    allow = (torch.arange(N, device=DEV) % 3) != 0
    res = G.kmeans(c, max_iter=2, allow=allow)
    assert (res[1][~allow] == -1).all() and torch.isneginf(res[2][~allow]).all() and (res[1][allow] >= 0).all()
    _check_assignment(G, res, allow=allow, what="filter")
    F = _gallery(G.read()[allow], normalize=False)                       # a fresh gallery of the allowed rows
    fres = F.kmeans(c, max_iter=2)
    F.close()
    assert torch.equal(_bits(res[0]), _bits(fres[0])) and torch.equal(res[3], fres[3]) and res[4:] == fres[4:]
    assert torch.equal(res[1][allow], fres[1]) and torch.equal(_bits(res[2][allow]), _bits(fres[2]))
    # a filter that allows nothing
    none = G.kmeans(c, max_iter=2, allow=torch.zeros(N, dtype=torch.bool, device=DEV))
    assert (none[1] == -1).all() and torch.isneginf(none[2]).all() and (none[3] == 0).all()
    assert torch.equal(_bits(none[0]), _bits(_normalised(c)))
    G.close()
    # an empty gallery
    E = engine.Gallery(D, 4, device=0)
    e = E.kmeans(c, max_iter=2)
    assert e[1].shape == (0,) and e[2].shape == (0,) and (e[3] == 0).all() and torch.equal(_bits(e[0]), _bits(_normalised(c)))
    E.close()


# ---- 8. iteration ------------------------------------------------------------------------------------------------------------
def _raw_read(G, start, n):
    labels = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=DEV)
    return G._lib.revo_gallery_kmeans_read(G._h, start, n, _lib.ptr(labels), _lib.ptr(scores), 1), labels[:n], scores[:n]


def test_three_steps_are_three_calls_of_one():
    D, N = 64, 900
    G = _gallery(_rows(N, D, 80))
    c = _rows(7, D, 81).to(DEV)
    whole = G.kmeans(c, max_iter=3)
    assert whole[4] == 3
    step = G.kmeans(c, max_iter=1)
    for _ in range(2):
        step = G.kmeans(step[0], max_iter=1, normalize=False)
    _same(whole[:4], step[:4], "three steps")
    _check_assignment(G, whole, what="three steps")
    G.close()


def test_blobs_converge_to_a_fixed_point_and_calls_repeat():
    D, N = 64, 2000
    gen = torch.Generator().manual_seed(82)
    centres = torch.nn.functional.normalize(torch.randn(8, D, generator=gen), dim=1)
    x = centres[torch.randint(0, 8, (N,), generator=gen)] + 0.03 * torch.randn(N, D, generator=gen)
    G = _gallery(x, extra=4)
    init = (centres + 0.02 * torch.randn(8, D, generator=gen)).to(DEV)
    res = G.kmeans(init, max_iter=20)
    assert res[5] is True and 1 <= res[4] < 20
    _check_assignment(G, res, what="blobs")
    again = G.kmeans(res[0], max_iter=20, normalize=False)               # a fixed point: a further call changes no byte
    _same(res[:4], again[:4], "fixed point")
    assert again[5] is True and again[4] == 1
    # two identical calls, an unrelated pairs / knn call in between
    a = G.kmeans(init, max_iter=2)
    G.pairs(0.9)
    G.knn(3)
    G.search_range(G.read(0, 3), 0.9)
    rc, labels, scores = _raw_read(G, 0, N)                              # the result survives them
    assert rc == 0 and torch.equal(labels, a[1]) and torch.equal(_bits(scores), _bits(a[2]))
    b = G.kmeans(init, max_iter=2)
    _same(a, b, "repeat")
    rc, part, _ = _raw_read(G, 100, 50)
    assert rc == 0 and torch.equal(part, a[1][100:150])
    assert _raw_read(G, N - 3, 4)[0] == -2 and b"past the result" in G._lib.revo_last_error()
    # a result read after add gives status -2
    G.add(x[:2].to(DEV))
    assert _raw_read(G, 0, 1)[0] == -2 and b"no result" in G._lib.revo_last_error()
    assert G._lib.revo_gallery_kmeans_centroids(G._h, None, None, 1) == -2
    G.close()


def test_refusals():
    D = 64
    G = _gallery(_rows(100, D, 83))
    bad = _rows(3, D, 84)
    bad[1] = 0.0
    with pytest.raises(_lib.RevoError, match="zero norm"):
        G.kmeans(bad.to(DEV))
    G.kmeans(bad.to(DEV), normalize=False, max_iter=0)                   # as given: a zero centroid is allowed
    bad[2, 5] = float("nan")
    with pytest.raises(_lib.RevoError, match="not finite"):
        G.kmeans(bad.to(DEV), normalize=False)
    with pytest.raises(_lib.RevoError, match="max_iter"):
        G.kmeans(_rows(3, D, 85).to(DEV), max_iter=1001)
    G.close()
    K = engine.Gallery(D, 10, device=0, keep_f32=False)
    K.add(_rows(10, D, 86).to(DEV))
    with pytest.raises(_lib.RevoError, match="keep_f32"):
        K.kmeans(_rows(3, D, 85).to(DEV))
    K.close()


# ---- 9. workspace regrow -------------------------------------------------------------------------------------------------------
def test_workspace_regrow_changes_no_byte():
    rows, cents = _between_two_centroids()
    G = _gallery(rows, experiments=True)
    want = G.kmeans(cents.to(DEV), max_iter=2, normalize=False)
    base = G.search_stats()
    try:
        assert G._lib.revo_debug_set_kmeans(64) == 0
        got = G.kmeans(cents.to(DEV), max_iter=2, normalize=False)
        small = G.search_stats()
    finally:
        G._lib.revo_debug_set_kmeans(0)
    _same(want, got, "regrow")
    print("passes:", base["join_passes"], "->", small["join_passes"])
    assert small["join_passes"] > base["join_passes"] and small["collected_rows"] == base["collected_rows"]
    G.close()


# ---- 10. store and facade ----------------------------------------------------------------------------------------------------
def test_store_themes():
    N, D = 600, 128
    gen = torch.Generator().manual_seed(90)
    centres = torch.nn.functional.normalize(torch.randn(6, D, generator=gen), dim=1)
    vec = centres[torch.randint(0, 6, (N,), generator=gen)] + 0.05 * torch.randn(N, D, generator=gen)
    payloads = [{"image_source": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2]} for r in range(N)]
    ids = [f"p{r}" for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(vec, ids, payloads)
    themes = st.themes(6, max_iter=10, seed=0)
    assert sum(t.size for t in themes) == N and [t.size for t in themes] == sorted((t.size for t in themes), reverse=True)
    assert sorted(i for t in themes for i in t.ids) == sorted(ids)
    init = st.gallery.read()[torch.from_numpy(store.seed_rows(np.ones(N, bool), 6, 0)).to(DEV)]
    _, labels, scores, sizes, _, _ = st.gallery.kmeans(init, max_iter=10)
    for t in themes:
        assert t.size == len(t.ids) and t.representative_id in t.ids
        rows = [int(i[1:]) for i in t.ids]
        assert rows == sorted(rows) and len(set(labels[rows].tolist())) == 1
        best = scores[rows].max()
        rep = int(t.representative_id[1:])
        assert float(scores[rep]) == float(best) == t.representative_score
        assert rep == min(r for r in rows if float(scores[r]) == float(best))
        assert t.representative_payload == payloads[rep]
    assert themes == st.themes(6, max_iter=10, seed=0)                   # seeded: reproducible
    assert [t.ids for t in st.themes(6, max_iter=0, seed=1)] != [t.ids for t in st.themes(6, max_iter=0, seed=0)]
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    cars = st.themes(4, seed=2, query_filter=flt)
    assert sum(t.size for t in cars) == N // 2 and all(int(i[1:]) % 2 == 0 for t in cars for i in t.ids)
    with pytest.raises(ValueError):
        st.themes(N // 2 + 1, query_filter=flt)


def test_summarize_database(tmp_path):
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, themes = r.summarize_database()
    assert text.startswith("❌") and themes == []
    folder = tmp_path / "images"
    folder.mkdir()
    rng = np.random.default_rng(91)
    for n in range(6):
        arr = (rng.integers(0, 256, (3,)) + rng.integers(0, 80, (96, 120, 3))) % 256
        Image.fromarray(arr.astype(np.uint8)).save(str(folder / f"img_{n}.jpg"), quality=90)
    assert "✅" in r.create_database(str(folder), "themes", use_direct_pe=True)
    db = r.vector_db
    text, themes = r.summarize_database(n_themes=2)
    assert text.startswith("🎯") and 1 <= len(themes) <= 2 and sum(t["size"] for t in themes) == len(db)
    for t in themes:
        assert set(t) == {"size", "ids", "representative"} and t["size"] == len(t["ids"])
        assert set(t["representative"]) == {"filename", "image_source", "bbox", "id", "score"}
        assert t["representative"]["id"] in t["ids"] and t["representative"]["filename"] in text
    text, themes = r.summarize_database(n_themes=len(db) + 1)            # the facade never raises to the UI
    assert text.startswith("❌") and themes == []
