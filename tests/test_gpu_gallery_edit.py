"""Removing and overwriting gallery rows in place (revo_gallery_remove / revo_gallery_update, include/revo.h EDIT;
Gallery.remove / update, GalleryStore.delete / update_vectors / set_payload / upsert(replace_existing=True),
SimpleReverso.delete_images).  The oracle is never the code under test: the rows an edit must leave are numpy on the master
bits read before it, and every search afterwards is compared, byte for byte, with the same search on a fresh gallery that
received those rows with normalize=False."""
import ctypes as C

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store
from reverso_amd.core_system import SimpleReverso

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _planted(N, D, seed, n_clusters=None):
    """N rows: random directions, and clusters of perturbed copies of a few of them (scores from about 0.8 to 0.95), so that
    thresholds, pairs and near-ties occur (as tests/test_gpu_range_search.py plants them)."""
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


def _gallery(x, keep_f32=True, extra=0, normalize=True, experiments=False):
    G = engine.Gallery(x.shape[1], max(1, x.shape[0] + extra), device=0, keep_f32=keep_f32, experiments=experiments)
    if x.shape[0]:
        G.add(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), normalize=normalize)
    return G


def _queries(x, Q, seed):
    """perturbed gallery rows (they hit their cluster) and a few random directions"""
    rng = np.random.default_rng(seed)
    N, D = x.shape
    q = rng.standard_normal((Q, D)).astype(np.float32)
    for i in range(0, Q, 2):
        r = int(rng.integers(N))
        q[i] = x[r] / np.linalg.norm(x[r]) + 0.3 * rng.standard_normal(D).astype(np.float32) / np.sqrt(D)
    for i in range(0, Q, 4):
        r = int(rng.integers(N))
        q[i] = x[r] + 0.02 * np.linalg.norm(x[r]) * rng.standard_normal(D).astype(np.float32) / np.sqrt(D)
    return torch.from_numpy(q).to(DEV)


def _read(G):
    """the fp32 master rows as numpy (an empty gallery has none to read)"""
    return G.read().cpu().numpy() if len(G) else np.zeros((0, G.dim), np.float32)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same(a, b, what):
    """two results (tuples of tensors): identical bytes -- scores, indices, counts, offsets and padding"""
    assert len(a) == len(b), what
    for j, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, j, u.shape, v.shape)
        assert _bytes(u) == _bytes(v), (what, j)


def _groups_of(n, seed):
    """group ids: runs of one to five rows, every ninth row in no group"""
    rng = np.random.default_rng(seed)
    g = np.repeat(np.arange(n), rng.integers(1, 6, size=n))[:n].astype(np.int32)
    g[::9] = -1
    return torch.from_numpy(g).to(DEV)


def _battery(G, q, which="all", allow=None, groups=None):
    """every search of the library on one gallery: name -> tuple of result tensors"""
    out = {}
    out["k10"] = G.search(q, k=10, allow=allow)
    out["range"] = G.search_range(q, 0.7, allow=allow)
    out["pairs"] = G.pairs(0.8, allow=allow)
    if which == "all":
        out["k10_thr"] = G.search(q, k=10, score_threshold=0.75, allow=allow)
        out["k50"] = G.search(q, k=50, allow=allow)
        out["k200"] = G.search(q, k=200, allow=allow)
        out["recommend"] = G.recommend(q[:3], q[3:5], k=20, allow=allow)
        out["mmr"] = G.search_mmr(q, k=10, diversity=0.5, allow=allow)
        if groups is not None:
            out["groups"] = G.search_groups(q, groups, limit=5, group_size=3, allow=allow)
            out["maxsim"] = G.search_maxsim(q[:4], groups, k=10, allow=allow, with_parts=True)
    return out


def _same_battery(G, F, q, which="all", allow=None, groups=None):
    a = _battery(G, q, which, allow, groups)
    b = _battery(F, q, which, allow, groups)
    assert a.keys() == b.keys()
    for name in a:
        _same(a[name], b[name], name)
    return a


def _masks(N, seed):
    """name -> bool [N]: the rows to remove"""
    rng = np.random.default_rng(seed)
    m = {"none": np.zeros(N, bool), "all": np.ones(N, bool)}
    for name, rows in (("row0", [0]), ("last", [N - 1]), ("middle", [N // 2])):
        m[name] = np.zeros(N, bool)
        m[name][rows] = True
    m["every_other"] = np.arange(N) % 2 == 0
    if N > 256:                                       # (a block across the boundary between rows 255 and 256 needs both)
        m["block"] = np.zeros(N, bool)
        m["block"][250:min(N, 262)] = True
    m["random_1pct"] = rng.random(N) < 0.01
    m["random_50pct"] = rng.random(N) < 0.5
    return m


def _mask_arg(mask, form):
    """the same rows in each form Gallery.remove takes"""
    if form == 0:
        return torch.from_numpy(mask).to(DEV)
    if form == 1:
        return torch.from_numpy(mask)                                 # host bool
    if form == 2:
        return torch.from_numpy(filters.pack_bits(mask))              # host packed bitmap
    if form == 3:
        return torch.from_numpy(filters.pack_bits(mask)).to(DEV)
    return torch.from_numpy(np.flatnonzero(mask).astype(np.int64)).to(DEV)


# ---- 1. remove: the rows move as numpy's rows[keep] ------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 1024])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000, 5000])
def test_remove_moves_the_rows(N, D):
    x = _planted(N, D, seed=N + D)
    tail = torch.from_numpy(_planted(3, D, seed=7)).to(DEV)
    for j, (name, mask) in enumerate(_masks(N, seed=N * 3 + D).items()):
        G = _gallery(x, extra=3)
        rows = G.read().cpu().numpy()                                 # the master bits before the edit
        removed = G.remove(_mask_arg(mask, j % 5))
        keep = ~mask
        assert removed == int(mask.sum()) and len(G) == int(keep.sum()), name
        assert _read(G).tobytes() == rows[keep].tobytes(), name
        # an append lands behind the survivors
        at = G.add(tail)
        assert at == int(keep.sum()) and len(G) == at + 3
        after = G.read().cpu().numpy()
        assert after[:at].tobytes() == rows[keep].tobytes(), name
        F = _gallery(np.zeros((0, D), np.float32), extra=3)
        F.add(tail)
        assert after[at:].tobytes() == F.read().cpu().numpy().tobytes(), name
        G.close(); F.close()


@pytest.mark.parametrize("case", ["row0", "random_30pct"])
def test_remove_across_many_chunks(case):
    """chunks of 64 rows on 5 000: about 80 chunk boundaries; removing row 0 alone moves every row by one, so every chunk's
    destination overlaps its own source rows (the staged form throughout); 30 % reaches the direct form after a few chunks"""
    N, D = 5000, 64
    lib = _lib.load_exp()
    x = _planted(N, D, seed=11)
    mask = np.zeros(N, bool)
    if case == "row0":
        mask[0] = True
    else:
        mask = np.random.default_rng(12).random(N) < 0.3
    assert lib.revo_debug_set_remove_chunk(64) == 0
    try:
        G = _gallery(x, experiments=True)
        rows = G.read().cpu().numpy()
        assert G.remove(torch.from_numpy(mask).to(DEV)) == int(mask.sum())
        assert G.read().cpu().numpy().tobytes() == rows[~mask].tobytes()
        F = _gallery(rows[~mask], normalize=False, experiments=True)
        q = _queries(x, 8, seed=13)
        _same(G.search(q, k=10), F.search(q, k=10), "k10")               # the bf16 scan copy moved with the master
        _same(G.pairs(0.8), F.pairs(0.8), "pairs")
        G.close(); F.close()
    finally:
        assert lib.revo_debug_set_remove_chunk(0) == 0


# ---- 2. remove: every search afterwards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,frac", [(5000, 64, 0.3), (3000, 1024, 0.5), (20000, 64, 0.01)])
def test_every_search_after_a_remove(N, D, frac):
    x = _planted(N, D, seed=N + 1)
    G = _gallery(x)
    rows = G.read().cpu().numpy()
    mask = np.random.default_rng(N + 2).random(N) < frac
    mask[0] = True
    assert G.remove(torch.from_numpy(mask).to(DEV)) == int(mask.sum())
    F = _gallery(rows[~mask], normalize=False)
    q = _queries(x[~mask], 16, seed=N + 3)
    res = _same_battery(G, F, q, groups=_groups_of(len(G), seed=5))
    assert int(res["pairs"][0].shape[0]) > 0 and int(res["range"][1].shape[0]) > 0       # the planted clusters are found
    G.close(); F.close()


def test_every_search_after_a_remove_with_a_filter_set_afterwards():
    N, D = 4000, 64
    x = _planted(N, D, seed=31)
    G = _gallery(x)
    rows = G.read().cpu().numpy()
    mask = np.random.default_rng(32).random(N) < 0.4
    G.remove(torch.from_numpy(mask))
    F = _gallery(rows[~mask], normalize=False)
    allow = torch.from_numpy(np.random.default_rng(33).random(len(G)) < 0.5).to(DEV)
    _same_battery(G, F, _queries(x[~mask], 16, seed=34), allow=allow, groups=_groups_of(len(G), seed=6))
    G.close(); F.close()


def test_search_after_a_remove_without_the_fp32_master():
    N, D = 4000, 64
    x = _planted(N, D, seed=41)
    mask = np.random.default_rng(42).random(N) < 0.3
    G = _gallery(x, keep_f32=False)
    assert G.remove(torch.from_numpy(mask).to(DEV)) == int(mask.sum())
    F = _gallery(x[~mask], keep_f32=False)
    q = _queries(x[~mask], 16, seed=43)
    _same(G.search(q, k=10), F.search(q, k=10), "k10")
    G.close(); F.close()


def test_removing_a_row_of_huge_norm_leaves_loose_maxima_and_exact_results():
    """a row of norm 1000 appended as given: the certificate's row maximum stays at 1000 on the edited gallery (an upper
    bound still) and is about 1 on the fresh one; the results are the same bytes"""
    N, D = 3000, 64
    x = _planted(N, D, seed=51)
    huge = (1000.0 * x[7] / np.linalg.norm(x[7])).astype(np.float32)[None]
    G = engine.Gallery(D, N + 1, device=0)
    G.add(torch.from_numpy(x[:1500]).to(DEV))
    G.add(torch.from_numpy(huge).to(DEV), normalize=False)
    G.add(torch.from_numpy(x[1500:]).to(DEV))
    rows = G.read().cpu().numpy()
    assert abs(float(np.linalg.norm(rows[1500])) - 1000.0) < 0.01
    assert G.remove(torch.tensor([1500])) == 1
    keep = np.ones(N + 1, bool)
    keep[1500] = False
    F = _gallery(rows[keep], normalize=False)
    _same_battery(G, F, _queries(x, 16, seed=52), groups=_groups_of(N, seed=7))
    G.close(); F.close()


# ---- 3. update ---------------------------------------------------------------------------------------------------------------
def _index_sets(N):
    return {"first": [0], "last": [N - 1],
            "scattered_descending": sorted(np.random.default_rng(61).choice(N, 37, replace=False).tolist(), reverse=True)}


@pytest.mark.parametrize("D", [64, 1024, 2112])          # (2112 > 2048: the normalisation kernel's path outside registers)
def test_update_writes_what_an_append_would(D):
    N = 1000
    x = _planted(N, D, seed=D)
    for name, idx in _index_sets(N).items():
        new = _planted(len(idx), D, seed=D + len(idx)) * 3.0          # not unit length: the update normalises
        G = _gallery(x)
        G.update(idx if name != "last" else torch.tensor(idx), torch.from_numpy(new).to(DEV) if name != "first" else torch.from_numpy(new))
        x2 = x.copy()
        x2[idx] = new
        F = _gallery(x2)                                              # had the new vectors there from the start
        assert G.read().cpu().numpy().tobytes() == F.read().cpu().numpy().tobytes(), name
        _same_battery(G, F, _queries(x2, 8, seed=D + 1), which="reduced")
        G.close(); F.close()


def test_update_with_normalize_off_stores_the_rows_as_given():
    N, D = 300, 64
    x = _planted(N, D, seed=71)
    G = _gallery(x)
    rows = G.read().cpu().numpy()
    new = (2.5 * _planted(2, D, seed=72)).astype(np.float32)
    G.update([5, 299], torch.from_numpy(new).to(DEV), normalize=False)
    rows[[5, 299]] = new
    assert G.read().cpu().numpy().tobytes() == rows.tobytes()
    G.close()


def test_filter_and_groups_set_before_an_update_still_work():
    N, D = 2000, 64
    x = _planted(N, D, seed=81)
    G = _gallery(x)
    lib, h = G._lib, G._h
    allow = torch.from_numpy(np.random.default_rng(82).random(N) < 0.5).to(DEV)
    bits = G.allow_bits(allow)
    groups = _groups_of(N, seed=8)
    st = _lib.current_stream()
    assert lib.revo_search_set_filter(h, _lib.ptr(bits), N, 1, st) == 0
    assert lib.revo_search_set_groups(h, _lib.ptr(groups), N, 1, st) == 0
    idx = [3, 1999, 1000]
    new = _planted(3, D, seed=83)
    G.update(idx, torch.from_numpy(new).to(DEV))
    x2 = x.copy()
    x2[idx] = new
    F = _gallery(x2)
    q = _queries(x2, 8, seed=84)
    try:
        _same(G.search(q, k=10), F.search(q, k=10, allow=allow), "filtered k10 through the handle's own filter")
        # the grouped search with the handle's own filter and group ids (Gallery.search_groups would set them anew)
        Q, L, S = q.shape[0], 5, 2
        s = torch.empty((Q, L, S), dtype=torch.float32, device=DEV)
        i = torch.empty((Q, L, S), dtype=torch.int64, device=DEV)
        hc = torch.empty((Q, L), dtype=torch.int32, device=DEV)
        gid = torch.empty((Q, L), dtype=torch.int32, device=DEV)
        gc = torch.empty((Q,), dtype=torch.int32, device=DEV)
        _lib.check(lib.revo_search_groups(h, _lib.ptr(q), Q, L, S, 0, 0.0, 0, _lib.ptr(s), _lib.ptr(i), _lib.ptr(hc), _lib.ptr(gid),
                                          _lib.ptr(gc), st), "revo_search_groups")
        _same((s, i, hc, gid, gc), F.search_groups(q, groups, limit=L, group_size=S, allow=allow), "groups")
    finally:
        lib.revo_search_set_filter(h, None, 0, 0, None)
        lib.revo_search_set_groups(h, None, 0, 0, None)
    G.close(); F.close()


# ---- 4. lifecycle and errors ---------------------------------------------------------------------------------------------------
def _held_results_are_gone(G):
    lib = G._lib
    assert lib.revo_gallery_pairs_read(G._h, 0, 0, None, None, 1) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_search_range_read(G._h, None, 0, 0, None, None, 1) == -2 and b"no result" in lib.revo_last_error()


@pytest.mark.parametrize("edit", ["remove", "update"])
def test_an_edit_invalidates_held_pairs_and_range_results(edit):
    N, D = 500, 64
    x = _planted(N, D, seed=91)
    G = _gallery(x)
    q = _queries(x, 4, seed=92)
    G.pairs(0.8)
    G.search_range(q, 0.7)
    lib = G._lib
    assert lib.revo_gallery_pairs_read(G._h, 0, 0, None, None, 1) == 0
    assert lib.revo_search_range_read(G._h, None, 0, 0, None, None, 1) == 0
    if edit == "remove":
        assert G.remove(torch.tensor([17])) == 1
    else:
        G.update([17], torch.from_numpy(x[:1]).to(DEV))
    _held_results_are_gone(G)
    G.close()


def test_a_filter_set_before_a_remove_fails_the_next_search():
    N, D = 500, 64
    G = _gallery(_planted(N, D, seed=101))
    lib, h = G._lib, G._h
    bits = G.allow_bits(torch.ones(N, dtype=torch.bool, device=DEV))
    assert lib.revo_search_set_filter(h, _lib.ptr(bits), N, 1, _lib.current_stream()) == 0
    assert G.remove(torch.tensor([1, 2])) == 2
    with pytest.raises(_lib.RevoError, match="the filter was set for 500 rows but the gallery holds 498"):
        G.search(torch.randn(1, D, device=DEV), k=3)
    lib.revo_search_set_filter(h, None, 0, 0, None)
    assert int(G.search(torch.randn(1, D, device=DEV), k=3)[2][0]) == 3
    G.close()


def test_argument_errors_and_no_ops():
    N, D = 300, 64
    x = _planted(N, D, seed=111)
    G = _gallery(x)
    rows = G.read().cpu().numpy()
    lib, h, st = G._lib, G._h, _lib.current_stream()
    n = C.c_int64(-5)
    bits = torch.zeros((N + 31) // 32 + 4, dtype=torch.int32, device=DEV)
    for wrong in (N - 1, N + 1, 0):
        assert lib.revo_gallery_remove(h, _lib.ptr(bits), wrong, 1, C.byref(n), st) == -2
        assert b"rows must equal revo_gallery_size" in lib.revo_last_error() and n.value == -5
    v = torch.from_numpy(x[:2].copy()).to(DEV)
    with pytest.raises(_lib.RevoError, match="given twice"):
        G.update([5, 5], v)
    for bad in ([5, N], [-1, 5]):
        with pytest.raises(_lib.RevoError, match="outside the gallery"):
            G.update(bad, v)
    with pytest.raises(IndexError):
        G.remove(torch.tensor([N]))
    with pytest.raises(ValueError):
        G.remove(torch.zeros(N - 1, dtype=torch.bool))
    G.update([], torch.empty((0, D)))                                  # n = 0: nothing happens
    assert G.remove(torch.zeros(N, dtype=torch.bool)) == 0
    # bits at or past `rows` are ignored: rows 288 .. 299 are bits 0 .. 11 of word 9
    bits[10:] = -1
    bits[9] = -(1 << 12)
    assert lib.revo_gallery_remove(h, _lib.ptr(bits), N, 1, C.byref(n), st) == 0 and n.value == 0
    assert len(G) == N and G.read().cpu().numpy().tobytes() == rows.tobytes()
    G.close()


def test_remove_on_an_empty_gallery_and_down_to_empty():
    D = 64
    G = engine.Gallery(D, 600, device=0)
    assert G.remove(torch.zeros(0, dtype=torch.bool)) == 0 and len(G) == 0
    x = _planted(500, D, seed=121)
    big = torch.from_numpy(50.0 * x[:1]).to(DEV)
    G.add(big, normalize=False)                                        # raises the row maxima, which an emptied gallery drops
    G.add(torch.from_numpy(x).to(DEV))
    assert G.remove(torch.ones(501, dtype=torch.bool, device=DEV)) == 501 and len(G) == 0
    q = _queries(x, 4, seed=122)
    s, i, c = G.search(q, k=3)
    assert int(c.sum()) == 0 and bool((i == -1).all())
    G.add(torch.from_numpy(x).to(DEV))
    F = _gallery(x)
    assert G.read().cpu().numpy().tobytes() == F.read().cpu().numpy().tobytes()
    _same_battery(G, F, q, groups=_groups_of(500, seed=9))
    G.close(); F.close()


# ---- 5. through the store and the facade ---------------------------------------------------------------------------------------
def _points(n, D, seed):
    x = _planted(n, D, seed=seed)
    ids = [f"p{j}" for j in range(n)]
    payloads = [{"image_source": f"/img/{j // 3}.jpg", "filename": f"{j // 3}.jpg", "n": j} for j in range(n)]
    return x, ids, payloads


def _hits(st, q, **kw):
    return [(h.id, h.score, h.payload) for h in st.search(q, 10, **kw)]


def _same_as_a_store_of(st, final, q):
    """the store answers like one built from the final points alone: same ids, scores and payloads"""
    ref = store.GalleryStore(st.dim, device=0, capacity=max(len(final), 1))
    if final:
        ref.gallery.add(torch.stack([v for _, v, _ in final]).to(DEV), normalize=False)
        ref.ids = [pid for pid, _, _ in final]
        ref.payloads = [pl for _, _, pl in final]
    assert st.ids == ref.ids and st.payloads == ref.payloads
    for j in range(q.shape[0]):
        assert _hits(st, q[j]) == _hits(ref, q[j])
        f = {"must": [{"key": "n", "range": {"gte": 40}}]}
        assert _hits(st, q[j], query_filter=f) == _hits(ref, q[j], query_filter=f)
    ref.close()


def test_store_delete_update_upsert_set_payload_and_reload(tmp_path):
    D, n = 64, 120
    x, ids, payloads = _points(n, D, seed=131)
    db = str(tmp_path / "db")
    st = store.GalleryStore(D, device=0, capacity=16, path=db)
    st.upsert(torch.from_numpy(x[:100]), ids[:100], [dict(p) for p in payloads[:100]])
    st.save()
    st.upsert(torch.from_numpy(x[100:]), ids[100:], [dict(p) for p in payloads[100:]])      # pending rows: flushed by the edit
    q = torch.from_numpy(x[[3, 50, 110]] + 0.01 * _planted(3, D, seed=132))
    st.search(q[0], 5, query_filter={"must": [{"key": "n", "range": {"gte": 40}}]})          # fills the caches an edit must drop

    def final_points():
        g = st.gallery.read().cpu()
        return [(pid, g[r], pl) for r, (pid, pl) in enumerate(zip(st.ids, st.payloads))]

    def norm(v):
        v = np.asarray(v, np.float32)
        return torch.from_numpy(v / np.linalg.norm(v, axis=-1, keepdims=True))

    # the expectation, kept by hand: id -> (vector as stored, payload), in row order
    want = [(pid, None, dict(pl)) for pid, pl in zip(ids, payloads)]
    before = st.gallery.read().cpu()
    want = [(pid, before[r], pl) for r, (pid, _, pl) in enumerate(want)]

    # delete by ids (one unknown), then by filter
    assert st.delete(["p3", "p50", "nobody"]) == 2 and len(st) == n - 2
    want = [w for w in want if w[0] not in ("p3", "p50")]
    _same_as_a_store_of(st, want, q)
    assert st.delete(filters.Filter(must=[filters.FieldCondition("image_source", match=filters.MatchValue("/img/7.jpg"))])) == 3
    want = [w for w in want if w[2]["image_source"] != "/img/7.jpg"]
    assert st.delete({"must": [{"key": "n", "range": {"gte": 1000}}]}) == 0
    _same_as_a_store_of(st, want, q)

    # new vectors for two points
    new = _planted(2, D, seed=133)
    st.update_vectors(["p110", "p0"], torch.from_numpy(new))
    with pytest.raises(KeyError):
        st.update_vectors(["p3"], torch.from_numpy(new[:1]))               # deleted above
    got = {w[0]: r for r, w in enumerate(want)}
    F = _gallery(new)                                                      # what an append of the new vectors stores
    stored = F.read().cpu()
    F.close()
    for j, pid in enumerate(["p110", "p0"]):
        want[got[pid]] = (pid, stored[j], want[got[pid]][2])
    _same_as_a_store_of(st, want, q)
    assert torch.equal(torch.stack([w[1] for w in want]), st.gallery.read().cpu())

    # payload only
    st.set_payload(["p1", "p2"], {"image_source": "/img/moved.jpg", "filename": "moved.jpg", "n": 77})
    with pytest.raises(KeyError):
        st.set_payload(["nobody"], {})
    for pid in ("p1", "p2"):
        want[got[pid]] = (pid, want[got[pid]][1], {"image_source": "/img/moved.jpg", "filename": "moved.jpg", "n": 77})
    _same_as_a_store_of(st, want, q)

    # the database's own upsert: p5 and p119 replaced in place, two new points appended; p3 comes back as a new point
    up = _planted(5, D, seed=134)
    up_ids = ["p5", "new0", "p119", "p3", "p5"]                            # p5 twice: the last entry counts
    up_pl = [{"n": 500 + j, "image_source": "/img/up.jpg"} for j in range(5)]
    st.upsert(torch.from_numpy(up), up_ids, up_pl, replace_existing=True)
    F = _gallery(up)
    stored = F.read().cpu()
    F.close()
    want[got["p5"]] = ("p5", stored[4], up_pl[4])
    want[got["p119"]] = ("p119", stored[2], up_pl[2])
    want += [("new0", stored[1], up_pl[1]), ("p3", stored[3], up_pl[3])]
    _same_as_a_store_of(st, want, q)
    assert len(st) == n - 5 + 2

    # the default still appends whatever the id
    st.upsert(torch.from_numpy(up[:1]), ["p5"], [up_pl[0]])
    want.append(("p5", stored[0], up_pl[0]))
    assert len(st) == n - 2 and st.ids.count("p5") == 2
    st.save()
    final = final_points()
    assert [w[0] for w in want] == [f[0] for f in final] and [w[2] for w in want] == [f[2] for f in final]
    assert torch.equal(torch.stack([w[1] for w in want]), torch.stack([f[1] for f in final]))
    st.close()

    # the manifest replays to the same store; a compact copy written elsewhere too
    re = store.GalleryStore.load(db, device=0)
    _same_as_a_store_of(re, final, q)
    assert torch.equal(re.gallery.read().cpu(), torch.stack([f[1] for f in final]))
    assert re.delete(["new0"]) == 1                                        # and goes on from there
    re.save()
    other = str(tmp_path / "compact")
    re.save(path=other)
    re.close()
    final = [f for f in final if f[0] != "new0"]
    for path in (db, other):
        again = store.GalleryStore.load(path, device=0)
        _same_as_a_store_of(again, final, q)
        again.close()
    recs = store.read_manifest(str(tmp_path / "compact" / store.MANIFEST))[1]
    assert len(recs) == 1 and "op" not in recs[0] and recs[0]["rows"] == len(final)


def test_facade_delete_images(tmp_path):
    D = 64
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "root"), max_batch=4)
    assert r.delete_images(["/img/0.jpg"]).startswith("❌ No database loaded")
    x, ids, payloads = _points(30, D, seed=141)
    db = str(tmp_path / "root" / "small")
    st = store.GalleryStore(D, device=0, capacity=64, collection="simple_reverso_small", path=db)
    st.upsert(torch.from_numpy(x), ids, payloads)
    st.save()
    r.vector_db, r.current_database = st, st.collection
    assert r.delete_images().startswith("❌ Please provide")
    assert r.delete_images("/img/nowhere.jpg").startswith("⚠️ No stored regions matched")
    msg = r.delete_images(["/img/0.jpg", "/img/4.jpg"])
    assert msg.startswith("✅ Deleted 6 regions (24 left") and len(st) == 24
    msg = r.delete_images(query_filter={"must": [{"key": "n", "range": {"gte": 27}}]})
    assert msg.startswith("✅ Deleted 3 regions (21 left")
    msg = r.delete_images("/img/1.jpg", query_filter={"must": [{"key": "n", "match": {"value": 4}}]})
    assert msg.startswith("✅ Deleted 1 regions (20 left")
    gone = {0, 1, 2, 12, 13, 14, 27, 28, 29, 4}
    assert st.ids == [f"p{j}" for j in range(30) if j not in gone]
    left = st.gallery.read().cpu()
    assert r.load_database("small").startswith("✅")                    # the directory is a finished database with the same points
    assert r.vector_db.ids == [f"p{j}" for j in range(30) if j not in gone]
    assert torch.equal(r.vector_db.gallery.read().cpu(), left)
    r.vector_db.close()
