"""Duplicate clusters of one gallery (revo_gallery_clusters, include/revo.h CLUSTERS; Gallery.clusters,
GalleryStore.duplicate_clusters, SimpleReverso.find_duplicate_clusters): against the pairs route (Gallery.pairs +
store.connected_groups) and an fp64 oracle, on a chain that only single linkage joins, on a cluster too dense for the pairs
route, on thresholds that sit exactly on a pair's fp32 score, through the result's lifecycle, and through the store and the
facade."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine, filters, store

from test_gpu_gallery_pairs import _delta, _gallery, _oracle, _planted

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _lists(offsets, members):
    return store.split_clusters(offsets.cpu().numpy(), members.cpu().numpy())


def _labels_of(groups, n, allow=None):
    """labels derived from the groups: a row of a group has the group's first row, any other allowed row itself"""
    lab = np.arange(n, dtype=np.int64)
    if allow is not None:
        lab[~allow] = -1
    for g in groups:
        lab[g] = g[0]
    return lab


def _check_shape(labels, offsets, members, n):
    """the contract's own invariants, whatever the data"""
    lab, off, mem = labels.cpu().numpy(), offsets.cpu().numpy(), members.cpu().numpy()
    assert lab.shape == (n,) and off[0] == 0 and off[-1] == mem.shape[0] and (np.diff(off) >= 2).all()
    groups = [mem[a:b] for a, b in zip(off[:-1], off[1:])]
    assert all((np.diff(g) > 0).all() for g in groups)                          # members ascend
    firsts = [int(g[0]) for g in groups]
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)         # clusters by lowest row
    assert all((lab[g] == g[0]).all() for g in groups)
    single = np.setdiff1d(np.arange(n), mem)
    assert ((lab[single] == single) | (lab[single] == -1)).all()


def _clear_threshold(rows, t, delta, allow=None):
    """t, moved up in steps of 1e-5 until no pair's fp64 score lies within the fp32 chain's band of it: (t, oracle groups)"""
    for step in range(50):
        tt = t + step * 1e-5
        must, may, score = _oracle(rows, tt, delta, allow=allow)
        if not {p for p in may if abs(score[p] - tt) <= delta}:
            return tt, store.connected_groups(np.array(sorted(must), dtype=np.int64).reshape(-1, 2), rows.shape[0])
    raise AssertionError("no threshold without a pair inside the band")


# ---- 1. equals the pairs route and the fp64 oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 1300, 4096])
@pytest.mark.parametrize("D", [64, 256])
def test_equals_the_pairs_route_and_the_fp64_oracle(N, D):
    _equals_the_pairs_route_and_the_fp64_oracle(N, D)


@pytest.mark.parametrize("N", [256, 257, 513, 5889])
def test_equals_the_pairs_route_where_the_tile_walk_turns(N):
    """the sizes of test_gpu_gallery_pairs.py's test of the same name: one full tile, a partial last tile with the wrap of tj,
    three tiles, and more tile pairs (276) than workgroups"""
    _equals_the_pairs_route_and_the_fp64_oracle(N, 64)


def _equals_the_pairs_route_and_the_fp64_oracle(N, D):
    x = _planted(N, D, seed=3 * N + D)
    G = _gallery(x)
    rows = G.read()
    n_groups = 0
    for t0 in (0.8, 0.9):
        t, want64 = _clear_threshold(rows, t0, _delta(D))
        labels, offsets, members = G.clusters(t)
        _check_shape(labels, offsets, members, N)
        pairs, _ = G.pairs(t)
        want = store.connected_groups(pairs.cpu().numpy(), N)
        assert _lists(offsets, members) == want == want64
        assert np.array_equal(labels.cpu().numpy(), _labels_of(want, N))
        n_groups += len(want)
    if N == 1:
        assert labels.tolist() == [0] and offsets.tolist() == [0] and members.shape == (0,)
    else:
        assert n_groups > 0
    G.close()


# ---- 2. single linkage across tiles ------------------------------------------------------------------------------------------
def _chain(L, D, rho, seed):
    """L unit rows (fp64): r[i + 1] = rho r[i] + sqrt(1 - rho^2) n[i], n[i] orthonormal to everything before -- the score
    of rows i and j is rho^|i - j|"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, L + 1)))
    r = np.empty((L, D))
    r[0] = q[:, 0]
    for i in range(L - 1):
        r[i + 1] = rho * r[i] + np.sqrt(1 - rho * rho) * q[:, i + 1]
    return r


def test_single_linkage_joins_a_chain_scattered_over_the_tiles():
    L, D, N = 200, 256, 1300
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pos = np.random.default_rng(22).permutation(N)[:L]                 # chain row i lives in gallery row pos[i]
    assert len({int(p) // 256 for p in pos}) >= 5                       # five row tiles and more: every tile pair, the diagonal
    x[pos] = _chain(L, D, 0.93, seed=23).astype(np.float32)
    # the construction, checked on the CPU over the rows as they are handed in (unit to fp32 rounding): consecutive scores
    # 0.93, every other pair of the gallery at most 0.93^2 = 0.8649 (to the same 2e-7), and every pair's bf16 score within
    # 9.5e-4 of its fp64 score -- so 0.9 and 0.94 separate the two kinds whichever path a pair takes
    rows = torch.from_numpy(x)
    S = rows.double() @ rows.double().T
    Sb = rows.bfloat16().double() @ rows.bfloat16().double().T
    assert (S[pos[:-1], pos[1:]] - 0.93).abs().max() <= 2e-7
    other = S.clone()
    other[pos[:-1], pos[1:]] = -1
    other[pos[1:], pos[:-1]] = -1
    other.fill_diagonal_(-1)
    assert other.max() <= 0.86490 + 2e-7
    assert (Sb - S).abs().fill_diagonal_(0).max() <= 9.5e-4
    G = _gallery(x)
    chain_rows = sorted(int(p) for p in pos)
    labels, offsets, members = G.clusters(0.9)
    _check_shape(labels, offsets, members, N)
    assert _lists(offsets, members) == [chain_rows]
    assert np.array_equal(labels.cpu().numpy(), _labels_of([chain_rows], N))
    assert int(labels[chain_rows[-1]]) == chain_rows[0]
    # without the chain's 100th row: two clusters of 99 and 100 rows
    allow = np.ones(N, dtype=bool)
    allow[pos[99]] = False
    halves = sorted([sorted(int(p) for p in pos[:99]), sorted(int(p) for p in pos[100:])])
    labels, offsets, members = G.clusters(0.9, allow=torch.from_numpy(allow).to(DEV))
    _check_shape(labels, offsets, members, N)
    assert _lists(offsets, members) == halves and sorted(len(h) for h in halves) == [99, 100]
    assert int(labels[pos[99]]) == -1
    assert np.array_equal(labels.cpu().numpy(), _labels_of(halves, N, allow))
    # above every score of the chain
    labels, offsets, members = G.clusters(0.94)
    assert offsets.tolist() == [0] and members.shape == (0,)
    assert np.array_equal(labels.cpu().numpy(), np.arange(N))
    G.close()


# ---- 3. a dense cluster past the pairs cap -----------------------------------------------------------------------------------
def _far_apart_rows(n, D, away_from, seed, limit=0.4):
    """n random unit rows whose scores with each other and with `away_from` stay below `limit` (random rows of D = 64 do
    reach 0.5 now and then: those are left out)"""
    cand = np.random.default_rng(seed).standard_normal((4 * n, D))
    cand /= np.linalg.norm(cand, axis=1, keepdims=True)
    kept = [away_from / np.linalg.norm(away_from)]
    for c in cand:
        if np.abs(np.stack(kept) @ c).max() < limit:
            kept.append(c)
            if len(kept) == n + 1:
                break
    assert len(kept) == n + 1
    return np.stack(kept[1:]).astype(np.float32)


def test_dense_cluster_past_the_pairs_cap():
    D, n, extra = 64, 24_000, 500         # 287 988 000 identical pairs: tests/test_gpu_gallery_pairs.py pins that pairs refuses
    v = np.random.default_rng(12).standard_normal(D).astype(np.float32)
    x = np.concatenate([np.repeat(v[None], n, 0), _far_apart_rows(extra, D, v.astype(np.float64), seed=31)])
    G = _gallery(x)
    labels, offsets, members = G.clusters(0.5)
    st = G.search_stats()
    assert offsets.tolist() == [0, n]
    assert torch.equal(members, torch.arange(n, device=DEV))
    assert torch.equal(labels[:n], torch.zeros(n, dtype=torch.int64, device=DEV))
    assert torch.equal(labels[n:], torch.arange(n, n + extra, device=DEV))         # the random rows stay singletons
    assert st["collected_rows"] == 0 and st["join_passes"] == 1                   # every edge is certain: nothing re-scored
    assert all(st[k] == 0 for k in ("uncertified", "bruteforced", "checked", "from_segments", "grouped_fallback",
                                    "large_k_fallback"))
    c = C.c_int64(-5)                                                             # the pairs route still refuses this input
    assert G._lib.revo_gallery_pairs(G._h, 0.5, C.byref(c), _lib.current_stream()) == -2
    assert b"candidate pairs exceed" in G._lib.revo_last_error()
    G.close()


# ---- 4. the ambiguous path, with teeth ---------------------------------------------------------------------------------------
def test_threshold_on_the_score_of_two_thousand_identical_rows():
    D, n = 64, 2000
    v = np.random.default_rng(10).standard_normal(D).astype(np.float32)
    x = np.repeat(v[None], n, 0)
    P = _gallery(x)                       # (a handle of its own: its pairs call grows the workspace the clusters call shares)
    s = P.pairs(0.5)[1][0].cpu().numpy()  # the exact fp32 score of every pair
    P.close()
    G = _gallery(x)
    labels, offsets, members = G.clusters(float(s))
    st = G.search_stats()
    assert offsets.tolist() == [0, n] and torch.equal(members, torch.arange(n, device=DEV))
    assert torch.equal(labels, torch.zeros(n, dtype=torch.int64, device=DEV))
    assert st["collected_rows"] == 1_999_000 and st["join_passes"] == 2           # every pair re-scored, behind a regrow
    again = G.clusters(float(s))
    assert all(torch.equal(a, b) for a, b in zip((labels, offsets, members), again))
    up = np.nextafter(s, np.float32(np.inf))
    labels, offsets, members = G.clusters(float(up))
    st = G.search_stats()
    assert offsets.tolist() == [0] and members.shape == (0,)
    assert torch.equal(labels, torch.arange(n, device=DEV))
    assert st["collected_rows"] == 1_999_000
    G.close()


def test_threshold_on_the_score_of_a_planted_pair():
    N, D = 1300, 256
    G = _gallery(_planted(N, D, seed=41))
    rows = G.read()
    delta = _delta(D)
    pairs, scores = G.pairs(0.8)
    pairs, scores = pairs.cpu().numpy(), scores.cpu().numpy()
    assert pairs.shape[0] >= 30
    done = 0
    for e in np.linspace(0, pairs.shape[0] - 1, 12).astype(int).tolist():
        i, j = int(pairs[e, 0]), int(pairs[e, 1])
        s = scores[e]
        up = np.nextafter(s, np.float32(np.inf))
        # the oracle at `up`: every other pair must be outside the band; the pair itself (fp32 score s < up) is no edge
        must, may, score = _oracle(rows, float(up), delta)
        if {p for p in may if abs(score[p] - float(up)) <= delta} != {(i, j)}:
            continue
        groups = store.connected_groups(np.array(sorted(must - {(i, j)}), dtype=np.int64).reshape(-1, 2), N)
        by_another_path = any(i in g and j in g for g in groups)
        labels, _, _ = G.clusters(float(s))
        assert int(labels[i]) == int(labels[j])                                   # t = the pair's own score bits: an edge
        labels, offsets, members = G.clusters(float(up))
        assert (int(labels[i]) == int(labels[j])) == by_another_path, (i, j, s)
        assert _lists(offsets, members) == groups
        done += 1
        if done == 3:
            break
    assert done == 3
    G.close()


# ---- 5. lifecycle and edges --------------------------------------------------------------------------------------------------
def _raw_read(G, which=(True, True, True), on_device=True):
    """revo_gallery_clusters_read with the chosen pointers (the others NULL) into buffers sized generously and pre-filled"""
    n = len(G)
    dev = DEV if on_device else "cpu"
    bufs = [torch.full((n + 2,), -7, dtype=torch.int64, device=dev) for _ in range(3)]
    ptrs = [(_lib.ptr(b) if on_device else b.data_ptr()) if w else None for b, w in zip(bufs, which)]
    rc = G._lib.revo_gallery_clusters_read(G._h, *ptrs, int(on_device))
    return rc, bufs


def test_result_lifecycle():
    N, D = 1300, 64
    x = _planted(N, D, seed=51, n_clusters=100)
    G = _gallery(x, extra=10)
    labels, offsets, members = G.clusters(0.85)
    nc, nm = offsets.shape[0] - 1, members.shape[0]
    assert nc > 10
    full = (labels, offsets, members)
    sizes = (N, nc + 1, nm)
    # NULL output pointers in every combination; host and device destinations
    for mask in range(8):
        which = tuple(bool(mask >> k & 1) for k in range(3))
        for on_device in (True, False):
            rc, bufs = _raw_read(G, which, on_device)
            assert rc == 0
            for b, w, want, size in zip(bufs, which, full, sizes):
                assert torch.equal(b[:size].cpu(), want.cpu()) if w else bool((b == -7).all())
                assert bool((b[size:] == -7).all())                                # nothing written past the result
    # a pairs and a range result survive a clusters call, and the clusters result survives them
    p1, s1 = G.pairs(0.85)
    off1, idx1, sc1 = G.search_range(G.read(0, 3), 0.85)
    again = G.clusters(0.85)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    pb = torch.empty_like(p1); sb = torch.empty_like(s1)
    assert G._lib.revo_gallery_pairs_read(G._h, 0, p1.shape[0], _lib.ptr(pb), _lib.ptr(sb), 1) == 0
    assert torch.equal(pb, p1) and torch.equal(sb, s1)
    ob = torch.empty_like(off1); ib = torch.empty_like(idx1); cb = torch.empty_like(sc1)
    assert G._lib.revo_search_range_read(G._h, _lib.ptr(ob), 0, idx1.shape[0], _lib.ptr(ib), _lib.ptr(cb), 1) == 0
    assert torch.equal(ob, off1) and torch.equal(ib, idx1) and torch.equal(cb, sc1)
    G.pairs(0.9)
    G.search_range(G.read(0, 3), 0.9)
    G.search(G.read(0, 3), k=5)
    rc, bufs = _raw_read(G)
    assert rc == 0 and all(torch.equal(b[:size], want) for b, want, size in zip(bufs, full, sizes))
    # every change of the rows drops the result
    def gone():
        rc, _ = _raw_read(G)
        return rc == -2 and b"no result" in G._lib.revo_last_error()
    G.add(torch.from_numpy(x[:5]).to(DEV))
    assert gone()
    G.clusters(0.85)
    G.update([3], torch.from_numpy(x[7:8]).to(DEV))
    assert gone()
    labels, _, _ = G.clusters(0.85)
    assert int(labels[3]) == int(labels[7])                                       # rows 3 and 7 are now identical
    assert G.remove(torch.tensor([0, 1], dtype=torch.int64)) == 2
    assert gone()
    G.clusters(0.85)
    assert _raw_read(G)[0] == 0
    G.clear()
    assert gone()
    G.close()


def test_refusals_and_empty_inputs():
    D = 64
    x = _planted(3000, D, seed=52)
    G = _gallery(x, extra=10)
    nc, nm = C.c_int64(-5), C.c_int64(-6)
    # a filter set for another size
    bits = G.allow_bits(torch.ones(3000, dtype=torch.bool, device=DEV))
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), 3000, 1, _lib.current_stream()) == 0
    G.add(torch.from_numpy(x[:10]).to(DEV))
    assert G._lib.revo_gallery_clusters(G._h, 0.9, C.byref(nc), C.byref(nm), _lib.current_stream()) == -2
    assert b"set it again" in G._lib.revo_last_error() and (nc.value, nm.value) == (-5, -6)
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    # a filter that allows no row
    labels, offsets, members = G.clusters(0.5, allow=torch.zeros(3010, dtype=torch.bool, device=DEV))
    assert offsets.tolist() == [0] and members.shape == (0,) and bool((labels == -1).all())
    labels, offsets, members = G.clusters(0.9)                                    # the filter was cleared again
    assert offsets.shape[0] > 1 and bool((labels >= 0).all())
    G.close()
    K = _gallery(x[:300], keep_f32=False)                                        # no fp32 master rows
    assert K._lib.revo_gallery_clusters(K._h, 0.9, C.byref(nc), C.byref(nm), _lib.current_stream()) == -2
    assert b"keep_f32" in K._lib.revo_last_error()
    with pytest.raises(_lib.RevoError):
        K.clusters(0.9)
    K.close()
    E = engine.Gallery(D, 10, device=0)                                           # an empty gallery
    labels, offsets, members = E.clusters(0.5)
    assert labels.shape == (0,) and offsets.tolist() == [0] and members.shape == (0,)
    st = E.search_stats()
    assert st["collected_rows"] == 0
    E.add(torch.from_numpy(x[:1]).to(DEV))                                        # a single row: its own label
    labels, offsets, members = E.clusters(-1.0)
    assert labels.tolist() == [0] and offsets.tolist() == [0]
    E.close()


# ---- 6. store and facade -----------------------------------------------------------------------------------------------------
def test_store_duplicate_clusters_equal_duplicate_groups():
    N, D = 6000, 256                       # the data of test_store_duplicate_groups_recover_the_planted_clusters
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
    assert st.duplicate_clusters(0.95) == groups
    assert st.duplicate_row_clusters(0.95) == st.duplicate_row_groups(0.95) == sorted(clusters)
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("car"))])
    filtered = st.duplicate_groups(0.95, query_filter=flt)
    assert 0 < len(filtered) < len(groups)
    assert st.duplicate_clusters(0.95, query_filter=flt) == filtered
    assert st.duplicate_clusters(0.95) == groups                                  # the filter was cleared again


def test_find_duplicate_clusters_on_a_database(tmp_path):
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    text, groups = r.find_duplicate_clusters()
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
    text0, groups0 = r.find_duplicates(similarity_threshold=0.95)
    assert len(groups0) >= 2
    text1, groups1 = r.find_duplicate_clusters(similarity_threshold=0.95, largest_first=False)
    assert groups1 == groups0 and text1 == text0
    text2, groups2 = r.find_duplicate_clusters(similarity_threshold=0.95)
    rows = {m["id"]: n for n, m in enumerate(m for g in groups0 for m in g)}     # storage order of the members
    assert groups2 == sorted(groups0, key=lambda g: (-len(g), rows[g[0]["id"]]))
    assert text2.startswith(f"🎯 Found {len(groups0)} groups")
    text, groups = r.find_duplicate_clusters(similarity_threshold=1.5)
    assert groups == [] and "No near-duplicates" in text
