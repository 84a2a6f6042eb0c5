"""Multi-vector search (revo_search_maxsim, include/revo.h MAXSIM; Gallery.search_maxsim, GalleryStore.search_multivector,
SimpleReverso.search_similar_all_regions): bit for bit against a composition of the range search (every query vector's score
of every row, the one fp32 chain) with the contract's formulas in numpy, the identities of the contract, planted groups that
only the widening of the bounds keeps, an fp64 oracle of the fp32 rows, filters, thresholds, ties, errors and lifecycle, the
level, the store and the facade."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _maxsim_checks import exhaustive, group_parts, ordered_sum  # noqa: E402
from test_gpu_recommend import _bf16, _chain_scores, _delta, _examples, _gallery, _normalised, _planted  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KS = (1, 10, 50, 51, 1024)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _layouts(R, seed, names=None):
    """the group layouts of the composition test, as int32 [R]"""
    rng = np.random.default_rng(seed)
    out = {}
    out["own"] = np.arange(R)
    runs = np.repeat(np.arange(R), rng.integers(1, 8, R))[:R]                    # contiguous runs of 1 - 7 rows
    out["runs"] = runs
    out["random"] = rng.integers(0, max(1, R // 3), R)                           # groups span tiles and slices
    ids = np.unique(np.r_[rng.integers(0, 2 ** 31 - 1, max(1, R // 3)), 2 ** 31 - 1, 0])
    out["sparse"] = ids[rng.integers(0, ids.shape[0], R)]                        # sparse ids up to 2^31 - 1
    if R > 2:
        out["sparse"][R // 2] = 2 ** 31 - 1
    minus = rng.integers(0, max(1, R // 3), R)
    minus[rng.random(R) < 0.1] = -1                                              # a tenth of the rows in no group
    out["minus"] = minus
    out["one"] = np.full(R, 12345)                                               # ONE group holding every row
    out["big"] = rng.integers(0, max(1, R // 150), R)                            # groups of more than 64 rows
    names = names or list(out)
    return {k: out[k].astype(np.int32) for k in names}


def _assert_equals(got, want, what=""):
    s, g, c, ps, pr = (t.cpu().numpy() for t in got)
    ws, wg, wc, wps, wpr = want
    assert int(c) == wc, (what, int(c), wc)
    assert np.array_equal(g, wg), (what, np.nonzero(g != wg)[0][:10], g[:12], wg[:12])
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (what, np.nonzero(s != ws)[0][:10])
    assert np.array_equal(pr, wpr), (what, np.argwhere(pr != wpr)[:10])
    assert np.array_equal(ps.view(np.uint32), wps.view(np.uint32)), (what, np.argwhere(ps != wps)[:10])


def _check(G, q, groups, S, ks=KS, allow=None, threshold=None, index_offset=0, what=""):
    """check 1: the call against the formulas over the range search's scores S [n, rows]; no tolerance"""
    allowed = np.ones(len(G), dtype=bool) if allow is None else allow.cpu().numpy()
    parts = group_parts(S, groups, allowed)
    gt = _t(groups)
    for k in ks:
        got = G.search_maxsim(q, gt, k=k, score_threshold=threshold, index_offset=index_offset, allow=allow, with_parts=True)
        _assert_equals(got, exhaustive(S, groups, allowed, k, threshold, index_offset, parts=parts), f"{what} k={k}")
    return parts


def _stats_are_the_maxsim_search(G, passes=1):
    st = G.search_stats()
    assert st["join_passes"] == passes, st
    assert st["uncertified"] == st["bruteforced"] == st["checked"] == st["from_segments"] == 0, st
    assert st["grouped_fallback"] == st["large_k_fallback"] == 0, st
    return st["collected_rows"]


# ---- 1. bit for bit against the composition --------------------------------------------------------------------------------
_NV = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64)


@pytest.mark.parametrize("n,D", [(n, [1024, 64, 768, 1280][i % 4]) for i, n in enumerate(_NV)])
def test_equals_the_composition_bit_for_bit(n, D):
    R = 20_037
    x = _planted(R, D, seed=R + D + n)
    G = _gallery(x)
    q = _examples(x, n, seed=n * 131)
    S = _chain_scores(G, q)
    for name, groups in _layouts(R, seed=n).items():
        parts = _check(G, q, groups, S, what=name)
        rows = _stats_are_the_maxsim_search(G)
        assert rows <= int((groups >= 0).sum())
        assert parts[0].shape[0] == np.unique(groups[groups >= 0]).shape[0]
    # two calls: identical bytes
    gt = _t(_layouts(R, seed=n, names=["random"])["random"])
    a = G.search_maxsim(q, gt, k=51, with_parts=True)
    b = G.search_maxsim(q, gt, k=51, with_parts=True)
    assert all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(a, b))
    # the part outputs are optional
    c = G.search_maxsim(q, gt, k=51)
    assert len(c) == 3 and torch.equal(c[0].view(torch.int32), a[0].view(torch.int32)) and torch.equal(c[1], a[1])
    G.close()


@pytest.mark.parametrize("n", [3, 64])
@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_small_galleries(n, R):
    D = 1024
    x = _planted(R, D, seed=R + n)
    G = _gallery(x)
    q = _examples(x, n, seed=n + R)
    S = _chain_scores(G, q)
    for name, groups in _layouts(R, seed=R, names=["own", "runs", "random", "sparse", "minus", "one"]).items():
        _check(G, q, groups, S, what=name)
    G.close()


# ---- 2. the identities of the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 1024])
def test_singleton_groups_are_the_large_k_search(D):
    R = 20_037
    x = _planted(R, D, seed=5 + D)
    G = _gallery(x)
    q = _examples(x, 1, seed=6)
    own = torch.arange(R, dtype=torch.int32, device=DEV)
    for k in (51, 1024):
        s, g, c, ps, pr = G.search_maxsim(q, own, k=k, with_parts=True)
        s1, i1, c1 = G.search(q, k=k)                                            # revo_search_topk_large
        assert int(c) == int(c1[0]) == k
        assert torch.equal(g.to(torch.int64), i1[0]) and torch.equal(s.view(torch.int32), s1[0].view(torch.int32))
        assert torch.equal(pr[:, 0], i1[0]) and torch.equal(ps[:, 0].view(torch.int32), s1[0].view(torch.int32))
    G.close()


def test_one_vector_gives_the_group_keys_of_the_grouped_search():
    R, D = 20_037, 768
    x = _planted(R, D, seed=15)
    G = _gallery(x)
    q = _examples(x, 1, seed=16)
    for name, groups in _layouts(R, seed=17, names=["runs", "random", "sparse", "minus"]).items():
        gt = _t(groups)
        for k in (1, 10, 50):
            s, g, c = G.search_maxsim(q, gt, k=k)
            gs, gi, hc, gid, gc = G.search_groups(q, gt, limit=k, group_size=1)
            assert int(c) == int(gc[0]) == k and torch.equal(g, gid[0]), (name, k)
            assert torch.equal(s.view(torch.int32), gs[0, :, 0].view(torch.int32))
    G.close()


def test_the_same_vector_twice_doubles_the_scores():
    R, D = 20_037, 1024
    x = _planted(R, D, seed=25)
    G = _gallery(x)
    q = _examples(x, 1, seed=26)
    gt = _t(_layouts(R, seed=27, names=["random"])["random"])
    s1, g1, c1 = G.search_maxsim(q, gt, k=1024)
    s2, g2, c2, ps, pr = G.search_maxsim(torch.cat([q, q]), gt, k=1024, with_parts=True)
    assert int(c1) == int(c2) == 1024 and torch.equal(g1, g2)
    m = s1.cpu().numpy()
    assert np.array_equal((m + m).astype(np.float32).view(np.uint32), s2.cpu().numpy().view(np.uint32))
    assert torch.equal(ps[:, 0], ps[:, 1]) and torch.equal(pr[:, 0], pr[:, 1])
    G.close()


# ---- 3. groups that only the widening keeps ----------------------------------------------------------------------------
def test_groups_below_the_level_in_bf16():
    """Two query vectors p0, p1; 1 500 planted groups of two rows, one near each vector, whose fp32 scores lie within about
    1e-4 of each other; k = 700 cuts through them.  By the bf16 scan scores alone (emulated: bf16-rounded rows and vectors,
    summed in fp64) the best 700 groups are not the fp32 best 700: without the widening by the rounding bounds the level
    would drop groups of the answer."""
    R, D, M, k = 20_037, 1024, 1500, 700
    rng = np.random.default_rng(43)
    x = _planted(R, D, seed=43)
    p = rng.standard_normal((2, D))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    where = rng.permutation(R)[:2 * M].reshape(M, 2)
    for j in range(2):
        u = rng.standard_normal((M, D))
        u -= (u @ p[j])[:, None] * p[j][None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        sc = 0.8 + 0.5e-4 * rng.standard_normal(M)
        x[where[:, j]] = (sc[:, None] * p[j][None, :] + np.sqrt(1.0 - sc * sc)[:, None] * u).astype(np.float32)
    groups = np.full(R, -1, dtype=np.int32)
    rest = np.setdiff1d(np.arange(R), where.reshape(-1))
    groups[rest] = 5000 + (np.arange(rest.shape[0]) // 3)
    groups[where[:, 0]] = np.arange(M)
    groups[where[:, 1]] = np.arange(M)
    G = _gallery(x)
    q = _t(p.astype(np.float32))
    rows, qn = G.read(), _normalised(q)
    S64 = (qn.to(torch.float64) @ rows.to(torch.float64).T).cpu().numpy()
    Sb = (_bf16(qn) @ _bf16(rows).T).cpu().numpy()
    allowed = np.ones(R, dtype=bool)
    ids64, M64, _ = group_parts(S64, groups, allowed)
    idsb, Mb, _ = group_parts(Sb, groups, allowed)
    assert np.array_equal(ids64, idsb)
    top64 = set(ids64[np.argsort(-ordered_sum(M64), kind="stable")[:k]].tolist())
    topb = set(idsb[np.argsort(-ordered_sum(Mb), kind="stable")[:k]].tolist())
    assert top64 <= set(range(M)) and len(top64 - topb) >= 10, "the construction lost its teeth"
    _check(G, q, groups, _chain_scores(G, q), ks=(k,))
    G.close()


# ---- 4. the fp64 oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,seed", [(1, 1024, 1), (4, 64, 2), (5, 768, 3), (33, 1280, 39), (64, 1024, 20)])
def test_matches_the_fp64_oracle(n, D, seed):
    """Independent of the library's chain: fp64 scores of the fp32 rows read back, the formulas in fp64.  The call's order is
    the oracle's up to swaps of adjacent places whose fp64 scores differ by at most the band: the chain's band per term
    plus the rounding of the fp32 sum of n terms of magnitude at most 1."""
    R = 20_037
    x = _planted(R, D, seed=100 + seed)
    G = _gallery(x)
    q = _examples(x, n, seed=200 + seed)
    groups = _layouts(R, seed=300 + seed, names=["random"])["random"]
    S64 = (_normalised(q).to(torch.float64) @ G.read().to(torch.float64).T).cpu().numpy()
    ids, M64, R64 = group_parts(S64, groups, np.ones(R, dtype=bool))
    score = ordered_sum(M64)
    order = np.lexsort((ids, -score))
    band = 2 * (n * _delta(D) + n * n * 2.0 ** -24)
    gt = _t(groups)
    for k in KS:
        # a property of the inputs: the k-th and the (k + 1)-th group are apart, so the SET of the answer is decided
        assert score[order[k - 1]] - score[order[k]] > band, (k, score[order[k - 1]] - score[order[k]], band)
        s, g, c, ps, pr = (t.cpu().numpy() for t in G.search_maxsim(q, gt, k=k, with_parts=True))
        want = ids[order[:k]]
        assert int(c) == k and set(g.tolist()) == set(want.tolist())
        place = {int(v): j for j, v in enumerate(want)}
        sc_of = dict(zip(ids.tolist(), score.tolist()))
        for j, v in enumerate(g.tolist()):
            if v != want[j]:
                assert abs(place[v] - j) == 1 and abs(sc_of[v] - sc_of[int(want[j])]) <= band, (k, j, v, want[j])
        assert np.abs(s.astype(np.float64) - np.array([sc_of[v] for v in g.tolist()])).max() <= band / 2
        # a part: the chain score of ITS row, and that row is the fp64 best of the group or within the band of it
        own = S64[np.arange(n)[None, :], pr]
        assert np.abs(ps.astype(np.float64) - own).max() <= _delta(D)
        assert (own >= M64[np.searchsorted(ids, g)] - 2 * _delta(D)).all()
    G.close()


# ---- 5. filters, threshold, offsets and ties ---------------------------------------------------------------------------
def test_filters():
    R, D, n = 20_037, 768, 6
    x = _planted(R, D, seed=51)
    G = _gallery(x)
    q = _examples(x, n, seed=52)
    S = _chain_scores(G, q)
    rng = np.random.default_rng(53)
    groups = _layouts(R, seed=54, names=["runs"])["runs"]
    half = rng.random(R) < 0.5
    heads = np.r_[True, groups[1:] != groups[:-1]]                               # exactly one row per group
    empties = np.isin(groups, rng.permutation(int(groups.max()) + 1)[:2000], invert=True)   # every row of 2 000 groups is out
    for name, mask in (("everything", np.ones(R, dtype=bool)), ("half", half), ("one per group", heads), ("empties", empties)):
        allow = _t(mask)
        parts = _check(G, q, groups, S, allow=allow, what=name)
        assert _stats_are_the_maxsim_search(G) <= int(mask.sum())
        if name == "empties":
            assert parts[0].shape[0] == int(groups.max()) + 1 - 2000
    none = torch.zeros(R, dtype=torch.bool, device=DEV)
    s, g, c, ps, pr = G.search_maxsim(q, _t(groups), k=10, allow=none, with_parts=True)
    assert int(c) == 0 and bool((g == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    assert bool((pr == -1).all()) and bool(torch.isinf(ps).all())
    assert _stats_are_the_maxsim_search(G, passes=0) == 0
    _check(G, q, groups, S, ks=(10,))                                            # the filter is gone afterwards
    G.close()


def test_thresholds_and_index_offset():
    R, D, n = 20_037, 1024, 4
    x = _planted(R, D, seed=61)
    G = _gallery(x)
    q = _examples(x, n, seed=62)
    S = _chain_scores(G, q)
    groups = _layouts(R, seed=63, names=["random"])["random"]
    ids, M, _ = _check(G, q, groups, S, ks=(10,))
    score = np.sort(ordered_sum(M))
    for t in (float(score[-30]), float(score[-6]), float(score[40]), 0.0, -4.0):     # in the middle of the result, below it
        _check(G, q, groups, S, ks=(10, 1024), threshold=t)
    s, g, c = G.search_maxsim(q, _t(groups), k=10, score_threshold=float(n) + 0.5)   # above everything
    assert int(c) == 0 and bool((g == -1).all())
    assert _stats_are_the_maxsim_search(G) == 0
    _check(G, q, groups, S, ks=(10, 51), index_offset=1_000_000_007)
    _check(G, q, groups, S, ks=(10,), index_offset=5, threshold=float(score[-6]))
    G.close()


def test_ties_between_groups_and_inside_a_group():
    R, D, n = 20_037, 1024, 3
    rng = np.random.default_rng(171)
    x = _planted(R, D, seed=71)
    # duplicated groups: groups 100 .. 1099 hold the same three vectors each; they tie and the lower id comes first
    trio = rng.standard_normal((3, D)).astype(np.float32)
    groups = np.full(R, -1, dtype=np.int32)
    groups[:3000] = 100 + (np.arange(3000) % 1000)                               # rows j, j + 1000, j + 2000 -> group 100 + j
    x[:3000] = np.repeat(trio, 1000, axis=0)
    # duplicated rows inside a group: group 7 holds 40 copies of one vector among other rows; the lowest row is reported
    v = rng.standard_normal(D).astype(np.float32)
    x[5000:5040] = v
    groups[4990:5060] = 7
    groups[6000:] = 2000 + (np.arange(R - 6000) // 4)
    G = _gallery(x)
    q = _t(np.stack([trio[0], trio[2], v]))
    S = _chain_scores(G, q)
    _check(G, q, groups, S, ks=(1, 50, 500, 1024))
    s, g, c, ps, pr = G.search_maxsim(q[:2], _t(groups), k=1000, with_parts=True)
    assert np.array_equal(g.cpu().numpy(), np.arange(100, 1100))                 # the tie: group ids ascending
    assert np.array_equal(pr.cpu().numpy(), np.stack([np.arange(1000), 2000 + np.arange(1000)], 1))
    s, g, c, ps, pr = G.search_maxsim(q[2:], _t(groups), k=1, with_parts=True)
    assert int(g[0]) == 7 and int(pr[0, 0]) == 5000
    G.close()


# ---- 6. errors and lifecycle ---------------------------------------------------------------------------------------------
def test_errors_lifecycle_and_results_that_survive():
    import ctypes as C
    from reverso_amd import _lib
    D, R = 1024, 20_037
    x = _planted(R, D, seed=81)
    q = _examples(x, 4, seed=82)
    G0 = _gallery(x[:300], keep_f32=False)
    with pytest.raises(RuntimeError, match="keep_f32"):
        G0.search_maxsim(q, torch.arange(300, dtype=torch.int32, device=DEV), k=5)
    G0.close()
    E = engine.Gallery(D, 16, device=0)
    s, g, c, ps, pr = E.search_maxsim(q, torch.zeros(0, dtype=torch.int32, device=DEV), k=7, with_parts=True)
    assert int(c) == 0 and bool((g == -1).all()) and bool(torch.isinf(s).all()) and bool((pr == -1).all())
    assert _stats_are_the_maxsim_search(E, passes=0) == 0
    E.close()

    G = engine.Gallery(D, R, device=0)
    G.add(_t(x[:15_000]))
    lay = _layouts(R, seed=83, names=["random", "runs"])

    def raw(k=5):
        s = torch.full((k,), 7.0, device=DEV)
        g = torch.full((k,), 7, dtype=torch.int32, device=DEV)
        c = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        with torch.cuda.device(0):
            rc = G._lib.revo_search_maxsim(G._h, _lib.ptr(q), 4, k, 0, 0.0, 0, _lib.ptr(s), _lib.ptr(g), _lib.ptr(c), None, None,
                                           _lib.current_stream())
        return rc, G._lib.revo_last_error(), s, g, c

    rc, err, *_ = raw()
    assert rc == -2 and b"no group ids" in err                                  # none set
    gids = _t(lay["random"][:15_000])
    _lib.check(G._lib.revo_search_set_groups(G._h, _lib.ptr(gids), 15_000, 1, _lib.current_stream()))
    rc, err, s, g, c = raw()
    assert rc == 0 and int(c) == 5
    first = (s.clone(), g.clone())
    pairs, psc = G.pairs(0.93)
    off, ridx, rsc = G.search_range(q[:2], 0.5)
    # a filter set for another size
    bits = torch.full(((15_000 + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), 15_000, 1, _lib.current_stream()) == 0
    G.add(_t(x[15_000:]))
    rc, err, s, g, c = raw()
    assert rc == -2 and b"set them again" in err and int(c) == 7 and float(s[0]) == 7.0      # ids for another size, outputs untouched
    G._lib.revo_search_set_groups(G._h, _lib.ptr(_t(lay["random"])), R, 1, _lib.current_stream())
    rc, err, *_ = raw()
    assert rc == -2 and b"filter was set for" in err
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    G._lib.revo_search_set_groups(G._h, None, 0, 0, None)
    # correct after re-setting; then other group ids on the same handle: the index is rebuilt
    S = _chain_scores(G, q)
    for name in ("random", "runs", "random"):
        _check(G, q, lay[name], S, ks=(10, 1024), what=name)
    with pytest.raises(RuntimeError, match=r"\[1, 64\]"):
        G.search_maxsim(_examples(x, 65, 1), _t(lay["runs"]), k=5)
    with pytest.raises(RuntimeError, match="1024"):
        G.search_maxsim(q, _t(lay["runs"]), k=1025)
    # the pairs and the range result of the handle were invalidated by the append, not by this search: take new ones
    pairs, psc = G.pairs(0.93)
    off, ridx, rsc = G.search_range(q[:2], 0.5)
    G.search_maxsim(q, _t(lay["runs"]), k=1024)
    p2, ps2 = torch.empty_like(pairs), torch.empty_like(psc)
    _lib.check(G._lib.revo_gallery_pairs_read(G._h, 0, pairs.shape[0], _lib.ptr(p2), _lib.ptr(ps2), 1))
    assert torch.equal(p2, pairs) and torch.equal(ps2, psc)
    off2, i2, s2 = torch.empty_like(off), torch.empty_like(ridx), torch.empty_like(rsc)
    _lib.check(G._lib.revo_search_range_read(G._h, _lib.ptr(off2), 0, ridx.shape[0], _lib.ptr(i2), _lib.ptr(s2), 1))
    assert torch.equal(off2, off) and torch.equal(i2, ridx) and torch.equal(s2, rsc)
    assert first[0].shape[0] == 5 and C.sizeof(C.c_void_p) == 8
    G.close()


# ---- 7. the level does its work ----------------------------------------------------------------------------------------
def _cert_eps(e_q, n_qb, Gm, Eg, D):
    """kernels.h cert_eps, restated in float64 (a little above the fp32 value the kernel uses or equal to it)"""
    gam1, gam2 = D * 2.0 ** -23, D * 2.0 ** -24
    return (e_q * Gm + n_qb * Eg + gam1 * n_qb * (Gm + Eg) + gam2 * (n_qb + e_q) * Gm) * 1.001 + 1e-30


def test_the_level_keeps_the_candidates_few():
    R, D, n, k = 20_037, 1024, 4, 10
    rng = np.random.default_rng(91)
    x = _planted(R, D, seed=91)
    groups = (np.arange(R) // 3).astype(np.int32)
    # the queries: perturbed copies of the rows of a few planted groups, so that the best groups are clearly apart
    for gsel in range(40):
        base = 3 * (100 + 97 * gsel)
        x[base:base + 3] = x[[900, 901, 902]] + 0.02 * (gsel + 1) * rng.standard_normal((3, D)).astype(np.float32) / np.sqrt(D) * np.linalg.norm(x[900])
    qv = x[[900, 901, 902, 900]] / np.linalg.norm(x[[900, 901, 902, 900]], axis=1, keepdims=True)
    G = _gallery(x)
    q = _t(qv.astype(np.float32))
    rows, qn = G.read(), _normalised(q)
    rb, qb = _bf16(rows), _bf16(qn)
    Sb = (qb @ rb.T).cpu().numpy()
    r64, q64 = rows.to(torch.float64), qn.to(torch.float64)
    Gm, Eg = float(r64.norm(dim=1).max()), float((rb - r64).norm(dim=1).max())
    e = np.array([_cert_eps(float((qb[i] - q64[i]).norm()), float(qb[i].norm()), Gm, Eg, D) for i in range(n)])
    ids, Mb, _ = group_parts(Sb, groups, np.ones(R, dtype=bool))
    a, A1, E = Mb.sum(1), np.abs(Mb).sum(1), e.sum()
    T = E * 1.001 + n * 2.4e-7 * (A1 + E) + 1e-30
    lb, ub = a - T - 4e-7 * (1 + np.abs(a) + T), a + T + 4e-7 * (1 + np.abs(a) + T)
    tau = np.sort(lb)[::-1][k - 1]
    # 2e-6: the emulation sums in fp64, the MFMA accumulates in fp32
    cand_rows = 3 * int((ub >= tau - 2e-6).sum())
    assert cand_rows < R // 4, cand_rows                                         # a property of the inputs
    _check(G, q, groups, _chain_scores(G, q), ks=(k,))
    got = _stats_are_the_maxsim_search(G)
    assert 3 * k <= got < R // 4, got
    G.close()


# ---- 8. store and facade -----------------------------------------------------------------------------------------------
def test_store_search_multivector():
    from reverso_amd import filters, store
    N, D = 5000, 256
    x = _planted(N, D, seed=95, n_clusters=N // 10)
    payloads = [{"image_source": f"img{r // 4}.jpg", "filename": f"img{r // 4}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1]} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    q = _examples(x, 3, seed=96)
    groups, values = st._group_ids("image_source")
    res = st.search_multivector(q.cpu().numpy(), "image_source", limit=12)
    s, g, c, ps, pr = st.gallery.search_maxsim(q, groups, k=12, with_parts=True)
    assert int(c) == 12 and len(res) == 12 and all(isinstance(r, store.MultiVectorResult) for r in res)
    assert [(r.value, r.score) for r in res] == [(values[j], sc) for j, sc in zip(g.tolist(), s.tolist())]
    for r, rows, scs in zip(res, pr.tolist(), ps.tolist()):
        assert [(h.id, h.score) for h in r.hits] == [(f"p{j}", sc) for j, sc in zip(rows, scs)]
        assert all(h.payload is st.payloads[int(h.id[1:])] and h.payload["image_source"] == r.value for h in r.hits)
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    fr = st.search_multivector(q, "image_source", limit=12, query_filter=flt, score_threshold=0.2)
    allow = torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    s, g, c, ps, pr = st.gallery.search_maxsim(q, groups, k=12, allow=allow, score_threshold=0.2, with_parts=True)
    assert [(r.value, r.score) for r in fr] == [(values[j], sc) for j, sc in zip(g.tolist()[:int(c)], s.tolist()[:int(c)])]
    assert len(fr) >= 1 and all(int(h.id[1:]) % 2 == 1 for r in fr for h in r.hits)
    with pytest.raises(ValueError, match="at least one"):
        st.search_multivector(np.zeros((0, D), dtype=np.float32), "image_source")


def test_search_similar_all_regions_on_a_region_database(tmp_path, dev):
    from reverso_amd.core_system import Regions, SimpleReverso
    from test_gpu_facade import _make_jpegs
    folder = str(tmp_path / "images")
    paths = _make_jpegs(folder, n=6, seed=4)

    def detector(pil, prompt):
        w, h = pil.size
        masks = np.zeros((3, h, w), dtype=bool)
        masks[0, 10:h // 2, 5:w // 2] = True
        masks[1, h // 3:h - 7, w // 4:w - 3] = True
        masks[2, 3:h // 3, w // 2:w - 9] = True
        return Regions([[5, 10, w // 2, h // 2], [w // 4, h // 3, w - 3, h - 7], [w // 2, 3, w - 9, h // 3]], mask=masks,
                       confidence=[0.9, 0.8, 0.7], class_id=[0, 1, 2], class_names=["person", "car", "building"])

    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8, detector=detector,
                      region_mode="crop")
    text, items = r.search_similar_all_regions()
    assert text == "❌ No query embeddings available. Please detect/process an image first." and items == []
    assert r.detect_regions(paths[2], "person . car . building") == 3
    embs, metas = r.extract_embeddings(paths[2])
    assert len(embs) == 3
    text, items = r.search_similar_all_regions()
    assert text == "❌ No database loaded. Please create or load a database first." and items == []
    assert "✅" in r.create_database(folder, "regions", text_prompt="person . car . building")
    assert len(r.vector_db.payloads) == 18
    r.detect_regions(paths[2], "person . car . building")
    embs, metas = r.extract_embeddings(paths[2])
    text, items = r.search_similar_all_regions(max_results=4)
    assert text.startswith("🎯 Found 4 images matching all 3 query regions") and len(items) == 4
    # the image whose regions were the query comes first, each query region matched by its own box
    assert os.path.basename(items[0]["image"]) == os.path.basename(paths[2]) and items[0]["score"] > 2.999
    assert all(reg["filename"] == os.path.basename(paths[2]) for reg in items[0]["regions"])
    assert [reg["bbox"] for reg in items[0]["regions"]] == [m["bbox"] for m in metas]
    assert all(len(it["regions"]) == 3 and set(it["regions"][0]) == {"bbox", "score", "id", "filename"} for it in items)
    assert all(abs(sum(reg["score"] for reg in it["regions"]) - it["score"]) < 1e-5 for it in items)
    assert len({it["image"] for it in items}) == 4
    want = r.vector_db.search_multivector(torch.stack(list(embs)), "image_source", limit=4)
    assert [(it["image"], it["score"]) for it in items] == [(w.value, w.score) for w in want]
    text, items = r.search_similar_all_regions(similarity_threshold=3.5)
    assert items == [] and "No images found" in text and "3.5" in text


def test_index_offset_at_and_above_2_31():
    from _search_checks import _assert_offset_moves_the_indices_only
    R = 20_037
    x = _planted(R, 1024, seed=61)
    G = _gallery(x)
    q = _examples(x, 4, seed=62)
    gt = _t(_layouts(R, seed=63, names=["random"])["random"])
    for k in (10, 51):
        _assert_offset_moves_the_indices_only(
            lambda off: G.search_maxsim(q, gt, k=k, index_offset=off, with_parts=True), {4})
    G.close()
