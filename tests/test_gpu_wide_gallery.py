"""Every search on two galleries that cross the 32-bit marks of the library's address and index arithmetic
(tests/_wide_gallery.py: W = 1024 x (2^21 + 300), L = 64 x (2^24 + 300)), against a torch fp64 reference over the very bits
that were appended.  Planted rows sit on both sides of every mark (byte 2^31 / 2^32 / 2^33 of the fp32 master and the bf16
copy, element 2^31, row 2^24): an address expression that wraps reads an unrelated bulk row, and both the returned score
and the returned set change.  What each mark is there for: DESIGN.md, testing.

Tolerances are the project's: delta = 3e-7 * max(1, D / 1024) (the fp32 chain's band), must / may bands of 2 delta around a
cut, returned scores within 1e-6 of fp64, order (score desc, index asc).

Measured on an MI355X: the fixture (append and both references) takes 0.6 s for W and 0.5 s for L; the largest bulk score the
reference found over the 300 queries is 0.1947 on W and 0.6802 on L; the pairs join on W takes 4.39 s (projected: 4.4 s, from
0.99 s at 1 M rows x 2.097^2), the slowest test of the module."""
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _discover_checks as dc  # noqa: E402
import _wide_gallery as wg  # noqa: E402
from _maxsim_checks import group_parts, ordered_sum  # noqa: E402
from _mmr_checks import greedy  # noqa: E402
from _recommend_checks import best_score  # noqa: E402
from _search_checks import _assert_indices_equal_up_to_fp32_ties  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = wg.DEV
HERE = os.path.dirname(os.path.abspath(__file__))

NQ = 300          # queries of the streamed reference: two query tiles, three range chunks on L
NV = 12           # vectors of the full score matrix (examples, pairs, a target; the filtered searches)
THRESHOLD = {"W": 0.5, "L": 0.85}      # only planted rows reach it (bulk maxima: the fixture prints what it found)


def _build(name):
    w = wg.Wide(name)
    # the handle, one chunk in both precisions, the references
    wg.need_free_gb(w.gb + 8)
    t0 = time.time()
    c = wg.Ctx()
    c.w, c.name, c.D, c.N, c.d = w, name, w.D, w.N, wg.delta(w.D)
    c.G = w.fill(engine.Gallery(w.D, w.N + 8, device=0))
    c.q = w.queries(NQ, seed=1)
    c.qn = wg.normalised(c.q)
    c.bs, c.br = wg.ref_best(c.qn, w.chunks(), keep=1100)
    c.S = wg.ref_scores(c.qn[:NV], w.chunks(), w.N)
    planted = torch.from_numpy(w.planted_rows).to(DEV)
    bulk = torch.where(torch.isin(c.br, planted), torch.full_like(c.bs, -np.inf), c.bs)
    c.bulk_max = float(bulk.max())
    torch.cuda.synchronize()
    c.seconds = time.time() - t0
    print(f"gallery {name}: {w.N} x {w.D}, fixture {c.seconds:.1f} s, largest bulk score of {NQ} queries {c.bulk_max:.4f}")
    return c


@pytest.fixture(scope="module")
def wide_w():
    c = _build("W")
    yield c
    c.G.close()


@pytest.fixture(scope="module")
def wide_l():
    c = _build("L")
    yield c
    c.G.close()


def _ctx(request, name):
    return request.getfixturevalue("wide_" + name.lower())


BOTH = pytest.mark.parametrize("name", ["W", "L"])


@pytest.fixture
def keep():
    """keep(G) registers a handle a test opens: it is closed whether the test passes or fails (a 6 - 13 GB handle left alive
    would make every later test skip itself for want of memory and hide its failure)"""
    handles = []

    def register(G):
        handles.append(G)
        return G
    yield register
    for G in handles:
        G.close()


# ---- rows ---------------------------------------------------------------------------------------------------------------
@BOTH
def test_len_and_read_at_every_site(request, name):
    c = _ctx(request, name)
    assert len(c.G) == c.N
    assert c.bulk_max < THRESHOLD[name] - 0.05, c.bulk_max
    for site in c.w.sites:
        start = min(site[0], c.N - 4)
        got = c.G.read(start, 4)
        assert torch.equal(got.view(torch.int32), c.w.rows_at(start, 4).view(torch.int32)), site


# ---- top-k --------------------------------------------------------------------------------------------------------------
def _check_queries(c, out, Q, k, what):
    s, i, cnt = out
    assert s.shape == (Q, k) and i.dtype == torch.int64
    for r in range(Q):
        wg.check_topk(s[r], i[r], cnt[r], c.bs[r], c.br[r], k, c.d, what=f"{what} query {r}")


@BOTH
@pytest.mark.parametrize("k", [10, 50])
def test_search(request, name, k):
    c = _ctx(request, name)
    ns = len(c.w.sites)
    for Q in (1, 64, 300):
        out = c.G.search(c.q[:Q], k=k)
        _check_queries(c, out, Q, k, f"{name} k={k} Q={Q}")
        s, i, _ = out
        # each site's rows come back first, in the planted order (sigma ascending = row ascending)
        for sq in range(min(ns, Q)):
            site = c.w.sites[sq]
            assert i[sq, :len(site)].tolist() == site, (name, k, Q, sq, i[sq, :6].tolist())
        if Q == 64:
            _assert_indices_equal_up_to_fp32_ties(i.cpu().numpy(), c.br[:Q, :k].cpu().numpy(), c.bs[:Q, :k].cpu().numpy(),
                                                  c.w.row, c.q[:Q].cpu().numpy())
        plan = c.G.search_plan(Q, k)
        assert plan["scan256"], plan
        if name == "L":
            assert plan["ksel"] == 64, plan                 # N >= SEARCH_WIDE_ROWS: the 64-entry candidate lists


@BOTH
@pytest.mark.parametrize("k", [200, 1024])
def test_search_large_k(request, name, k):
    c = _ctx(request, name)
    for Q in (1, 20):
        _check_queries(c, c.G.search(c.q[:Q], k=k), Q, k, f"{name} k={k} Q={Q}")


def test_search_without_the_fp32_rows_L(request, keep):
    """keep_f32=False (2.1 GB): the scan's own bf16-input scores, which the project holds to 1e-2 of fp64
    (test_k50_edges_smallest_scan256_gallery_and_no_fp32_rows): the planted rows first and in order (their scores are 0.02
    and more apart), every returned score within 1e-2 of the fp64 score of its row, no row 2e-2 below the 10th."""
    c = _ctx(request, "L")
    wg.need_free_gb(4)
    G = c.w.fill(keep(engine.Gallery(c.D, c.N, device=0, keep_f32=False)))
    Q, k = 64, 10
    s, i, cnt = G.search(c.q[:Q], k=k)
    G.close()
    assert bool((cnt == k).all())
    for sq, site in enumerate(c.w.sites):
        assert i[sq, :len(site)].tolist() == site, (sq, i[sq, :6].tolist())
    for r in range(Q):
        rows, order = torch.sort(c.br[r])
        pos = torch.searchsorted(rows, i[r]).clamp(max=rows.shape[0] - 1)
        assert bool((rows[pos] == i[r]).all()), r
        ref = c.bs[r][order][pos]
        assert float((s[r].to(torch.float64) - ref).abs().max()) <= 1e-2
        assert bool((ref >= c.bs[r, k - 1] - 2e-2).all())


# ---- range --------------------------------------------------------------------------------------------------------------
def _range_chunk(N):
    """The queries per candidate pass of revo_search_range.  RANGE_CHUNK is read from kernels.h; row_index_bits and the clamp
    to 2^(32 - b) are a MIRROR of candidate_search.hip's revo_search_range written out here, not a value the library reports (it has no
    hook for it): the assertion says which regime the gallery was chosen for, and would not notice a changed clamp.  That
    the chunked call is right is what the comparison with the reference checks."""
    src = open(os.path.join(HERE, "..", "revers-o_amd", "csrc", "kernels.h")).read()
    chunk = int(re.search(r"constexpr int RANGE_CHUNK = (\d+);", src).group(1))
    b = 1
    while N > 1 and (1 << b) < N:
        b += 1
    return min(chunk, 1 << (32 - b)), b


@BOTH
def test_search_range_planted_rows_only(request, name):
    c = _ctx(request, name)
    qc, b = _range_chunk(c.N)
    if name == "L":
        assert b == 25 and qc == 128 and qc < NQ          # the sort key's query field clamps the chunk: three chunks
    else:
        assert b == 22 and qc >= NQ
    t = THRESHOLD[name]
    off, idx, sc = c.G.search_range(c.q, t)
    n_must = wg.check_range(off, idx, sc, c.bs, c.br, t, c.d, what=name)
    planted = torch.from_numpy(c.w.planted_rows).to(DEV)
    assert bool(torch.isin(idx, planted).all()) and idx.shape[0] == n_must
    cnt = (off[1:] - off[:-1]).tolist()
    for sq, site in enumerate(c.w.sites):
        assert cnt[sq] == len(site) and idx[int(off[sq]):int(off[sq + 1])].tolist() == site, (name, sq)
    assert sum(1 for n in cnt[128:] if n > 0) > 50        # the later chunks return rows too


def test_search_range_thousands_of_bulk_hits_W(request):
    c = _ctx(request, "W")
    S = c.S[4:8]
    t = 0.0966                                            # 3.09 sigma of the bulk's N(0, 1 / 1024): about 2 000 rows a query
    off, idx, sc = c.G.search_range(c.q[4:8], t)
    wg.check_range_full(off, idx, sc, S, t, c.d, what="W bulk")
    assert 4 * 1000 < idx.shape[0] < 4 * 4000, idx.shape


# ---- pairs --------------------------------------------------------------------------------------------------------------
def test_pairs_W(request):
    """t = 0.5 on W: every pair inside a site at or above t, nothing else.  A pair of random unit rows at D = 1024 scores
    N(0, 1 / 1024); reaching 0.5 is 16 sigma, probability about exp(-128) a pair, times 2.2e12 pairs: never.  A bulk row
    against a planted one is the same.  Projected 4.4 s (0.99 s at 1 M rows x 2.097^2); measured: 4.39 s."""
    c = _ctx(request, "W")
    t = 0.5
    torch.cuda.synchronize()
    t0 = time.time()
    pairs, scores = c.G.pairs(t)
    torch.cuda.synchronize()
    print(f"pairs on W: {time.time() - t0:.2f} s (projected 4.4 s), {pairs.shape[0]} pairs")
    want = wg.planted_pairs(c.w, t, c.d)
    assert len(want) >= 2 * len(c.w.marks)
    assert pairs.cpu().tolist() == [[a, bb] for a, bb, _ in want]
    assert np.abs(scores.cpu().numpy().astype(np.float64) - np.array([s for _, _, s in want])).max() <= 1e-6


# ---- recommend, discover --------------------------------------------------------------------------------------------------
@BOTH
def test_recommend(request, name):
    """P, N = 4, 2 against the fp64 score matrix through _recommend_checks.best_score; rows on the formula's jump
    (|sp - sn| <= 2 delta) are left out, at most 0.1 % of the rows (test_gpu_recommend.py's cap); the count is printed."""
    c = _ctx(request, name)
    S = c.S[:6].cpu().numpy()
    score = best_score(S, 4)
    jump = np.abs(S[:4].max(0) - S[4:].max(0)) <= 2 * c.d
    print(f"{name}: rows on the jump: {int(jump.sum())} of {c.N}")
    assert jump.sum() <= 0.001 * c.N
    for k in (10, 1024):
        s, i, cnt = c.G.recommend(c.q[:4], c.q[4:6], k=k)
        wg.check_score_row(s, i, cnt, score, k, c.d, exclude=jump, what=f"{name} k={k}")
        assert set(i[:10].tolist()) <= set(c.w.planted_rows.tolist())      # the positives' sites come first


@BOTH
@pytest.mark.parametrize("has_target", [True, False])
def test_discover(request, name, has_target):
    """n = 4 pairs with a target, n = 3 without, against _discover_checks.score in fp64 with test_gpu_discover.py's
    tolerances (tol(v), and the excuse of rows with a pair inside 2 delta in the discovery search, capped at 0.1 % of the rows).
    The context search's first two pairs are each other's mirror image: no row is on the positive side of both, so the best
    rows are bulk rows anywhere in the gallery and not the first k rows of the eighth of it whose loss is exactly 0."""
    c = _ctx(request, name)
    n = 4 if has_target else 3
    S = c.S.cpu().numpy()
    ip, im = ([1, 2, 3, 4], [5, 6, 7, 8]) if has_target else ([1, 5, 2], [5, 1, 6])
    SP, SN = S[ip], S[im]
    score = dc.score(S[0] if has_target else None, SP, SN)
    jump = (np.abs(SP - SN) <= 2 * c.d).any(axis=0) if has_target else np.zeros(c.N, dtype=bool)
    print(f"{name}: rows with a pair inside the band: {int(jump.sum())} of {c.N}")
    assert jump.sum() <= 0.001 * c.N
    ops = 1 if has_target else n

    def tol(v):
        return ops * (2 * c.d + 3.5e-7) + ops * 2.0 ** -24 * np.abs(v) + np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)

    for k in (10, 1024):
        s, i, cnt = c.G.discover(c.q[0] if has_target else None, c.q[ip], c.q[im], k=k)
        kth = np.partition(score, c.N - k)[c.N - k]
        wg.check_score_row(s, i, cnt, score, k, float(tol(kth)) / 2, exclude=jump, tol=tol, what=f"{name} k={k}")


# ---- groups -------------------------------------------------------------------------------------------------------------
def _groups(c):
    if not hasattr(c, "groups"):
        c.groups_np = wg.group_runs(c.N, seed=7, marks=c.w.marks)
        c.groups = torch.from_numpy(c.groups_np).to(DEV)
        for m in c.w.marks:                                               # a group straddles every mark
            assert c.groups_np[m - 1] == c.groups_np[m] == c.groups_np[m + 1] >= 0
        assert int(c.groups_np.max()) == 2 ** 31 - 1
    return c.groups


def _check_maxsim(c, S, got, parts, k, n, what, allowed=None):
    """test_gpu_maxsim.test_matches_the_fp64_oracle's tolerances with must / may bands in place of a decided set: band =
    2 (n delta + n^2 2^-24) around the k-th group score; each part is the chain score of ITS row, a row of the group that
    is the fp64 best of the group or within 2 delta of it."""
    ids, M, R = parts
    s, g, cnt, ps, pr = got
    score = M[:, 0].clone()
    for j in range(1, n):
        score = score + M[:, j]
    band = 2 * (n * c.d + n * n * 2.0 ** -24)
    want = min(k, ids.shape[0])
    assert int(cnt) == want, (what, int(cnt), want)
    s, g, ps, pr = s[:want], g[:want].to(torch.int64), ps[:want], pr[:want]
    assert torch.unique(g).shape[0] == want
    at = torch.searchsorted(ids, g)
    assert bool((ids[at.clamp(max=ids.shape[0] - 1)] == g).all()), (what, "a group id that does not exist")
    kth = torch.topk(score, want).values[-1]
    must = ids[score >= kth + band]
    assert bool(torch.isin(must, g).all()), (what, "missing", must[~torch.isin(must, g)][:10].tolist())
    assert bool((score[at] >= kth - band).all()), what
    assert float((s.to(torch.float64) - score[at]).abs().max()) <= band / 2, what
    assert bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (g[:-1] < g[1:]))).all()), (what, "order")
    # the matched row of every vector
    assert bool((c.groups[pr].to(torch.int64) == g[:, None]).all()), (what, "a part row outside its group")
    if allowed is not None:
        assert bool(allowed[pr].all()), (what, "a part row the filter does not allow")
    own = S[torch.arange(n, device=DEV)[None, :], pr]
    assert float((ps.to(torch.float64) - own).abs().max()) <= c.d, what
    assert bool((own >= M[at] - 2 * c.d).all()), what


@BOTH
@pytest.mark.parametrize("n", [1, 4, 33])
def test_search_maxsim(request, name, n):
    """n query vectors, with_parts.  On L the group index sorts 16.7 M keys: the radix sort's tile leaves its 4096-key floor
    (n > SORT_MAX_BLOCKS * 4096) and its offsets scan covers all 2048 blocks."""
    c = _ctx(request, name)
    groups = _groups(c)
    if n <= NV:
        S, q = c.S[:n], c.q[:n]
    else:
        q = c.q[:n]
        S = wg.ref_scores(c.qn[:n], c.w.chunks(), c.N)
    parts = wg.group_parts_torch(S, groups)
    if name == "W" and n == 4:                           # the device statement of the reference equals the project's numpy one
        ids, M, R = group_parts(S.cpu().numpy(), c.groups_np, np.ones(c.N, dtype=bool))
        assert np.array_equal(ids, parts[0].cpu().numpy()) and np.array_equal(M, parts[1].cpu().numpy())
        assert np.array_equal(R, parts[2].cpu().numpy())
        assert np.array_equal(ordered_sum(M), ordered_sum(parts[1].cpu().numpy()))
    for k in (10, 1024):
        got = c.G.search_maxsim(q, groups, k=k, with_parts=True)
        _check_maxsim(c, S, got, parts, k, n, f"{name} n={n} k={k}")
        if k == 10 and n == 1:                           # the site of rows 0, 1: the best group's row is planted
            assert int(got[4][0, 0]) in c.w.sites[0]
    del S, parts


@BOTH
def test_search_groups(request, name):
    """limit 5 x group_size 2 for 8 queries against the fp64 matrix: the groups by their best row, each with its best rows.
    The fixture's scores around every cut are more than 2 delta apart (asserted: a property of the inputs), so groups and
    rows are compared exactly and the scores to 1e-6."""
    c = _ctx(request, name)
    groups = _groups(c)
    Q, limit, gs = 8, 5, 2
    s, i, hits, gids, ng = c.G.search_groups(c.q[:Q], groups, limit=limit, group_size=gs)
    assert bool((ng == limit).all())
    rows = torch.nonzero(groups >= 0)[:, 0]
    ids, inv = torch.unique(groups[rows].to(torch.int64), return_inverse=True)
    for r in range(Q):
        sr = c.S[r, rows]
        best = torch.full((ids.shape[0],), -np.inf, dtype=torch.float64, device=DEV).scatter_reduce(0, inv, sr, "amax")
        top = torch.topk(best, limit + 1)
        assert float((top.values[:-1] - top.values[1:]).min()) > 2 * c.d, "group scores inside the band: change the seed"
        assert gids[r].tolist() == ids[top.indices[:limit]].tolist(), (name, r)
        for j in range(limit):
            members = rows[inv == top.indices[j]]
            ms, mo = torch.sort(c.S[r, members], descending=True)
            m = min(gs, members.shape[0])
            assert int(hits[r, j]) == m
            if members.shape[0] > m:
                assert float(ms[m - 1] - ms[m]) > 2 * c.d
            if m > 1:
                assert float((ms[:m - 1] - ms[1:m]).min()) > 2 * c.d
            assert i[r, j, :m].tolist() == members[mo[:m]].tolist(), (name, r, j)
            assert float((s[r, j, :m].to(torch.float64) - ms[:m]).abs().max()) <= 1e-6
    # the straddling groups of the marks are the best groups of their sites' queries
    for sq in range(1, len(c.w.marks) + 1):
        assert int(gids[sq, 0]) == int(c.groups_np[c.w.marks[sq - 1]]) or int(gids[sq, 1]) == int(c.groups_np[c.w.marks[sq - 1]])


# ---- MMR ----------------------------------------------------------------------------------------------------------------
@BOTH
def test_search_mmr(request, name):
    """k = 10 of 100 candidates, diversity 0.5.  Greedy MMR is discontinuous (test_gpu_mmr.py): the library's picks are
    replayed in fp64 over the reference's candidates and their fp64 similarities, every pick within 2 (delta + 3 * 2^-24) of
    the fp64 maximum; where every step of the replay decides its pick by more than that, the picks are those of
    _mmr_checks.greedy over the same candidates."""
    c = _ctx(request, name)
    Q, k, C, div = 8, 10, 100, 0.5
    s, v, i, cnt = c.G.search_mmr(c.q[:Q], k=k, candidates=C, diversity=div)
    assert bool((cnt == k).all())
    bound = 2.0 * (c.d + 3.0 * 2.0 ** -24)
    cand_rows = c.br[:Q, :C]
    g = c.w.gather(cand_rows.reshape(-1)).to(torch.float64).view(Q, C, c.D)
    decided = 0
    for r in range(Q):
        assert float(c.bs[r, C - 1] - c.bs[r, C]) > 2 * c.d, "the candidate cut is inside the band: change the seed"
        cand = cand_rows[r].cpu().tolist()
        rel = c.bs[r, :C].cpu().numpy()
        sim = (g[r] @ g[r].T).cpu().numpy()
        where = {row: n for n, row in enumerate(cand)}
        picks = i[r].cpu().tolist()
        assert set(picks) <= set(cand), (name, r)
        alive = np.ones(C, dtype=bool)
        m = np.full(C, -np.inf)
        margin = np.inf
        for step, row in enumerate(picks):
            val = 0.5 * rel if step == 0 else 0.5 * rel - 0.5 * m
            p = where[row]
            assert alive[p]
            top2 = np.sort(val[alive])[-2:]
            margin = min(margin, float(top2[1] - top2[0]))
            assert float(val[alive].max() - val[p]) <= bound, (name, r, step)
            assert abs(float(v[r, step]) - float(val[p])) <= bound, (name, r, step)
            assert abs(float(s[r, step]) - float(rel[p])) <= 1e-6
            alive[p] = False
            m = np.maximum(m, sim[p])
        if margin > 2 * bound:
            gp, _ = greedy(rel, sim, k, div)
            assert [cand[p] for p in gp.tolist()] == picks, (name, r)
            decided += 1
    print(f"{name}: {decided} of {Q} queries decided every pick by more than the rounding")
    assert decided >= Q // 2


# ---- filters ------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("which", ["from the last mark on", "a random half"])
def test_filters(request, name, which):
    """top-k, range, recommend and MaxSim under an allow-bitmap, as a bool mask (checked against the fp64 matrix) and as the
    packed bitmap (the same bytes)."""
    c = _ctx(request, name)
    groups = _groups(c)
    last = c.w.marks[-1]
    if which == "a random half":
        g = torch.Generator(device=DEV).manual_seed(99)
        allow = torch.rand(c.N, generator=g, device=DEV) < 0.5
    else:
        allow = torch.arange(c.N, device=DEV) >= last
    allow_np = allow.cpu().numpy()
    # the packed bitmap is made here, not by the library: bit r & 31 of word r >> 5, little-endian inside the word
    padded = np.zeros((c.N + 31) // 32 * 32, dtype=bool)
    padded[:c.N] = allow_np
    bits = torch.from_numpy(np.packbits(padded, bitorder="little").view("<i4").copy()).to(DEV)
    assert bits.dtype == torch.int32 and bits.shape[0] == (c.N + 31) // 32
    assert torch.equal(c.G.allow_bits(allow), bits)                      # the library's own packing of the mask, every word
    Q, k = 4, 10
    S = c.S[:6].cpu().numpy()

    def same(a, b):
        for x, y in zip(a, b):
            assert torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(x.view(torch.int32), y.view(torch.int32))

    out = c.G.search(c.q[:Q], k=k, allow=allow)
    for r in range(Q):
        wg.check_score_row(out[0][r], out[1][r], out[2][r], S[r], k, c.d, allowed=allow_np, what=f"{name} {which} query {r}")
    assert bool((out[1] >= (last if which != "a random half" else 0)).all())
    same(out, c.G.search(c.q[:Q], k=k, allow=bits))
    out = c.G.search(c.q[:Q], k=200, allow=allow)
    for r in range(Q):
        wg.check_score_row(out[0][r], out[1][r], out[2][r], S[r], 200, c.d, allowed=allow_np, what=f"{name} {which} k=200 query {r}")
    # range: the planted rows the filter allows (and, from the last mark on, a threshold low enough for bulk rows of W)
    t = THRESHOLD[name] if (name == "L" or which == "a random half") else 0.05
    rg = c.G.search_range(c.q[:Q], t, allow=allow)
    n_must = wg.check_range_full(*rg, c.S[:Q], t, c.d, allow=allow, what=f"{name} {which}")
    assert n_must >= 2 and bool(allow[rg[1]].all())
    same(rg, c.G.search_range(c.q[:Q], t, allow=bits))
    score = best_score(S[:6], 4)
    jump = np.abs(S[:4].max(0) - S[4:6].max(0)) <= 2 * c.d
    rec = c.G.recommend(c.q[:4], c.q[4:6], k=k, allow=allow)
    wg.check_score_row(*rec, score, k, c.d, exclude=jump, allowed=allow_np, what=f"{name} {which} recommend")
    same(rec, c.G.recommend(c.q[:4], c.q[4:6], k=k, allow=bits))
    n = 4
    parts = wg.group_parts_torch(c.S[:n], groups, allowed=allow)
    ms = c.G.search_maxsim(c.q[:n], groups, k=k, allow=allow, with_parts=True)
    _check_maxsim(c, c.S[:n], ms, parts, k, n, f"{name} {which} maxsim", allowed=allow)
    same(ms, c.G.search_maxsim(c.q[:n], groups, k=k, allow=bits, with_parts=True))


# ---- the scan's 24-bit relative row index -----------------------------------------------------------------------------------
def test_65536_queries_scan_L_in_one_slice(request):
    """65 536 queries are 256 query tiles, one slice each (tests/test_scan_plan.py): the longest slice this gallery can have.
    Its pre-pass takes 2 048 of the 2^24 + 300 rows, so the slice stays within the 2^24 rows of the relative index and the
    call is answered: the first 300 queries are the reference's."""
    c = _ctx(request, "L")
    plan = c.G.search_plan(65_536, 10)
    assert plan["slices"] == 1 and (1 << 24) - 4096 < c.N - plan["prepass_rows"] <= 1 << 24, plan
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.cat([c.q, torch.randn(65_536 - NQ, c.D, generator=g, device=DEV)])
    s, i, cnt = c.G.search(q, k=10)
    assert bool((cnt == 10).all()) and bool(((i >= 0) & (i < c.N)).all())
    _check_queries(c, (s[:NQ], i[:NQ], cnt[:NQ]), NQ, 10, "L, 65 536 queries")


def test_a_call_whose_slice_would_pass_2_24_rows_is_refused(keep):
    """2^24 + 4 096 rows (bf16 only, 2.1 GB; no reference needed): behind the 2 048-row pre-pass of 65 536 queries more than
    2^24 rows are left for the one slice.  The call is refused with the launch's message, not answered wrongly, and the
    handle answers a smaller call afterwards."""
    from reverso_amd import _lib
    D, N = 64, (1 << 24) + 4096
    wg.need_free_gb(4)
    g = torch.Generator(device=DEV).manual_seed(4)
    G = keep(engine.Gallery(D, N, device=0, keep_f32=False))
    for s0 in range(0, N, 1 << 21):
        G.add(torch.randn(min(1 << 21, N - s0), D, generator=g, device=DEV))
    q = torch.randn(65_536, D, generator=g, device=DEV)
    with pytest.raises(_lib.RevoError, match=r"a gallery slice holds at most 2\^24 rows"):
        G.search(q, k=10)
    torch.cuda.synchronize()
    s, i, cnt = G.search(q[:4], k=10)
    assert bool((cnt == 10).all()) and bool(((i >= 0) & (i < N)).all()) and bool((s[:, :-1] >= s[:, 1:]).all())
    G.close()
