"""Every form of the filtered search kernels (revo_search_set_filter / Gallery.search(allow=...)) against three references:
(a) the fp64 CPU oracle over the allowed rows, (b) bit-for-bit equality with the unfiltered search of a gallery holding
only the allowed rows (indices mapped back), (c) bit-for-bit equality with an experiment-library twin forced through the
filtered brute force.  Masks mix every kind of 64-bit word (all, none, random, only bit 0, only bit 63, only bits 31 and 32)
so that the early return of s256_apply_allow, both halves of each word and every lane's shift are exercised.

The scan form a case runs is named <KSEL, ROWS, MARGIN> after the template parameters of topk_scan256_kernel<KSEL, ROWS,
MARGIN, FILTER = true> (topk256.hip): KSEL 32 for k <= 16 else 64; ROWS 64 / 128 / 192 for at most that many queries (192 only without the
margin), 0 beyond; MARGIN for k > 25 with at most 128 queries (a filtered scan of more queries runs without it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine
from oracle import search as osearch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _search_checks import _check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SCAN_STATS = 1 << 14                                          # revo_op_set_gemm_debug: count scan events


# ---- masks ------------------------------------------------------------------------------------------------------------
def _mixed_mask(N, seed):
    """Each 64-row block is one of: all allowed, none, random 50 %, only bit 0, only bit 63, only bits 31 and 32 (every
    kind present at least once)."""
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


def _random_mask(N, frac, seed):
    return np.random.default_rng(seed).random(N) < frac


# ---- data -------------------------------------------------------------------------------------------------------------
def _rows(N, D, seed):
    return np.random.default_rng(seed).standard_normal((N, D), dtype=np.float32)


def _queries(gal, Q, seed):
    """Q queries: half near gallery rows (high-scoring hits), half random directions."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((Q, gal.shape[1]), dtype=np.float32)
    near = rng.integers(0, gal.shape[0], Q // 2)
    q[: Q // 2] = gal[near] * 4 + q[: Q // 2] * 0.5
    return q


def _gallery(gal, capacity=None, keep_f32=True, experiments=False):
    G = engine.Gallery(gal.shape[1], capacity or gal.shape[0], device=0, keep_f32=keep_f32, experiments=experiments)
    G.add(torch.from_numpy(gal).to(DEV))
    return G


def _twin(G):
    """A librevo_exp.so handle holding G's fp32 rows bit for bit, forced through the (filtered) brute force."""
    Gx = engine.Gallery(G.dim, len(G), device=0, experiments=True)
    Gx.add(G.read(0, len(G)), normalize=False)
    Gx.set_search_mode("bruteforce")
    return Gx


def _sub(G, m):
    """A gallery of the allowed rows only (G's stored fp32 rows, added as they are: identical fp32 and bf16 rows)."""
    allowed = np.flatnonzero(m)
    S = engine.Gallery(G.dim, max(allowed.size, 1), device=0)
    if allowed.size:
        S.add(G.read(0, len(G))[torch.from_numpy(allowed).to(DEV)], normalize=False)
    return S, allowed


def _mapped(out, allowed, index_offset=0):
    s, i, c = (t.cpu() for t in out)
    assert int(i.max()) < allowed.size
    a = torch.from_numpy(allowed)
    return s, torch.where(i >= 0, a[i.clamp(min=0)] + index_offset, i), c


def _eq(got, want, what):
    for name, x, y in zip("sic", got, want):
        assert torch.equal(x.cpu(), y.cpu()), (what, name)


class _Case:
    """One gallery, its brute-force twin and (per mask) its sub-gallery; ``check`` runs one filtered search against the
    three references."""

    def __init__(self, gal, capacity=None):
        self.gal = gal
        self.G = _gallery(gal, capacity)
        self.Gx = _twin(self.G)
        self._subs = {}

    def sub(self, name, m):
        if name not in self._subs:
            for S, _ in self._subs.values():
                S.close()
            self._subs = {name: _sub(self.G, m)}
        return self._subs[name]

    def check(self, qr, k, thr, name, m, index_offset=0):
        q = torch.from_numpy(qr).to(DEV)
        md = torch.from_numpy(m).to(DEV)
        got = self.G.search(q, k, thr, index_offset=index_offset, allow=md)
        # (a) the fp64 oracle over the allowed rows
        rs, ri, rc = osearch.search(self.gal, qr, k, thr, allow=m)
        ri = np.where(ri >= 0, ri + index_offset, ri)
        _check(got, (rs, ri, rc), atol=1e-5, near_tie=3e-7)
        # (b) the unfiltered search of the sub-gallery, indices mapped back
        S, allowed = self.sub(name, m)
        if allowed.size:
            _eq(got, _mapped(S.search(q, k, thr), allowed, index_offset), (name, k, thr, "sub-gallery"))
        else:
            assert (got[2] == 0).all() and (got[1] == -1).all()
        # (c) the brute-force twin under the same filter
        _eq(got, self.Gx.search(q, k, thr, index_offset=index_offset, allow=md), (name, k, thr, "brute force"))
        i = got[1].cpu().numpy()
        assert m[i[i >= 0] - index_offset].all()
        return got

    def close(self):
        for S, _ in self._subs.values():
            S.close()
        self.G.close()
        self.Gx.close()


def _ksel(k):
    return 32 if k <= 16 else 64


# ---- 1. every <KSEL, ROWS, MARGIN> form of the filtered 256 x 256 scan ----------------------------------------------------
MATRIX = [
    (1, 1),       # <32, 64>
    (64, 10),     # <32, 64>
    (64, 20),     # <64, 64>
    (64, 50),     # <64, 64, M>
    (100, 10),    # <32, 128>
    (100, 20),    # <64, 128>
    (100, 50),    # <64, 128, M>
    (129, 16),    # <32, 192>
    (129, 17),    # <64, 192>
    (160, 10),    # <32, 192>
    (160, 20),    # <64, 192>
    (160, 50),    # <64, 192>  (filtered, more than 128 queries: no margin; uncertified queries go to the collect pass)
    (192, 26),    # <64, 192>  (the same, at the form's last query)
    (193, 26),    # <64, 0>    (one query past it: the 256-row form)
    (300, 10),    # <32, 0>    (and the ragged 44-query tail, when launched on its own: <32, 64>)
    (300, 50),    # <64, 0>    (tail: <64, 64>)
]


def test_instantiation_matrix():
    """N = 70 001, D = 128: the scan-256 path with a ragged last tile, every filtered form with a mixed mask and a random
    30 % mask, with and without a threshold."""
    N, D = 70_001, 128
    gal = _rows(N, D, 1)
    case = _Case(gal)
    qall = _queries(gal, 300, 2)
    try:
        for name, m in (("mixed", _mixed_mask(N, 3)), ("random30", _random_mask(N, 0.3, 4))):
            for Q, k in MATRIX:
                plan = case.G.search_plan(Q, k)
                assert plan["scan256"] and plan["ksel"] == _ksel(k), (Q, k, plan)
                for thr in (None, 0.3):
                    case.check(qall[:Q], k, thr, name, m)
    finally:
        case.close()


# ---- 2. the small scan (N < 16 384): topk_scan_filtered_kernel<32 | 64> -----------------------------------------------------
@pytest.mark.parametrize("N", [4097, 12_345, 16_383])
@pytest.mark.parametrize("D", [64, 1536])
def test_small_scan(N, D):
    gal = _rows(N, D, N + D)
    case = _Case(gal)
    m = _mixed_mask(N, N)
    try:
        assert not case.G.search_plan(70, 10)["scan256"]
        for Q in (1, 70):
            qr = _queries(gal, Q, Q + D)
            for k in (10, 20):                                   # ksel 32 and 64
                case.check(qr, k, None, "mixed", m)
            case.check(qr, 10, 0.1, "mixed", m)
    finally:
        case.close()


# ---- 3. other widths on the 256 x 256 scan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 768, 1536])
def test_scan256_widths(D):
    N = 20_001
    gal = _rows(N, D, D)
    case = _Case(gal)
    m = _mixed_mask(N, D + 1)
    qr = _queries(gal, 64, D + 2)
    try:
        assert case.G.search_plan(64, 10)["scan256"]
        case.check(qr, 10, None, "mixed", m)                     # <32, 64>
        case.check(qr, 50, None, "mixed", m)                     # <64, 64, M>
    finally:
        case.close()


# ---- 4. the filtered scan's retry ladder ------------------------------------------------------------------------------------
def _scan_stats(Gx, qr, k, m):
    """The experiment twin in certified mode with the scan's counters on: (result, counters); counters[2] = retry passes
    (a tile recomputed in column groups)."""
    exp = _lib.load_exp()
    out = (C.c_int64 * 8)()
    Gx.set_search_mode("certified")
    try:
        _lib.check(exp.revo_debug_scan_stats(out))           # (clears the counters)
        _lib.check(exp.revo_op_set_gemm_debug(SCAN_STATS))
        got = Gx.search(torch.from_numpy(qr).to(DEV), k, allow=torch.from_numpy(m).to(DEV))
        _lib.check(exp.revo_debug_scan_stats(out))
    finally:
        exp.revo_op_set_gemm_debug(0)
        Gx.set_search_mode("bruteforce")
    return got, list(out)


def _stripes_and_runs(N, seed):
    runs = np.zeros(N, dtype=bool)
    for s in np.random.default_rng(seed).integers(0, N, 40):
        runs[s: s + 300] = True
    return (("stripes", np.arange(N) % 2 == 0), ("runs", runs))


def test_ramp_gallery_under_stripes_and_runs():
    """Scores rise with the row index (test_adversarial_order_forces_queue_overflow's gallery): every tile brings rows that
    beat the running bound.  Whether a tile overflows here depends on how far the bounds the slices share have risen by
    then, i.e. on timing, so the retry ladder is not asserted: the next test forces it."""
    N, D, Q, k = 40_000, 64, 300, 10
    rng = np.random.default_rng(5)
    qr = rng.standard_normal((Q, D), dtype=np.float32)
    ramp = np.linspace(0.0, 4.0, N, dtype=np.float32)[:, None]
    gal = qr.mean(0)[None] * ramp + rng.standard_normal((N, D), dtype=np.float32)
    case = _Case(gal)
    try:
        for name, m in _stripes_and_runs(N, 6):
            got = case.check(qr, k, None, name, m)
            twin, st = _scan_stats(case.Gx, qr, k, m)
            assert st[4] > 0, st                                 # survivors were appended under the filter
            _eq(got, twin, (name, "experiment build, certified"))
    finally:
        case.close()


@pytest.mark.parametrize("kind", ["mixed", "stripes", "runs"])
def test_retry_ladder_when_the_prepass_allows_fewer_than_ksel_rows(kind):
    """test_every_late_row_beats_the_seed's gallery: the pre-pass rows are unrelated, every later row is close to every
    query.  Only 20 pre-pass rows are allowed (fewer than ksel = 32): the seeded bound stays at -inf, the first scanned tile
    admits every allowed score, overflows and is recomputed in column groups -- with the recomputed tile's allow-bits
    reloaded for every pass.  The counters of the experiment build prove that the ladder ran."""
    D, Q, k = 64, 300, 10
    rng = np.random.default_rng(11)
    base = rng.standard_normal(D).astype(np.float32)
    qr = base[None] + 0.3 * rng.standard_normal((Q, D), dtype=np.float32)
    gal = np.concatenate([rng.standard_normal((8192, D), dtype=np.float32),
                          base[None] + 0.3 * rng.standard_normal((9000, D), dtype=np.float32)])
    N = gal.shape[0]
    case = _Case(gal)
    try:
        n_pre = case.G.search_plan(Q, k)["prepass_rows"]
        assert 20 < n_pre <= 8192
        m = _mixed_mask(N, 12) if kind == "mixed" else dict(_stripes_and_runs(N, 14))[kind]
        m[:n_pre] = False
        m[np.random.default_rng(13).permutation(n_pre)[:20]] = True
        got = case.check(qr, k, None, kind, m)
        assert int(got[1].min()) >= 8192
        twin, st = _scan_stats(case.Gx, qr, k, m)
        assert st[2] > 0, st                                     # retry passes
        _eq(got, twin, "experiment build, certified")
    finally:
        case.close()


# ---- 5. the filtered collect pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [64, 100, 200])
def test_collect_ladder_with_disallowed_duplicate_columns(Q):
    """test_collect_pass_appends_every_row_once_when_its_retry_ladder_deepens's tile (column 0 and every odd column of one
    256-row tile are duplicates of the queries) with duplicate columns 1, 5, 9, ... disallowed: the collect pass's ladder
    deepens under the filter, and the result is the first k ALLOWED duplicates in index order."""
    N, D, k = 150_000, 64, 10
    rng = np.random.default_rng(5 + Q)
    gal = rng.standard_normal((N, D), dtype=np.float32)
    v = rng.standard_normal(D).astype(np.float32)
    T = 256 * 400
    dup = [T] + [T + c for c in range(1, 256, 2)]
    gal[dup] = v
    qr = np.repeat(v[None], Q, axis=0)
    qr[Q - 3:] = rng.standard_normal((3, D), dtype=np.float32)
    m = _mixed_mask(N, Q)
    m[T: T + 256] = True
    m[[T + c for c in range(1, 256, 4)]] = False                 # column 1 among them
    case = _Case(gal)
    try:
        s, i, c = case.check(qr, k, None, "dups", m)
        st = case.G.search_stats()
        assert st["uncertified"] >= Q - 3 and st["bruteforced"] == 0, st
        want = sorted(r for r in dup if m[r])[:k]
        assert want[:2] == [T, T + 3]
        for q in range(Q - 3):
            assert i[q].cpu().tolist() == want, (q, i[q].cpu().tolist())
            assert torch.all(s[q] == s[q, 0])
    finally:
        case.close()


@pytest.mark.parametrize("Q", [40, 100, 200])
def test_collect_mode_runs_every_filtered_collect_form(Q):
    """Every query through the collect pass (experiment build, mode "collect"): collect256<64> for 40 queries, <128> for
    100, <0> for 200 -- each filtered -- equal to the product's certified result and the references."""
    N, D = 50_001, 128
    gal = _rows(N, D, 21)
    case = _Case(gal)
    Gc = _gallery(gal, experiments=True)
    Gc.set_search_mode("collect")
    m = _mixed_mask(N, 22)
    qr = _queries(gal, Q, 23)
    try:
        for k, thr in ((10, None), (50, None), (10, 0.3)):
            got = case.check(qr, k, thr, "mixed", m)
            _eq(Gc.search(torch.from_numpy(qr).to(DEV), k, thr, allow=torch.from_numpy(m).to(DEV)), got, ("collect", k, thr))
            assert Gc.search_stats()["uncertified"] == Q
    finally:
        Gc.close()
        case.close()


# ---- 6. a scan launch of several phases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Q,k", [(70_003, 2300, 10), (33_000, 3000, 50)])
def test_multi_phase_launch(N, Q, k):
    """Eight query tiles and more under a random 50 % mask (the scan launch is a sequence of phases); best rows planted at
    every query tile's edges, in the gallery's last row and its second half."""
    D = 64
    rng = np.random.default_rng(N + Q + k)
    gal = rng.standard_normal((N, D), dtype=np.float32)
    qr = rng.standard_normal((Q, D), dtype=np.float32)
    plant = sorted(set([0, 255, 256, 257, Q - 1] + [t * 256 for t in range(1, Q // 256)] +
                       [t * 256 - 1 for t in range(1, Q // 256 + 1)]))
    rows = np.linspace(N - 1, N // 2, num=len(plant)).astype(np.int64)
    rows[0] = N - 1
    for qi, r in zip(plant, rows):
        gal[r] = qr[qi]
    m = _random_mask(N, 0.5, N)
    m[rows] = True
    case = _Case(gal)
    try:
        plan = case.G.search_plan(Q, k)
        assert plan["scan256"] and plan["ksel"] == _ksel(k), plan
        s, i, c = case.check(qr, k, None, "random50", m)
        for qi, r in zip(plant, rows):
            assert int(i[qi, 0]) == int(r), (qi, r)
        case.check(qr, k, 0.35, "random50", m)
    finally:
        case.close()


# ---- 7. bitmap edges ---------------------------------------------------------------------------------------------------------
def _search_with_host_bits(G, q, k, bits_np):
    """A search whose filter was set from a HOST bitmap (revo_search_set_filter, src_on_device = 0)."""
    Q = q.shape[0]
    s = torch.empty((Q, k), dtype=torch.float32, device=DEV)
    i = torch.empty((Q, k), dtype=torch.int64, device=DEV)
    c = torch.empty((Q,), dtype=torch.int32, device=DEV)
    bits_np = np.ascontiguousarray(bits_np, dtype=np.int32)
    st = _lib.current_stream()
    _lib.check(G._lib.revo_search_set_filter(G._h, bits_np.ctypes.data, len(G), 0, st), "set_filter")
    try:
        _lib.check(G._lib.revo_search_topk(G._h, _lib.ptr(q), Q, k, 0, 0.0, 0, _lib.ptr(s), _lib.ptr(i), _lib.ptr(c), st),
                   "search")
    finally:
        G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    return s, i, c


def _with_junk(bits, N):
    """The packed bitmap with every bit past row N of its last word set."""
    b = bits.clone()
    if N % 32:
        junk = np.array(~((1 << (N % 32)) - 1) & 0xffffffff, dtype=np.uint32).view(np.int32)
        b[-1] |= int(junk)
    return b


@pytest.mark.parametrize("N", [32 * 601, 64 * 601, 256 * 601, 256 * 601 + 1, 70_001, 5001])
def test_bitmap_sizes_junk_bits_and_host_bitmaps(N):
    """Gallery sizes at every word and tile alignment (N = 32 m, 64 m, 256 m, 256 m + 1, 70 001, and one small-scan size);
    a packed bitmap with junk bits past N, and the same bitmap handed over from the host, give the clean result; one
    gallery has room for more rows than it holds."""
    D, Q = 64, 64
    gal = _rows(N, D, N)
    case = _Case(gal, capacity=N + 29_999 if N == 70_001 else None)
    m = _mixed_mask(N, N + 1)
    qr = _queries(gal, Q, N + 2)
    q = torch.from_numpy(qr).to(DEV)
    try:
        assert case.G.search_plan(Q, 10)["scan256"] == (N >= 16_384)
        for k in (10, 50):
            want = case.check(qr, k, None, "mixed", m)
            bits = case.G.allow_bits(torch.from_numpy(m).to(DEV))
            junk = _with_junk(bits, N)
            assert N % 32 == 0 or not torch.equal(junk, bits)
            _eq(case.G.search(q, k, allow=junk), want, (k, "junk bits past N"))
            _eq(_search_with_host_bits(case.G, q, k, junk.cpu().numpy()), want, (k, "host bitmap"))
    finally:
        case.close()


@pytest.mark.parametrize("N", [70_001, 5001])
def test_masks_at_the_edges_of_the_gallery(N):
    """Only the last row; only the rows of the ragged last tile; only the last 64 pre-pass rows; exactly k rows; k - 1
    rows."""
    D = 128
    gal = _rows(N, D, N + 7)
    qr = _queries(gal, 70, N + 8)
    qr[0] = gal[N - 1]
    case = _Case(gal)
    try:
        for Q in (1, 70):
            masks = {}
            last = np.zeros(N, dtype=bool)
            last[N - 1] = True
            masks["last row"] = last
            tile = 256 if N >= 16_384 else 128
            ragged = np.zeros(N, dtype=bool)
            ragged[(N - 1) // tile * tile:] = True
            masks["ragged tile"] = ragged
            n_pre = case.G.search_plan(Q, 10)["prepass_rows"]
            if n_pre:
                pre = np.zeros(N, dtype=bool)
                pre[n_pre - 64: n_pre] = True
                masks["last 64 pre-pass rows"] = pre
            for k in (10, 50):
                for n in (k, k - 1):
                    few = np.zeros(N, dtype=bool)
                    few[np.random.default_rng(n + Q).permutation(N)[:n]] = True
                    masks[f"{n} rows"] = few
            for name, m in masks.items():
                for k in (10, 50):
                    s, i, c = case.check(qr[:Q], k, None, f"{name} Q{Q}", m)
                    assert (c.cpu().numpy() == min(k, int(m.sum()))).all(), (name, k)
            del masks
    finally:
        case.close()


# ---- 8. exact ties across the mask -------------------------------------------------------------------------------------------
def test_tie_groups_across_words_and_tiles():
    """300 identical rows across a 64-row word and a 256-row tile boundary (one group in the pre-pass, one in the scanned
    rows), every third allowed: the first k allowed members in index order, all with the same score."""
    N, D = 70_001, 128
    gal = _rows(N, D, 31)
    rng = np.random.default_rng(32)
    starts = (256 * 20 - 150, 256 * 100 - 150)               # spans rows 5120 and 25 600
    vecs = rng.standard_normal((2, D)).astype(np.float32)
    m = _random_mask(N, 0.3, 33)
    for s0, v in zip(starts, vecs):
        gal[s0: s0 + 300] = v
        m[s0: s0 + 300] = (np.arange(300) % 3) == 0
    case = _Case(gal)
    try:
        n_pre = case.G.search_plan(64, 10)["prepass_rows"]
        assert starts[0] + 300 <= n_pre <= starts[1]
        for Q in (2, 64, 300):
            qr = _queries(gal, Q, 34 + Q)
            qr[0], qr[1] = vecs[0], vecs[1] * 3.0
            for k in (10, 50):
                s, i, c = case.check(qr, k, None, "ties", m)
                for qi, s0 in ((0, starts[0]), (1, starts[1])):
                    assert i[qi].cpu().tolist() == list(range(s0, s0 + 3 * k, 3)), (Q, k, qi)
                    assert torch.all(s[qi] == s[qi, 0])
    finally:
        case.close()


# ---- 9. threshold, index_offset, keep_f32=False -----------------------------------------------------------------------------
def test_threshold_and_index_offset_under_a_filter():
    N, D = 50_000, 128
    gal = _rows(N, D, 41)
    qr = _queries(gal, 64, 42)
    m = _mixed_mask(N, 43)
    case = _Case(gal)
    try:
        for k in (10, 50):
            s, i, c = case.check(qr, k, 0.27, "mixed", m)
            c = c.cpu().numpy()
            assert (c < k).any() and (c > 0).any(), c               # the threshold cuts filtered lists short
            off = 1_000_000
            so, io, co = case.check(qr, k, 0.27, "mixed", m, index_offset=off)
            assert torch.equal(co.cpu(), torch.from_numpy(c)) and torch.equal(so, s)
            assert torch.equal(io, torch.where(i >= 0, i + off, i))
            assert (io.cpu().numpy()[np.arange(k)[None] >= c[:, None]] == -1).all()          # padding stays -1
    finally:
        case.close()


def test_keep_f32_false_filtered_equals_the_sub_gallery():
    """No fp32 rows: the result is the bf16 scan's own selection, with the scan's own scores.  A filtered search of such a
    gallery equals the search of a keep_f32=False gallery of the allowed rows bit for bit.  (Pre-pass rows are scored by a
    GEMM of their own, so the mask allows every pre-pass row and both galleries have the same pre-pass: N = 70 655 keeps
    17 408 pre-pass rows down to 69 632 rows.  The mixed words lie in the scanned rows, at most 1 023 rows disallowed.)
    Scores only within the bf16 scan's tolerance of the oracle, for this mask and for a mixed mask over the whole gallery."""
    N, D, Q = 70_655, 256, 40
    gal = _rows(N, D, 51)
    qr = _queries(gal, Q, 52)
    q = torch.from_numpy(qr).to(DEV)
    G = _gallery(gal, keep_f32=False)
    n_pre = G.search_plan(Q, 10)["prepass_rows"]
    assert n_pre == 17_408
    m = np.ones(N, dtype=bool)
    m[n_pre + 512: n_pre + 1536] = _mixed_mask(1024, 53)
    m[N - 1] = False
    allowed = np.flatnonzero(m)
    assert N - 1023 <= allowed.size < N
    S = _gallery(gal[allowed], keep_f32=False)
    try:
        assert S.search_plan(Q, 10)["prepass_rows"] == n_pre
        for k in (10, 50):
            for name, mk in (("pre-pass allowed", m), ("mixed", _mixed_mask(N, 54))):
                got = G.search(q, k, allow=torch.from_numpy(mk).to(DEV))
                assert G.search_stats()["uncertified"] == -1
                if mk is m:
                    _eq(got, _mapped(S.search(q, k), allowed), (name, k))
                rs, ri, rc = osearch.search(gal, qr, k, allow=mk)
                s, i, c = (t.cpu().numpy() for t in got)
                assert np.array_equal(c, rc) and np.abs(s - rs).max() <= 1e-2, (name, k)
                assert mk[i[i >= 0]].all()
                assert (np.sort(i[:, :10], axis=1) == np.sort(ri[:, :10], axis=1)).mean() >= 0.9
    finally:
        S.close()
        G.close()
