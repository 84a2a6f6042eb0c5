"""Every search at the admitted widths the towers do not have: D = 128, 192, 320 and 2112, i.e. 2, 3, 5 and 33 K-tiles of 64.

gemm256_mainloop (revers-o_amd/csrc/gemm256_core.h) walks K two tiles per trip and peels an odd last tile into a block of
its own; every scan, join and pass kernel instantiates it.  D = 128 is the one-trip case in which no tile t + 2 is ever
requested, 192 the smallest peeled tail, 320 a trip with refills and then the tail, 2112 an odd count past the 2048 elements
the normalisation kernel holds in registers.  Galleries of 20 037 rows (above SEARCH_SMALL_ROWS: the 256 x 256 scan, ragged
last tile) and 3 000 rows (the small-gallery scan on the gemm_core.h ring); standard-normal rows and queries
(tests/_scan_bounds.py: the same data as the CPU teeth in tests/test_scan_bounds_teeth.py).

1. The scan's own sums.  An exact search re-scores its candidates in fp32, so a main loop that is slightly wrong can still
   return the right answer on easy data.  A gallery without the fp32 master returns the scan's scores as they are: each is
   held to |s - qb . gb| <= D 2^-23 ||qb|| ||gb|| (cert_eps's gam1 term; qb, gb the bf16 roundings of the rows as the
   library normalised them, the dot product in fp64), and the returned indices to the fp64 ranking of qb . gb up to rows
   within twice that bound of the k-th score.  Q = 1, 64, 100, 160, 300 (the scan's row modes 64, 64, 128, 192 and 256 with
   a partly empty second query tile) x k = 10, 50 (32 and 64 kept candidates) x filtered or not x both gallery sizes.
2. Every exact search family against the exhaustive reference its own module has, at the tolerances those modules use.
3. The normalisation at insert against fp64, per element.

Largest |s - qb . gb| / bound measured on an MI355X, over all Q and k (the test prints every (Q, k); an error in one K-tile
gives 20 to 2 10^4, tests/test_scan_bounds_teeth.py, where a strict left-to-right fp32 chain gives 0.004 ... 0.001):

    D      20 037 rows, plain   filtered 50 %   3 000 rows, plain   filtered 50 %
    128    0.0052               0.0042          0.0052              0.0049
    192    0.0032               0.0029          0.0032              0.0027
    320    0.0018               0.0019          0.0018              0.0017
    2112   0.0003               0.0003          0.0003              0.0003

Normalisation, largest |y - ref| / bound: 0.045 (D = 128), 0.031 (192), 0.017 (320), 0.0029 (2112).

Not reachable: a keep_f32 = 0 gallery never runs the scan with the admission margin (search.hip: the margin needs the fp32
rows), so the margin forms are covered by the plain search at k = 50 (section 2) and not by section 1."""
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_bounds as sb  # noqa: E402
from _search_checks import _check  # noqa: E402
import test_gpu_clusters as t_clusters  # noqa: E402
import test_gpu_discover as t_discover  # noqa: E402
import test_gpu_gallery_edit as t_edit  # noqa: E402
import test_gpu_gallery_pairs as t_pairs  # noqa: E402
import test_gpu_grouped_search as t_groups  # noqa: E402
import test_gpu_maxsim as t_maxsim  # noqa: E402
import test_gpu_mmr as t_mmr  # noqa: E402
import test_gpu_range_search as t_range  # noqa: E402
import test_gpu_recommend as t_recommend  # noqa: E402
from test_gpu_search import _bruteforce_twin  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = sb.N_SCAN256
QS = (1, 64, 100, 160, 300)
NEAR_TIE = 3e-7


class _Width:
    """One width's shared, read-only data: the raw rows and queries, the product gallery, the rows and queries as the
    library normalised them (its own kernel: an append), and the exhaustive fp64 scores of those fp32 rows."""

    def __init__(self, D):
        self.D = D
        self.x = sb.rows(N, D, DEV)
        self.q = sb.queries(D, DEV)
        self.G = engine.Gallery(D, N, device=0)
        self.G.add(self.x)
        self.rows = self.G.read()
        T = engine.Gallery(D, sb.Q_MAX, device=0)
        T.add(self.q)
        self.qn = T.read()
        T.close()
        self.S64 = sb.reference(self.qn, self.rows)              # fp64 sums of the fp32 rows [Q_MAX, N]
        self.S32 = self.S64.float()                              # ... rounded once: the score the oracle ranks
        self.qb = sb.bf16_round(self.qn)
        self.gb = sb.bf16_round(self.rows)

    def close(self):
        self.G.close()


@pytest.fixture(scope="module", params=sb.W, ids=[f"D{d}" for d in sb.W])
def wd(request, dev):
    w = _Width(request.param)
    yield w
    w.close()


def _oracle_topk(S32, k, thr=None, allow=None):
    """oracle.search's rule on scores that are already there (fp64 sums rounded once to fp32, on the device): the best k
    allowed rows by (score desc, index asc), cut at score >= fp32(thr), padded with -inf / -1.  numpy, as oracle.search."""
    s = S32 if allow is None else torch.where(allow[None, :], S32, torch.full_like(S32, float("-inf")))
    n_ok = S32.shape[1] if allow is None else int(allow.sum())
    ss, ii = torch.sort(s, dim=1, descending=True, stable=True)             # stable: equal scores stay in index order
    kk = min(k, n_ok)
    out_s = torch.full((S32.shape[0], k), float("-inf"), device=S32.device)
    out_i = torch.full((S32.shape[0], k), -1, dtype=torch.int64, device=S32.device)
    out_s[:, :kk], out_i[:, :kk] = ss[:, :kk], ii[:, :kk]
    if thr is not None:
        cut = out_s < torch.tensor(thr, dtype=torch.float32)
        out_s[cut], out_i[cut] = float("-inf"), -1
    return out_s.cpu().numpy(), out_i.cpu().numpy(), (out_i >= 0).sum(1).to(torch.int32).cpu().numpy()


def _same_bits(a, b, what):
    for j, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), (what, j)


# ---- 1. the scan's own sums -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [sb.N_SCAN256, sb.N_SMALL])
def test_scan_sums_against_fp64(wd, n_rows):
    D = wd.D
    Gs = engine.Gallery(D, n_rows, device=0, keep_f32=False)
    Gs.add(wd.x[:n_rows])                                        # the same kernel, row by row: the bf16 of wd.rows[:n_rows]
    assert Gs.search_plan(64, 10)["scan256"] == (n_rows >= 16384)
    gb = wd.gb[:n_rows]
    ref, bnd = sb.reference(wd.qb, gb), sb.bound(wd.qb, gb)
    mask = sb.allow_mask(n_rows, D, DEV)
    try:
        for allow, tag in ((None, "plain"), (mask, "filtered 50 %")):
            worst = {}
            for Q in QS:
                for k in (10, 50):
                    s, i, c = Gs.search(wd.q[:Q], k, allow=allow)
                    worst[(Q, k)] = float(sb.check_topk(s, i, c, ref[:Q], bnd[:Q], k, allow).max())
            print(f"[scan sums D={D} N={n_rows} {tag}] max |s - qb.gb| / bound = {max(worst.values()):.4f}; per (Q, k): "
                  + ", ".join(f"({Q}, {k}) {v:.4f}" for (Q, k), v in worst.items()))
    finally:
        Gs.close()


# ---- 2. the exact search families ----------------------------------------------------------------------------------------
def test_plain_search(wd):
    D = wd.D
    Gx = _bruteforce_twin(wd.G)                                  # librevo_exp.so, the same fp32 rows, brute force
    try:
        for Q in QS:
            q = wd.q[:Q]
            for k in (10, 50):
                for thr in (None, D ** -0.5):
                    out = wd.G.search(q, k, thr)
                    st = wd.G.search_stats()
                    _check(out, _oracle_topk(wd.S32[:Q], k, thr), atol=1e-5, near_tie=NEAR_TIE)
                    Gx.set_search_mode("bruteforce")
                    _same_bits(out, Gx.search(q, k, thr), ("bruteforce", Q, k, thr))
                    Gx.set_search_mode("collect")                # the collect pass's ROWS forms
                    _same_bits(out, Gx.search(q, k, thr), ("collect", Q, k, thr))
                    if thr is None:
                        print(f"[plain search D={D} Q={Q} k={k}] stats {st}")
    finally:
        Gx.close()


def test_filtered_search(wd):
    Gx = _bruteforce_twin(wd.G)
    try:
        for frac in (0.5, 0.01):
            m = sb.allow_mask(N, wd.D, DEV, frac)
            for Q in (1, 100, 300):
                q = wd.q[:Q]
                for k in (10, 50):
                    out = wd.G.search(q, k, allow=m)
                    _check(out, _oracle_topk(wd.S32[:Q], k, None, m), atol=1e-5, near_tie=NEAR_TIE)
                    _same_bits(out, Gx.search(q, k, allow=m), ("bruteforce", frac, Q, k))
                    assert bool(m[out[1][out[1] >= 0]].all())
    finally:
        Gx.close()


def test_large_k_search(wd):
    for k in (300, 1024):
        for Q in (20, 150, 300):
            out = wd.G.search(wd.q[:Q], k)
            _check(out, _oracle_topk(wd.S32[:Q], k), atol=1e-5, near_tie=NEAR_TIE)
            assert wd.G.search_stats()["large_k_fallback"] == 0


def test_range_search(wd):
    D = wd.D
    t = 2.5 * D ** -0.5                                          # in the bulk: ~0.6 % of the rows per query
    hits = (wd.S64 >= t).sum(1)
    assert 10 <= int(hits.min()) and int(hits.max()) <= 5000, (int(hits.min()), int(hits.max()))
    for Q in (1, 100, 300):
        off, idx, sc = wd.G.search_range(wd.q[:Q], t)
        t_range._check_against_oracle(off, idx, sc, wd.qn[:Q], wd.rows, t, t_range._delta(D))
        assert int(off[-1]) >= int((wd.S64[:Q] >= t + t_range._delta(D)).sum())


def test_pairs(wd):
    D = wd.D
    t, delta = 4.0 * D ** -0.5, t_pairs._delta(D)                # in the bulk: ~3e-5 of the 2e8 pairs
    must, may, score = t_pairs._oracle(wd.rows, t, delta)
    assert 10 ** 3 <= len(must) <= 10 ** 6, len(must)
    pairs, scores = wd.G.pairs(t)
    t_pairs._check_against_oracle(pairs, scores, must, may, score, delta)


def test_clusters(wd):
    from reverso_amd import store
    D = wd.D
    t, want64 = t_clusters._clear_threshold(wd.rows, 4.0 * D ** -0.5, t_pairs._delta(D))
    assert 10 ** 3 <= sum(len(g) for g in want64) <= 10 ** 6
    labels, offsets, members = wd.G.clusters(t)
    t_clusters._check_shape(labels, offsets, members, N)
    pairs, _ = wd.G.pairs(t)
    want = store.connected_groups(pairs.cpu().numpy(), N)
    assert t_clusters._lists(offsets, members) == want == want64
    assert np.array_equal(labels.cpu().numpy(), t_clusters._labels_of(want, N))


@pytest.mark.parametrize("P,Nn", [(1, 0), (32, 32), (100, 28)])
def test_recommend(wd, P, Nn):
    pos, neg = wd.q[:P], (wd.q[P:P + Nn] if Nn else None)
    t_recommend._check_composition(wd.G, pos, neg)
    t_recommend._stats_are_the_recommend_search(wd.G)


@pytest.mark.parametrize("n,has_target", [(8, True), (63, True), (8, False), (63, False)])
def test_discover(wd, n, has_target):
    t_discover._check_composition(wd.G, wd.q[:2 * n + int(has_target)], n, has_target)


@pytest.mark.parametrize("n", [1, 5, 64])
def test_maxsim(wd, n):
    groups = (np.arange(N) // 3).astype(np.int32)
    q = wd.q[:n]
    t_maxsim._check(wd.G, q, groups, t_recommend._chain_scores(wd.G, q))
    t_maxsim._stats_are_the_maxsim_search(wd.G)


@pytest.mark.parametrize("k,C", [(10, 100), (50, 1024)])
def test_mmr(wd, k, C):
    t_mmr._check(wd.G, wd.q[:3], k, C, 0.5)


def test_grouped_search(wd):
    groups = (np.arange(N) // 3).astype(np.int32)
    groups[::11] = -1
    Q = 48
    for L, S in ((5, 3), (10, 1)):
        got = wd.G.search_groups(wd.q[:Q], torch.from_numpy(groups).to(DEV), limit=L, group_size=S)
        ref = t_groups._oracle_groups(None, groups, None, L, S, sc=wd.S32[:Q].cpu().numpy())
        t_groups._check_oracle(got, ref)


def test_search_after_remove_and_update(wd):
    """30 % of the rows removed and 200 overwritten: the rows and every plain search equal a fresh gallery's, byte for
    byte (the gather's D / 4 and D / 8 units at these widths)."""
    D = wd.D
    g = torch.Generator().manual_seed(D)
    gone = (torch.rand(N, generator=g) < 0.3).to(DEV)
    kept = wd.x[~gone].clone()
    at = torch.randperm(kept.shape[0], generator=g)[:200]
    new = torch.randn(200, D, generator=g).to(DEV)
    G = engine.Gallery(D, N, device=0)
    G.add(wd.x)
    assert G.remove(gone) == int(gone.sum())
    G.update(at, new)
    kept[at.to(DEV)] = new
    F = engine.Gallery(D, N, device=0)
    F.add(kept)
    try:
        assert len(G) == len(F) == kept.shape[0]
        t_edit._same((G.read(),), (F.read(),), "rows")
        for Q, k in ((1, 10), (100, 50), (300, 10)):
            t_edit._same(G.search(wd.q[:Q], k), F.search(wd.q[:Q], k), (Q, k))
    finally:
        G.close()
        F.close()


# ---- 3. the normalisation at insert ----------------------------------------------------------------------------------------
def test_normalisation_against_fp64(wd):
    """y = x * (1 / sqrtf(sum of squares)) per element against x / ||x|| in fp64.  Relative error bound, in units of 2^-24:
    D / 2 for the sum of squares under the square root (an fp32 fma chain and a wave reduction: at most D additions of
    relative error 2^-24 each, halved by the root), 2 for sqrtf (1 ulp: the HIP math API's table of single-precision
    functions lists sqrtf at 1 ulp), 2 for the division (1 ulp; hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt
    makes both correctly rounded, half of that), 1 for the rounding of the product: D / 2 + 5.  The ROCm tree this was
    written against ships the compiler's option help but not the HIP math API pages; the figures are the published ones.
    Measured on an MI355X, largest error / bound: 0.045 (D = 128), 0.031 (192), 0.017 (320), 0.0029 (2112; the loop that
    does not hold the row in registers)."""
    D = wd.D
    rel = (D / 2 + 5) * 2.0 ** -24
    worst = 0.0
    for x, y in ((wd.x, wd.rows), (wd.q, wd.qn)):
        x64 = x.double()
        ref = x64 / x64.norm(dim=1, keepdim=True)
        worst = max(worst, float(((y.double() - ref).abs() / (rel * ref.abs())).max()))
    print(f"[normalisation D={D}] max |y - ref| / bound = {worst:.4f} (bound: relative {rel:.3e})")
    assert worst <= 1.0
