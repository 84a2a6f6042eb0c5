"""The in-place edits (Gallery.remove / update, include/revo.h EDIT) on the two galleries of tests/_wide_gallery.py, whose
rows cross byte 2^31 / 2^32 / 2^33 of the fp32 master and the bf16 copy and row 2^24: the remove gather's source and
destination offsets, the staged and the direct gather, the update's destination rows and the append behind an edit.  The
reference is torch fp64 over the appended bits, computed once per gallery and carried through each edit (rows are
independent: dropping, renumbering and adding list entries is the reference of the edited rows).  Every test builds its own
handle (an append of regenerated chunks), closed by the `keep` fixture whatever the outcome; one handle is alive at a time.

Tolerances: tests/test_gpu_wide_gallery.py.  Measured on an MI355X: the reference of the 64 queries takes 0.1 s per gallery,
an append of all chunks 0.1 s (W) and 0.4 s (L); each test takes 0.4 - 0.8 s, the update on W 4.5 s (its pairs join: 4.4 s)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wide_gallery as wg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = wg.DEV
NQ = 64
THRESHOLD = {"W": 0.5, "L": 0.85}
SIGMA_NEW = 0.3                       # the rows an update writes score 1 / sqrt(1 + 0.09) = 0.958 against their direction


def _build(name):
    w = wg.Wide(name)
    wg.need_free_gb(w.gb + 8)
    t0 = time.time()
    c = wg.Ctx()
    c.w, c.name, c.D, c.N, c.d = w, name, w.D, w.N, wg.delta(w.D)
    # the rows an update writes: one new direction per mark and for row N - 1, descending row order
    c.upd_rows = sorted(list(w.marks) + [w.N - 1], reverse=True)
    rng = np.random.default_rng(w.seed + 77)
    cn = rng.standard_normal((len(c.upd_rows), w.D))
    cn /= np.linalg.norm(cn, axis=1, keepdims=True)
    u = rng.standard_normal(cn.shape)
    u -= (u * cn).sum(1, keepdims=True) * cn
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c.upd_dirs = torch.from_numpy(cn.astype(np.float32)).to(DEV)
    c.upd_vecs = torch.nn.functional.normalize(torch.from_numpy((cn + SIGMA_NEW * u).astype(np.float32)).to(DEV), dim=-1)
    # queries: the site directions, the update's directions, perturbed sites and random directions
    q = w.queries(NQ, seed=2)
    ns = len(w.sites)
    q[ns:ns + len(c.upd_rows)] = c.upd_dirs
    c.q, c.ns = q, ns
    c.qn = wg.normalised(q)
    c.bs, c.br = wg.ref_best(c.qn, w.chunks(), keep=1100)
    torch.cuda.synchronize()
    print(f"gallery {name}: reference of {NQ} queries {time.time() - t0:.1f} s")
    return c


@pytest.fixture(scope="module")
def ref_w():
    return _build("W")


@pytest.fixture(scope="module")
def ref_l():
    return _build("L")


def _ctx(request, name):
    return request.getfixturevalue("ref_" + name.lower())


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


def _handle(c, keep):
    wg.need_free_gb(c.w.gb + 4)
    t0 = time.time()
    G = c.w.fill(keep(engine.Gallery(c.D, c.N + 8, device=0)))
    torch.cuda.synchronize()
    print(f"gallery {c.name}: append {time.time() - t0:.1f} s")
    return G


BOTH = pytest.mark.parametrize("name", ["W", "L"])


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _searches_match(c, G, bs, br, what):
    """k = 10 and the range search of the planted rows against the reference of the edited rows"""
    s, i, cnt = G.search(c.q, k=10)
    for r in range(NQ):
        wg.check_topk(s[r], i[r], cnt[r], bs[r], br[r], 10, c.d, what=f"{what} query {r}")
    t = THRESHOLD[c.name]
    off, idx, sc = G.search_range(c.q, t)
    n = wg.check_range(off, idx, sc, bs, br, t, c.d, what=what)
    assert n == idx.shape[0] and n >= 4
    return off, idx


def _append_lands_at_the_end(c, G, n_before):
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.nn.functional.normalize(torch.randn(5, c.D, generator=g, device=DEV), dim=-1)
    assert G.add(x, normalize=False) == n_before and len(G) == n_before + 5
    assert _same_bits(G.read(n_before, 5), x)
    s, i, _ = G.search(x[:2], k=1)
    assert i[:, 0].tolist() == [n_before, n_before + 1] and float((s[:, 0] - 1).abs().max()) <= 1e-6


def _check_reads(c, G, kept_old, around):
    """read(j - 4, 8) around the new rows `around` equals the source rows kept_old[j - 4: j + 4]"""
    n = len(G)
    for j in around:
        a = max(0, min(int(j) - 4, n - 8))
        assert _same_bits(G.read(a, 8), c.w.gather(kept_old(a, 8))), (c.name, int(j))


@BOTH
def test_remove_three_rows_shifts_every_later_row_across_every_mark(request, name, keep):
    """Rows 3 and the two middle rows of the first mark's site leave: every chunk behind them is gathered through the staging
    buffer and copied down by one to three rows, across every byte mark of both arrays."""
    c = _ctx(request, name)
    m0 = c.w.marks[0]
    gone = [3, m0 - 1, m0]
    G = _handle(c, keep)
    assert G.remove(torch.tensor(gone, dtype=torch.int64, device=DEV)) == 3 and len(G) == c.N - 3
    removed = torch.zeros(c.N, dtype=torch.bool, device=DEV)
    removed[torch.tensor(gone, device=DEV)] = True
    kept_rows = torch.nonzero(~removed)[:, 0]
    new_index = torch.cumsum((~removed).to(torch.int64), 0) - 1
    around = [0, 4] + [m + s for m in c.w.marks for s in (-3, 0)] + [c.N - 3 - 4]
    _check_reads(c, G, lambda a, n: kept_rows[a:a + n], around)
    bs, br = wg.edit_reference(c.bs, c.br, removed=removed, new_index=new_index)
    off, idx = _searches_match(c, G, bs, br, f"{name} remove 3")
    assert idx[int(off[1]):int(off[2])].tolist() == [m0 - 3, m0 - 2]      # the first mark's site: its outer rows, now adjacent
    _append_lands_at_the_end(c, G, c.N - 3)
    G.close()


def test_remove_a_random_30_percent_L(request, keep):
    """256 chunks of 65 536 rows: after the first few the kept rows land in front of their chunk and the gather writes them
    directly; the 11.7 M rows left still cross byte 2^31 of the fp32 master (row 2^23)."""
    c = _ctx(request, "L")
    g = torch.Generator(device=DEV).manual_seed(30)
    removed = torch.rand(c.N, generator=g, device=DEV) < 0.3
    n_gone = int(removed.sum())
    G = _handle(c, keep)
    assert G.remove(removed) == n_gone and len(G) == c.N - n_gone
    assert len(G) > (1 << 23) + 1000
    kept_rows = torch.nonzero(~removed)[:, 0]
    new_index = torch.cumsum((~removed).to(torch.int64), 0) - 1
    shifted = [int(new_index[m]) for m in c.w.marks]                      # where the old marks' rows went (or their successors)
    around = [0, 65536, 3 * 65536, 1 << 22, 1 << 23] + shifted + [len(G) - 4]
    _check_reads(c, G, lambda a, n: kept_rows[a:a + n], around)
    bs, br = wg.edit_reference(c.bs, c.br, removed=removed, new_index=new_index)
    _searches_match(c, G, bs, br, "L remove 30 %")
    _append_lands_at_the_end(c, G, c.N - n_gone)
    G.close()


@BOTH
def test_update_overwrites_the_rows_at_every_mark(request, name, keep):
    """The row at every mark and row N - 1 get new planted directions (descending row order, normalize=False): read returns
    them and leaves their neighbours alone, k = 10 finds them, and the overwritten planted rows are gone from the pairs (W)
    and from the range search of their site (L)."""
    c = _ctx(request, name)
    G = _handle(c, keep)
    rows = torch.tensor(c.upd_rows, dtype=torch.int64)
    G.update(rows, c.upd_vecs, normalize=False)
    assert len(G) == c.N
    for j, r in enumerate(c.upd_rows):
        got = G.read(r - 1, 2) if r == c.N - 1 else G.read(r - 1, 3)
        assert _same_bits(got[1], c.upd_vecs[j]), (name, r)
        assert _same_bits(got[0], c.w.rows_at(r - 1, 1)[0]), (name, r)
        if r < c.N - 1:
            assert _same_bits(got[2], c.w.rows_at(r + 1, 1)[0]), (name, r)
    overwritten = torch.zeros(c.N, dtype=torch.bool, device=DEV)
    overwritten[rows.to(DEV)] = True
    extra = c.qn.to(torch.float64) @ c.upd_vecs.to(torch.float64).T
    bs, br = wg.edit_reference(c.bs, c.br, removed=overwritten, extra_rows=rows.to(DEV), extra_scores=extra)
    off, idx = _searches_match(c, G, bs, br, f"{name} update")
    s, i, _ = G.search(c.q, k=10)
    for j, r in enumerate(c.upd_rows):                                    # the update's directions find their rows
        assert int(i[c.ns + j, 0]) == r and abs(float(s[c.ns + j, 0]) - (1 + SIGMA_NEW ** 2) ** -0.5) <= 1e-5
    for sq in range(c.ns):                                                # the sites' queries no longer see the old rows
        got = idx[int(off[sq]):int(off[sq + 1])].tolist()
        assert got == [r for r in c.w.sites[sq] if r not in c.upd_rows], (name, sq, got)
    if name == "W":
        want = wg.planted_pairs(c.w, 0.5, c.d, without=set(c.upd_rows))
        pairs, scores = G.pairs(0.5)
        assert pairs.cpu().tolist() == [[a, b] for a, b, _ in want]
        assert np.abs(scores.cpu().numpy().astype(np.float64) - np.array([x for _, _, x in want])).max() <= 1e-6
    G.close()
