"""Two galleries that cross every 32-bit mark of the library's address and index arithmetic, and their fp64 reference
(tests/test_gpu_wide_gallery.py, tests/test_gpu_wide_gallery_edit.py; DESIGN.md, testing).

W (wide): 1024 x (2^21 + 300).  fp32 master: byte 2^31 at row 2^19, 2^32 at row 2^20, 2^33 at row 2^21; bf16 copy: byte 2^31
          at row 2^20, 2^32 at row 2^21; element index 2^31 at row 2^21.
L (long): 64 x (2^24 + 300).  Row index 2^24 (the scan's 24-bit relative index, fp32-exact integers, a 25-bit row field in
          the sort keys, the radix sort's tile above 4096 keys); fp32 master: byte 2^31 at row 2^23, 2^32 at row 2^24; bf16
          copy: byte 2^31 at row 2^24.

The bulk rows are random unit directions, generated chunk by chunk from a device generator seeded per chunk and normalised by
torch in fp32: any chunk can be made again, so the source is never kept, and the rows are appended with normalize=False, so
the master bits are known without reading them back through the library.  The chunk lengths divide none of the marks: the
appends straddle every one of them.

A SITE is the rows m - 2 .. m + 1 around a mark m; rows 0, 1 and N - 2, N - 1 are sites as well.  Each site has a unit
direction c; its rows are c + sigma * u with u a unit vector orthogonal to c and one sigma per row, so a site row scores
1 / sqrt(1 + sigma^2) against c whatever the dimension (W: about 0.94, 0.86, 0.74, 0.61; L: 0.96, 0.93, 0.89, 0.86), far
above anything a bulk row reaches (W: about 0.17; L: about 0.7 against a unit query).  An address that wraps at 2^k reads
an unrelated bulk row instead: the returned score and the returned set both change.

The reference is torch fp64 over those bits, never the library: ref_scores() (the full matrix, a handful of vectors) and
ref_best() (streamed, hundreds of queries: the best `keep` rows of each in (score desc, row asc) order)."""
import numpy as np
import torch

DEV = torch.device("cuda", 0)

SPECS = {
    "W": dict(D=1024, N=(1 << 21) + 300, chunk=300_007, seed=2101, marks=(1 << 19, 1 << 20, 1 << 21),
              sigmas=(0.35, 0.6, 0.9, 1.3), gb=12.9),
    "L": dict(D=64, N=(1 << 24) + 300, chunk=1_000_003, seed=2402, marks=(1 << 23, 1 << 24),
              sigmas=(0.3, 0.4, 0.5, 0.6), gb=6.4),
}


def delta(D):
    """the fp32 chain's band (tests/test_gpu_range_search.py _delta)"""
    return 3e-7 * max(1.0, D / 1024)


class Wide:
    """the rows of one of the two galleries: chunks(), rows_at(), the sites and their directions"""

    def __init__(self, name):
        sp = SPECS[name]
        self.name, self.D, self.N, self.chunk, self.seed = name, sp["D"], sp["N"], sp["chunk"], sp["seed"]
        self.marks, self.sigmas, self.gb = sp["marks"], sp["sigmas"], sp["gb"]      # gb: the handle, in 1e9 bytes
        N = self.N
        self.sites = [[0, 1]] + [[m - 2, m - 1, m, m + 1] for m in self.marks] + [[N - 2, N - 1]]
        rng = np.random.default_rng(self.seed)
        c = rng.standard_normal((len(self.sites), self.D))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        self.centres = torch.from_numpy(c.astype(np.float32)).to(DEV)        # [sites, D] (fp32; unit up to rounding)
        rows, vecs = [], []
        for s, site in enumerate(self.sites):
            for j, r in enumerate(site):
                u = rng.standard_normal(self.D)
                u -= (u @ c[s]) * c[s]
                u /= np.linalg.norm(u)
                rows.append(r)
                vecs.append(c[s] + self.sigmas[j] * u)
        self.planted_rows = np.array(rows, dtype=np.int64)
        self.planted = torch.nn.functional.normalize(torch.from_numpy(np.array(vecs, dtype=np.float32)).to(DEV), dim=-1)
        self.site_of = {int(r): s for s, site in enumerate(self.sites) for r in site}

    def n_chunks(self):
        return (self.N + self.chunk - 1) // self.chunk

    def chunk_rows(self, ci):
        """(first row, fp32 rows [n, D]) of chunk ci: the bits the gallery holds"""
        s0 = ci * self.chunk
        n = min(self.chunk, self.N - s0)
        g = torch.Generator(device=DEV).manual_seed(self.seed * 1000 + ci)
        x = torch.nn.functional.normalize(torch.randn(n, self.D, generator=g, device=DEV), dim=-1)
        inside = np.nonzero((self.planted_rows >= s0) & (self.planted_rows < s0 + n))[0]
        if inside.shape[0]:
            x[torch.from_numpy(self.planted_rows[inside] - s0).to(DEV)] = self.planted[torch.from_numpy(inside).to(DEV)]
        return s0, x

    def chunks(self):
        for ci in range(self.n_chunks()):
            yield self.chunk_rows(ci)

    def rows_at(self, start, n):
        """fp32 rows [start, start + n) (made again from their chunks)"""
        out = []
        for ci in range(start // self.chunk, (start + n - 1) // self.chunk + 1):
            s0, x = self.chunk_rows(ci)
            out.append(x[max(start - s0, 0): start + n - s0].clone())
        return torch.cat(out)

    def gather(self, rows):
        """the fp32 rows `rows` (int64 device tensor, any order) in one pass over the chunks"""
        out = torch.empty((rows.shape[0], self.D), dtype=torch.float32, device=DEV)
        for s0, x in self.chunks():
            m = (rows >= s0) & (rows < s0 + x.shape[0])
            if bool(m.any()):
                out[m] = x[rows[m] - s0]
        return out

    def row(self, r):
        return self.rows_at(int(r), 1)[0].cpu().numpy()

    def fill(self, G):
        for _, x in self.chunks():
            G.add(x, normalize=False)
        return G

    def queries(self, Q, seed):
        """Q raw queries: the site directions, perturbed copies of them, random directions"""
        g = torch.Generator(device=DEV).manual_seed(self.seed + seed)
        q = torch.randn(Q, self.D, generator=g, device=DEV)
        ns = len(self.sites)
        q[:ns] = self.centres
        for j in range(ns, Q):
            if j % 3 != 2:                                                   # two of three: a perturbed site direction
                q[j] = self.centres[j % ns] + 0.25 * q[j] / self.D ** 0.5
        return q


def need_free_gb(gb):
    """skip (printing the need) only when the stated memory (in 1e9 bytes) is not free"""
    import pytest
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 1e9:
        print(f"needs {gb:.1f} GB of free HBM, {free / 1e9:.1f} GB free")
        pytest.skip(f"needs {gb:.1f} GB of free HBM")


class Ctx:
    """what a module's fixture holds of one gallery (the rows' description, queries, references, maybe a handle)"""


def normalised(q):
    """the fp32 query rows the library scores (the same normalisation kernel as an append), through a throw-away gallery"""
    from reverso_amd import engine
    T = engine.Gallery(q.shape[1], q.shape[0], device=0)
    try:
        T.add(q)
        return T.read()
    finally:
        T.close()


def ref_scores(vectors, chunks, n_rows):
    """S [vectors, rows] fp64 (device) of a few normalised fp32 vectors (16; 33 for the widest multi-vector query) against
    the fp32 rows of `chunks`"""
    v = vectors.to(torch.float64)
    assert v.shape[0] <= 33
    S = torch.empty((v.shape[0], n_rows), dtype=torch.float64, device=DEV)
    for s0, x in chunks:
        for a in range(0, x.shape[0], 1 << 18):
            S[:, s0 + a: s0 + min(a + (1 << 18), x.shape[0])] = v @ x[a: a + (1 << 18)].to(torch.float64).T
    return S


def ref_best(vectors, chunks, keep=1100):
    """streamed: per vector the best `keep` rows, (scores [Q, keep] fp64, rows [Q, keep] int64) in (score desc, row asc) order"""
    v = vectors.to(torch.float64)
    Q = v.shape[0]
    bs = torch.full((Q, keep), -np.inf, dtype=torch.float64, device=DEV)
    br = torch.full((Q, keep), -1, dtype=torch.int64, device=DEV)
    for s0, x in chunks:
        for a in range(0, x.shape[0], 1 << 18):
            part = x[a: a + (1 << 18)]
            S = v @ part.to(torch.float64).T
            ts, ti = torch.topk(S, min(keep, S.shape[1]), dim=1)
            cs, cr = torch.cat([bs, ts], 1), torch.cat([br, ti + (s0 + a)], 1)
            o = torch.argsort(cs, dim=1, descending=True, stable=True)[:, :keep]      # (earlier rows first among equals)
            bs, br = torch.gather(cs, 1, o), torch.gather(cr, 1, o)
    return bs, br


def check_range_full(off, idx, sc, S, t, d, allow=None, what=""):
    """test_gpu_range_search._check_against_oracle over a given fp64 score matrix S [Q, rows] (device)"""
    Q, N = S.shape
    assert off.shape == (Q + 1,) and int(off[0]) == 0 and int(off[-1]) == idx.shape[0] == sc.shape[0], what
    assert bool((off[1:] >= off[:-1]).all())
    ok = torch.ones(N, dtype=torch.bool, device=DEV) if allow is None else allow
    qe = torch.repeat_interleave(torch.arange(Q, device=DEV), off[1:] - off[:-1])
    assert bool(((idx >= 0) & (idx < N)).all()), what
    got = torch.zeros((Q, N), dtype=torch.bool, device=DEV)
    got[qe, idx] = True
    assert int(got.sum()) == idx.shape[0], (what, "a row twice")
    must = (S >= t + d) & ok[None, :]
    may = (S >= t - d) & ok[None, :]
    assert not bool((must & ~got).any()), (what, torch.nonzero(must & ~got)[:10].tolist())
    assert not bool((got & ~may).any()), (what, torch.nonzero(got & ~may)[:10].tolist())
    if idx.shape[0]:
        assert float((sc.to(torch.float64) - S[qe, idx]).abs().max()) <= 1e-6, what
        same = qe[1:] == qe[:-1]
        ordered = (sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (idx[:-1] < idx[1:]))
        assert bool((ordered | ~same).all()), (what, "order")
    return int(must.sum())


def group_parts_torch(S, groups, allowed=None):
    """_maxsim_checks.group_parts on the device (a 33 x 16.7 M matrix is minutes of numpy): (ids [G] ascending, M [G, n]
    fp64, rows [G, n] int64), the LOWEST row attaining each maximum.  Held against the numpy function where that is cheap."""
    ok = groups >= 0 if allowed is None else (groups >= 0) & allowed
    rows = torch.nonzero(ok)[:, 0]
    ids, inv = torch.unique(groups[rows].to(torch.int64), return_inverse=True)
    n, ng = S.shape[0], ids.shape[0]
    M = torch.empty((ng, n), dtype=S.dtype, device=DEV)
    R = torch.empty((ng, n), dtype=torch.int64, device=DEV)
    for i in range(n):
        s = S[i, rows]
        mx = torch.full((ng,), -np.inf, dtype=S.dtype, device=DEV).scatter_reduce(0, inv, s, "amax", include_self=True)
        first = torch.where(s == mx[inv], rows, torch.full_like(rows, 1 << 62))
        M[:, i] = mx
        R[:, i] = torch.full((ng,), 1 << 62, dtype=torch.int64, device=DEV).scatter_reduce(0, inv, first, "amin", include_self=True)
    return ids, M, R


def check_topk(s, i, c, best_s, best_r, k, d, what=""):
    """One query's top-k (s [k] fp32, i [k] int64, count) against its reference list (best_s fp64 desc, best_r; at least
    k + 1 entries, or every allowed row): every row at least 2 d above the k-th reference score is returned, none is more
    than 2 d below it, each score is within 1e-6 of the fp64 score of ITS row, the order is (score desc, index asc)."""
    n_ref = int((best_r >= 0).sum())
    want = min(k, n_ref)
    assert int(c) == want, (what, int(c), want)
    assert bool((i[want:] == -1).all())
    s, i = s[:want], i[:want]
    assert torch.unique(i).shape[0] == want, what
    r, order = torch.sort(best_r[:n_ref])
    pos = torch.searchsorted(r, i).clamp(max=n_ref - 1)
    assert bool((r[pos] == i).all()), (what, "rows outside the reference's best list", i[r[pos] != i][:10].tolist())
    ref = best_s[:n_ref][order][pos]
    assert float((s.to(torch.float64) - ref).abs().max()) <= 1e-6, (what, float((s.to(torch.float64) - ref).abs().max()))
    if want == k and n_ref > k:
        kth = best_s[k - 1]
        must = best_r[:n_ref][best_s[:n_ref] >= kth + 2 * d]
        assert bool(torch.isin(must, i).all()), (what, "missing", must[~torch.isin(must, i)][:10].tolist())
        assert bool((ref >= kth - 2 * d).all()), what
        assert float(best_s[n_ref - 1]) < float(kth) - 2 * d, (what, "reference list too short")
    else:
        assert bool(torch.isin(best_r[:want], i).all()), what
    assert bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all()), (what, "order")


def check_score_row(s, i, c, score, k, d, exclude=None, allowed=None, what="", tol=None):
    """A top-k over a per-row fp64 score (numpy [rows]; plain, recommend, discover): the must / may bands (2 d) around the
    k-th score, each returned score within 1e-6 (or tol(value)), the order; rows of `exclude` (the formula's jump) are left
    out of every check.  Returns the number of excluded rows among the results."""
    s, i = s.cpu().numpy(), i.cpu().numpy()
    R = score.shape[0]
    ok = np.ones(R, dtype=bool) if allowed is None else allowed
    ex = np.zeros(R, dtype=bool) if exclude is None else exclude
    want = min(k, int(ok.sum()))
    assert int(c) == want and len(set(i[:want].tolist())) == want, (what, int(c), want)
    s, i = s[:want], i[:want]
    assert ok[i].all(), what
    masked = np.where(ok, score, -np.inf)
    kth = np.partition(masked, R - want)[R - want]
    got = np.zeros(R, dtype=bool)
    got[i] = True
    must = (masked >= kth + 2 * d) & ~ex
    assert not (must & ~got).any(), (what, np.nonzero(must & ~got)[0][:10])
    assert not (got & ~ex & (masked < kth - 2 * d)).any(), (what, np.nonzero(got & ~ex & (masked < kth - 2 * d))[0][:10])
    keep = ~ex[i]
    err = np.abs(s[keep].astype(np.float64) - score[i][keep])
    assert (err <= (1e-6 if tol is None else tol(score[i][keep]))).all(), (what, err.max(initial=0.0))
    assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all(), (what, "order")
    return int(ex[i].sum())


def check_range(off, idx, sc, best_s, best_r, t, d, allow=None, what=""):
    """A range search of Q queries against their reference lists, as test_gpu_range_search._check_against_oracle asserts it:
    the CSR layout, no row twice, every allowed row >= t + d returned, none < t - d, each score within 1e-6, the order
    (score desc, index asc).  The lists must reach below t - d (asserted): they then hold every row that may be returned."""
    Q, keep = best_s.shape
    assert off.shape == (Q + 1,) and int(off[0]) == 0 and int(off[-1]) == idx.shape[0] == sc.shape[0], what
    assert bool((off[1:] >= off[:-1]).all())
    n_valid = (best_r >= 0).sum(1)
    assert int(n_valid.min()) >= 1
    last = best_s.gather(1, (n_valid - 1)[:, None])
    assert float(last.max()) < t - d, (what, "reference lists too short for this threshold")
    cnt = off[1:] - off[:-1]
    qe = torch.repeat_interleave(torch.arange(Q, device=DEV), cnt)
    # position of every returned (query, row) in the query's list
    key_ref = (torch.arange(Q, device=DEV)[:, None] << 32 | best_r.clamp(min=0)).reshape(-1)
    valid = (best_r >= 0).reshape(-1)
    key_ref = torch.where(valid, key_ref, torch.full_like(key_ref, -1))
    ks, order = torch.sort(key_ref)
    key_got = qe << 32 | idx
    assert torch.unique(key_got).shape[0] == idx.shape[0], (what, "a row twice")
    pos = torch.searchsorted(ks, key_got).clamp(max=ks.shape[0] - 1)
    assert bool((ks[pos] == key_got).all()), (what, "rows outside the reference lists", idx[ks[pos] != key_got][:10].tolist())
    ref = best_s.reshape(-1)[order][pos]
    ok = torch.ones_like(best_r, dtype=torch.bool) if allow is None else allow[best_r.clamp(min=0)]
    if allow is not None:
        assert bool(allow[idx].all()), (what, "a row the filter does not allow")
    must = (best_s >= t + d) & ok & (best_r >= 0)
    got = torch.zeros(Q * keep, dtype=torch.bool, device=DEV)
    got[order[pos]] = True
    got = got.view(Q, keep)
    assert not bool((must & ~got).any()), (what, "missing", torch.nonzero(must & ~got)[:10].tolist())
    if idx.shape[0]:
        assert bool((ref >= t - d).all()), (what, "below the band")
        assert float((sc.to(torch.float64) - ref).abs().max()) <= 1e-6, what
        same = qe[1:] == qe[:-1]
        ordered = (sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (idx[:-1] < idx[1:]))
        assert bool((ordered | ~same).all()), (what, "order")
    return int(must.sum())


def group_runs(n, seed, marks):
    """group ids int32 [n] (numpy): runs of one to five rows with ascending sparse ids up to 2^31 - 1, every ninth row in no
    group (tests/test_gpu_gallery_edit.py _groups_of); the run over each mark is widened so that it straddles the mark"""
    rng = np.random.default_rng(seed)
    run = np.repeat(np.arange(n, dtype=np.int64), rng.integers(1, 6, size=n))[:n]
    for m in marks:
        if m + 1 < n:
            run[m - 1: m + 2] = run[m - 1]
    n_runs = int(run[-1]) + 1
    step = (2 ** 31 - 1) // n_runs
    ids = np.arange(n_runs, dtype=np.int64) * step
    ids[-1] = 2 ** 31 - 1
    g = ids[run].astype(np.int32)
    g[::9] = -1
    for m in marks:                                                           # (a ninth row must not cut the straddling run)
        if m + 1 < n:
            g[m - 1: m + 2] = ids[run[m - 1]]
    return g


def edit_reference(best_s, best_r, removed=None, new_index=None, extra_rows=None, extra_scores=None):
    """The best lists after an edit of the gallery: the entries of `removed` rows (bool [N], device) dropped, the rows
    renumbered through new_index (int64 [N]), the rows extra_rows [m] with their fp64 scores extra_scores [Q, m] merged in.
    Rows are independent, so the result is what ref_best() gives on the edited rows, down to its last valid entry (the
    lists are padded with -inf / -1)."""
    s, r = best_s.clone(), best_r.clone()
    if removed is not None:
        gone = removed[r.clamp(min=0)] | (r < 0)
        s[gone], r[gone] = -np.inf, -1
    if new_index is not None:
        r = torch.where(r >= 0, new_index[r.clamp(min=0)], r)
    if extra_rows is not None:
        s = torch.cat([s, extra_scores], 1)
        r = torch.cat([r, extra_rows[None, :].expand(s.shape[0], -1)], 1)
    o = torch.argsort(s, dim=1, descending=True, stable=True)[:, :best_s.shape[1]]
    return torch.gather(s, 1, o), torch.gather(r, 1, o)


def planted_pairs(w, t, d, without=()):
    """the pairs (i, j, fp64 score) of planted rows at or above t, ordered by (i, j), leaving out the rows `without`; a
    planted pair inside the band of 2 d around t is an error of the fixture (change the seed)"""
    P = w.planted.to(torch.float64)
    S = (P @ P.T).cpu().numpy()
    rows = w.planted_rows
    want = []
    for a in range(len(rows)):
        for b in range(len(rows)):
            if rows[a] < rows[b] and S[a, b] >= t - 2 * d and rows[a] not in without and rows[b] not in without:
                assert S[a, b] >= t + 2 * d, "a planted pair inside the band: change the seed"
                assert w.site_of[int(rows[a])] == w.site_of[int(rows[b])]
                want.append((int(rows[a]), int(rows[b]), float(S[a, b])))
    return sorted(want)
