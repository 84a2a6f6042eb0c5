"""The bf16 scan's own sums against fp64: reference, bound and checks shared by tests/test_gpu_search_widths.py (the
kernels, on the GPU) and tests/test_scan_bounds_teeth.py (planted main-loop errors, on the CPU).  torch only, any device.

A gallery without the fp32 master copy (keep_f32 = 0) returns the scan's scores as they are.  With qb / gb the bf16
roundings of the fp32-normalised query and gallery row, every product qb[d] * gb[d] is exact in fp32 (8 x 8 significant
bits), so a scan score differs from the fp64 dot product only by its D fp32 additions:

    |s - qb . gb| <= D * 2^-23 * ||qb|| * ||gb||

which is cert_eps's gam1 term (revers-o_amd/csrc/kernels.h: the MFMA chain's accumulation, truncation allowed).  A K-tile
left out, added twice or multiplied against the wrong columns moves a score by about 8 / D (64 products of size 1 / D)
against a bound of D 2^-23: some 10^4 times the bound at D = 128, some 30 times at D = 2112."""
import torch

# K-tiles of 64: 2 (one trip of the two-tile loop, no tail), 3 (the smallest peeled tail), 5 (a trip with refills, then the
# tail), 33 (odd, and past the 2048 elements the normalisation kernel holds in registers)
W = (128, 192, 320, 2112)
TILE = 64
N_SCAN256 = 20_037            # above SEARCH_SMALL_ROWS = 16 384 (the 256 x 256 scan), ragged last gallery tile
N_SMALL = 3_000               # the small-gallery scan (the gemm_core.h ring)
Q_MAX = 300


def rows(N, D, device="cpu"):
    """the gallery of (N, D): standard-normal fp32 rows, the same on every device (drawn on the host)"""
    g = torch.Generator().manual_seed(1000 * D + N)
    return torch.randn(N, D, generator=g).to(device)


def queries(D, device="cpu", Q=Q_MAX):
    """the queries of D: the first Q of Q_MAX standard-normal fp32 rows"""
    g = torch.Generator().manual_seed(77 * D + 1)
    return torch.randn(Q_MAX, D, generator=g)[:Q].to(device)


def allow_mask(N, D, device="cpu", frac=0.5):
    g = torch.Generator().manual_seed(3 * N + D + int(frac * 1000))
    return (torch.rand(N, generator=g) < frac).to(device)


def bf16_round(x):
    """fp32 -> bf16 (round to nearest even, as the kernels' conversion) -> fp32"""
    return x.float().bfloat16().float()


def reference(qb, gb, chunk=4096):
    """fp64 dot products [Q, N] of the bf16-rounded rows, in row chunks"""
    q = qb.double()
    return torch.cat([q @ gb[r0:r0 + chunk].double().T for r0 in range(0, gb.shape[0], chunk)], dim=1)


def bound(qb, gb):
    """D * 2^-23 * ||qb|| * ||gb|| per (query, row), fp64"""
    D = qb.shape[1]
    return D * 2.0 ** -23 * qb.double().norm(dim=1)[:, None] * gb.double().norm(dim=1)[None, :]


def returned_ratio(scores, indices, ref, bnd):
    """per query: the largest |s - ref| / bound over the entries a search returned (index -1 = padding; none: 0)"""
    ok = indices >= 0
    idx = indices.clamp(min=0)
    r = (scores.double() - ref.gather(1, idx)).abs() / bnd.gather(1, idx)
    return torch.where(ok, r, torch.zeros_like(r)).max(dim=1).values


def topk_ratio(s_all, k, ref, bnd):
    """per query: returned_ratio of the top-k of a full score matrix (what a search over these scores would return)"""
    s, i = torch.sort(s_all, dim=1, descending=True, stable=True)
    return returned_ratio(s[:, :k], i[:, :k], ref, bnd)


def check_topk(scores, indices, counts, ref, bnd, k, allow=None):
    """The result of a top-k search by scan scores (scores [Q, k], indices [Q, k] padded with -1, counts [Q]) against
    the fp64 reference: every returned score within its bound; counts equal; the index set equal to the reference
    top-k's (score desc, index asc, allowed rows only) except for rows whose reference score lies within twice their
    bound of the k-th reference score.  Returns the per-query score ratios."""
    Q, N = ref.shape
    r = ref if allow is None else torch.where(allow[None, :], ref, torch.full_like(ref, float("-inf")))
    n_ok = N if allow is None else int(allow.sum())
    want = min(k, n_ok)
    assert torch.equal(counts.long().cpu(), torch.full((Q,), want, dtype=torch.long)), (counts, want)
    assert bool((indices[:, :want] >= 0).all()) and bool((indices[:, want:] == -1).all())
    assert bool((indices < N).all())
    if allow is not None:
        assert bool(allow[indices[:, :want].reshape(-1)].all()), "a row outside the filter was returned"
    ratios = returned_ratio(scores, indices, ref, bnd)
    assert float(ratios.max()) <= 1.0, float(ratios.max())
    rs, ri = torch.sort(r, dim=1, descending=True, stable=True)
    kth = rs[:, want - 1]
    got = torch.zeros(Q, N, dtype=torch.bool, device=ref.device)
    got.scatter_(1, indices[:, :want], True)
    assert bool((got.sum(1) == want).all()), "a row was returned twice"
    exp = torch.zeros_like(got)
    exp.scatter_(1, ri[:, :want], True)
    diff = got ^ exp
    near = (ref - kth[:, None]).abs() <= 2.0 * bnd
    bad = diff & ~near
    assert not bool(bad.any()), ("index sets differ beyond the bound", bad.nonzero()[:8].tolist())
    assert bool((scores[:, :want - 1] >= scores[:, 1:want]).all()), "scores not sorted"
    return ratios


# ------------------------------------------------------------------ emulations (fp32, strict left to right) ----
def fp32_chain(qb, gb, qcols, gcols):
    """sum over j of qb[:, qcols[j]] * gb[:, gcols[j]] accumulated in fp32, one rounding per addition, in list order"""
    acc = torch.zeros(qb.shape[0], gb.shape[0], dtype=torch.float32, device=qb.device)
    gt = gb.float().T.contiguous()
    q = qb.float()
    for a, b in zip(qcols, gcols):
        acc = acc + q[:, a:a + 1] * gt[b:b + 1, :]           # the product of two bf16 values is exact in fp32
    return acc


def emulate(qb, gb, what):
    """what: "chain" (the correct sum), "last tile left out", "last tile added twice", "last tile from the previous
    tile's gallery columns" (a stale LDS stage)"""
    D = qb.shape[1]
    cols = list(range(D))
    last = list(range(D - TILE, D))
    if what == "chain":
        return fp32_chain(qb, gb, cols, cols)
    if what == "last tile left out":
        return fp32_chain(qb, gb, cols[:D - TILE], cols[:D - TILE])
    if what == "last tile added twice":
        return fp32_chain(qb, gb, cols + last, cols + last)
    if what == "last tile from the previous tile's gallery columns":
        return fp32_chain(qb, gb, cols, cols[:D - TILE] + [c - TILE for c in last])
    raise ValueError(what)


PLANTED = ("last tile left out", "last tile added twice", "last tile from the previous tile's gallery columns")
