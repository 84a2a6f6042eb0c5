"""The fp32 attention-pool head's kernels against fp64 with per-element bounds derived from their rounding
(tests/_head_bounds.py): probe_qk_kernel, layernorm_kernel / layernorm_logits_kernel with the pool's logits,
pool_accumulate_kernel, pool_accumulate_masked_kernel and gemm_f32_skinny_kernel, each through the C ABI of the product library
at the smallest shapes that reach every launch form and edge (tests/test_head_bounds_teeth.py asserts that they do).
|got - ref| <= bound everywhere; the largest |got - ref| / bound of each case is printed.  Padding columns of the inputs hold
NaN and change nothing; padding columns and guard rows of the outputs keep their sentinel; the bit-for-bit contracts of
include/revo.h hold across the forms reached here."""
import pytest
import torch

import _head_bounds as hb
import reverso_amd  # noqa: F401
from reverso_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def plib():
    return _lib.load()


def _report(op, label, r):
    print(f"[{op} {label}] max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0, (op, label, r)


def _padded(t, ld):
    """t [rows, cols] in a [rows, ld] buffer whose other columns are NaN"""
    buf = torch.full((t.shape[0], ld), float("nan"), device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def _guarded(rows, cols, ld, dev):
    """([rows + 2, ld] of SENTINEL, its middle rows): a guard row on either side, padding columns from cols on"""
    buf = torch.full((rows + 2, ld), SENTINEL, device=dev)
    return buf, buf[1:rows + 1]


def _untouched(buf, cols):
    return bool((buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all() and (buf[1:-1, cols:] == SENTINEL).all())


# ------------------------------------------------------------------ probe ----
@pytest.mark.parametrize("W,heads", hb.PROBE_CASES)
def test_probe_qk_within_bound(plib, dev, W, heads):
    q, Wk, bk = hb.probe_inputs(W, heads, dev)
    qbuf, qk = _guarded(heads, W, W, dev)
    cbuf, ck = _guarded(1, heads, heads, dev)
    _lib.check(plib.revo_op_probe_qk(_lib.ptr(q), _lib.ptr(Wk), _lib.ptr(bk), W, heads, _lib.ptr(qk), _lib.ptr(ck),
                                     _lib.current_stream()))
    torch.cuda.synchronize()
    assert _untouched(qbuf, W) and _untouched(cbuf, heads)
    P = hb.ProbeQk
    (rqk, rck), (bqk, bck) = P.reference(q, Wk, bk, heads), P.bound(q, Wk, bk, heads)
    _report("probe qk", f"W{W} heads{heads}", hb.ratio(qk, rqk, bqk))
    _report("probe ck", f"W{W} heads{heads}", hb.ratio(ck[0], rck, bck))


def test_probe_qk_refuses_heads_that_do_not_divide_the_width(plib, dev):
    t = torch.zeros(64, device=dev)
    rc = plib.revo_op_probe_qk(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 8, 3, _lib.ptr(t), _lib.ptr(t), _lib.current_stream())
    assert rc == -2 and b"multiple of heads" in plib.revo_last_error()
    assert plib.revo_op_probe_qk(None, _lib.ptr(t), _lib.ptr(t), 8, 2, _lib.ptr(t), _lib.ptr(t), _lib.current_stream()) == -2


# ------------------------------------------------------------------ pooled rows ----
def _pool(plib, x, lg, pad=0):
    """revo_op_pool_rows on x [B, S, W] laid out with ldx = W + pad (NaN in the padding), u between guard rows"""
    B, S, W = x.shape
    H = lg.shape[1]
    xb = _padded(x.reshape(B * S, W), W + pad)
    ubuf, u = _guarded(B * H, W, W, x.device)
    _lib.check(plib.revo_op_pool_rows(_lib.ptr(xb), W + pad, _lib.ptr(lg), B, S, W, H, _lib.ptr(u), _lib.current_stream()))
    torch.cuda.synchronize()
    assert _untouched(ubuf, W)
    return u.view(B, H, W).clone()


@pytest.mark.parametrize("spec", hb.POOL_CASES, ids=hb.pool_id)
def test_pool_rows_within_bound(plib, dev, spec):
    x, lg = hb.pool_inputs(spec, dev)
    B = spec["B"]
    u = _pool(plib, x, lg, spec["pad"])
    P = hb.PoolRows
    _report("pool", hb.pool_id(spec), hb.ratio(u, P.reference(x, lg), P.bound(x, lg)))
    for b in sorted({0, B // 2, B - 1}):                         # an image alone (the narrow form) = its image in the batch
        assert torch.equal(_pool(plib, x[b:b + 1], lg[b:b + 1].contiguous())[0], u[b]), b


def test_pool_rows_refuses_a_probability_table_beyond_lds(plib, dev):
    """H = 16, S = 2300 in the four-column form: the H S probabilities and 64 KB of partial sums pass the 160 KB of LDS: a
    status and no launch.  (The one-column form's 163 584 bytes still fit: it is the batch that is refused.)"""
    B, S, W, H = hb.POOL_REFUSED
    x = torch.zeros(B * S, W, device=dev)
    lg = torch.zeros(B, H, S, device=dev)
    ubuf, u = _guarded(B * H, W, W, dev)
    rc = plib.revo_op_pool_rows(_lib.ptr(x), W, _lib.ptr(lg), B, S, W, H, _lib.ptr(u), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -2 and b"sequence too long" in plib.revo_last_error()
    assert (ubuf == SENTINEL).all()


def _pool_masked(plib, x, lg, ri, allow, pad=0):
    B, S, W = x.shape
    H, R = lg.shape[1], ri.shape[0]
    xb = _padded(x.reshape(B * S, W), W + pad)
    ubuf, u = _guarded(R * H, W, W, x.device)
    bits = hb.pack_bits(allow).to(x.device)
    _lib.check(plib.revo_op_pool_rows_masked(_lib.ptr(xb), W + pad, _lib.ptr(lg), _lib.ptr(ri.to(torch.int32).to(x.device)),
                                             _lib.ptr(bits), R, B, S, W, H, _lib.ptr(u), _lib.current_stream()))
    torch.cuda.synchronize()
    assert _untouched(ubuf, W)
    return u.view(R, H, W).clone()


@pytest.mark.parametrize("spec", hb.MASKED_CASES, ids=lambda s: hb.pool_id(s) + f" R{s['R']}")
def test_masked_pool_rows_within_bound(plib, dev, spec):
    x, lg = hb.pool_inputs(spec, dev)
    ri, allow = hb.masked_regions(spec)
    u = _pool_masked(plib, x, lg, ri, allow, spec["pad"])
    P = hb.PoolRows
    ref, bound = P.reference(x, lg, (ri, allow)), P.bound(x, lg, (ri, allow))
    for r, kind in enumerate(hb.REGION_KINDS):
        print(f"[masked pool {hb.pool_id(spec)} region {kind}] max |got - ref| / bound = {hb.ratio(u[r], ref[r], bound[r]):.3f}")
    _report("masked pool", hb.pool_id(spec) + f" R{spec['R']}", hb.ratio(u, ref, bound))
    full, empty, one = (hb.REGION_KINDS.index(k) for k in ("all tokens", "empty", "one token"))
    assert torch.equal(u[full], _pool(plib, x, lg)[int(ri[full])])                  # a full mask = the unmasked pool, bit for bit
    assert torch.equal(u[empty], torch.zeros_like(u[empty]))
    s = int(torch.nonzero(allow[one])[0])
    assert torch.equal(u[one], x[int(ri[one]), s].expand(spec["H"], -1))
    for r in (one, full, 6, spec["R"] - 1):                                    # a region alone (the narrow form) = in the call
        assert torch.equal(_pool_masked(plib, x, lg, ri[r:r + 1], allow[r:r + 1])[0], u[r]), r


# ------------------------------------------------------------------ ln_post + logits ----
def _ln(plib, x, w, b, qk, ck, S, pads=(0, 0)):
    rows, W = x.shape
    H = qk.shape[0]
    xb = _padded(x, W + pads[0])
    obuf, out = _guarded(rows, W, W + pads[1], x.device)
    lbuf, lg = _guarded(1, rows * H, rows * H, x.device)
    _lib.check(plib.revo_op_layernorm_logits(_lib.ptr(xb), W + pads[0], _lib.ptr(w), _lib.ptr(b), hb.LN_EPS, rows, W, _lib.ptr(out),
                                             W + pads[1], _lib.ptr(qk), _lib.ptr(ck), H, S, _lib.ptr(lg), _lib.current_stream()))
    torch.cuda.synchronize()
    assert _untouched(obuf, W) and _untouched(lbuf, rows * H)
    return out[:, :W].clone(), lg.view(rows // S, H, S).clone()


@pytest.mark.parametrize("spec", hb.LN_CASES, ids=hb.ln_id)
def test_ln_logits_within_bound(plib, dev, spec):
    x, w, b, qk, ck = hb.ln_inputs(spec, dev)
    B, S, W, H = spec["B"], spec["S"], spec["W"], spec["H"]
    out, lg = _ln(plib, x, w, b, qk, ck, S, spec["pads"])
    L = hb.LnLogits
    (ry, rlg), (by, blg) = L.reference(x, w, b, hb.LN_EPS, qk, ck, S), L.bound(x, w, b, hb.LN_EPS, qk, ck, S)
    _report("ln rows", hb.ln_id(spec), hb.ratio(out, ry, by))
    _report("ln logits", hb.ln_id(spec), hb.ratio(lg, rlg, blg))
    if B * S < 4096:
        return
    # every image on its own takes the one-row-per-wave form: the same bits, whichever form the batch took
    o1, l1 = torch.full_like(out, SENTINEL), torch.full_like(lg, SENTINEL)
    for i in range(B):
        _lib.check(plib.revo_op_layernorm_logits(_lib.ptr(x[i * S:]), W, _lib.ptr(w), _lib.ptr(b), hb.LN_EPS, S, W, _lib.ptr(o1[i * S:]), W,
                                                 _lib.ptr(qk), _lib.ptr(ck), H, S, _lib.ptr(l1[i]), _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(o1, out) and torch.equal(l1, lg)


# ------------------------------------------------------------------ skinny fp32 GEMM ----
def _linear(plib, c, pads=(0, 0, 0)):
    """the case through revo_op_linear_f32 (or _grouped: the groups' K columns side by side in a row of A, a_group_stride
    = K), operands with NaN padding, C between guard rows with SENTINEL padding"""
    M, N, K = c.a.shape[0], c.w.shape[0], c.K
    lda, ldw, ldc = c.a.shape[1] + pads[0], K + pads[1], N + pads[2]
    ab, wb = _padded(c.a, lda), _padded(c.w, ldw)
    cbuf, C = _guarded(M, N, ldc, c.a.device)
    C[:, :N] = c.c0
    st = _lib.current_stream()
    if c.group_cols:
        rc = plib.revo_op_linear_f32_grouped(c.epi, _lib.ptr(ab), lda, K, c.group_cols, _lib.ptr(wb), ldw, _lib.ptr(c.bias), M, N, K,
                                             _lib.ptr(C), ldc, st)
    else:
        rc = plib.revo_op_linear_f32(c.epi, _lib.ptr(ab), lda, _lib.ptr(wb), ldw, _lib.ptr(c.bias), M, N, K, _lib.ptr(C), ldc, st)
    _lib.check(rc)
    torch.cuda.synchronize()
    assert _untouched(cbuf, N)
    return C[:, :N].clone()


@pytest.mark.parametrize("spec", hb.LINEAR_CASES, ids=hb.linear_id)
def test_linear_f32_within_bound(plib, dev, spec):
    c = hb.linear_case(spec, dev)
    M = spec["M"]
    got = _linear(plib, c, spec["pads"])
    G = hb.LinearF32
    _report("linear", hb.linear_id(spec), hb.ratio(got, G.reference(c), G.bound(c)))
    for r in sorted({r for r in hb.LINEAR_ALONE_ROWS + (M - 1,) if r < M}):       # a row alone (M = 1) = its row in the batch
        assert torch.equal(_linear(plib, c.rows(r, r + 1))[0], got[r]), r


def test_linear_f32_grouped_equals_the_plain_op_group_by_group(plib, dev):
    """group g's columns are revo_op_linear_f32 on group g's rows of A and rows of W, bit for bit; the launcher's grouping
    refusals come through as statuses"""
    spec = dict(M=17, N=48, K=32, epi=1, fixture="randn", bias=True, pads=(0, 0, 0), group_cols=16)
    c = hb.linear_case(spec, dev)
    got = _linear(plib, c)
    for g in range(3):
        cols = slice(g * 16, (g + 1) * 16)
        one = hb.LinearCase(c.a[:, g * 32:(g + 1) * 32].contiguous(), c.w[cols], c.bias[cols], c.c0[:, cols].contiguous(), 1)
        assert torch.equal(_linear(plib, one), got[:, cols]), g
    p, st = _lib.ptr, _lib.current_stream()
    C = torch.zeros(17, 48, device=dev)
    assert plib.revo_op_linear_f32_grouped(0, p(c.a), 96, 32, 8, p(c.w), 32, None, 17, 48, 32, p(C), 48, st) == -2
    assert b"bad A grouping" in plib.revo_last_error()
    assert plib.revo_op_linear_f32_grouped(0, p(c.a), 96, 30, 16, p(c.w), 32, None, 17, 48, 32, p(C), 48, st) == -2
    torch.cuda.synchronize()
    assert not C.any()
