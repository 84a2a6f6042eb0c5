"""Every GEMM launch form and epilogue against fp64 with per-element bounds (tests/_kernel_bounds.py GemmF32, GemmResid, GemmRope,
GemmLnIn, LnStats, SplitkResidLn), at the towers' shapes: kb.GEMM_FORM_CASES.

Each case runs on librevo_exp.so, asserts the exact set of launch forms its call issued (revo_debug_gemm_forms) and holds
EVERY element of every output to its bound -- the reference is fp64 on the GPU, in row chunks.  Where the size heuristic
chooses the form (no forced variant), the product library runs the same call and must give the same bits.  A second run
gives the same bits; with `pad`, the NaN margin past N and the rows past M of a padded output stay NaN.  bf16 outputs of a
million or more are also held to the rounding-direction statistic (kb.rounding_bias).  The largest |got - ref| / bound of
each case is printed."""
import ctypes
import time

import pytest
import torch

import _kernel_bounds as kb
import reverso_amd  # noqa: F401
from reverso_amd import _lib

pytestmark = pytest.mark.gpu

EPI = {"bf16": 0, "gelu": 1, "resid": 2, "f32": 3}
CHUNK_ELEMS = 1 << 25                  # rows per fp64 chunk: CHUNK_ELEMS / max(N, K)


@pytest.fixture(scope="module")
def plib():
    return _lib.load()


@pytest.fixture(scope="module")
def xlib():
    return _lib.load_exp()


def _sync():
    torch.cuda.synchronize()


def _case_data(kind, M, N, K, opts, dev):
    """(GemmCase on the device, tower dict or None)"""
    seed = M + 7 * N + 3 * K
    t = kb.TOWERS.get(opts.get("tower", ""))
    if kind.startswith("ln_in"):
        epi = "rope" if kind == "ln_in_rope" else kind.split(":")[1]
        rope = epi == "rope"
        return kb.ln_in_case(M, N, K, seed, epi, dev, S=t["S"] if t else 1, hd=t["hd"] if t else 64,
                             rope_cols=2 * t["W"] if rope else 0, cs=kb.tower_rope(opts["tower"]).to(dev) if rope else None), t
    if kind.startswith("resid"):
        planes = kind.split(":")[1] if ":" in kind else "none"
        return kb.resid_case(M, N, K, seed, dev, planes_in=planes in ("in", "inout"), ksplit=opts.get("ksplit", 1)), t
    c = kb.plain_case(M, N, K, seed, dev)
    if kind == "rope":
        c = c.with_(cs=kb.tower_rope(opts["tower"]).to(dev), S=t["S"], hd=t["hd"], rope_cols=2 * t["W"])
    return c, t


def _run(lib, kind, c, M, N, K, opts):
    """one call of the op on `lib`; returns the outputs (dict of device tensors)"""
    dev = c.a.device
    st = _lib.current_stream()
    P = _lib.ptr
    pad = 64 if opts.get("pad") else 0
    out = {}
    if kind in ("f32", "bf16", "gelu", "rope") or kind.startswith("ln_in"):
        dt = torch.float32 if kind == "f32" else torch.bfloat16
        buf = torch.full((M + pad, N + pad), float("nan"), device=dev, dtype=dt)
        ldc = N + pad
        if kind == "rope":
            rc = lib.revo_op_gemm_rope(P(c.a), K, P(c.b), K, M, N, K, P(buf), ldc, P(c.bias), P(c.cs), c.S, c.hd, c.rope_cols, st)
        elif kind == "ln_in_rope":
            rc = lib.revo_op_gemm_ln_in_rope(P(c.a), K, P(c.b), K, M, N, K, P(buf), ldc, P(c.bias), P(c.csum), P(c.stats),
                                             c.stats.shape[1], c.eps, P(c.cs), c.S, c.hd, c.rope_cols, st)
        elif kind.startswith("ln_in"):
            rc = lib.revo_op_gemm_ln_in(EPI[c.epi], P(c.a), K, P(c.b), K, M, N, K, P(buf), ldc, P(c.bias), P(c.csum),
                                        P(c.stats), c.stats.shape[1], c.eps, None, st)
        else:
            rc = lib.revo_op_gemm(EPI[kind], P(c.a), K, P(c.b), K, M, N, K, P(buf), ldc, P(c.bias), None, st)
        _lib.check(rc, kind)
        out["c"] = buf
        return out
    cbuf = c.x.clone()
    if kind == "resid":
        _lib.check(lib.revo_op_gemm(2, P(c.a), K, P(c.b), K, M, N, K, P(cbuf), N, P(c.bias), P(c.gamma), st), kind)
        out["x"] = cbuf
        return out
    if kind == "resid_norm":
        h = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
        fused = ctypes.c_int32(-1)
        _lib.check(lib.revo_op_gemm_resid_norm(P(c.a), K, P(c.b), K, M, N, K, P(cbuf), N, P(c.bias), P(c.gamma), P(h), N, c.eps,
                                               ctypes.byref(fused), st), kind)
        _sync()
        assert fused.value == 1, f"the LayerNorm was not fused (*fused = {fused.value})"
        out["x"], out["h"] = cbuf, h
        return out
    planes = kind.split(":")[1]
    pin, pout = planes in ("in", "inout"), planes in ("out", "inout")
    xb = c.hi.clone() if pin else torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
    xlo = c.lo.clone() if pin else (torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16) if pout else None)
    stats = None if planes == "in" else torch.full((M, N // 256, 2), float("nan"), device=dev)
    done = ctypes.c_int32(-1)
    _lib.check(lib.revo_op_gemm_resid_ln(P(c.a), K, P(c.b), K, M, N, K, P(cbuf), N, P(c.bias), P(c.gamma), P(xb), N, P(stats),
                                         ctypes.byref(done), P(xlo), int(pin), int(pout), st), kind)
    _sync()
    assert done.value == (0 if planes == "in" else 1), f"*done = {done.value}"
    out["x"], out["xb"] = cbuf, xb
    if xlo is not None:
        out["lo"] = xlo
    if stats is not None:
        out["stats"] = stats
    return out


def _chunked(c, M, width, fn):
    """max over row chunks of fn(sub-case, r0, r1)"""
    step = max(64, CHUNK_ELEMS // width)
    worst = 0.0
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        worst = max(worst, fn(c.rows(r0, r1), r0, r1))
    return worst


def _check(kind, c, out, M, N, K, opts, label):
    """{name: max ratio} of every output of the case"""
    ratios = {}
    width = max(N, K)
    if kind in ("f32", "bf16", "gelu"):
        got = out["c"][:M, :N]
        if kind == "f32":
            ratios["c"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(got[a:b], kb.GemmF32.reference(s), kb.GemmF32.bound(s)))
        else:
            g = kind == "gelu"
            ratios["c"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(got[a:b], kb.GemmBf16.reference(s.a, s.b, s.bias, g),
                                                                      kb.GemmBf16.bound(s.a, s.b, s.bias, g)))
    elif kind == "rope":
        got = out["c"][:M, :N]
        ratios["c"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(got[a:b], kb.GemmRope.reference(s), kb.GemmRope.bound(s)))
    elif kind.startswith("ln_in"):
        got = out["c"][:M, :N]
        ratios["c"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(got[a:b], kb.GemmLnIn.reference(s), kb.GemmLnIn.bound(s)))
    elif kind == "resid" or kind == "resid_norm":
        x = out["x"]
        ratios["x"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(x[a:b], kb.GemmResid.reference(s), kb.GemmResid.bound(s)))
        if kind == "resid_norm":
            H = kb.SplitkResidLn
            ratios["h"] = kb.ratio(out["h"], H.h_reference(x, c.eps), H.h_bound(x, c.eps))
    else:
        planes = kind.split(":")[1]
        pout = planes in ("out", "inout")
        if pout:
            xnew = out["xb"].double() + out["lo"].double()
            assert kb.planes_ok(out["xb"], out["lo"]), "|lo| > ulp_bf16(hi) / 2"
        else:
            xnew = out["x"].double()
            if planes == "none":                                   # the bf16 copy is bf16(x_new), bit for bit
                assert torch.equal(out["xb"], out["x"].bfloat16()), "xb != bf16(x_new)"
        ratios["x"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(xnew[a:b], kb.GemmResid.reference(s),
                                                                    kb.GemmResid.bound(s, pout)))
        if "stats" in out:
            L = kb.LnStats
            ratios["stats"] = _chunked(c, M, width, lambda s, a, b: kb.ratio(out["stats"][a:b], L.reference(xnew[a:b]),
                                                                            L.bound(xnew[a:b], pout)))
    if "c" in out and out["c"].dtype == torch.bfloat16 and M * N >= kb.ROUNDING_MIN_OUTPUTS:
        got = out["c"][:M, :N]
        ref_fn = {"rope": kb.GemmRope.reference}.get(kind)
        step = max(64, CHUNK_ELEMS // width)
        tot, cnt = 0.0, 0
        for r0 in range(0, M, step):
            s = c.rows(r0, min(M, r0 + step))
            if kind.startswith("ln_in"):
                ref = kb.GemmLnIn.reference(s)
            elif ref_fn:
                ref = ref_fn(s)
            else:
                ref = kb.GemmBf16.reference(s.a, s.b, s.bias, kind == "gelu")
            m, n = kb.rounding_bias(got[r0:r0 + s.a.shape[0]], ref)
            tot, cnt = tot + m * n, cnt + n
        if cnt >= kb.ROUNDING_MIN_OUTPUTS:
            ratios["rounding bias / limit"] = abs(tot / cnt) / kb.ROUNDING_BIAS_MAX
    return ratios


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _equal_bits(a, b):
    bad = [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]
    return bad


@pytest.mark.parametrize("case", kb.GEMM_FORM_CASES, ids=[c[0] for c in kb.GEMM_FORM_CASES])
def test_gemm_within_bound(plib, xlib, dev, case):
    label, kind, M, N, K, opts, want = case
    t0 = time.time()
    c, _ = _case_data(kind, M, N, K, opts, dev)
    forced = "variant" in opts or "qstores" in opts
    try:
        if "variant" in opts:
            xlib.revo_op_set_variant(opts["variant"])
        if "qstores" in opts:
            xlib.revo_op_set_qstores(opts["qstores"])
        _sync()
        xlib.revo_debug_gemm_forms(1)
        out = _run(xlib, kind, c, M, N, K, opts)
        _sync()
        forms = kb.form_names(xlib.revo_debug_gemm_forms(1))
        again = _run(xlib, kind, c, M, N, K, opts)
        _sync()
    finally:
        xlib.revo_op_set_variant(0)
        xlib.revo_op_set_qstores(1)
    t_run = time.time() - t0
    assert forms == sorted(want), f"launch forms {forms}, expected {sorted(want)}"
    bad = _equal_bits(out, again)
    assert not bad, f"a second run changed {bad}"
    if opts.get("pad"):
        buf = out["c"]
        assert torch.isnan(buf[:, N:].float()).all() and torch.isnan(buf[M:].float()).all(), "the padding was written"
    if not forced:
        prod = _run(plib, kind, c, M, N, K, opts)
        _sync()
        bad = _equal_bits(out, prod)
        assert not bad, f"librevo.so differs from librevo_exp.so in {bad}"
    t1 = time.time()
    ratios = _check(kind, c, out, M, N, K, opts, label)
    _sync()
    worst = max(ratios.values())
    print(f"[gemm {label}] forms {'+'.join(forms)}: max |got - ref| / bound = {worst:.3f} ("
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f"); run {t_run:.1f} s, fp64 check {time.time() - t1:.1f} s")
    assert worst <= 1.0, (label, ratios)
