"""The embed kernels against fp64 with per-element bounds derived from their rounding (tests/_kernel_bounds.py): attention,
RoPE, LayerNorm, the fp32 -> bf16 conversion and the GEMM's bf16 epilogues, each called through the C ABI of the product
library at the shapes the towers run.  |got - ref| <= bound everywhere; the largest |got - ref| / bound of each case is
printed.  (A module of its own: test_gpu_kernels.py runs every test once per GEMM tile, which none of these depend on.)"""
import pytest
import torch

import _kernel_bounds as kb
import reverso_amd  # noqa: F401
from reverso_amd import _lib

pytestmark = pytest.mark.gpu

EPI_BF16, EPI_BF16_GELU = 0, 1


@pytest.fixture(scope="module")
def plib():
    return _lib.load()


def _report(op, label, r):
    print(f"[{op} {label}] max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0, (op, label, r)


@pytest.mark.parametrize("case", kb.ATTENTION_CASES, ids=[c[0] for c in kb.ATTENTION_CASES])
def test_attention_within_bound(plib, dev, case):
    label, B, S, H, hd, ld, ldo = case
    W = H * hd
    ld, ldo = ld or 3 * W, ldo or W
    qkv = kb.attention_qkv(B, S, H, hd, ld).to(dev)
    out = torch.full((B * S, ldo), float("nan"), device=dev, dtype=torch.bfloat16)
    _lib.check(plib.revo_op_attention(_lib.ptr(qkv), ld, _lib.ptr(out), ldo, B, S, H, hd, _lib.current_stream()))
    torch.cuda.synchronize()
    if ldo > W:                                                   # the columns past W belong to someone else
        assert torch.isnan(out[:, W:].float()).all()
    worst = 0.0
    for b in range(B):                                            # the fp64 reference image by image (L14 b64: 1024 pairs)
        rows = slice(b * S, (b + 1) * S)
        q, k, v = kb.attention_split(qkv[rows], 1, S, H, hd)
        got = kb.attention_unsplit(out[rows], 1, S, H, hd)
        worst = max(worst, kb.ratio(got, kb.Attention.reference(q, k, v), kb.Attention.bound(q, k, v)))
    _report("attention", label, worst)


@pytest.mark.parametrize("case", kb.ATTENTION_HDR_CASES, ids=[c["label"] for c in kb.ATTENTION_HDR_CASES])
def test_attention_hdr_within_bound(plib, dev, case):
    """The planted high-dynamic-range inputs (kb.ATTENTION_HDR_CASES): the optimistic softmax's reference moves late, more
    than once, for one row of a wave with its 31 mates rescaling accumulators that still count, or not at all with l near
    2^75 -- the path each head takes is asserted on the CPU (tests/test_kernel_bounds_teeth.py).  Every output finite and
    within the fp64 per-element bound, every (image, head) pair."""
    B, S, H, hd = case["B"], case["S"], case["H"], case["hd"]
    W = H * hd
    qkv = kb.attention_hdr_qkv(case).to(dev)
    out = torch.full((B * S, W), float("nan"), device=dev, dtype=torch.bfloat16)
    _lib.check(plib.revo_op_attention(_lib.ptr(qkv), 3 * W, _lib.ptr(out), W, B, S, H, hd, _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    q, k, v = kb.attention_split(qkv, B, S, H, hd)
    got = kb.attention_unsplit(out, B, S, H, hd)
    ref, bound = kb.Attention.reference(q, k, v), kb.Attention.bound(q, k, v)
    for h in range(H):
        pairs = [b * H + h for b in range(B)]
        print(f"[attention hdr {case['label']} h{h}] max |got - ref| / bound = {kb.ratio(got[pairs], ref[pairs], bound[pairs]):.3f}")
    _report("attention hdr", case["label"], kb.ratio(got, ref, bound))


@pytest.mark.parametrize("case", kb.ROPE_CASES, ids=[c[0] for c in kb.ROPE_CASES])
def test_rope_within_bound(plib, dev, case):
    label, grid, H, hd, cls, B = case
    W = H * hd
    cs = kb.rope_table(grid, hd, cls)
    qkv0, S = kb.rope_qkv(grid, H, hd, cls, B)
    qkv = qkv0.to(dev)
    _lib.check(plib.revo_op_rope(_lib.ptr(qkv), 3 * W, _lib.ptr(cs.to(dev)), B * S, S, W, H, _lib.current_stream()))
    torch.cuda.synchronize()
    got = qkv.cpu()
    assert torch.equal(got[:, 2 * W:], qkv0[:, 2 * W:])           # v untouched, bit for bit
    worst = 0.0
    for which in (0, 1):
        x = kb.rope_heads(qkv0, B, S, H, hd, which)
        worst = max(worst, kb.ratio(kb.rope_heads(got, B, S, H, hd, which), kb.Rope.reference(x, cs), kb.Rope.bound(x, cs)))
    _report("rope", label, worst)


@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("W", kb.LAYERNORM_WIDTHS)
def test_layernorm_within_bound(plib, dev, W, out_bf16):
    x, w, b = kb.layernorm_rows(W, out_bf16)
    rows, eps = x.shape[0], 1e-5
    assert rows % 4 != 0
    out = torch.full((rows, W), float("nan"), device=dev, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    _lib.check(plib.revo_op_layernorm(_lib.ptr(xd), W, _lib.ptr(wd), _lib.ptr(bd), eps, rows, W, _lib.ptr(out), W, out_bf16,
                                      _lib.current_stream()))
    torch.cuda.synchronize()
    L = kb.LayerNorm
    _report("layernorm", f"W{W} {'bf16' if out_bf16 else 'fp32'}",
            kb.ratio(out, L.reference(xd, wd, bd, eps), L.bound(xd, wd, bd, eps, out_bf16)))
    const = int(torch.nonzero((x == x[:, :1]).all(1))[0])        # a constant row normalises to exactly the bias
    assert torch.equal(out[const].float().cpu(), b.bfloat16().float() if out_bf16 else b)


@pytest.mark.parametrize("cols,ld_src", [(64, 64), (64, 65), (61, 64), (45, 47)],
                         ids=["aligned", "odd ld_src", "ragged cols", "ragged cols, odd ld_src"])
def test_f32_to_bf16_is_round_to_nearest_even(plib, dev, cols, ld_src):
    """Bit for bit against torch's round-to-nearest-even .bfloat16() for every special class (+-0, fp32 subnormals, +-inf,
    NaN, ties rounding down and up, values rounding up to inf), in the 16-byte aligned path and in the scalar path (odd
    ld_src: rows past the first are misaligned; cols not a multiple of 8: the last chunk).  Columns cols .. ld_dst - 1 are
    written as zeros.  fp32 subnormals are converted, not flushed: the conversion keeps bf16's subnormal range."""
    specials = kb.f32_from_bits(kb.f32_special_values())
    ld_dst = (cols + 7) // 8 * 8 + 8
    rows = 9
    g = torch.Generator(device="cpu").manual_seed(cols + ld_src)
    src = torch.randn(rows, ld_src, generator=g) * torch.exp2(torch.randint(-30, 30, (rows, ld_src), generator=g).float())
    for r in range(rows):                                          # every row holds every special, at a different offset
        idx = (torch.arange(len(specials)) * 7 + r * 5) % cols
        src[r, idx] = specials
    dst = torch.full((rows, ld_dst), -1, dtype=torch.int16, device=dev)
    _lib.check(plib.revo_op_f32_to_bf16(_lib.ptr(src.to(dev)), ld_src, _lib.ptr(dst), ld_dst, rows, cols, _lib.current_stream()))
    torch.cuda.synchronize()
    got = dst.cpu()
    assert (got[:, cols:] == 0).all()                              # zero padding
    got = got[:, :cols].view(torch.bfloat16)
    want = src[:, :cols].bfloat16()
    nan = torch.isnan(src[:, :cols])
    assert torch.isnan(got[nan].float()).all()                    # NaN stays NaN (its payload is not part of the contract)
    same = kb.bf16_bits(got[~nan]) == kb.bf16_bits(want[~nan])
    bad = (~same).nonzero().flatten()[:8]
    assert bool(same.all()), [(hex(int(src[:, :cols][~nan][i].view(torch.int32))), hex(int(kb.bf16_bits(got[~nan][i]))),
                               hex(int(kb.bf16_bits(want[~nan][i])))) for i in bad]
    print(f"[f32_to_bf16] {rows} x {cols} (ld_src {ld_src}, ld_dst {ld_dst}): bit exact, padding zero")


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("MNK", kb.GEMM_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in kb.GEMM_CASES])
def test_gemm_bf16_epilogue_within_bound(plib, dev, MNK, gelu):
    M, N, K = MNK
    a, b, bias = (t.to(dev) for t in kb.gemm_case(M, N, K))
    c = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
    _lib.check(plib.revo_op_gemm(EPI_BF16_GELU if gelu else EPI_BF16, _lib.ptr(a), K, _lib.ptr(b), K, M, N, K, _lib.ptr(c), N,
                                 _lib.ptr(bias), None, _lib.current_stream()), "gemm")
    torch.cuda.synchronize()
    G = kb.GemmBf16
    _report("gemm", f"{M}x{N}x{K} {'gelu' if gelu else 'bf16'}",
            kb.ratio(c, G.reference(a, b, bias, gelu), G.bound(a, b, bias, gelu)))
