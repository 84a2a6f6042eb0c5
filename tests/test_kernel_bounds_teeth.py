"""The per-element bounds of tests/_kernel_bounds.py have teeth and are not flaky (CPU only, no GPU).

For each op and each shape the GPU tier (test_gpu_kernel_bounds.py) runs: every listed mutation exceeds the bound by its
required ratio somewhere (3x; 1.5x for the softmax scale off by 1 %), and the emulation of the kernel's rounding stays at
<= 0.75x of the bound everywhere.  Mutations listed in NOT_CAUGHT must really stay under their ratio at those cases.  The
bound is per element, so the large attention shapes are checked on a sample of (image, head) pairs."""
import pytest
import torch

import _kernel_bounds as kb

EMULATION_MAX = 0.75


def _check(op, label, case, ref, bound, emulated, mutations):
    em = kb.ratio(emulated, ref, bound)
    worst, lines, failures = float("inf"), [], []
    for name, mutated, need in mutations:
        if mutated is None:
            lines.append(f"{name}: n/a")
            continue
        r = kb.ratio(mutated, ref, bound)
        lines.append(f"{name}: {r:.3g}")
        if kb.not_caught(op, name, case):
            if r >= need:
                failures.append(f"{name} is listed as not caught but reaches {r:.3g} >= {need}")
            continue
        worst = min(worst, r)
        if r < need:
            failures.append(f"{name} reaches only {r:.3g} x the bound (needs {need})")
    print(f"[{op} {label}] emulation/bound max {em:.3f}; smallest mutation/bound {worst:.3g}; "
          + "; ".join(lines))
    assert em <= EMULATION_MAX, (op, label, em)
    assert not failures, (op, label, failures)


@pytest.mark.parametrize("case", kb.ATTENTION_CASES, ids=[c[0] for c in kb.ATTENTION_CASES])
def test_attention_bound_has_teeth(case):
    label, B, S, H, hd, ld, ldo = case
    qkv = kb.attention_qkv(B, S, H, hd, ld)
    N = B * H
    pairs = sorted({0, N // 3, 2 * N // 3, N - 1})
    q, k, v = kb.attention_split(qkv, B, S, H, hd, pairs)
    A = kb.Attention
    ref, bound = A.reference(q, k, v), A.bound(q, k, v)
    _check("attention", label, {"S": S}, ref, bound, A.emulate(q, k, v),
           [(name, f(q, k, v), need) for name, f, need in A.MUTATIONS])


@pytest.mark.parametrize("case", kb.ROPE_CASES, ids=[c[0] for c in kb.ROPE_CASES])
def test_rope_bound_has_teeth(case):
    label, grid, H, hd, cls, B = case
    cs = kb.rope_table(grid, hd, cls)
    qkv, S = kb.rope_qkv(grid, H, hd, cls, B)
    x = torch.cat([kb.rope_heads(qkv, B, S, H, hd, 0), kb.rope_heads(qkv, B, S, H, hd, 1)])     # q and k
    R = kb.Rope
    _check("rope", label, {"cls": cls}, R.reference(x, cs), R.bound(x, cs), R.emulate(x, cs),
           [(name, f(x, cs, cls), need) for name, f, need in R.MUTATIONS])


@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("W", kb.LAYERNORM_WIDTHS)
def test_layernorm_bound_has_teeth(W, out_bf16):
    x, w, b = kb.layernorm_rows(W, out_bf16)
    L, eps = kb.LayerNorm, 1e-5
    _check("layernorm", f"W{W} {'bf16' if out_bf16 else 'fp32'}", {"bf16": bool(out_bf16)}, L.reference(x, w, b, eps),
           L.bound(x, w, b, eps, out_bf16), L.emulate(x, w, b, eps, out_bf16),
           [(name, f(x, w, b, eps), need) for name, f, need in L.MUTATIONS])


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("MNK", kb.GEMM_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in kb.GEMM_CASES])
def test_gemm_bf16_bound_has_teeth(MNK, gelu):
    a, b, bias = kb.gemm_case(*MNK)
    G = kb.GemmBf16
    _check("gemm", f"{'x'.join(map(str, MNK))} {'gelu' if gelu else 'bf16'}", {"gelu": gelu}, G.reference(a, b, bias, gelu),
           G.bound(a, b, bias, gelu), G.emulate(a, b, bias, gelu),
           [(name, f(a, b, bias, gelu), need) for name, f, need in G.MUTATIONS])


def test_f32_to_bf16_specials_are_what_the_gpu_test_expects():
    """The CPU side of the bit-exact conversion test: torch's round-to-nearest-even on the special classes (ties both ways,
    overflow to inf, subnormals kept), which test_gpu_kernel_bounds.py holds the kernel to."""
    x = kb.f32_from_bits(kb.f32_special_values())
    got = kb.bf16_bits(x.bfloat16()).tolist()
    want = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0xbf808000: 0xbf80, 0xbf818000: 0xbf82, 0x7f7f8000: 0x7f80,
            0xff7f8000: 0xff80, 0x7f7fffff: 0x7f80, 0x3fff8000: 0x4000, 0x00008000: 0x0000, 0x00018000: 0x0002,
            0x00408000: 0x0040, 0x007fffff: 0x0080, 0x00010000: 0x0001, 0x80000000: 0x8000}
    for bits, out in zip(kb.f32_special_values(), got):
        if bits in want:
            assert out == want[bits], (hex(bits), hex(out))
    nan = torch.isnan(x)
    assert int(nan.sum()) == 5 and torch.isnan(x.bfloat16()[nan]).all()
