"""The per-element bounds of tests/_kernel_bounds.py have teeth and are not flaky (CPU only, no GPU).

For each op and each shape the GPU tier (test_gpu_kernel_bounds.py) runs: every listed mutation exceeds the bound by its
required ratio somewhere (3x; 1.5x for the softmax scale off by 1 %), and the emulation of the kernel's rounding stays at
<= 0.75x of the bound everywhere.  Mutations listed in NOT_CAUGHT must really stay under their ratio at those cases.  The
bound is per element, so the large attention shapes are checked on a sample of (image, head) pairs.  The GEMM family
(GemmF32, GemmResid, GemmRope, GemmLnIn, LnStats, SplitkResidLn) runs at the GPU cases' N, K, slot counts, S and head_dim
with M cut to a few hundred rows; the rounding-direction statistic and the coverage of the launch-form record are checked
here too.  The planted high-dynamic-range attention cases (kb.ATTENTION_HDR_CASES) are checked head by head against a model
of the kernel's optimistic softmax: the predicted move schedule is the stated one, and every way of getting a move wrong
leaves the bound.  The patch embedding (kb.PatchEmbed) runs at every tower's patch size, width and padded K with the grid cut
to a few hundred rows of two or more images: the index, order and scale mutations on every fixture, the dropped low parts on
the coherent fixtures (on random data they add incoherently and are printed only)."""
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


def _hdr_ids():
    return [f"{c['label']} h{h}" for c in kb.ATTENTION_HDR_CASES for h in range(c["H"])]


@pytest.mark.parametrize("case,h", [(c, h) for c in kb.ATTENTION_HDR_CASES for h in range(c["H"])], ids=_hdr_ids())
def test_attention_hdr_takes_its_path_and_the_bound_has_teeth(case, h):
    """Each head of each planted high-dynamic-range case: the fp32 model of the kernel's optimistic softmax predicts the
    move schedule the case states (the GPU test cannot observe the path: this condition on the inputs stands in for it),
    stays within EMULATION_MAX of the fp64 bound, and every way of getting a move wrong leaves the bound by 3 x."""
    B, S, H, hd = case["B"], case["S"], case["H"], case["hd"]
    qkv = kb.attention_hdr_qkv(case)
    q, k, v = kb.attention_split(qkv, B, S, H, hd, [b * H + h for b in range(B)])
    A = kb.Attention
    em = A.emulate_optimistic(q, k, v, kb.attention_k_lo(S))
    facts, failures, text = kb.attention_hdr_schedule(case, h, em)
    print(f"[attention hdr {case['label']} h{h}] predicted schedule: {text}")
    assert not failures, (case["label"], h, failures)
    _check("attention hdr", f"{case['label']} h{h}", facts, A.reference(q, k, v), A.bound(q, k, v), em["out"],
           [(name, f(q, k, v), need) for name, f, need in A.HDR_MUTATIONS + A.MUTATIONS])


def test_attention_hdr_cases_cover_what_they_claim():
    """Structure of the family: the four shapes with their prelude / ragged tile, the wave-mates pattern on each, boosted
    rows in wave groups served by waves 0-3 and by waves 4-7, late rises in tile 1, a middle tile and the last tile."""
    shapes = {(c["S"], c["hd"]) for c in kb.ATTENTION_HDR_CASES}
    assert shapes == {(577, 64), (197, 64), (257, 96), (130, 96)}
    assert [kb.attention_k_lo(S) for S in (577, 197, 257, 130)] == [1, 0, 1, 0]
    late = set()
    for c in kb.ATTENTION_HDR_CASES:
        assert c["B"] <= 2 and c["H"] == 2
        nt = (c["S"] - kb.attention_k_lo(c["S"]) + 63) // 64
        for head in c["heads"]:
            for p in head["plants"]:
                if head["name"].startswith("late rise"):
                    late.add("tile 1" if p["moves"] == (1,) else "last" if p["moves"] == (nt - 1,) else "middle")
    assert late == {"tile 1", "middle", "last"}
    for S, hd in shapes:
        mates = [head for c in kb.ATTENTION_HDR_CASES if (c["S"], c["hd"]) == (S, hd) for head in c["heads"]
                 if head["name"].startswith("wave mates")]
        assert mates, (S, hd)
        waves = {(pos // 32) % 8 for head in mates for p in head["plants"] for pos in p["qpos"]}
        assert waves & {0, 1, 2, 3} and waves & {4, 5, 6, 7}, (S, hd, waves)
        for head in mates:                                            # exactly one boosted row per 32-row wave group
            groups = [pos // 32 for p in head["plants"] for pos in p["qpos"]]
            assert len(groups) == len(set(groups))


@pytest.mark.parametrize("parts", [2, 4], ids=["32x32x16", "16x16x32"])
def test_attention_hdr_model_of_both_kernels(parts):
    """attn16_fwd_kernel sums 16 keys per lane where attn_fwd_kernel sums 32 (four partial sums against the 2^80 test
    instead of two); the wave group is 32 rows in both.  On the head_dim-64 cases both models take the stated path and stay
    inside the bound."""
    for case in kb.ATTENTION_HDR_CASES:
        if case["hd"] != 64:
            continue
        B, S, H, hd = case["B"], case["S"], case["H"], case["hd"]
        qkv = kb.attention_hdr_qkv(case)
        for h in range(H):
            q, k, v = kb.attention_split(qkv, B, S, H, hd, [h])
            em = kb.Attention.emulate_optimistic(q, k, v, kb.attention_k_lo(S), parts=parts)
            _, failures, _ = kb.attention_hdr_schedule(case, h, em)
            assert not failures, (case["label"], h, parts, failures)
            r = kb.ratio(em["out"], kb.Attention.reference(q, k, v), kb.Attention.bound(q, k, v))
            assert r <= EMULATION_MAX, (case["label"], h, parts, r)


@pytest.mark.parametrize("S,hd,scale", kb.HUGE_LOGITS_CASES)
def test_attention_huge_logits_model_against_the_bound(S, hd, scale):
    """The data of test_attention_huge_logits: where the model of the optimistic softmax stays within EMULATION_MAX of the
    fp64 bound, the GPU test asserts the bound next to its absolute tolerance (kb.HUGE_LOGITS_BOUND)."""
    B, H = 2, 2
    qkv = kb.attention_huge_logits_qkv(S, hd, scale, B, H)
    q, k, v = kb.attention_split(qkv, B, S, H, hd)
    em = kb.Attention.emulate_optimistic(q, k, v, kb.attention_k_lo(S))
    r = kb.ratio(em["out"], kb.Attention.reference(q, k, v), kb.Attention.bound(q, k, v))
    moves = (em["moved"] & torch.isfinite(em["m_before"])).any(1).sum(-1).float().mean()
    print(f"[attention huge logits S{S} hd{hd} x{scale}] emulation/bound max {r:.3f}; {float(moves):.1f} tiles with a move per pair")
    assert (r <= EMULATION_MAX) == kb.HUGE_LOGITS_BOUND[(S, hd, scale)], r


def test_attention_peaked_model_against_the_bound():
    qkv = kb.attention_peaked_qkv()
    q, k, v = kb.attention_split(qkv, 1, 577, 1, 64)
    em = kb.Attention.emulate_optimistic(q, k, v, 1)
    r = kb.ratio(em["out"], kb.Attention.reference(q, k, v), kb.Attention.bound(q, k, v))
    print(f"[attention peaked] emulation/bound max {r:.3f}")
    assert (r <= EMULATION_MAX) == kb.PEAKED_BOUND, r


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


# ---------------------------------------------------------------- the GEMM family ----
TEETH_ROWS = 160


def _mut(c, muts):
    return [(name, f(c), need) for name, f, need in muts]


@pytest.mark.parametrize("MNK", kb.GEMM_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in kb.GEMM_CASES])
def test_gemm_f32_bound_has_teeth(MNK):
    c = kb.plain_case(*MNK, seed=sum(MNK))
    G = kb.GemmF32
    _check("gemm f32", "x".join(map(str, MNK)), {"K": MNK[2]}, G.reference(c), G.bound(c), G.emulate(c), _mut(c, G.MUTATIONS))


@pytest.mark.parametrize("case", kb.RESID_CASES, ids=[x[0] for x in kb.RESID_CASES])
def test_gemm_resid_bound_has_teeth(case):
    label, N, K, ksplit, planes = case
    c = kb.resid_case(TEETH_ROWS, N, K, seed=N + K, planes_in=planes in ("in", "inout"), ksplit=ksplit)
    G, pout = kb.GemmResid, planes in ("out", "inout")
    _check("resid", label, {"K": K}, G.reference(c), G.bound(c, pout), G.emulate(c, pout), _mut(c, G.MUTATIONS))
    if pout:                                                      # the planes the emulation writes keep their invariant
        x = G.emulate(c).float()
        hi = x.bfloat16()
        assert kb.planes_ok(hi, (x - hi.float()).bfloat16())


@pytest.mark.parametrize("MNK", kb.GEMM_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in kb.GEMM_CASES])
def test_gemm_resid_small_shapes_have_teeth(MNK):
    c = kb.resid_case(*MNK, seed=sum(MNK))
    G = kb.GemmResid
    _check("resid", "x".join(map(str, MNK)), {"K": MNK[2]}, G.reference(c), G.bound(c), G.emulate(c), _mut(c, G.MUTATIONS))


@pytest.mark.parametrize("tower", ["L14", "G14"])
def test_gemm_rope_bound_has_teeth(tower):
    t = kb.TOWERS[tower]
    W = t["W"]
    c = kb.plain_case(t["S"] + 23, 3 * W, W, seed=W)
    c = c.with_(cs=kb.tower_rope(tower), S=t["S"], hd=t["hd"], rope_cols=2 * W)
    G = kb.GemmRope
    _check("gemm rope", tower, {}, G.reference(c), G.bound(c), G.emulate(c), _mut(c, G.MUTATIONS))


@pytest.mark.parametrize("case", kb.LN_IN_CASES, ids=[x[0] for x in kb.LN_IN_CASES])
def test_gemm_ln_in_bound_has_teeth(case):
    label, N, K, epi, tower = case
    t = kb.TOWERS[tower]
    rope = epi == "rope"
    M = t["S"] + 23 if rope else TEETH_ROWS
    c = kb.ln_in_case(M, N, K, seed=N + K, epi=epi, S=t["S"], hd=t["hd"], rope_cols=2 * t["W"] if rope else 0,
                      cs=kb.tower_rope(tower) if rope else None)
    G = kb.GemmLnIn
    _check("gemm ln_in", label, {}, G.reference(c), G.bound(c), G.emulate(c), _mut(c, G.MUTATIONS))


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("N", [512, 768, 1024, 1536])
def test_ln_stats_bound_has_teeth(N, planes):
    c = kb.resid_case(TEETH_ROWS, N, 1024, seed=N)
    x = kb.GemmResid.emulate(c, planes_out=planes)                # the kernel's row (fp32, or hi + lo)
    L = kb.LnStats
    # the emulation runs on the fp32 row the kernel holds; with planes the reference sees hi + lo of it
    x32 = kb.GemmResid.emulate(c).float()
    emu = L.emulate(x32)
    _check("ln stats", f"N{N}{' planes' if planes else ''}", {}, L.reference(x), L.bound(x, planes), emu,
           [(name, f(x), need) for name, f, need in L.MUTATIONS])


@pytest.mark.parametrize("case", kb.SPLITK_LN_CASES, ids=[x[0] for x in kb.SPLITK_LN_CASES])
def test_splitk_resid_ln_bound_has_teeth(case):
    label, N, K, ksplit = case
    c = kb.resid_case(TEETH_ROWS, N, K, seed=N * 3 + K, ksplit=ksplit)
    G, H, eps = kb.GemmResid, kb.SplitkResidLn, 1e-5
    _check("splitk ln x", label, {"K": K}, G.reference(c), G.bound(c), G.emulate(c), _mut(c, G.MUTATIONS))
    x_new = G.emulate(c).float()                                  # the values the kernel stores and normalises
    muts = [(name, f(x_new, eps), need) for name, f, need in H.MUTATIONS_H]
    muts.append(("normalised the old row instead of the new one", H.h_reference(c.x, eps), 3.0))
    muts.append(("a plane dropped before the normalisation",
                 H.h_reference(G.reference(c, kb._acc_drop_plane(c)).float(), eps), 3.0))
    _check("splitk ln h", label, {}, H.h_reference(x_new, eps), H.h_bound(x_new, eps), H.h_emulate(x_new, eps), muts)


def _patch_teeth_params():
    return [(tower, grid, B, fixture, u8) for tower, grid, B in kb.PATCH_TEETH_CASES for fixture in kb.PATCH_FIXTURES
            for u8 in (True, False) if not (u8 and fixture == "special")]


@pytest.mark.parametrize("tower,grid,B,fixture,u8", _patch_teeth_params(),
                         ids=[f"{t} {f} {'u8' if u else 'f32'}" for t, _, _, f, u in _patch_teeth_params()])
def test_patch_embed_bound_has_teeth(tower, grid, B, fixture, u8):
    c = kb.patch_case(tower, fixture, u8, B, seed=7, grid=grid)
    assert c.B >= 2 and 150 <= c.M <= 400 and c.Kp == (kb.PATCH_TOWERS[tower]["P"] ** 2 * 3 + 63) // 64 * 64
    P = kb.PatchEmbed
    ref, bound = P.reference(c), P.bound(c)
    label = f"{tower} {fixture} {'u8' if u8 else 'f32'} images"
    parts = [(name, f(c), need) for name, f, need in P.PART_MUTATIONS]
    muts = [(name, f(c), need) for name, f, need in P.MUTATIONS]
    if fixture == "coherent":
        g = c.gemm()
        lo_w = g.b[:, c.Kp:c.Kp + c.Kreal].float()
        assert (lo_w > 0).all() and (c.a32(c.cols()) > 0).all()      # every dropped term has one sign
        if not u8:
            assert (g.a[:, 2 * c.Kp:2 * c.Kp + c.Kreal].float() > 0).all()
        muts = muts + parts
    else:
        print(f"[patch embed {label}] not asserted (incoherent): "
              + "; ".join(f"{n}: {'n/a' if m is None else format(kb.ratio(m, ref, bound), '.3g')}" for n, m, _ in parts))
    if fixture == "special":
        x = c.images
        assert (x == 0).any() and (x == 1).any() and (x == -1).any() and (x.abs() > 1).any()
        assert ((x.abs() > 0) & (x.abs() < 1e-29)).any()
    _check("patch embed", label, {}, ref, bound, P.emulate(c), muts)
    if c.cls is not None:                                             # one fp32 add of two inputs: the rounded exact sum
        assert torch.equal(P.class_rows(c), (c.cls.double() + c.pos[0].double()).float())


def test_every_patch_gemm_launch_form_has_a_gpu_case():
    """The GPU cases of the patch embedding (kb.PATCH_FORM_CASES): each states the launch form that gemm.hip's rule
    (kb.patch_gemm_form) gives its shape; for uint8 and for fp32 images they cover every kernel the launcher can send
    EPI_PATCH through; every tower has a one-image forward, and the three product towers a batch just under and one just
    at use_256, the first batch on the persistent kernel, and uint8 batches on both sides of the band-patchify condition
    with the first band batch also forced to the gather form."""
    cases = kb.PATCH_FORM_CASES
    assert len(set(cases)) == len(cases)
    forms = {}                                                        # (tower, u8) -> {batch: form}
    for tower, fixture, u8, B, gather, form in cases:
        t = kb.PATCH_TOWERS[tower]
        M, Kp = B * (t["image"] // t["P"]) ** 2, (3 * t["P"] ** 2 + 63) // 64 * 64
        assert form == kb.patch_gemm_form(M, t["W"], (2 if u8 else 3) * Kp), (tower, B)
        assert not gather or kb.patch_band(tower, u8, B), "the gather form is forced only where the band form would run"
        forms.setdefault((tower, u8), {})[B] = form
    for u8 in (True, False):
        assert {f for (_, u), d in forms.items() if u == u8 for f in d.values()} == set(kb.PATCH_FORMS)
    for (tower, u8), d in forms.items():
        assert 1 in d
        if tower not in ("B16", "L14", "G14"):
            continue
        at256 = min(B for B, f in d.items() if f == "256_TILE")
        assert d[at256 - 1] in ("128_64", "128_128")
        t = kb.PATCH_TOWERS[tower]
        G2, K = (t["image"] // t["P"]) ** 2, (2 if u8 else 3) * ((3 * t["P"] ** 2 + 63) // 64 * 64)
        first_p = min(B for B, f in d.items() if f == "256P")         # the smallest batch on the persistent kernel
        assert kb.patch_gemm_form((first_p - 1) * G2, t["W"], K) == "256_TILE"
        if u8:
            band = min(B for B in d if kb.patch_band(tower, True, B))
            assert band - 1 in d and not kb.patch_band(tower, True, band - 1)
            assert (tower, "random", True, band, True, d[band]) in cases
    assert forms[("L14", True)][10] == "128_64" and forms[("L14", True)][11] == "256_TILE"


def test_bf16_rounding_direction_statistic_has_teeth():
    """Round-to-nearest stores average to ~0 ulp of signed error; truncating stores to ~-0.5 (per-element bounds of one
    ulp cannot tell them apart)."""
    c = kb.ln_in_case(400, 4096, 1024, seed=7, epi="gelu")
    ref, bound = kb.GemmLnIn.reference(c), kb.GemmLnIn.bound(c)
    rstd, mr = kb.fold_merge32(c.stats, c.eps)
    v = c.acc(dtype=torch.float32) * rstd[:, None] + (c.csum.float()[None, :] * mr[:, None] + c.bias.float()[None, :])
    v = torch.nn.functional.gelu(v)
    near, n = kb.rounding_bias(v.bfloat16(), ref)
    trunc, _ = kb.rounding_bias(kb.bf16_truncate(v), ref)
    assert n >= kb.ROUNDING_MIN_OUTPUTS, n
    print(f"[rounding direction] {n} outputs: round-to-nearest {near:+.4f}, truncation {trunc:+.4f} (limit {kb.ROUNDING_BIAS_MAX})")
    assert abs(near) <= kb.ROUNDING_BIAS_MAX
    assert abs(trunc) > 3 * kb.ROUNDING_BIAS_MAX
    # and the truncated outputs stay within the per-element bound: only the statistic sees them
    assert kb.ratio(kb.bf16_truncate(v), ref, bound) <= 1.0


def test_every_gemm_launch_form_has_a_gpu_case():
    """The GPU cases (kb.GEMM_FORM_CASES, each asserting the exact set of forms it runs) cover every bit of the launcher's
    form record, and that record is kernels.h's GemmForm enum, in order: a new launch form without a case fails here."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "revers-o_amd", "csrc",
                            "kernels.h")).read()
    enum = re.findall(r"GF_(\w+) = 1u << (\d+)", src)
    assert [n for n, _ in enum] == kb.GEMM_FORMS and [int(b) for _, b in enum] == list(range(len(enum)))
    reached = set()
    for case in kb.GEMM_FORM_CASES:
        reached |= set(case[-1])
    assert reached == set(kb.GEMM_FORMS), sorted(set(kb.GEMM_FORMS) - reached)
