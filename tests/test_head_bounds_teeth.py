"""The per-element bounds of the fp32 pooling head (tests/_head_bounds.py) have teeth and are not flaky (CPU only).

On every case the GPU tier (tests/test_gpu_head_bounds.py) runs: the emulation of the kernel's roundings stays at or below
EMULATION_MAX of the bound, and every listed mutation leaves the bound by its ratio somewhere, or is listed in
kb.NOT_CAUGHT with the reason and really stays under the ratio there.  And the case lists reach every launch form: the three
launchers' choices are restated in _head_bounds.py and the set of forms reached must be the full set."""
import pytest
import torch

import _head_bounds as hb
from test_kernel_bounds_teeth import EMULATION_MAX, _check  # noqa: F401


def _flat(*ts):
    return torch.cat([t.reshape(-1) for t in ts])


@pytest.mark.parametrize("spec", hb.POOL_CASES, ids=hb.pool_id)
def test_pool_rows_bound_has_teeth(spec):
    x, lg = hb.pool_inputs(spec)
    P = hb.PoolRows
    _check("pool", hb.pool_id(spec), hb.pool_facts(spec, lg), P.reference(x, lg), P.bound(x, lg), P.emulate(x, lg),
           [(name, f(x, lg), need) for name, f, need in P.MUTATIONS])


@pytest.mark.parametrize("spec", hb.MASKED_CASES, ids=hb.pool_id)
def test_masked_pool_rows_bound_has_teeth(spec):
    """The same bound over the allowed tokens: every region kind on its own (a mutation must show in the regions that can
    show it, not only somewhere in the call), then the whole call."""
    x, lg = hb.pool_inputs(spec)
    ri, allow = hb.masked_regions(spec)
    P = hb.PoolRows
    ref, bound, em = P.reference(x, lg, (ri, allow)), P.bound(x, lg, (ri, allow)), P.emulate(x, lg, (ri, allow))
    assert torch.equal(ref[hb.REGION_KINDS.index("empty")], torch.zeros_like(ref[0]))
    assert torch.equal(ref[hb.REGION_KINDS.index("all tokens")], P.reference(x, lg)[ri[hb.REGION_KINDS.index("all tokens")]])
    _check("pool", hb.pool_id(spec) + f" R{spec['R']}", hb.pool_facts(spec, lg[ri], allow), ref, bound, em,
           [(name, f(x, lg, (ri, allow)), need) for name, f, need in P.MUTATIONS])
    for kind in ("3 %", "50 %", "all tokens"):
        r = hb.REGION_KINDS.index(kind)
        one = (ri[r:r + 1], allow[r:r + 1])
        facts = dict(hb.pool_facts(spec, lg[ri[r]], allow[r]), S=int(allow[r].sum()))
        if facts["S"] == 1:
            continue
        _check("pool", hb.pool_id(spec) + f" region {kind}", facts, ref[r:r + 1], bound[r:r + 1], em[r:r + 1],
               [(name, f(x, lg, one), need) for name, f, need in P.MUTATIONS])


@pytest.mark.parametrize("spec", hb.LN_CASES, ids=hb.ln_id)
def test_ln_logits_bound_has_teeth(spec):
    x, w, b, qk, ck = hb.ln_inputs(spec)
    L, S, eps = hb.LnLogits, spec["S"], hb.LN_EPS
    args = (x, w, b, eps, qk, ck, S)
    (y, lg), (by, blg), (ey, elg) = L.reference(*args), L.bound(*args), L.emulate(*args)
    wa, ba = L.affine(x, w, b)
    _check("ln rows", hb.ln_id(spec), {"H": spec["H"]}, y, by, ey,
           [(name, f(x, wa, ba, eps), need) for name, f, need in hb.LayerNorm.MUTATIONS])
    _check("ln logits", hb.ln_id(spec), {"H": spec["H"]}, lg, blg, elg,
           [(name, f(*args), need) for name, f, need in L.MUTATIONS]
           + [(name + " (through the logits)", hb._lg_rows_mutated(f)(*args), need) for name, f, need in hb.LayerNorm.MUTATIONS])


@pytest.mark.parametrize("spec", hb.LINEAR_CASES, ids=hb.linear_id)
def test_linear_f32_bound_has_teeth(spec):
    c = hb.linear_case(spec)
    G = hb.LinearF32
    facts = dict(spec, kper=hb.skinny_kper(spec["K"]))
    _check("linear", hb.linear_id(spec), facts, G.reference(c), G.bound(c), G.emulate(c),
           [(name, f(c), need) for name, f, need in G.MUTATIONS])


@pytest.mark.parametrize("W,heads", hb.PROBE_CASES)
def test_probe_qk_bound_has_teeth(W, heads):
    q, Wk, bk = hb.probe_inputs(W, heads)
    P = hb.ProbeQk
    muts = []
    for name, f, need in P.MUTATIONS:
        m = f(q, Wk, bk, heads)
        muts.append((name, None if m is None else _flat(*m), need))
    _check("probe", f"W{W} heads{heads}", {"heads": heads, "hd": W // heads}, _flat(*P.reference(q, Wk, bk, heads)),
           _flat(*P.bound(q, Wk, bk, heads)), _flat(*P.emulate(q, Wk, bk, heads)), muts)


def test_case_lists_reach_every_launch_form():
    lin = {hb.linear_form(c["M"], c["N"], c["K"]) for c in hb.LINEAR_CASES}
    assert lin == hb.LINEAR_FORMS, lin
    for form, shapes in hb.LINEAR_SHAPES.items():
        assert {hb.linear_form(*s) for s in shapes} == {form}, form
    grouped = {hb.linear_form(c["M"], c["N"], c["K"]) for c in hb.LINEAR_CASES if c["group_cols"]}
    assert grouped == hb.LINEAR_FORMS, grouped
    # the wave ranges: some waves without work and all at work, a last working wave cut short and not, an odd number of
    # chunks behind trips of the 32-wide loop (K = 1040: five chunks) and alone (K = 16); the even counts are
    # test_head_linear_f32_rows_do_not_depend_on_the_batch's K = 1024 and 4096
    facts = {hb.linear_wave_facts(c["K"]) for c in hb.LINEAR_CASES}
    assert {f[0] for f in facts} == {True, False} and {f[1] for f in facts} == {True, False} and any(f[2] for f in facts)
    assert {16, 48, 272, 1040} <= {c["K"] for c in hb.LINEAR_CASES}
    assert any(c["M"] > 64 and hb.linear_form(c["M"], c["N"], c["K"]) == "c" and c["M"] % 64 for c in hb.LINEAR_CASES)
    for epi in (0, 1, 2):
        sub = [c for c in hb.LINEAR_CASES if c["epi"] == epi]
        assert {hb.linear_form(c["M"], c["N"], c["K"]) for c in sub} == hb.LINEAR_FORMS
        assert any(not c["bias"] for c in sub) and any(any(c["pads"]) for c in sub) and any(c["N"] < 16 for c in sub)

    pool = {hb.pool_form(c["B"], c["W"]) for c in hb.POOL_CASES}
    assert pool == hb.POOL_FORMS, pool
    for form, shapes in hb.POOL_SHAPES.items():
        assert {hb.pool_form(B, W) for B, S, W, H in shapes} == {form}, form
    assert {hb.pool_form(c["R"], c["W"]) for c in hb.MASKED_CASES} == hb.POOL_FORMS
    assert hb.pool_form(hb.POOL_REFUSED[0], hb.POOL_REFUSED[2]) == "wide"
    # the eight-row loop's end (s + 112 < S), waves without a row, every count of heads in the last pass of four
    S_all = {c["S"] for c in hb.POOL_CASES}
    assert {1, 15, 16, 17, 112, 113, 128, 129, 241} <= S_all
    assert {c["H"] % 4 for c in hb.POOL_CASES + hb.MASKED_CASES} == {0, 1, 2, 3} and {1, 5, 9, 16} <= {c["H"] for c in hb.POOL_CASES}
    assert any(c["W"] % 64 for c in hb.POOL_CASES) and any(c["pad"] for c in hb.POOL_CASES)

    ln = {hb.ln_form(c["B"] * c["S"], c["W"], c["H"]) for c in hb.LN_CASES}
    assert ln == hb.LN_FORMS, ln
    big = [c for c in hb.LN_CASES if c["B"] * c["S"] >= 4096]
    assert {hb.ln_form(c["B"] * c["S"], c["W"], c["H"])[0] for c in big if c["H"] > 8 or c["W"] > 1536} == {"row"}
    assert any((c["B"] * c["S"]) % 16 for c in big) and any((c["B"] * c["S"]) % 16 == 0 for c in big)
    assert any(not c["affine"] for c in hb.LN_CASES)


def test_launcher_restatements():
    assert [hb.linear_form(*s) for s in [(16, 4096, 16), (17, 3056, 16), (17, 3057, 16), (64, 3072, 16)]] == ["a", "b", "c", "c"]
    assert [hb.skinny_kper(K) for K in (16, 48, 256, 272, 1040, 4096)] == [16, 16, 16, 32, 80, 256]
    assert hb.linear_wave_facts(272) == (True, True, True) and hb.linear_wave_facts(4096) == (False, False, False)
    assert hb.pool_form(191, 256) == "narrow" and hb.pool_form(96, 260) == "wide"
    assert hb.ln_form(4096, 1536, 8) == ("batch", 6) and hb.ln_form(4095, 1536, 8) == ("row", 6)
    assert hb.ln_form(4096, 1540, 8) == ("row", 8) and hb.ln_form(4096, 256, 9) == ("row", 1)
