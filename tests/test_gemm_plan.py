"""CPU: the launch plan of the body GEMMs (csrc/gemm_plan.h gemm_plan, host logic) through the experiment library's
revo_debug_gemm_plan -- no device needed.

launch_gemm executes this plan and records its form bits (revo_debug_gemm_forms), so what is checked here is what runs:
 a. every case of kb.GEMM_FORM_CASES plans the forms tests/test_gpu_gemm_bounds.py asserts on the device;
 b. the cases DESIGN.md quotes, with their numbers (tile rows, leftover rows, split-K parts, XCD arrangement);
 c. over a sweep of row counts x the towers' (N, K) x every epilogue, with every switch default and each flipped singly:
    the steps partition the rows, the grids fit the chip, every step meets the preconditions its kernel states, the folded
    LayerNorm and the planes ride only on a single whole-rows persistent step, and planes without one are refused;
 d. the form bits equal, row for row, those the library of the commit before gemm_plan.h issued on the device
    (tests/golden/gemm_forms_parent.json, recorded by scripts/gemm_forms_record.py)."""
import ctypes as C
import json
import os

import pytest

import _kernel_bounds as kb
from reverso_amd import _lib

WS = 16 << 20                              # the workspace revo_op_gemm* give the residual epilogue (api.hip OP_WS_ELEMS)
EPI = {"bf16": 0, "gelu": 1, "resid": 2, "f32": 3, "patch": 4, "rope": 5}
LN, FOLD, XP_IN, XP_OUT, LNC, PREFER256 = 1, 2, 4, 8, 16, 32
PLANES = {"none": 0, "out": XP_OUT, "inout": XP_IN | XP_OUT, "in": XP_IN}
STEP_FIELDS = ["form", "row0", "rows", "gy", "nslot", "grid_x", "grid_y", "t192_tiles", "t192_tall", "qtail_rows", "S", "reduce_ln",
               "xp", "fold"]
SWEEP_M = [1, 64, 65, 197, 577, 1023, 1024, 4616, 17000, 32768, 33000, 36928, 73856]
TOWER_OF_WIDTH = {t["W"]: name for name, t in kb.TOWERS.items()}
KERNEL_FORMS = kb.GEMM_FORMS[:13]          # one per kernel; the rest are properties of the call


def tower_pairs():
    out = []
    for t in kb.TOWERS.values():
        out += [(3 * t["W"], t["W"]), (t["W"], t["W"]), (t["Md"], t["W"]), (t["W"], t["Md"])]
    return out


def problem(kind, N, K, pad=False):
    """(epi, ws_elems, offers, rope triple, ldc) of the call tests/test_gpu_gemm_bounds.py (and scripts/gemm_forms_record.py)
    makes for `kind`"""
    rope = (0, 0, 0)
    if kind in ("rope", "ln_in_rope"):
        t = kb.TOWERS[TOWER_OF_WIDTH[N // 3]]                         # qkv: N = 3 W
        rope = (t["S"], t["hd"], 2 * t["W"])
    ldc = N + (64 if pad else 0)
    if kind in ("f32", "bf16", "gelu", "patch"):
        return EPI[kind], 0, 0, rope, ldc
    if kind == "f32:prefer256":                                       # the search pre-pass: few rows x very many columns
        return 3, 0, PREFER256, rope, ldc
    if kind == "rope":
        return 5, 0, 0, rope, ldc
    if kind == "ln_in_rope":
        return 5, 0, LNC, rope, ldc
    if kind.startswith("ln_in:"):
        return EPI[kind.split(":")[1]], 0, LNC, rope, ldc
    if kind == "resid":
        return 2, WS, 0, rope, ldc
    if kind == "resid_norm":
        return 2, WS, LN, rope, ldc
    planes = kind.split(":")[1]
    return 2, WS, (0 if planes == "in" else FOLD) | PLANES[planes], rope, ldc


def plan(epi, M, N, K, ws=0, offers=0, rope=(0, 0, 0), ldc=None, lda=None, ldb=None):
    """(form bits or -1, [step dict])"""
    lib = _lib.load_exp()
    out = (C.c_int64 * 32)()
    rc = lib.revo_debug_gemm_plan(epi, M, N, K, lda or K, ldb or K, ldc or N, ws, offers, *rope, out, 32)
    assert rc == out[0] and rc >= -1, (rc, epi, M, N, K)
    steps = [dict(zip(STEP_FIELDS, (int(out[2 + 14 * i + j]) for j in range(14)))) for i in range(int(out[1]))]
    return int(rc), steps


def plan_kind(kind, M, N, K, pad=False):
    epi, ws, offers, rope, ldc = problem(kind, N, K, pad)
    return plan(epi, M, N, K, ws, offers, rope, ldc)


class knobs:
    """the library's switches set for a block and restored to the defaults after it"""

    def __init__(self, variant=0, qstores=1, tile=0, ln_fold=1, phase_groups=0, debug=None):
        self.v = (variant, qstores, tile, ln_fold, phase_groups, debug)

    def __enter__(self):
        lib = _lib.load_exp()
        variant, qstores, tile, ln_fold, phase_groups, debug = self.v
        if debug is not None:
            lib.revo_op_set_gemm_debug(debug)          # (sets the variant bits too)
        else:
            lib.revo_op_set_variant(variant)
        lib.revo_op_set_qstores(qstores)
        lib.revo_op_set_gemm_tile(tile)
        lib.revo_op_set_ln_fold(ln_fold)
        lib.revo_op_set_phase_groups(phase_groups)

    def __exit__(self, *exc):
        lib = _lib.load_exp()
        lib.revo_op_set_gemm_debug(0)
        lib.revo_op_set_qstores(1)
        lib.revo_op_set_gemm_tile(0)
        lib.revo_op_set_ln_fold(1)
        lib.revo_op_set_phase_groups(0)


def names(bits):
    return kb.form_names(bits)


# ---- a. the expectations the GPU suite holds -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", kb.GEMM_FORM_CASES, ids=[c[0] for c in kb.GEMM_FORM_CASES])
def test_plan_names_the_forms_the_gpu_cases_assert(case):
    label, kind, M, N, K, opts, want = case
    with knobs(variant=opts.get("variant", 0), qstores=opts.get("qstores", 1)):
        bits, steps = plan_kind(kind, M, N, K, opts.get("pad", False))
    assert bits >= 0, "refused"
    assert names(bits) == sorted(want), (label, steps)
    if "ksplit" in opts:
        assert [s["S"] for s in steps if s["S"]] == [opts["ksplit"]], (label, steps)


# ---- b. the cases the design quotes --------------------------------------------------------------------------------------
def test_the_cases_the_design_quotes():
    L = 36928                                                          # PE-L14 at batch 64: 64 x 577 rows
    bits, (s,) = plan(2, L, 1024, 1024, WS, FOLD)                      # out-proj, fold offered: three whole rounds of 192-row tiles
    assert names(bits) == ["256P_192", "LN_FOLDED"] and s["fold"] == 1 and (s["row0"], s["rows"]) == (0, L)
    assert (s["t192_tiles"], s["t192_tall"], s["gy"], s["nslot"], s["grid_x"]) == (192, 4, 1, 32, 256)
    bits, (s,) = plan(1, L, 4096, 1024, ldc=4160)                      # fc1: nine whole rounds, the 64 rows left ride along
    assert names(bits) == ["256Q_QTAIL"]
    assert (s["rows"], s["qtail_rows"], s["gy"], s["nslot"], s["grid_x"]) == (36864, 64, 2, 32, 256)
    bits, (s,) = plan(2, 4616, 1024, 4096, WS)                         # fc2 at batch 8: 76 tiles, K in thirds on the 256 kernel
    assert names(bits) == ["SPLITK_256"] and (s["S"], s["gy"], s["grid_x"], s["grid_y"], s["reduce_ln"]) == (3, 2, 80, 3, 0)
    bits, (s,) = plan(2, 577, 1024, 4096, WS, LN)                      # fc2 of one image: the ring kernel, LayerNorm in the reduce
    assert names(bits) == ["SPLITK_RING_LN"] and (s["S"], s["grid_x"], s["grid_y"], s["reduce_ln"]) == (3, 80, 3, 1)
    bits, (s,) = plan(2, 577, 1024, 4096, 0, LN)                       # ... without a workspace: never split-K
    assert names(bits) == ["128R"] and s["S"] == 0 and s["reduce_ln"] == 0 and s["grid_x"] == 80


# ---- c. invariants over a sweep ------------------------------------------------------------------------------------------
KNOB_SETTINGS = {
    "default": {}, "no 192-row tiles": dict(variant=1 << 3), "no tail split": dict(variant=1 << 12),
    "one workgroup per tile": dict(variant=1 << 16), "no split-K": dict(variant=1 << 17), "no minimum for 256 tiles": dict(variant=1 << 18),
    "no ring": dict(variant=1 << 19), "gy 1": dict(variant=1 << 4), "gy 2": dict(variant=2 << 4), "gy 4": dict(variant=4 << 4),
    "gy 8": dict(variant=8 << 4), "no queued stores": dict(qstores=0), "no fused leftover rows": dict(qstores=1 | 32),
    "queued stores for RoPE too": dict(qstores=3), "tile 128": dict(tile=128), "tile 256": dict(tile=256),
    "no fold": dict(ln_fold=0), "fold, fp32 stream": dict(ln_fold=2), "phase groups": dict(phase_groups=2), "debug form": dict(debug=1),
    "stagger": dict(debug=1 << 28),
}
SWEEP_KINDS = ["bf16", "gelu", "f32", "f32:prefer256", "patch", "resid", "resid_norm", "resid_ln:none", "resid_ln:out", "resid_ln:inout", "resid_ln:in",
               "ln_in:gelu", "rope", "ln_in_rope"]
FORMS_256 = {"256_TILE", "256P", "256P_192", "256Q", "256Q_QTAIL", "SPLITK_256"}
PERSISTENT = {"256P", "256P_192", "256Q", "256Q_QTAIL"}


def check_plan(kind, M, N, K, bits, steps, skips_work=False):
    epi, ws, offers, _, ldc = problem(kind, N, K)
    planes = offers & (XP_IN | XP_OUT)
    if bits < 0:
        assert planes, "only planes that no step can carry are refused"
        return
    assert 1 <= len(steps) <= 2
    row, acc = 0, 0
    for s in steps:
        (form,) = names(s["form"])
        assert form in KERNEL_FORMS
        acc |= s["form"]
        assert s["row0"] == row and s["rows"] >= 1
        row += s["rows"] + s["qtail_rows"]
        rows = s["rows"]
        if form in FORMS_256:
            assert s["gy"] in (1, 2, 4, 8)
        if form in PERSISTENT:
            assert 1 <= s["nslot"] <= 32 and (s["grid_x"], s["grid_y"]) == (8 * s["nslot"], 1)
        if form in ("256Q", "256Q_QTAIL"):
            assert epi in (0, 1, 5) and N % 256 == 0 and K >= 128 and ldc % 8 == 0
        assert (s["qtail_rows"] > 0) == (form == "256Q_QTAIL")
        if s["qtail_rows"]:
            assert s["qtail_rows"] <= 64 and K % 256 == 0 and N % 16 == 0
        if form.startswith("SKINNY"):
            assert rows <= 64 and K % 256 == 0 and N >= 256 and epi not in (4, 5)
        if form == "128R":
            assert N % 64 == 0 and K >= 512 and s["grid_x"] == (rows + 127) // 128 * (N // 64) <= 256
        if form.startswith("SPLITK"):
            assert epi == 2 and 2 <= s["S"] <= 8 and s["S"] * rows * N <= ws
            assert (K // 64) // s["S"] >= (4 if s["reduce_ln"] else 8)
            assert s["reduce_ln"] == (form == "SPLITK_RING_LN") and s["grid_y"] == s["S"]
        else:
            assert s["S"] == 0 and s["reduce_ln"] == 0
        if s["reduce_ln"]:
            assert offers & LN and len(steps) == 1
        if form == "256P_192":
            T, e = s["t192_tiles"], s["t192_tall"]
            assert epi == 2 and rows == M == 192 * T + 16 * e and 0 <= e <= min(T, 8)
        else:
            assert s["t192_tiles"] == 0 and s["t192_tall"] == 0
        if s["fold"] or s["xp"]:
            assert epi == 2 and len(steps) == 1 and form in ("256P", "256P_192") and rows == M
            assert N % 256 == 0 and N // 256 <= 6 and ldc % 8 == 0
        assert s["fold"] == 0 or offers & FOLD
        assert s["xp"] == {0: 0, XP_OUT: 1, XP_IN | XP_OUT: 2, XP_IN: 3}[planes]
    # (the work-skipping debug kernels -- wrong results by design -- take the place of the queued-stores kernel without the
    #  leftover rows that kernel would have done in the same launch)
    assert row == M or (skips_work and epi == 0 and row == M - M % 256), "the steps partition [0, M)"
    props = ((kb.form_bits(["LN_FOLDED"]) if steps[0]["fold"] else 0) | (kb.form_bits(["LN_CONSUMED"]) if offers & LNC else 0)
             | (kb.form_bits(["PLANES_IN"]) if steps[0]["xp"] in (2, 3) else 0) | (kb.form_bits(["PLANES_OUT"]) if steps[0]["xp"] in (1, 2) else 0))
    assert bits == acc | props


@pytest.mark.parametrize("setting", KNOB_SETTINGS, ids=list(KNOB_SETTINGS))
def test_every_plan_of_the_sweep_is_sound(setting):
    with knobs(**KNOB_SETTINGS[setting]):
        for N, K in tower_pairs():
            for M in SWEEP_M:
                got = {}
                for kind in SWEEP_KINDS:
                    if kind in ("rope", "ln_in_rope") and N != 3 * K:
                        continue
                    bits, steps = got[kind] = plan_kind(kind, M, N, K)
                    try:
                        check_plan(kind, M, N, K, bits, steps, skips_work=setting == "debug form")
                    except AssertionError as e:
                        raise AssertionError(f"{setting}: {kind} {M} x {N} x {K}: forms {bits}, steps {steps}") from e
                if setting == "default":                          # the patch epilogue has no entry point to record: its restatement
                    assert names(got["patch"][0]) == [kb.patch_gemm_form(M, N, K)], (M, N, K)
                # the fold is offered or not, the planes asked for or not: the same step either carries them all or none
                folds = got["resid_ln:none"][1][0]["fold"] == 1
                for k2 in ("resid_ln:out", "resid_ln:inout", "resid_ln:in"):
                    assert (got[k2][0] >= 0) == folds, (setting, k2, M, N, K)


@pytest.mark.parametrize("tower", sorted(kb.TOWERS))
def test_the_forwards_stream_decision_is_the_plans(tower):
    """The forward decides for a whole run whether the residual stream lives in planes by asking gemm_resid_folds for its two
    residual shapes: the plan of the bare problem with the fold offered.  Its launches then carry a workspace and both
    LayerNorm offers: they must fold, and take the planes, exactly when the bare problem does."""
    t = kb.TOWERS[tower]
    for batch in (1, 8, 32, 64):
        M = batch * t["S"]
        for N, K in ((t["W"], t["W"]), (t["W"], t["Md"])):
            bare, (s0, *_) = plan(2, M, N, K, 0, FOLD)
            full, fs = plan(2, M, N, K, WS, FOLD | LN)
            assert (fs[0]["fold"] == 1) == (s0["fold"] == 1), (tower, batch, N, K)
            asked, _ = plan(2, M, N, K, WS, FOLD | LN | XP_IN | XP_OUT)
            assert (asked >= 0) == (s0["fold"] == 1), (tower, batch, N, K)
    # PE-L14 at batch 64 is the shape the planes were built for
    if tower == "L14":
        assert plan(2, 64 * 577, 1024, 4096, 0, FOLD)[1][0]["fold"] == 1 and plan(2, 577, 1024, 4096, 0, FOLD)[1][0]["fold"] == 0


# ---- d. the parent's record ----------------------------------------------------------------------------------------------
def _parent_rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_forms_parent.json")) as f:
        return json.load(f)["rows"]


def test_form_bits_equal_the_parents_record():
    rows = _parent_rows()
    assert len(rows) > 1500 and {r[1] for r in rows} >= set(SWEEP_M)
    bad = []
    for kind, M, N, K, variant, qstores, want in rows:
        with knobs(variant=variant, qstores=qstores):
            bits, steps = plan_kind(kind, M, N, K)
        if bits != want:
            bad.append((kind, M, N, K, variant, qstores, names(want) if want >= 0 else want, names(bits) if bits >= 0 else bits))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ from the parent: {bad[:10]}"
