"""CPU: every GEMM launch the two towers can make is held to fp64 per-element bounds by some GPU case.

tests/test_kernel_bounds_teeth.py::test_every_gemm_launch_form_has_a_gpu_case asks that each form BIT appears in a case.  A
launch is more: a kernel form compiled for an epilogue, with or without the folded LayerNorm's consumer, the fold and the
planes, on the main rows or on leftover rows from a row offset -- kb.gemm_signatures.  This module enumerates, through
revo_debug_gemm_plan (no device), the signatures of every launch_gemm call of tower.h body_blocks (restated in
kb.body_gemm_launches; tests/test_gpu_forward_forms.py pins the restatement to the forward on the device) over

  the image towers of reverso_amd.config (B16, L14, G14) at batch 1 .. 64,
  the text towers of reverso_amd.config (L14: width 1024, context 32; G14: width 1280, context 72) at every row count
  B * S, B in 1 .. 256 (TextEngine's default max_batch), S in 1 .. context_length,

and asserts that each is the signature of a step of some case of kb.GEMM_FORM_CASES (planned under that case's own
variant / qstores) or of kb.GEMM_CASES x {bf16, gelu} (tests/test_gpu_kernel_bounds.py test_gemm_bf16_epilogue_within_bound).
The miniature towers are outside the domain: the GPU suite runs them whole."""
import functools

import pytest

import _kernel_bounds as kb
from reverso_amd import config
from test_gemm_plan import knobs, plan, problem

IMAGE_BATCHES = range(1, 65)
TEXT_MAX_BATCH = 256


@functools.lru_cache(maxsize=None)
def _plan(epi, M, N, K, ws, offers, rope):
    bits, steps = plan(epi, M, N, K, ws, offers, rope)
    return bits, tuple(steps)


def cached_plan(epi, M, N, K, ws=0, offers=0, rope=(0, 0, 0)):
    """tests/test_gemm_plan.py plan under the default switches, each distinct problem planned once"""
    return _plan(epi, M, N, K, ws, offers, tuple(rope))


def image_towers():
    return {n: c for n, c in config.VARIANTS.items() if n.startswith("PE-Core")}


def text_towers():
    """the distinct real text towers (B16 and L14 share one)"""
    seen = {}
    for n, c in config.TEXT_VARIANTS.items():
        if n.startswith("PE-Core"):
            seen.setdefault((c.width, c.mlp_dim, c.context_length, c.layers), (n, c))
    return dict(seen.values())


def image_launches(cfg, batch, layers=None):
    return kb.body_gemm_launches(cached_plan, cfg.width, cfg.mlp_dim, batch * cfg.seq, layers or cfg.layers, "rope",
                                 (cfg.seq, cfg.head_dim, 2 * cfg.width))


def text_launches(cfg, rows, layers=None):
    return kb.body_gemm_launches(cached_plan, cfg.width, cfg.mlp_dim, rows, layers or cfg.layers, "bf16")


def reached_signatures():
    """{signature: ((M, N, K), description of the smallest launch that reaches it)}: fewest rows, then columns, then K"""
    reached = {}

    def add(launches, rows, who):
        for name, block, epi, N, K, offers, bits, steps in launches:
            for sig in kb.gemm_signatures(epi, offers, steps):
                size = (rows, N, K)
                if sig not in reached or size < reached[sig][0]:
                    reached[sig] = (size, f"{who} {name} of block {block}: {rows} x {N} x {K}, offers {offers}")

    with knobs():
        _plan.cache_clear()
        for name, cfg in image_towers().items():
            for b in IMAGE_BATCHES:
                add(image_launches(cfg, b), b * cfg.seq, f"image {name} batch {b}")
        for name, cfg in text_towers().items():
            first = {}                                           # distinct row counts once, each under its smallest batch
            for b in range(1, TEXT_MAX_BATCH + 1):
                for s in range(1, cfg.context_length + 1):
                    first.setdefault(b * s, (b, s))
            for rows, (b, s) in sorted(first.items()):
                add(text_launches(cfg, rows), rows, f"text {name} {b} x {s}")
    return reached


def covered_signatures(cases=None):
    """{signature: label of a GPU case that holds it}; cases: the table (default: kb.GEMM_FORM_CASES)"""
    covered = {}
    for label, kind, M, N, K, opts, _ in (kb.GEMM_FORM_CASES if cases is None else cases):
        with knobs(variant=opts.get("variant", 0), qstores=opts.get("qstores", 1)):
            epi, ws, offers, rope, ldc = problem(kind, N, K, opts.get("pad", False))
            bits, steps = plan(epi, M, N, K, ws, offers, rope, ldc)
        assert bits >= 0, label
        for sig in kb.gemm_signatures(epi, offers, steps):
            covered.setdefault(sig, label)
    with knobs():
        for M, N, K in kb.GEMM_CASES:
            for kind in ("bf16", "gelu"):
                epi, ws, offers, rope, ldc = problem(kind, N, K)
                bits, steps = plan(epi, M, N, K, ws, offers, rope, ldc)
                assert bits >= 0
                for sig in kb.gemm_signatures(epi, offers, steps):
                    covered.setdefault(sig, f"GEMM_CASES {M} x {N} x {K} {kind}")
    return covered


@pytest.fixture(scope="module")
def reached():
    return reached_signatures()


def test_every_reached_signature_has_a_gpu_case(reached):
    covered = covered_signatures()
    missing = sorted((size, kb.signature_text(sig), where) for sig, (size, where) in reached.items() if sig not in covered)
    print(f"[gemm coverage] signatures reached {len(reached)}, covered {len(reached) - len(missing)}")
    assert not missing, (f"{len(missing)} of {len(reached)} reached launch signatures have no fp64-bounded GPU case:\n"
                         + "\n".join(f"  {text}: smallest {where}" for _, text, where in missing))


def test_removing_a_signature_case_loses_a_signature(reached):
    """every case of kb.GEMM_SIGNATURE_CASES is the only one that holds some reached signature: none is there twice"""
    assert all(c in kb.GEMM_FORM_CASES for c in kb.GEMM_SIGNATURE_CASES)
    for case in kb.GEMM_SIGNATURE_CASES:
        covered = covered_signatures([c for c in kb.GEMM_FORM_CASES if c is not case])
        assert [s for s in reached if s not in covered], f"{case[0]}: every signature of this case is held by another one"


def test_the_domain_is_the_one_stated(reached):
    """the enumeration saw the towers it says it does, and everyday paths that only a per-signature view shows"""
    assert sorted(c.width for c in image_towers().values()) == [768, 1024, 1536]
    assert sorted((c.width, c.mlp_dim, c.context_length) for c in text_towers().values()) == [(1024, 4096, 32), (1280, 5120, 72)]
    assert ("128R", "resid", False, False, False, 0, "main") in reached          # one B16 image: its out-proj
    assert ("SPLITK_RING", "resid", False, False, False, 0, "main") in reached     # a last fc2 of a few L14 prompts
    assert ("256P", "resid", False, False, True, 1, "main") in reached             # G14: fold + planes out on 256-row tiles
    assert ("256P", "resid", False, False, False, 3, "main") in reached            # ... and its last fc2


def test_the_model_passes_through_every_state_in_two_blocks():
    """The GPU test that pins the model to the forward runs two blocks: block 0, a fc2 with a LayerNorm behind it, a block
    that starts from what that fc2 left, and the last fc2.  The signatures of a two-block run are those of the whole tower."""
    sig = lambda ls: {s for _, _, epi, _, _, offers, _, steps in ls for s in kb.gemm_signatures(epi, offers, steps)}
    with knobs():
        for cfg in image_towers().values():
            for b in IMAGE_BATCHES:
                assert sig(image_launches(cfg, b, 2)) == sig(image_launches(cfg, b)), (cfg.name, b)
        for cfg in text_towers().values():
            for rows in (1, 13, 65, 144, 577, 2048, 4608, 18432):
                assert sig(text_launches(cfg, rows, 2)) == sig(text_launches(cfg, rows)), (cfg.name, rows)
