"""CPU: the hot kernels' register allocation, from hipcc's own report (`-Rpass-analysis=kernel-resource-usage`; hipcc
cross-compiles for gfx950 without a GPU).

These kernels sit AT their register limit (256 VGPRs for the 256 x 256 main loop and the scan built on it, 128 for the
attention kernel's four waves per SIMD): a few more live values -- two pointers and a branch were enough in round 4 -- and
the compiler spills inside the loop.  That cost the plain 256-row scan 5 % at 10 000 queries and 17 % at 256 before an A/B
against the previous commit's library caught it.  The numbers below are the allocation the measured
kernels have; a change that moves them is not necessarily wrong, but it must be measured (scripts/scan_regression_ab.sh,
scripts/step_regression_ab.sh) before the bound here is moved."""
import os
import re
import subprocess

import pytest

from _hipcc_report import listing as _listing, scratch_in_loops as _scratch_in_loops, usage as _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _find(d, *parts):
    hits = [k for k in d if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits)
    return d[hits[0]]


@pytest.fixture(scope="module")
def scan_usage():
    return _usage("topk256.hip")


def test_plain_scan_forms_do_not_spill_vectors(scan_usage):
    """topk_scan256_kernel<KSEL, ROWS, MARGIN = false, FILTER = false>: the forms every search with k <= 25 runs.
    (Round 5: the slice bounds as 32-bit scalars -- as `long` they lived in vector registers, the hardware has no scalar 64-bit order compare --
    took the 192-row forms from 9 spilled registers to 2 and the margin form from 16 to 4; the 256-row forms park one
    register outside the tile loop.)"""
    # (the 32-candidate 192-row form moves between 2 and 5 with edits to OTHER kernels of topk256.hip -- the segment reduce's
    #  gather took it from 2 to 5; measured with 5: 129-192 queries 0.511-0.522 ms per scan against 0.527-0.533 at the round's
    #  start, profiles/r05_search_small_q.json)
    for ksel in (32, 64):
        for rows, allowed in ((0, 1), (64, 0), (128, 0), (192, 5 if ksel == 32 else 2)):
            u = _find(scan_usage, "topk_scan256_kernel", f"ILi{ksel}ELi{rows}ELb0ELb0E")
            assert u["VGPRs"] <= 256 and u["VGPRs Spill"] <= allowed, (ksel, rows, u)
    # the margin forms (k > 25) are allowed their handful; the 192-row margin form must not exist (464 spills when built)
    for rows, allowed in ((0, 4), (64, 0), (128, 2)):
        u = _find(scan_usage, "topk_scan256_kernel", f"ILi64ELi{rows}ELb1ELb0E")
        assert u["VGPRs Spill"] <= allowed, (rows, u)
    assert not [k for k in scan_usage if "topk_scan256_kernel" in k and "ELi192ELb1E" in k]
    assert not [k for k in scan_usage if re.search(r"topk_scan256_kernelILi32ELi\d+ELb1E", k)]


def test_no_scratch_traffic_inside_the_tile_loop_of_the_scans():
    """WHERE the parked registers are touched: never inside a scan's loop over gallery tiles, let alone its K loop, on the path
    every tile takes.  A reload there waits for ALL vector memory (scratch shares the counter), i.e. for the next tile's
    first operands, which are requested before the selection so that they fly during it: one build of round 5 reloaded an
    LDS address in the per-tile flush and lost 9 % with a clean K loop.  Allowed: the 192-row forms' one reload in the
    flush (measured with it), and the margin forms' reload of the drop-flag pointer on the retry path (rare)."""
    seen = 0
    # (the plain forms, FILTER = false; the filtered ones: tests/test_filtered_scan_registers.py, from the same listing)
    for m, hot in _scratch_in_loops(_listing("topk256.hip"),
                                    r"_ZN4revo19topk_scan256_kernelILi(\d+)ELi(\d+)ELb(\d)ELb0EEEvNS_11Scan256ArgsE"):
        rows, margin = int(m.group(3)), int(m.group(4))
        seen += 1
        assert not [h for h in hot if h[0] >= 2], (m.group(1), hot)            # K loop and the selection's inner loops
        allowed = 1 if (rows == 192 or margin) else 0
        if rows == 192 and int(m.group(2)) == 32:
            allowed = 12                                   # (see above: this form's five, reloaded around its flush)
        assert len(hot) <= allowed, (m.group(1), hot)
    assert seen == 11, seen


def test_attention_kernel_keeps_four_waves_per_simd():
    d = _usage("attention.hip")
    u = _find(d, "attn_fwd_kernel", "ILi64ELi8ELi0E")
    assert u["VGPRs"] <= 128 and u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, u
    u = _find(d, "attn_fwd_kernel", "ILi96ELi8ELi0E")
    assert u["VGPRs"] <= 256 and u["VGPRs Spill"] == 0, u


def test_body_gemm_kernels_stay_within_their_allocation():
    d = _usage("gemm.hip")
    # gemm256p_kernel<EPI, BMR>: EPI 1 = GELU (fc1), 2 = residual (out-proj, fc2), 5 = RoPE (qkv); the handful of spilled
    # registers are epilogue values, outside the main loop (measured kernels: DESIGN.md section 6).  Round 5 (the folded
    # LayerNorm's statistics merged in front of the main loop and applied in the epilogues, GELU on two fragments side by
    # side): the bf16 forms park 5-9 registers around the tile loop -- all OUTSIDE the K loop, which the next test checks
    # (one version of the merge kept a lane id alive across the main loop and put an accumulator spill INSIDE the RoPE
    # kernel's K loop: that is what the next test is for).
    # (later in round 5: tile coordinates moved to scalar registers right after their integer divisions, the epilogue's lane
    #  id read from the hardware behind the main loop in the GELU / residual forms: 6 -> 2, 2 -> 0, 10 -> 7, 8 -> 7)
    # (round 6: the folded consumer's telemetry -- two ballots and up to three scalar atomics per column-tile-0 wave, one more
    #  kernel argument -- costs the GELU form one more parked register, 2 -> 3, outside the K loop; step A/B'd against the
    #  round-5 library)
    for epi, bmr, allowed in ((1, 256, 3), (2, 256, 0), (2, 192, 0), (5, 256, 7), (0, 256, 7)):
        u = _find(d, "gemm256p_kernel", f"ILi{epi}ELi{bmr}ELi0E")
        assert u["VGPRs"] <= 256 and u["VGPRs Spill"] <= allowed, (epi, bmr, u)
    # the residual stream in two bf16 planes: one instantiation per format pair (XP 1..3).  With the formats as run-time
    # tests inside one kernel these spilled 35 registers, as four copies inside one kernel 160 -- inside the epilogue,
    # where every scratch reload also drains the queue of outstanding stores
    for bmr in (192, 256):
        for xp in (1, 2, 3):
            u = _find(d, "gemm256p_kernel", f"ILi2ELi{bmr}ELi{xp}E")
            assert u["VGPRs"] <= 256 and u["VGPRs Spill"] == 0, (bmr, xp, u)
    for epi in (0, 1, 2, 5):
        u = _find(d, "gemm256_kernel", f"ILi{epi}ELi0E")
        assert u["VGPRs Spill"] == 0, (epi, u)
    # gemm256q_kernel<EPI> (round 6, queued stores; fc1's GELU form and the plain bf16 form run on it): NOTHING parked.  Its
    # epilogue keeps the next tile's DMA and this tile's stores in flight while it computes, and every scratch access is
    # guarded by an s_waitcnt vmcnt(0) that drains both (hipcc's wait counts leave LDS-DMA out) -- the first builds parked
    # 11-28 registers (zero vectors of two-sided selects, a lane id kept across the main loop, a zero offset of the telemetry
    # atomics) and lost what the kernel was built for.  (The RoPE form, EPI 5, is built but not the default: 128 spilled.)
    for epi in (0, 1):
        u = _find(d, "gemm256q_kernel", f"ILi{epi}E")
        assert u["VGPRs"] <= 256 and u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (epi, u)


def test_no_scratch_traffic_inside_the_k_loop_of_the_body_gemms():
    """What the spill counts above cannot say: WHERE the spilled values are reloaded.  A scratch load inside the K loop
    (the innermost loop of the persistent kernels, `Depth=2` in hipcc's listing) costs every K-tile; behind it -- once per
    output tile -- it costs a queue drain at most.  Round 5 moved epilogue code twice before the listing was clean."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-S",
                          "--cuda-device-only", "gemm.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    asm = out.stdout
    checked = 0
    for m in re.finditer(r"^(_ZN4revo15gemm256p_kernelILi\d+ELi\d+ELi\d+EEEvNS_8GemmArgsEi):", asm, flags=re.M):
        body = asm[m.end(): asm.index(".Lfunc_end", m.end())].splitlines()
        depth, inner_mfma, inner_scratch = 0, 0, []
        for ln in body:
            if ln.startswith(".LBB") or ln.startswith("; %bb."):       # a basic block: hipcc notes the loop it belongs to
                dm = re.search(r"Depth=(\d+)", ln)
                depth = int(dm.group(1)) if dm else 0
            elif depth >= 2:
                inner_mfma += "v_mfma" in ln
                if "scratch_" in ln:
                    inner_scratch.append(ln.strip())
        if inner_mfma == 0:
            continue                      # (a listing whose loop nest hipcc printed differently: nothing to judge)
        checked += 1
        assert not inner_scratch, (m.group(1), inner_scratch[:4])
    assert checked >= 4, checked
