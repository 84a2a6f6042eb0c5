"""CPU: the filtered forms of the 256 x 256 scan (topk_scan256_filtered_kernel, every ksel / rows / margin form that is
built) from hipcc's resource report: at or below the spill numbers pinned for the plain forms
(tests/test_kernel_register_budget.py), and no scratch traffic inside the tile loop beyond what the plain forms have."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"]

# (ksel, rows, margin) -> spilled VGPRs allowed: the plain forms' pinned numbers (the 256-row margin form is not built
# filtered: filtered searches of more than 128 queries scan without the margin)
PINNED = {(32, 0, 0): 1, (32, 64, 0): 0, (32, 128, 0): 0, (32, 192, 0): 5,
          (64, 0, 0): 1, (64, 64, 0): 0, (64, 128, 0): 0, (64, 192, 0): 2,
          (64, 64, 1): 0, (64, 128, 1): 2}


@pytest.fixture(scope="module")
def usage():
    out = subprocess.run([HIPCC, *FLAGS, "-c", "topk256.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    cur, d = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        for key, pat in (("VGPRs", r" VGPRs: (\d+)"), ("VGPRs Spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                d[cur][key] = int(m.group(1))
    return d


def test_filtered_scan_forms_spill_no_more_than_the_plain_forms(usage):
    seen = set()
    for name, u in usage.items():
        m = re.search(r"28topk_scan256_filtered_kernelILi(\d+)ELi(\d+)ELb(\d)E", name)
        if not m:
            continue
        form = tuple(int(x) for x in m.groups())
        assert form in PINNED, form
        assert u["VGPRs"] <= 256 and u["VGPRs Spill"] <= PINNED[form], (form, u)
        seen.add(form)
    assert seen == set(PINNED), sorted(set(PINNED) - seen)
    assert not [k for k in usage if "topk_scan256_filtered_kernelILi64ELi0ELb1E" in k]
    # the plain kernels' names are untouched: the filtered form is not an instantiation of topk_scan256_kernel
    assert not [k for k in usage if "topk_scan256_kernel" in k and "filtered" in k]


def test_filtered_scans_keep_scratch_out_of_the_hot_loops():
    out = subprocess.run([HIPCC, *FLAGS, "-S", "--cuda-device-only", "topk256.hip", "-o", "-"], cwd=CSRC,
                         capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    asm = out.stdout
    seen = 0
    for m in re.finditer(r"^(_ZN4revo28topk_scan256_filtered_kernelILi(\d+)ELi(\d+)ELb(\d)EEEvNS_11Scan256ArgsE):", asm,
                         flags=re.M):
        body = asm[m.end(): asm.index(".Lfunc_end", m.end())].splitlines()
        depth, hot = 0, []
        for ln in body:
            if ln.startswith(".LBB") or ln.startswith("; %bb."):
                dm = re.search(r"Depth=(\d+)", ln)
                depth = int(dm.group(1)) if dm else 0
            elif depth >= 1 and "scratch_" in ln:
                hot.append((depth, ln.strip()))
        seen += 1
        assert not [h for h in hot if h[0] >= 2], (m.group(1), hot)
        allowed = 1 if (int(m.group(3)) == 192 or int(m.group(4))) else 0
        if int(m.group(3)) == 192 and int(m.group(2)) == 32:
            allowed = 12
        assert len(hot) <= allowed, (m.group(1), hot)
    assert seen == 10, seen
