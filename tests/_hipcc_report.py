"""hipcc's own resource report of the kernels of one source file (`-Rpass-analysis=kernel-resource-usage`; hipcc cross-compiles
for gfx950 without a GPU) and its device listing, for the CPU tests that hold kernels to a register allocation.  Both are
compiled once per source file and test run, whichever test modules ask."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_FIELDS = (("VGPRs", r" VGPRs: (\d+)"), ("VGPRs Spill", r"VGPRs Spill: (\d+)"), ("SGPRs Spill", r"SGPRs Spill: (\d+)"),
           ("ScratchSize", r"ScratchSize \[bytes/lane\]: (\d+)"), ("LDS Size", r"LDS Size \[bytes/block\]: (\d+)"))


@functools.lru_cache(maxsize=None)
def usage(src):
    """{mangled kernel name: {"VGPRs": n, "VGPRs Spill": n, "SGPRs Spill": n, "ScratchSize": n, "LDS Size": n}} for one
    source file of csrc/."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-c", src,
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True,
                         text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    cur, d = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        for key, pat in _FIELDS:
            m = re.search(pat, line)
            if m and cur:
                d[cur][key] = int(m.group(1))
    return d


@functools.lru_cache(maxsize=None)
def listing(src):
    """hipcc's device listing (`-S --cuda-device-only`) of one source file of csrc/."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-S",
                          "--cuda-device-only", src, "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def scratch_in_loops(asm, name_pattern):
    """[(regex match of the function's label, [(loop depth, line)])] for every function of a listing whose label matches
    `name_pattern`: the lines that touch scratch inside a loop, with the depth hipcc notes at the head of their basic block."""
    found = []
    for m in re.finditer(r"^(" + name_pattern + r"):", asm, flags=re.M):
        body = asm[m.end(): asm.index(".Lfunc_end", m.end())].splitlines()
        depth, hot = 0, []
        for ln in body:
            if ln.startswith(".LBB") or ln.startswith("; %bb."):
                dm = re.search(r"Depth=(\d+)", ln)
                depth = int(dm.group(1)) if dm else 0
            elif depth >= 1 and "scratch_" in ln:
                hot.append((depth, ln.strip()))
        found.append((m, hot))
    return found


def assert_no_spill(src, name_part, count):
    """Every kernel of `src` whose name holds `name_part` -- there are `count` of them -- has no VGPR spills and no scratch."""
    d = usage(src)
    names = [k for k in d if name_part in k]
    assert len(names) == count, names
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
