"""hipcc's own resource report of the kernels of one source file (`-Rpass-analysis=kernel-resource-usage`; hipcc cross-compiles
for gfx950 without a GPU), for the CPU tests that hold kernels to a register allocation."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_FIELDS = (("VGPRs", r" VGPRs: (\d+)"), ("VGPRs Spill", r"VGPRs Spill: (\d+)"), ("SGPRs Spill", r"SGPRs Spill: (\d+)"),
           ("ScratchSize", r"ScratchSize \[bytes/lane\]: (\d+)"), ("LDS Size", r"LDS Size \[bytes/block\]: (\d+)"))


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


def assert_no_spill(src, name_part, count):
    """Every kernel of `src` whose name holds `name_part` -- there are `count` of them -- has no VGPR spills and no scratch."""
    d = usage(src)
    names = [k for k in d if name_part in k]
    assert len(names) == count, names
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
