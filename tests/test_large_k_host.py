"""CPU: the large-k search's argument checks (they return before the device is touched) and the register allocation of its
kernels (topk_large.hip, from hipcc's own resource report: hipcc cross-compiles for gfx950 without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import reverso_amd  # noqa: F401
from reverso_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _call(lib, g, Q, k, q=True):
    buf = C.create_string_buffer(64)
    qp = C.cast(buf, C.c_void_p) if q else None
    out = C.cast(buf, C.c_void_p)
    return lib.revo_search_topk_large(g, qp, Q, k, 0, 0.0, 0, out, out, out, None)


def test_argument_checks_without_a_device():
    lib = _lib.load()
    assert _call(lib, None, 1, 100) == -2 and b"null" in lib.revo_last_error()
    # a stand-in handle: these checks come before the handle is read
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    assert _call(lib, fake, 1, 0) == -2 and b"k must be in [1, 1024]" in lib.revo_last_error()
    assert _call(lib, fake, 1, 1025) == -2 and b"k must be in [1, 1024]" in lib.revo_last_error()
    assert _call(lib, fake, -1, 100) == -2 and b"negative query count" in lib.revo_last_error()
    assert _call(lib, fake, 1, 100, q=False) == -2 and b"null" in lib.revo_last_error()


def test_binding_and_export():
    assert "revo_search_topk_large" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "revo_search_topk_large") and hasattr(_lib.load_exp(), "revo_search_topk_large")


def test_large_k_kernels_do_not_spill():
    """Every kernel of topk_large.hip: no VGPR spills and no scratch (the count pass runs the 256 x 256 main loop at up to
    256 VGPRs; a spill inside its tile loop would wait for the next tile's operand DMA)."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-c",
                          "topk_large.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC,
                         capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    cur, d = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        for key, pat in (("VGPRs Spill", r"VGPRs Spill: (\d+)"), ("ScratchSize", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                d[cur][key] = int(m.group(1))
    names = [k for k in d if "topk_large" in k]
    assert len(names) >= 8, names            # sample, count x 3 row modes, level, rescore, sort, fallback score + select
    for k in names:
        assert d[k]["VGPRs Spill"] == 0 and d[k]["ScratchSize"] == 0, (k, d[k])
