"""CPU: the text tower's entry points refuse bad arguments before the device is touched -- through ctypes, and under
AddressSanitizer + UBSan through the stand-alone tests/native/text_host_check.cpp (`make text_check`)."""
import ctypes as C
import os
import subprocess

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")


def test_refusals_through_the_binding():
    lib = _lib.load()
    tok = np.ones((3, 5), dtype=np.int32)
    out = np.zeros((3, 64), dtype=np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.revo_text_forward(None, p(tok), 3, 5, p(out), 1, None) == -2 and b"null argument" in lib.revo_last_error()
    assert lib.revo_text_forward(None, p(tok), 0, 5, p(out), 1, None) == -2 and b"at least 1" in lib.revo_last_error()
    assert lib.revo_text_forward(None, p(tok), 3, 0, p(out), 1, None) == -2 and b"at least 1" in lib.revo_last_error()
    assert lib.revo_text_destroy(None) == 0
    h = C.c_void_p()
    cfg = _lib.TextCfg(16, 64, 128, 2, 4, 512, 64, 0, 1e-5)        # head_dim 32
    arr = (_lib.Tensor * 1)()
    assert lib.revo_text_create(C.byref(cfg), arr, 0, 0, 4, C.byref(h)) == -2 and b"head_dim must be 64" in lib.revo_last_error()
    cfg = _lib.TextCfg(129, 64, 128, 2, 2, 512, 64, 0, 1e-5)
    assert lib.revo_text_create(C.byref(cfg), arr, 0, 0, 4, C.byref(h)) == -2 and b"context_length above 128" in lib.revo_last_error()
    cfg = _lib.TextCfg(16, 64, 128, 2, 2, 512, 64, 0, 1e-5)
    assert lib.revo_text_create(C.byref(cfg), arr, 0, 0, 4, C.byref(h)) == -2
    assert b"missing weight tensor: token_embedding.weight" in lib.revo_last_error()
    assert lib.revo_op_attention_causal(p(out), 192, p(out), 64, 1, 8, 1, 96, None) == -2
    assert lib.revo_op_embed_tokens(None, p(out), p(out), 1, 1, 64, 8, p(out), 8, None) == -2
    assert lib.revo_op_pool_eot(None, p(out), 64, 1, 5, 64, p(out), None) == -2 and b"null argument" in lib.revo_last_error()
    assert lib.revo_op_pool_eot(p(tok), p(out), 32, 1, 5, 64, p(out), None) == -2 and b"row stride below width" in lib.revo_last_error()
    # the hooks that stop a forward early exist in the experiment library only
    assert not hasattr(lib, "revo_text_set_debug_layers") and hasattr(_lib.load_exp(), "revo_text_set_debug_layers")


def test_text_entry_points_under_address_and_ub_sanitizers():
    subprocess.run(["make", "-C", CSRC, "-j", "4", "all", "text_check"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "text_host_check")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("create: null arguments", "create: shapes the kernels do not take", "create: the checkpoint, by name",
                 "forward: refusals that need no handle", "ops: refusals", "create: a complete checkpoint reaches the device"):
        assert case in r.stdout
