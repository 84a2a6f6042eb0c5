"""Record which GEMM launch forms the experiment library takes over a sweep of shapes: tests/golden/gemm_forms_parent.json.

    python scripts/gemm_forms_record.py OUT.json          (needs a GPU and librevo_exp.so)

The table is the reference of tests/test_gemm_plan.py (CPU tier): the host plan (csrc/gemm_plan.h, dumped through
revo_debug_gemm_plan) must name, row for row, the forms recorded here.  The committed table was recorded with the library
built from the commit BEFORE the launcher was rewritten around gemm_plan.h; regenerate it only from a build whose launch
choices are known good, never to make a failing test pass.

Every operand is allocated once per shape and never initialised: the job launches, reads revo_debug_gemm_forms and checks
nothing else.  A call the library refuses (the residual stream in planes at a shape whose form cannot fold) is recorded
as -1.  Rows: [kind, M, N, K, variant, qstores, form bits]; the kinds are those of tests/_kernel_bounds.py GEMM_FORM_CASES.
The patch-embedding epilogue has no single-kernel entry point and is not recorded."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _kernel_bounds as kb  # noqa: E402
import reverso_amd  # noqa: E402,F401
from reverso_amd import _lib  # noqa: E402

SWEEP_M = [1, 64, 65, 197, 577, 1023, 1024, 4616, 17000, 32768, 33000, 36928, 73856]
EPI = {"bf16": 0, "gelu": 1, "resid": 2, "f32": 3}
RESID_LN = ["resid_ln:none", "resid_ln:out", "resid_ln:inout", "resid_ln:in"]


def tower_pairs():
    """(N, K, tower name or None for the pairs without RoPE) of the four body GEMMs of every tower"""
    out = []
    for name, t in kb.TOWERS.items():
        W, Md = t["W"], t["Md"]
        out += [(3 * W, W, name), (W, W, None), (Md, W, None), (W, Md, None)]
    return out


def kinds_at(N, K, tower):
    kinds = ["bf16", "gelu", "f32", "resid", "resid_norm"] + RESID_LN
    if K % 256 == 0 and K // 256 <= 6:
        kinds.append("ln_in:gelu")
    if tower:
        kinds.append("rope")
        if K % 256 == 0 and K // 256 <= 6:
            kinds.append("ln_in_rope")
    return kinds


class Buffers:
    """Everything any kind reads or writes at one shape, uninitialised."""

    def __init__(self, M, N, K, tower, dev):
        e = lambda *s, dt=torch.float32: torch.empty(*s, device=dev, dtype=dt)      # noqa: E731
        bf = torch.bfloat16
        self.a, self.b = e(M, K, dt=bf), e(N, K, dt=bf)
        self.c = e(M, N)                                   # fp32 rows; the bf16 epilogues use its first half
        self.bias, self.gamma, self.csum = e(N), e(N), e(N)
        self.xb, self.xlo, self.h = e(M, N, dt=bf), e(M, N, dt=bf), e(M, N, dt=bf)
        self.stats_out = e(M, max(1, N // 256), 2)
        self.stats_in = e(M, max(1, K // 256), 2)
        t = kb.TOWERS[tower] if tower else None
        self.S, self.hd = (t["S"], t["hd"]) if t else (1, 64)
        self.cs = e(self.S, self.hd // 2, 2)


def launch(lib, kind, buf, M, N, K):
    """one call; returns the library's status"""
    P, st = _lib.ptr, _lib.current_stream()
    if kind in EPI:
        return lib.revo_op_gemm(EPI[kind], P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias),
                                P(buf.gamma) if kind == "resid" else None, st)
    if kind == "rope":
        return lib.revo_op_gemm_rope(P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias), P(buf.cs), buf.S, buf.hd,
                                     2 * K, st)
    if kind == "ln_in_rope":
        return lib.revo_op_gemm_ln_in_rope(P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias), P(buf.csum),
                                           P(buf.stats_in), K // 256, 1e-5, P(buf.cs), buf.S, buf.hd, 2 * K, st)
    if kind.startswith("ln_in:"):
        return lib.revo_op_gemm_ln_in(EPI[kind.split(":")[1]], P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias),
                                      P(buf.csum), P(buf.stats_in), K // 256, 1e-5, None, st)
    if kind == "resid_norm":
        fused = ctypes.c_int32(0)
        return lib.revo_op_gemm_resid_norm(P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias), P(buf.gamma), P(buf.h), N,
                                           1e-5, ctypes.byref(fused), st)
    planes = kind.split(":")[1]
    pin, pout = planes in ("in", "inout"), planes in ("out", "inout")
    done = ctypes.c_int32(0)
    return lib.revo_op_gemm_resid_ln(P(buf.a), K, P(buf.b), K, M, N, K, P(buf.c), N, P(buf.bias), P(buf.gamma), P(buf.xb), N,
                                     None if planes == "in" else P(buf.stats_out), ctypes.byref(done),
                                     P(buf.xlo) if planes != "none" else None, int(pin), int(pout), st)


def record(lib, kind, buf, M, N, K, variant=0, qstores=1):
    try:
        lib.revo_op_set_variant(variant)
        lib.revo_op_set_qstores(qstores)
        lib.revo_debug_gemm_forms(1)
        rc = launch(lib, kind, buf, M, N, K)
        bits = lib.revo_debug_gemm_forms(1)
    finally:
        lib.revo_op_set_variant(0)
        lib.revo_op_set_qstores(1)
    return [kind, M, N, K, variant, qstores, bits if rc == 0 else -1]


def main(out_path):
    dev = torch.device("cuda", 0)
    lib = _lib.load_exp()
    rows = []
    for N, K, tower in tower_pairs():
        for M in SWEEP_M:
            buf = Buffers(M, N, K, tower, dev)
            for kind in kinds_at(N, K, tower):
                rows.append(record(lib, kind, buf, M, N, K))
            torch.cuda.synchronize()
            del buf
    # the forced variants, only at the shapes where GEMM_FORM_CASES already runs them
    for _, kind, M, N, K, opts, _ in kb.GEMM_FORM_CASES:
        if "variant" in opts or "qstores" in opts:
            buf = Buffers(M, N, K, opts.get("tower"), dev)
            rows.append(record(lib, kind, buf, M, N, K, opts.get("variant", 0), opts.get("qstores", 1)))
            torch.cuda.synchronize()
            del buf
    with open(out_path, "w") as f:
        f.write('{"columns": ["kind", "M", "N", "K", "variant", "qstores", "forms"], "rows": [\n')
        f.write(",\n".join(json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} rows -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
