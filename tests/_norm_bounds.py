"""Bounds of the row normaliser (elementwise.hip l2norm_rows_kernel) and of the rounding norms it measures for the exactness
certificate (kernels.h cert_eps), in the conventions of tests/_head_bounds.py: `reference` (fp64 on the exact fp32 input),
`bound` (what the kernel's rounding steps as written allow), `emulate` (those roundings in fp32, the kernel's lane assignment
and its xor butterfly) and planted errors (the reference with a plausible bug in it).  The case list at the end is shared by
the CPU teeth test (tests/test_norm_bounds_teeth.py) and the GPU test (tests/test_gpu_norm_bounds.py).

The kernel, per row (one wave; lane l holds columns l, l + 64, ...: n = ceil(D / 64) of them):
  q = fma(x, x, q) per lane     n roundings                             E_CHAIN
  wave_sum(q)                   the butterfly 32, 16 .. 1: 6 roundings   E_TREE
  s = sqrtf(q)                  E_SQRT
  inv = 1.0f / s                E_DIV
  y = x * inv                   E_MUL (the output's own rounding); a subnormal y is off by up to half the subnormal spacing,
                                which ties attain: one whole spacing, SUB, is allowed (as _head_bounds allows a whole ulp)
All terms of q are non-negative, so its error is relative: (n + 6) U_F32.  An fma whose result lands below 2^-126 errs by
SUB / 2 absolute instead, whatever its size (sums of subnormals are exact), and such errors add over the row's D fmas, not
along one path: D SUB / 2 on q is the bound's absolute term.  It is nothing against the relative part from
||x|| ~ sqrt(D) 2^-62 up, grows below, and ends the claim where q has lost its bits (||x|| ~ sqrt(D) 2^-74).  So the bound holds
wherever the fp32 sum of squares neither overflows nor vanishes: at ||x|| >= NORM_HI = 2^64 q = +inf, inv = 0 and the row
comes out as zeros; once every x^2 rounds to 0 (|x| <= 2^-75) q = 0 and the row is left as it is.  NORM_LO = 2^-63: from
there up q is a normal number.

sqrtf and the division.  The build passes no fast-math flag, and for HIP device code the compiler's default is
-fhip-fp32-correctly-rounded-divide-sqrt: the IR of `1.0f / x` and `sqrtf(x)` carries no !fpmath accuracy note, i.e. both
are CORRECTLY ROUNDED (half an ulp: U_F32 relative).  Denormals are not flushed (-fgpu-flush-denormals-to-zero is off by
default): gradual underflow, hence SUB and not 2^-126.  No constant here is fitted to GPU output.

The statistics.  For the row y the kernel returned and b = bf16(y) (round to nearest even; b - y is exact in fp32) it sums
y^2, b^2 and (b - y)^2 as above, on the row times 2^k (k from the exponent of the largest |y|: exact), takes sqrtf and
scales back by 2^-k (exact unless the root is subnormal: SUB, as above).  Above D = 2048 the loop form adds runs of 32 steps
into the row's total: min(n, 32) + ceil(n / 32) - 1 + 6 roundings.  Non-negative terms: a relative bound, halved by the
root, plus E_SQRT.  Reference: the fp64 norms of the rows the kernel actually returned."""
import math

import torch

from _kernel_bounds import NOT_CAUGHT, U_F32, not_caught, ratio  # noqa: F401

SECOND = 1 + 2.0 ** -10                # second-order terms of a few hundred roundings
SUB = 2.0 ** -149                      # fp32's subnormal spacing
NV = 32                                # the register form holds 64 NV columns; the loop form sums in runs of NV steps
NORM_LO, NORM_HI = 2.0 ** -63, 2.0 ** 64   # normalize = 1: the fp32 sum of squares is a normal number for NORM_LO <= ||x|| < NORM_HI
D_MAX = (2 ** 31 // 512 - 1) // 64 * 64    # the largest D a search launcher accepts (kernels.h g256_check_operands)
E_SQRT, E_DIV, E_MUL = U_F32, U_F32, U_F32
CERT_ROUNDINGS = 13                    # fp32 operations of cert_eps that can round (D 2^-23 and D 2^-24 are exact)


def _up(a, b):
    return -(-a // b)


def chain_roundings(D, runs):
    """roundings of one sum of squares: the lane's chain (in runs of NV added to a total if `runs` and D > 64 NV), the tree"""
    n = _up(D, 64)
    return (n if not runs or n <= NV else NV + _up(n, NV) - 1) + 6


# ------------------------------------------------------------------ fp32 pieces of the emulation ----
def _fma(a, b, c):
    """fp32 fma: the product is exact in fp64, the sum rounds to 53 bits before it rounds to 24 (torch has no fma)"""
    return (a.double() * b.double() + c.double()).float()


def _lanes(v):
    """[rows, D] -> [rows, n, 64]: element (i, l) is column l + 64 i, zeros past D (fma(0, 0, q) = q: as if skipped)"""
    rows, D = v.shape
    n = _up(D, 64)
    p = torch.zeros(rows, n * 64, dtype=v.dtype)
    p[:, :D] = v
    return p.view(rows, n, 64)


def wave_sum32(p):
    """common.h wave_sum on [rows, 64] fp32: v += shfl_xor(v, o) for o = 32, 16 .. 1; every lane ends with the total"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, idx ^ o]
    return p[:, 0]


def lane_sums32(v, runs=False, lanes=None):
    """the per-lane fp32 sums of squares of v [rows, D], [rows, 64]"""
    p = _lanes(v.float())
    rows, n, _ = p.shape
    total = torch.zeros(rows, 64)
    if not runs or n <= NV:
        for i in range(n):
            total = _fma(p[:, i], p[:, i], total)
        return total
    for i0 in range(0, n, NV):
        run = torch.zeros(rows, 64)
        for i in range(i0, min(n, i0 + NV)):
            run = _fma(p[:, i], p[:, i], run)
        total = total + run
    return total


def sumsq32(v, runs=False):
    return wave_sum32(lane_sums32(v, runs))


def bf16_rne(y32):
    return y32.bfloat16().float()


def bf16_trunc(y32):
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def finite_rows(x):
    return torch.isfinite(x).all(-1)


# ------------------------------------------------------------------ the rows ----
class Rows:
    """x: fp32 [rows, D], every row finite; normalize = 1 (normalize = 0 is a bit copy: no bound to hold)."""

    @staticmethod
    def reference(x, cols=None):
        xd = x.double()
        q = (xd if cols is None else xd[:, :cols]).pow(2).sum(-1, keepdim=True)
        y = torch.where(q > 0, xd / q.sqrt(), xd)
        if cols is not None:
            y[:, cols:] = 0
        return y

    @staticmethod
    def bound(x):
        xd = x.double()
        D = x.shape[1]
        m = chain_roundings(D, False)
        q = xd.pow(2).sum(-1, keepdim=True)
        e_chain, e_tree = (m - 6) * U_F32 / 2, 6 * U_F32 / 2            # on the root of q
        e_abs = torch.where(q > 0, D * (SUB / 2) / q / 2, torch.zeros_like(q))
        rel = (e_chain + e_tree + E_SQRT + E_DIV + E_MUL + e_abs) * SECOND
        rel = torch.where(e_abs < 0.25, rel, torch.full_like(rel, math.inf))     # (no claim once q has lost its bits)
        return Rows.reference(x).abs() * rel + SUB

    @staticmethod
    def emulate(x):
        x = x.float()
        q = sumsq32(x)[:, None]
        inv = torch.where(q > 0, 1.0 / q.sqrt(), torch.ones_like(q))
        return x * inv


def _rows_last_register(x):
    D = x.shape[1]
    return Rows.reference(x, 64 * (NV - 1)) if 64 * (NV - 1) < D <= 64 * NV else None


def _rows_loop_stops(x):
    D = x.shape[1]
    return Rows.reference(x, D // 64 * 64) if D > 64 * NV else None


Rows.MUTATIONS = [
    ("last register of the register form dropped", _rows_last_register, 3.0),
    ("loop form stops at D rounded down to 64", _rows_loop_stops, 3.0),
]


# ------------------------------------------------------------------ the statistics ----
class Stats:
    """y: the fp32 rows as returned [rows, D] (finite).  Results [rows, 3]: ||bf16(y) - y||, ||bf16(y)||, ||y|| -- row_stats'
    two columns and the quantity max_stats[0] takes its maximum of."""

    @staticmethod
    def reference(y, cols=None, lanes=None, trunc=False):
        y = y.float()
        b = bf16_trunc(y) if trunc else bf16_rne(y)
        yd, bd = y.double(), b.double()
        keep = torch.ones(y.shape[1], dtype=torch.bool)
        if cols is not None:
            keep[cols:] = False
        if lanes is not None:
            keep &= lanes[torch.arange(y.shape[1]) % 64]
        w = keep.double()
        return torch.stack([((bd - yd).pow(2) * w).sum(-1).sqrt(), (bd.pow(2) * w).sum(-1).sqrt(), (yd.pow(2) * w).sum(-1).sqrt()], -1)

    @staticmethod
    def sigma(D):
        """the relative error of one statistic"""
        return (chain_roundings(D, True) / 2 + E_SQRT / U_F32) * U_F32 * SECOND

    @staticmethod
    def bound(y):
        return Stats.reference(y) * Stats.sigma(y.shape[1]) + SUB

    @staticmethod
    def scale(y):
        """elementwise.hip stat_scale: (2^k, 2^-k) per row, k = 127 - the exponent field of the largest |y|, within +-126"""
        E = (y.float().abs().max(-1).values.view(torch.int32) >> 23) & 0xff
        k = (127 - E).clamp(-126, 126)
        two = lambda e: ((127 + e).to(torch.int32) << 23).view(torch.float32)[:, None]        # 2^e from its exponent field
        return two(k), two(-k)

    @staticmethod
    def emulate(y, scaled=True):
        """scaled = False: the sums of squares in plain fp32, as the kernel took them before it scaled the row"""
        y = y.float()
        b = bf16_rne(y)
        sc, rs = Stats.scale(y) if scaled else (torch.ones(len(y), 1), torch.ones(len(y), 1))
        return torch.stack([sumsq32((b - y) * sc, True).sqrt() * rs[:, 0], sumsq32(b * sc, True).sqrt() * rs[:, 0],
                            sumsq32(y * sc, True).sqrt() * rs[:, 0]], -1)


def maxima(stats, initial=(0.0, 0.0)):
    """max_stats after a call over rows with these stats [rows, 3] (rows that are not finite already taken out):
    (max ||y||, max ||bf16(y) - y||), never below what it held"""
    z = stats.new_tensor(initial)
    if len(stats) == 0:
        return z
    return torch.maximum(z, torch.stack([stats[:, 2].max(), stats[:, 0].max()]))


_LANE0 = torch.zeros(64, dtype=torch.bool)
_LANE0[0] = True
_LANES63 = torch.ones(64, dtype=torch.bool)
_LANES63[63] = False


def _st_no_reduction(y):
    s = Stats.reference(y)
    s[:, 0] = Stats.reference(y, lanes=_LANE0)[:, 0]
    return s


def _st_norm_swapped(y):
    s = Stats.reference(y)
    s[:, 1] = s[:, 2]
    return s


def _st_last_register(y):
    D = y.shape[1]
    return Stats.reference(y, cols=64 * (NV - 1)) if 64 * (NV - 1) < D <= 64 * NV else None


def _st_loop_stops(y):
    D = y.shape[1]
    return Stats.reference(y, cols=D // 64 * 64) if D > 64 * NV else None


# on [rows, 3]; the maxima follow from them (maxima())
Stats.MUTATIONS = [
    ("error norm without its wave reduction", _st_no_reduction, 3.0),
    ("sums over 63 lanes", lambda y: Stats.reference(y, lanes=_LANES63), 3.0),
    ("||y|| written where ||bf16(y)|| belongs", _st_norm_swapped, 3.0),
    ("error norm against a truncated bf16", lambda y: Stats.reference(y, trunc=True), 3.0),
    ("last register of the register form dropped", _st_last_register, 3.0),
    ("loop form stops at D rounded down to 64", _st_loop_stops, 3.0),
]

_SAME = "the mutation is the identity there: "
NOT_CAUGHT.update({
    ("norm stats", "error norm without its wave reduction"): (
        lambda c: c["exact_bf16"] or c["D"] == 1, _SAME + "the error norm is exactly 0 (every element is a bf16 number), or lane 0 holds the whole row"),
    ("norm stats", "sums over 63 lanes"): (
        lambda c: c["D"] < 64 or c["lane63_empty"], _SAME + "lane 63 holds no column below D = 64, or only zeros (one-hot rows elsewhere)"),
    ("norm stats", "||y|| written where ||bf16(y)|| belongs"): (
        lambda c: c["exact_bf16"] or c["fixture"] == "spike" or c["D"] == 1,
        "bf16(y) = y on one-hot and zero rows; a row that is one element of 1 or 1 - 2^-24 (D = 1; a spike beside 1e-6's) "
        "rounds to a bf16 row whose norm differs by an fp32 ulp at most"),
    ("norm stats", "error norm against a truncated bf16"): (lambda c: c["exact_bf16"], _SAME + "bf16(y) = y either way"),
    ("norm stats", "loop form stops at D rounded down to 64"): (lambda c: c["D"] % 64 == 0, _SAME + "D is a multiple of 64"),
    ("norm rows", "loop form stops at D rounded down to 64"): (lambda c: c["D"] % 64 == 0, _SAME + "D is a multiple of 64"),
})


def facts(spec, y):
    """what NOT_CAUGHT's predicates ask of a case (y: the finite rows as returned)"""
    y = y.float()
    lane63 = y[:, 63::64]
    return dict(spec, exact_bf16=bool((bf16_rne(y) == y).all()), lane63_empty=bool((lane63 == 0).all()))


# ------------------------------------------------------------------ the certificate ----
def cert_eps32(e_q, n_qb, G, Eg, D):
    """kernels.h cert_eps in fp32, operation by operation (not contracted; a contraction only removes roundings)"""
    f = lambda t: torch.as_tensor(t, dtype=torch.float32)
    e_q, n_qb, G, Eg = f(e_q), f(n_qb), f(G), f(Eg)
    gam1, gam2 = f(float(D)) * f(1.1920929e-7), f(float(D)) * f(5.9604645e-8)
    eps = e_q * G + n_qb * Eg + gam1 * n_qb * (G + Eg) + gam2 * (n_qb + e_q) * G
    return eps * f(1.001) + f(1e-30)


def cert_eps64(e_q, n_qb, G, Eg, D):
    """the same formula in fp64 on exact norms, with neither the 1.001 nor the 1e-30"""
    return e_q * G + n_qb * Eg + D * 2.0 ** -23 * n_qb * (G + Eg) + D * 2.0 ** -24 * (n_qb + e_q) * G


UNIT_QUERY = (2.0 ** -10, 1.0, 1.0)     # a query as every search makes them: unit length, a typical rounding norm (exact in fp32)


def direction_holds(stats32, max32, exact, D):
    """every pair (row as query, maxima as gallery), and UNIT_QUERY against the maxima: eps from the kernel's own fp32 numbers
    (stats32 [rows, 2], max32 [2]) is at least eps from the fp64 norms `exact` [rows, 3] of the same rows.  Returns (ok, the
    smallest eps32 / eps64)."""
    if len(exact) == 0:
        return True, math.inf
    G, Eg = exact[:, 2].max(), exact[:, 0].max()
    unit = torch.tensor([UNIT_QUERY])
    stats32, exact = torch.cat([stats32[:, :2].float(), unit[:, :2]]), torch.cat([exact, unit.double()])
    got = cert_eps32(stats32[:, 0], stats32[:, 1], max32[0], max32[1], D).double()
    want = cert_eps64(exact[:, 0], exact[:, 1], G, Eg, D)
    r = torch.where(want > 0, got / want, torch.full_like(want, math.inf))
    return bool((got >= want).all()), float(r.min())


def slack_covers(D, runs=True):
    """1.001 against the worst case of the analysis: both stats of every product understated by sigma(D), every one of the
    CERT_ROUNDINGS operations rounding down.  (Absolute parts: a subnormal stat is off by SUB / 2; the 1e-30 covers its
    product with any norm up to 1e14.)"""
    sigma = (chain_roundings(D, runs) / 2 + 1) * U_F32 * SECOND
    return 1.001 * (1 - sigma) ** 2 * (1 - U_F32) ** CERT_ROUNDINGS >= 1.0


# ------------------------------------------------------------------ the cases ----
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


DIMS = [1, 63, 64, 65, 128, 1000, 1024, 2048, 2049, 2112, 4160]
ROWS = [1, 3, 4, 5, 67]
OUTS = ["both", "f32", "bf16", "none"]
FIXTURES = ["randn", "randn as given", "one-hot", "midpoint", "spike", "x 2^40", "x 2^-40", "subnormal", "negative zero",
            "zero row", "nan inf", "huge", "tiny"]
AS_GIVEN = {"randn as given", "midpoint", "huge", "tiny"}            # normalize = 0
FIXTURE_SHAPES = [(128, 5), (1000, 4), (2112, 5)]
HUGE_NORM, TINY_NORM = 1e20, 1e-20


def _cases():
    out = []
    for i, D in enumerate(DIMS):
        for j, R in enumerate(ROWS):
            if (i + j) % 2 == 0 or D in (128, 2048, 2049):
                k = len(out)
                out.append(dict(D=D, rows=R, fixture="randn", outs=OUTS[k % 4], pads=(3, 5, 7) if k % 2 else (0, 0, 0)))
    for D, R in FIXTURE_SHAPES:
        for f in FIXTURES[1:]:
            out.append(dict(D=D, rows=R, fixture=f, outs="both", pads=(0, 0, 0)))
    return out


CASES = _cases()


def case_id(c):
    return f"D{c['D']} rows{c['rows']} {c['fixture']} {c['outs']}" + (" padded" if any(c["pads"]) else "")


def normalize_of(spec):
    return 0 if spec["fixture"] in AS_GIVEN else 1


def midpoint_rows(x):
    """every element moved to just above a bf16 rounding midpoint (test_certificate_error_bound_is_rigorous): bf16(y) - y has
    the sign of y and nearly its largest size, 2^-9 |y|"""
    u = x.abs().contiguous().view(torch.int32)
    return ((u & -65536) | 0x8001).view(torch.float32)


def case_rows(spec):
    """the fp32 source rows [rows, D] of a case (CPU)"""
    D, R, f = spec["D"], spec["rows"], spec["fixture"]
    g = _gen(D, R, f)
    x = torch.randn(R, D, generator=g)
    unit = (x.double() / x.double().norm(dim=-1, keepdim=True))
    r = torch.arange(R)
    if f == "one-hot":
        x = torch.zeros(R, D)
        col = (63 + 37 * r) % D                     # row 0 in lane 63 (from D = 64 on)
        x[r, col] = torch.where(r % 2 == 0, 1.0, -1.0) * (1.0 + r.float())
    elif f == "midpoint":
        x = midpoint_rows(unit.float())
    elif f == "spike":
        x[r, (torch.full_like(r, 63) + 64 * r) % D] = 1e6
    elif f == "x 2^40":
        x = x * 2.0 ** 40
    elif f == "x 2^-40":
        x = x * 2.0 ** -40
    elif f == "subnormal":
        x[:, 1::5] = 1e-40
        x[:, 3::7] = -3e-42
    elif f == "negative zero":
        x[:, ::3] = -0.0
    elif f == "zero row":
        x[R // 2] = 0.0
    elif f == "nan inf":
        x[1, D // 3] = math.nan                     # rows 1 and 2 of the first four-row workgroup, good rows around them
        x[2, D // 2] = math.inf
    elif f == "huge":
        x = unit.float()
        x[1] = (unit[1] * HUGE_NORM).float()
    elif f == "tiny":
        x = (unit * TINY_NORM).float()
    elif f == "randn as given":
        x[:, 2::11] = 1e-40
        x[:, 5::13] = -0.0
    return x


# ---- the other duties: the row map, the maxima across calls, the arrays cleared
CLEAR_COUNTS = [0, 1, 255, 256, 257, 300001]
CLEAR_ROWS = [1, 67]


def row_map(rows, n_dst):
    """distinct destination rows, not in order, none equal to its source row where that can be avoided"""
    g = _gen(rows, n_dst, "map")
    m = torch.randperm(n_dst, generator=g)[:rows]
    return torch.where(m == torch.arange(rows), (m + 1) % n_dst, m) if rows == 1 else m


def stats_at_destination(stats, m):
    """planted: row_stats indexed by the destination row (entries past the array are lost, the others keep what they held: 0)"""
    out = torch.zeros_like(stats)
    ok = m < len(stats)
    out[m[ok]] = stats[ok]
    return out


def cleared(words, whole_blocks_only=False):
    """what an array of `words` ones holds after the clearing loop (planted: the words past the last whole block of 256 missed)"""
    a = torch.ones(words, dtype=torch.int32)
    a[:words // 256 * 256 if whole_blocks_only else words] = 0
    return a
