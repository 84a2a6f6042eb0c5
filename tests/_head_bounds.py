"""Per-element error bounds of the fp32 attention-pool head (head.hip, region_pool.hip, the ln_post kernels with logits in
elementwise.hip), in the conventions of tests/_kernel_bounds.py: for every op `reference` (fp64 on the exact fp32 inputs),
`bound` (elementwise |kernel - reference| allowed by the kernel's rounding steps as written), `emulate` (the reference with
those roundings in fp32) and `MUTATIONS` (plausible bugs: the reference with the bug in it).  The case lists at the end are
shared by the CPU teeth test (tests/test_head_bounds_teeth.py) and the GPU test (tests/test_gpu_head_bounds.py).

Device math.  The ROCm device-library documentation installed with the toolchain states no accuracy for expf, erff or
rsqrtf, so expf and erff are ASSUMED to be within MATH_ULPS = 4 ulp (a relative 4 x 2^-23); rsqrtf is inside
kb.LayerNorm.bound, which the body's LayerNorm already holds.  No constant here is fitted to GPU output.

fp32 subnormals: an exp or a probability below 2^-126 may be flushed to zero; the TINY terms allow that."""
import math

import torch

from _kernel_bounds import (GELU_SLOPE_MAX, NOT_CAUGHT, U_F32, LayerNorm, _gelu64, f32_ulp, layernorm_rows,  # noqa: F401
                            not_caught, ratio, ulp)

MATH_ULPS = 4                          # assumed accuracy of the device's expf and erff (see above)
E_MATH = MATH_ULPS * 2 * U_F32         # ... as a relative error
SECOND = 1 + 2.0 ** -10                # the second-order terms of chains of a few hundred roundings
TINY = 2.0 ** -126                     # the smallest normal fp32


def _up(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ pooled rows ----
# Kernels (head.hip pool_accumulate_kernel<1 | 4>, region_pool.hip pool_accumulate_masked_kernel<1 | 4>; the masked one does
# the same steps over the allowed tokens only).  Per (image, head), with t_s = lg_s - m:
#   lg - m                    one rounding: U_F32 |t_s| absolute in the exponent = relative in e_s
#   expf                      E_MATH relative (assumed); a result below 2^-126 may be flushed: TINY absolute
#   sum of the e_s            ceil(S / 64) - 1 adds per lane, then the 6-level wave tree, positive terms: n_sum U_F32 relative
#   1 / sum                   one ulp = 2 U_F32 (correctly rounded unless the build says otherwise)
#   p = e * inv               U_F32, TINY absolute
# so p_s is off by p_s (eps_s + sum_j p_j eps_j + (n_sum + 3) U_F32) with eps_s = U_F32 |t_s| + E_MATH: the error of a
# probability is weighted by the probability, a token 100 below the maximum costs nothing.  (The e_j's own errors enter
# the sum as their p-weighted mean.)  Then per column
#   acc = fma(p, x, acc)      wave w takes s = w, w + 16, ...: a chain of ceil(S / 16) roundings
#   the 16-way LDS sum        15 adds in wave order
# each against sum_s p_s |x_s|.  The last add is the output's rounding: ulp_f32(ref) covers it once more.
class PoolRows:
    """x: fp32 [B, S, W] (the columns the kernel is given), logits: fp32 [B, H, S]; regions None (revo_op_pool_rows) or
    (region_image int64 [R], allow bool [R, S]) (revo_op_pool_rows_masked: the result is [R, H, W])."""

    @staticmethod
    def gather(x, logits, regions):
        xd, lg = x.double(), logits.double()
        if regions is None:
            return xd, lg, torch.ones(lg.shape[0], lg.shape[2], dtype=torch.bool, device=lg.device)
        ri, allow = regions
        return xd[ri.to(x.device)], lg[ri.to(x.device)], allow.to(x.device)

    @staticmethod
    def probs(lg, allow):
        """softmax over the allowed tokens (zeros for a region without one) and t = lg - max (0 where p is 0)"""
        lg = lg.masked_fill(~allow[:, None, :], -math.inf)
        m = lg.max(-1, keepdim=True).values
        t = lg - m
        e = torch.exp(t)
        p = torch.nan_to_num(e / e.sum(-1, keepdim=True), nan=0.0)
        return p, torch.where(p > 0, t, torch.zeros_like(t))

    @staticmethod
    def weighted(p, xd):
        return torch.einsum("bhs,bsw->bhw", p, xd)

    @staticmethod
    def reference(x, logits, regions=None):
        xd, lg, allow = PoolRows.gather(x, logits, regions)
        return PoolRows.weighted(PoolRows.probs(lg, allow)[0], xd)

    @staticmethod
    def bound(x, logits, regions=None):
        xd, lg, allow = PoolRows.gather(x, logits, regions)
        S = lg.shape[-1]
        p, t = PoolRows.probs(lg, allow)
        eps_e = U_F32 * t.abs() + E_MATH
        n_sum = _up(S, 64) - 1 + 6
        eps_p = eps_e + (p * eps_e).sum(-1, keepdim=True) + (n_sum + 2 + 1) * U_F32
        n_acc = _up(S, 16) + 15
        ax = xd.abs()
        d = PoolRows.weighted(p * (eps_p + n_acc * U_F32), ax) * SECOND + 3 * TINY * ax.sum(1)[:, None, :]
        return f32_ulp(PoolRows.weighted(p, xd)) + d

    @staticmethod
    def emulate(x, logits, regions=None):
        xd, lg, allow = PoolRows.gather(x, logits, regions)
        lg = lg.float().masked_fill(~allow[:, None, :], -math.inf)
        e = torch.exp(lg - lg.max(-1, keepdim=True).values)
        p = torch.nan_to_num(e * (1.0 / e.sum(-1, keepdim=True)), nan=0.0)
        return PoolRows.weighted(p, xd.float()).double()


def _pool_last_dropped(x, logits, regions=None):
    xd, lg, allow = PoolRows.gather(x, logits, regions)
    S = allow.shape[1]
    last = (allow * torch.arange(1, S + 1, device=allow.device)).max(-1).values - 1          # -1: no token
    allow = allow.clone()
    rows = torch.nonzero(last >= 0)[:, 0]
    allow[rows, last[rows]] = False
    p, _ = PoolRows.probs(lg, allow)
    # (a region left without a token: 0 / 0 in a kernel that drops its only row)
    p = torch.where(allow.any(-1)[:, None, None] | (last < 0)[:, None, None], p, torch.full_like(p, math.nan))
    return PoolRows.weighted(p, xd)


def _pool_heads_shifted(x, logits, regions=None):
    return PoolRows.reference(x, torch.roll(logits, -1, dims=1), regions)


def _pool_probs_bf16(x, logits, regions=None):
    xd, lg, allow = PoolRows.gather(x, logits, regions)
    return PoolRows.weighted(PoolRows.probs(lg, allow)[0].bfloat16().double(), xd)


def _pool_logits_bsh(x, logits, regions=None):
    B, H, S = logits.shape
    return PoolRows.reference(x, logits.reshape(B, S, H).permute(0, 2, 1), regions)


def _pool_no_max(x, logits, regions=None):
    xd, lg, allow = PoolRows.gather(x, logits, regions)
    e = torch.exp(lg.float().masked_fill(~allow[:, None, :], -math.inf))                  # fp32: overflows above 88.7
    p = (e / e.sum(-1, keepdim=True)).double()
    p = torch.where(allow.any(-1)[:, None, None], p, torch.zeros_like(p))
    return PoolRows.weighted(p, xd)


PoolRows.MUTATIONS = [
    ("last token dropped", _pool_last_dropped, 3.0),
    ("heads' logits shifted by one head", _pool_heads_shifted, 3.0),
    ("probabilities rounded to bf16", _pool_probs_bf16, 3.0),
    ("logits read as [B, S, H]", _pool_logits_bsh, 3.0),
    ("maximum not subtracted", _pool_no_max, 3.0),
]


# ------------------------------------------------------------------ ln_post + logits ----
# Kernels (elementwise.hip layernorm_kernel<MAXC, false> with lg.qk set: one row per wave; layernorm_logits_kernel<MAXC, 4, 8>:
# four rows per wave).  Read against kb.LayerNorm.bound: both take the mean from (v0 + v1) + (v2 + v3) per chunk, at most
# ceil(W / 256) chunks per lane, then the 64-lane tree (wave_sum; wave_sum_transposed adds the same tree); d = x - mean and
# q = fma(d, d, q) in the same lane order and the same tree; rstd = rsqrtf(q / W + eps); y = fma((x - mean) rstd, g, be).
# Those are the steps that bound counts, in both kernels, so the rows are held to it unchanged (out_bf16 = False).
# The logits: lacc_h = fma(y_c, qk_hc, lacc_h) over the lane's columns, 4 per chunk: a chain of 4 ceil(W / 256) roundings,
# then the 6-level wave tree, against sum_c |y_c| |qk_hc|; the computed y_c carries its own error: sum_c |qk_hc| bound_y_c;
# t + ck is the output's rounding: ulp_f32(ref).
class LnLogits:
    """x: fp32 [rows, W]; w / b: fp32 [W] or None (no affine); qk: fp32 [H, W]; ck: fp32 [H]; rows = B S.
    reference / bound / emulate return (rows [rows, W], logits [B, H, S])."""

    @staticmethod
    def affine(x, w, b):
        W = x.shape[-1]
        return (torch.ones(W, device=x.device) if w is None else w), (torch.zeros(W, device=x.device) if b is None else b)

    @staticmethod
    def logits_of(y, qk, ck, S):
        t = y @ qk.double().T + (0 if ck is None else ck.double())
        return t.view(-1, S, qk.shape[0]).permute(0, 2, 1)

    @staticmethod
    def reference(x, w, b, eps, qk, ck, S):
        w, b = LnLogits.affine(x, w, b)
        y = LayerNorm.reference(x, w, b, eps)
        return y, LnLogits.logits_of(y, qk, ck, S)

    @staticmethod
    def bound(x, w, b, eps, qk, ck, S):
        w, b = LnLogits.affine(x, w, b)
        W = x.shape[-1]
        y, lg = LnLogits.reference(x, w, b, eps, qk, ck, S)
        by = LayerNorm.bound(x, w, b, eps, False)
        aq = qk.double().abs().T
        n = 4 * _up(W, 256) + 6
        d = by @ aq + n * U_F32 * SECOND * (y.abs() @ aq)
        return by, f32_ulp(lg) + d.view(-1, S, qk.shape[0]).permute(0, 2, 1)

    @staticmethod
    def emulate(x, w, b, eps, qk, ck, S):
        w, b = LnLogits.affine(x, w, b)
        y = LayerNorm.emulate(x, w, b, eps, False)
        t = (y.float() @ qk.float().T + ck.float()).double()
        return y, t.view(-1, S, qk.shape[0]).permute(0, 2, 1)


def _lg_rows_mutated(f):
    """a LayerNorm mutation of the rows, seen through the logits as well"""
    def g(x, w, b, eps, qk, ck, S):
        w, b = LnLogits.affine(x, w, b)
        return LnLogits.logits_of(f(x, w, b, eps), qk, ck, S)
    return g


def _lg_no_ck(x, w, b, eps, qk, ck, S):
    return LnLogits.logits_of(LnLogits.reference(x, w, b, eps, qk, ck, S)[0], qk, None, S)


def _lg_next_head(x, w, b, eps, qk, ck, S):
    return LnLogits.logits_of(LnLogits.reference(x, w, b, eps, qk, ck, S)[0], torch.roll(qk, -1, dims=0), ck, S)


def _lg_before_affine(x, w, b, eps, qk, ck, S):
    if w is None and b is None:
        return None
    return LnLogits.logits_of(LnLogits.reference(x, None, None, eps, qk, ck, S)[0], qk, ck, S)


# on the logits; the rows are checked with kb.LayerNorm.MUTATIONS
LnLogits.MUTATIONS = [
    ("ck dropped", _lg_no_ck, 3.0),
    ("qk of head h + 1", _lg_next_head, 3.0),
    ("logits from the rows before gain and shift", _lg_before_affine, 3.0),
]


# ------------------------------------------------------------------ skinny fp32 GEMM ----
# Kernel (head.hip gemm_f32_skinny_kernel<EPI, MB>).  K is cut into 16 wave ranges of kper = 16 ceil(K / 256); a wave adds
# its range's products into one accumulator with v_mfma_f32_16x16x4_f32, four k per instruction in an order the hardware
# does not state: one rounding per product added, kper of them, plus one for the product itself should the unit round it
# before adding.  Then the 16-way LDS sum (15 adds, wave order): (kper + 16) U_F32 (|A||W|^T) -- the kernel's real chain,
# K / 16 + at most 31, not K.  After that
#   t += bias                 U_F32 (|acc| + |bias|)
#   epi 1, exact GELU         z = t * fp32(1 / sqrt 2): the constant and the product, 2 U_F32 |z| into erf, whose slope is
#                             erf'(z); erff: E_MATH |erf z| (assumed); 1 + erf: U_F32 (1 + erf z); together times 0.5 |x|
#                             -- an ABSOLUTE error proportional to |x| where 1 + erf cancels (the negative tail), the term
#                             kb.GemmBf16.bound carries as |x| (1e-6 + 2^-22) for its own erf; 0.5 * t is exact and the last
#                             product is the output's rounding; the error of t passes through with gelu' <= GELU_SLOPE_MAX
#   epi 2, C += t             the output's rounding
# and ulp_f32(ref) for the output's rounding.
class LinearCase:
    """a: fp32 [M, G K] (G groups side by side; G = 1 without groups), w: fp32 [N, K], bias: fp32 [N] or None, c0: fp32
    [M, N] (what C holds before the call), epi 0 / 1 / 2, group_cols (0: no groups)."""

    def __init__(self, a, w, bias, c0, epi, group_cols=0):
        self.a, self.w, self.bias, self.c0, self.epi, self.group_cols = a, w, bias, c0, epi, group_cols

    @property
    def K(self):
        return self.w.shape[1]

    @property
    def groups(self):
        return _up(self.w.shape[0], self.group_cols) if self.group_cols else 1

    def with_(self, **kw):
        c = LinearCase(self.a, self.w, self.bias, self.c0, self.epi, self.group_cols)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def rows(self, r0, r1):
        return self.with_(a=self.a[r0:r1], c0=self.c0[r0:r1])

    def acc(self, k0=0, k1=None, absolute=False, dtype=torch.float64, group0=False):
        """A . W^T over k in [k0, k1), group by group"""
        K, gc = self.K, self.group_cols
        k1 = K if k1 is None else k1
        f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
        a, w = f(self.a), f(self.w)
        if not gc:
            return a[:, k0:k1] @ w[:, k0:k1].T
        out = []
        for g in range(self.groups):
            ag = a[:, (0 if group0 else g) * K:][:, k0:k1]
            out.append(ag @ w[g * gc:(g + 1) * gc, k0:k1].T)
        return torch.cat(out, dim=1)

    def finish(self, acc, bias=True, epi=None):
        epi = self.epi if epi is None else epi
        x = acc + (self.bias.double() if bias and self.bias is not None else 0)
        if epi == 1:
            x = _gelu64(x)
        if epi == 2:
            x = x + self.c0.double()
        return x


def skinny_kper(K):
    return _up(K // 16, 16) * 16


class LinearF32:
    @staticmethod
    def reference(c):
        return c.finish(c.acc())

    @staticmethod
    def bound(c):
        acc = c.acc()
        d = (skinny_kper(c.K) + 16) * U_F32 * SECOND * c.acc(absolute=True)
        ab = c.bias.double().abs() if c.bias is not None else 0
        d_bias = U_F32 * (acc.abs() + ab) if c.bias is not None else 0
        x = c.finish(acc, epi=0)
        if c.epi == 0:                                   # the bias add is the output's rounding
            return f32_ulp(x) + d
        if c.epi == 2:
            return f32_ulp(c.finish(acc)) + d + d_bias
        z = x / math.sqrt(2.0)
        erf = torch.erf(z)
        slope = 2.0 / math.sqrt(math.pi) * torch.exp(-z * z)
        own = 0.5 * x.abs() * (2 * U_F32 * z.abs() * slope + E_MATH * erf.abs() + U_F32 * (1 + erf))
        return f32_ulp(_gelu64(x)) + GELU_SLOPE_MAX * (d + d_bias) + own

    @staticmethod
    def emulate(c):
        x = c.acc(dtype=torch.float32)
        if c.bias is not None:
            x = x + c.bias.float()
        if c.epi == 1:
            x = torch.nn.functional.gelu(x)
        if c.epi == 2:
            x = x + c.c0.float()
        return x.double()


def _lin_drop_last_chunk(c):
    return c.finish(c.acc(k1=c.K - 16)) if c.K > 16 else c.finish(torch.zeros_like(c.acc()))


def _lin_gelu_before_bias(c):
    if c.epi != 1 or c.bias is None:
        return None
    return _gelu64(c.acc()) + c.bias.double()


def _lin_tanh_gelu(c):
    if c.epi != 1:
        return None
    return torch.nn.functional.gelu(c.finish(c.acc(), epi=0), approximate="tanh")


LinearF32.MUTATIONS = [
    ("last 16-k chunk of the last working wave dropped", _lin_drop_last_chunk, 3.0),
    ("bias dropped", lambda c: c.finish(c.acc(), bias=False) if c.bias is not None else None, 3.0),
    ("A rounded to bf16", lambda c: c.with_(a=c.a.bfloat16().float()).finish(c.with_(a=c.a.bfloat16().float()).acc()), 3.0),
    ("GELU before the bias", _lin_gelu_before_bias, 3.0),
    ("tanh-approximate GELU", _lin_tanh_gelu, 3.0),
    ("epi 2 overwriting C", lambda c: c.finish(c.acc(), epi=0) if c.epi == 2 else None, 3.0),
    ("group g's columns reading group 0's rows", lambda c: c.finish(c.acc(group0=True)) if c.groups > 1 else None, 3.0),
]


# ------------------------------------------------------------------ probe keys ----
# Kernel (head.hip probe_qk_kernel): qk[h][i] = fma(q[o], Wk[o][i], acc) over the head's hd rows o: a chain of hd roundings
# against sum_o |q_o| |Wk_oi|; ck[h]: lane l takes o = l, l + 64, ...: ceil(hd / 64) roundings, then the 6-level wave tree,
# against sum_o |q_o| |bk_o|.  The chains' last roundings are the outputs' own: ulp_f32(ref) covers them once more.
class ProbeQk:
    """q: fp32 [W], Wk: fp32 [W, W], bk: fp32 [W]; heads divides W.  Results (qk [heads, W], ck [heads])."""

    @staticmethod
    def parts(q, Wk, bk, heads, f=lambda t: t.double()):
        W = q.shape[0]
        hd = W // heads
        qh = f(q).view(heads, hd)
        return torch.einsum("ho,hoi->hi", qh, f(Wk).view(heads, hd, W)), (qh * f(bk).view(heads, hd)).sum(-1)

    @staticmethod
    def reference(q, Wk, bk, heads):
        return ProbeQk.parts(q, Wk, bk, heads)

    @staticmethod
    def bound(q, Wk, bk, heads):
        hd = q.shape[0] // heads
        qk, ck = ProbeQk.parts(q, Wk, bk, heads)
        aqk, ack = ProbeQk.parts(q, Wk, bk, heads, lambda t: t.double().abs())
        return f32_ulp(qk) + hd * U_F32 * SECOND * aqk, f32_ulp(ck) + (_up(hd, 64) + 6) * U_F32 * SECOND * ack

    @staticmethod
    def emulate(q, Wk, bk, heads):
        qk, ck = ProbeQk.parts(q, Wk, bk, heads, lambda t: t.float())
        return qk.double(), ck.double()


def _probe_whole_q(q, Wk, bk, heads):
    qk = (q.double() @ Wk.double()).expand(heads, -1)
    return qk, (q.double() * bk.double()).sum().expand(heads)


def _probe_ck_first_trip(q, Wk, bk, heads):
    W = q.shape[0]
    hd = W // heads
    if hd <= 64:
        return None
    qk, _ = ProbeQk.parts(q, Wk, bk, heads)
    return qk, (q.double() * bk.double()).view(heads, hd)[:, :64].sum(-1)


ProbeQk.MUTATIONS = [
    ("q not restricted to the head's slice", _probe_whole_q, 3.0),
    ("ck without the lanes' second trip", _probe_ck_first_trip, 3.0),
]


# ------------------------------------------------------------------ not caught ----
_SAME = "the mutation is the identity there: "
NOT_CAUGHT.update({
    ("pool", "heads' logits shifted by one head"): (lambda c: c["H"] == 1, _SAME + "one head"),
    ("pool", "logits read as [B, S, H]"): (lambda c: c["H"] == 1 or c["S"] == 1, _SAME + "[B, 1, S] and [B, H, 1] have one layout"),
    ("pool", "probabilities rounded to bf16"): (lambda c: c["S"] == 1, _SAME + "one token, probability exactly 1"),
    ("pool", "maximum not subtracted"): (lambda c: not c["exp_overflows"],
                                         "softmax is the same function with or without the maximum until the sum of expf "
                                         "overflows (logits near 88.7): the peaked and offset fixtures are the ones that tell"),
    ("linear", "A rounded to bf16"): (lambda c: c["fixture"] == "cancelling",
                                      "v and -v round to bf16 symmetrically, so the cancellation survives; what is left is the "
                                      "rounding against the 1e-3 noise of w, below a bound that follows |A||W|"),
    ("linear", "tanh-approximate GELU"): (lambda c: c["fixture"] in ("x100", "x1e-3") or (c["fixture"] == "cancelling" and c["K"] >= 272),
                                          "the two forms differ by at most ~5e-4, around |x| = 2-3: the scaled fixtures have "
                                          "no pre-activation there (all far out, or all near 0), and the cancelling fixture's "
                                          "bound, which follows |A||W| ~ K, passes 5e-4 from K = 272"),
    ("ln logits", "qk of head h + 1"): (lambda c: c["H"] == 1, _SAME + "one head"),
    ("probe", "q not restricted to the head's slice"): (lambda c: c["heads"] == 1, _SAME + "one head"),
})


# ------------------------------------------------------------------ the launchers' choices, restated ----
def linear_form(M, N, K):
    """head.hip launch_skinny_f32: 'a' one pass of up to 16 rows (MB 1), 'b' 16 rows per workgroup on grid.y (MB 1) where 16
    columns per workgroup leave CUs idle, 'c' 64-row passes (MB 4)."""
    if M > 16 and _up(N, 16) < 192:
        return "b"
    return "a" if M <= 16 else "c"


LINEAR_FORMS = {"a", "b", "c"}


def linear_wave_facts(K):
    """what the 16 wave ranges of K look like: (not every wave has work, the last working wave's range is cut short by K,
    some range has an odd number of 16-k chunks: the tail of the 32-wide loop)"""
    kper = skinny_kper(K)
    lens = [max(0, min(K, (w + 1) * kper) - w * kper) for w in range(16)]
    working = [n for n in lens if n]
    return len(working) < 16, working[-1] < kper, any((n // 16) % 2 for n in working)


def pool_form(B, W):
    """head.hip launch_pool_head_rows (region_pool.hip: B = the regions of the launch)"""
    return "wide" if B * _up(W, 256) >= 192 else "narrow"


POOL_FORMS = {"narrow", "wide"}


def ln_form(rows, W, H):
    """elementwise.hip launch_layernorm with logits, fp32 output"""
    chunks = _up(W // 4, 64)
    if rows >= 4096 and H <= 8 and chunks <= 6:
        return "batch", 3 if chunks <= 3 else 4 if chunks <= 4 else 6
    return "row", 1 if chunks <= 1 else 3 if chunks <= 3 else 4 if chunks <= 4 else 6 if chunks <= 6 else 8


LN_FORMS = {("row", 1), ("row", 3), ("row", 4), ("row", 6), ("row", 8), ("batch", 3), ("batch", 4), ("batch", 6)}


# ------------------------------------------------------------------ the cases ----
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


# ---- linear: dicts of M, N, K, epi, fixture, bias (bool), pads (lda, ldw, ldc extra), group_cols
LINEAR_SHAPES = {
    "a": [(1, 16, 16), (5, 48, 16), (16, 17, 48), (15, 1, 256), (7, 1000, 272)],
    "b": [(17, 40, 272), (33, 48, 1280), (64, 15, 1040), (65, 32, 1040), (130, 3056, 16)],
    "c": [(17, 3057, 16), (64, 3072, 48), (65, 3072, 272), (130, 3073, 32)],
}
LINEAR_GROUPED = [(1, 48, 32, 16), (17, 48, 32, 16), (65, 48, 32, 16), (65, 3072, 16, 384)]
LINEAR_FIXTURES = ["randn", "tails", "cancelling", "x100", "x1e-3"]
LINEAR_FIXTURE_SHAPES = [(5, 48, 16), (7, 1000, 272), (33, 48, 1280), (65, 3072, 272)]
LINEAR_ALONE_ROWS = (0, 15, 16, 63, 64)


def _linear_cases():
    out = []
    shapes = [s for f in "abc" for s in LINEAR_SHAPES[f]]
    for i, (M, N, K) in enumerate(shapes):
        for epi in (0, 1, 2):
            out.append(dict(M=M, N=N, K=K, epi=epi, fixture="randn", bias=(i + epi) % 3 != 2,
                            pads=(4, 8, 12) if i % 2 else (0, 0, 0), group_cols=0))
    for i, (M, N, K, gc) in enumerate(LINEAR_GROUPED):
        for epi in (0, 1, 2):
            out.append(dict(M=M, N=N, K=K, epi=epi, fixture="randn", bias=(i + epi) % 3 != 2,
                            pads=(0, 8, 12) if i % 2 else (0, 0, 0), group_cols=gc))
    for i, (M, N, K) in enumerate(LINEAR_FIXTURE_SHAPES):
        for fixture in LINEAR_FIXTURES[1:]:
            for epi in (0, 1, 2):
                out.append(dict(M=M, N=N, K=K, epi=epi, fixture=fixture, bias=True, pads=(0, 0, 0), group_cols=0))
    return out


LINEAR_CASES = _linear_cases()


def linear_id(c):
    return (f"{c['M']}x{c['N']}x{c['K']} epi{c['epi']} {c['fixture']}" + ("" if c["bias"] else " nobias")
            + (" padded" if any(c["pads"]) else "") + (f" groups of {c['group_cols']}" if c["group_cols"] else ""))


def linear_case(spec, device="cpu"):
    """The inputs of a case (CPU generator, then moved).  randn: pre-activations of order 1.  tails: the bias walks -12 .. 12
    across the columns (GELU's negative tail, where 1 + erf cancels, to its linear end).  cancelling: a = [v, -v] against
    w = [u, u] + noise: results near 0 under |A||W| of order K.  x100 / x1e-3: both operands scaled (bias and C by the square)."""
    M, N, K, fixture = spec["M"], spec["N"], spec["K"], spec["fixture"]
    groups = _up(N, spec["group_cols"]) if spec["group_cols"] else 1
    g = _gen(M, N, K, spec["epi"], fixture)
    a = torch.randn(M, groups * K, generator=g)
    w = torch.randn(N, K, generator=g) * (0.5 / math.sqrt(K))
    bias = torch.randn(N, generator=g)
    c0 = torch.randn(M, N, generator=g)
    if fixture == "tails":
        bias = torch.linspace(-12.0, 12.0, N) + 0.01 * bias
    elif fixture == "cancelling":
        v, u = torch.randn(M, K // 2, generator=g), torch.randn(N, K // 2, generator=g)
        a = torch.cat([v, -v], dim=1)
        w = torch.cat([u, u], dim=1) + 1e-3 * torch.randn(N, K, generator=g)
    elif fixture in ("x100", "x1e-3"):
        s = 100.0 if fixture == "x100" else 1e-3
        a, w, bias, c0 = a * s, w * s, bias * (s * s), c0 * (s * s)
    mv = lambda t: t.to(device)
    return LinearCase(mv(a), mv(w), mv(bias) if spec["bias"] else None, mv(c0), spec["epi"], spec["group_cols"])


# ---- pool: dicts of B, S, W, H, pad (ldx - W), fixture
POOL_SHAPES = {
    "narrow": [(2, 1, 64, 1), (3, 15, 4, 5), (2, 16, 68, 4), (2, 17, 60, 16), (1, 112, 256, 8), (1, 113, 260, 8), (2, 128, 64, 9),
               (2, 129, 252, 3), (2, 241, 64, 8), (1, 577, 1024, 8), (1, 1025, 128, 16)],
    "wide": [(192, 17, 64, 3), (192, 113, 4, 1), (96, 129, 260, 16), (200, 17, 192, 3)],
}
POOL_FIXTURES = ["randn", "peaked", "offset", "rows x1e4", "rows x1e-4", "rows spike"]
POOL_FIXTURE_SHAPES = [(2, 128, 64, 9), (2, 241, 64, 8), (1, 577, 1024, 8), (96, 129, 260, 16)]
POOL_REFUSED = (192, 2300, 4, 16)          # H S probabilities + the wide form's partial sums: more than 160 KB of LDS


def _pool_cases():
    out = []
    for i, (B, S, W, H) in enumerate(POOL_SHAPES["narrow"] + POOL_SHAPES["wide"]):
        out.append(dict(B=B, S=S, W=W, H=H, pad=(0, 4, 12)[i % 3], fixture="randn"))
    for B, S, W, H in POOL_FIXTURE_SHAPES:
        for fixture in POOL_FIXTURES[1:]:
            out.append(dict(B=B, S=S, W=W, H=H, pad=0, fixture=fixture))
    return out


POOL_CASES = _pool_cases()


def pool_id(c):
    return f"B{c['B']} S{c['S']} W{c['W']} H{c['H']} {c['fixture']}" + (f" ldx+{c['pad']}" if c["pad"] else "")


def pool_inputs(spec, device="cpu"):
    """x [B, S, W], logits [B, H, S] (all finite).  peaked: head 0 one token + 60, head 1 times 20, head 2 all equal, head 3
    its maximum at s = 0, head 4 at s = S - 1 (heads mod H).  offset: every logit + 3e4.  rows x1e4 / x1e-4: the rows
    scaled.  rows spike: one element of 1e6 per image."""
    B, S, W, H, fixture = spec["B"], spec["S"], spec["W"], spec["H"], spec["fixture"]
    g = _gen(B, S, W, H, fixture)
    x = torch.randn(B, S, W, generator=g)
    lg = torch.randn(B, H, S, generator=g) * 2
    if fixture == "peaked":
        lg[:, 0 % H, S // 2] += 60.0
        lg[:, 1 % H] *= 20.0
        lg[:, 2 % H] = 0.75
        lg[:, 3 % H, 0] = lg[:, 3 % H].max(-1).values + 10.0
        lg[:, 4 % H, S - 1] = lg[:, 4 % H].max(-1).values + 10.0
    elif fixture == "offset":
        lg = lg + 3e4
    elif fixture == "rows x1e4":
        x = x * 1e4
    elif fixture == "rows x1e-4":
        x = x * 1e-4
    elif fixture == "rows spike":
        x[torch.arange(B), torch.arange(B) % S, (torch.arange(B) * 7 + 3) % W] = 1e6
    return x.to(device), lg.to(device)


def pool_facts(spec, logits, allow=None):
    """what NOT_CAUGHT's predicates ask of a pool case; logits [.., H, S] of the images (or of the regions' images, with
    their allow [.., S]); exp_overflows: the fp32 sum of expf(logit) over some head's tokens is not finite"""
    lg = logits.float()
    if allow is not None:
        lg = lg.masked_fill(~allow[..., None, :], -math.inf)
    return {"H": spec["H"], "S": spec["S"], "exp_overflows": bool(torch.isinf(torch.exp(lg).sum(-1)).any())}


# ---- masked pool: the shapes with their region counts; the first six regions are fixed, the rest random
MASKED_CASES = [dict(B=2, S=17, W=128, H=2, R=9, pad=0, fixture="randn"), dict(B=4, S=129, W=260, H=5, R=200, pad=4, fixture="randn"),
                dict(B=4, S=129, W=260, H=5, R=200, pad=0, fixture="peaked")]
REGION_KINDS = ["one token", "last token", "all tokens", "3 %", "50 %", "empty"]


def masked_regions(spec):
    """(region_image int64 [R], allow bool [R, S]): REGION_KINDS first, then random regions of 3 % .. 90 %, images not in order"""
    B, S, R = spec["B"], spec["S"], spec["R"]
    g = _gen(B, S, R, "regions")
    ri = torch.randint(0, B, (R,), generator=g)
    frac = torch.tensor([0.03, 0.2, 0.5, 0.9])[torch.randint(0, 4, (R,), generator=g)]
    allow = torch.rand(R, S, generator=g) < frac[:, None]
    allow[0] = False; allow[0, S // 3] = True
    allow[1] = False; allow[1, S - 1] = True
    allow[2] = True
    allow[3] = torch.rand(S, generator=g) < 0.03
    allow[3, (S * 2) // 3] = True                      # (3 % of 17 tokens may be none: at least one)
    allow[4] = torch.rand(S, generator=g) < 0.5
    allow[5] = False
    ri[1], ri[2] = B - 1, B - 1
    return ri, allow


def pack_bits(allow):
    """bool [R, S] -> int32 [R, ceil(S / 32)]: token s at bit s & 31 of word s >> 5"""
    R, S = allow.shape
    words = _up(S, 32)
    pad = torch.zeros(R, words * 32, dtype=torch.int64)
    pad[:, :S] = allow.long()
    v = (pad.view(R, words, 32) << torch.arange(32)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


# ---- ln_post + logits: dicts of B, S, W, H, affine (bool), pads (ldx - W, ldo - W)
def _ln_cases():
    out = []
    row = [(4, 1), (128, 3), (256, 8), (260, 9), (768, 16), (772, 1), (1024, 8), (1280, 3), (1536, 9), (1540, 16), (2048, 8)]
    for i, (W, H) in enumerate(row):
        out.append(dict(B=3, S=21, W=W, H=H, affine=True, pads=(4, 8) if i % 2 else (0, 0)))
    out.append(dict(B=3, S=21, W=1024, H=8, affine=False, pads=(0, 0)))
    for B, S, W, H in [(241, 17, 128, 1), (256, 16, 768, 5), (241, 17, 768, 8), (241, 17, 1024, 8), (256, 16, 1024, 1), (256, 16, 1280, 5),
                       (241, 17, 1536, 8)]:
        out.append(dict(B=B, S=S, W=W, H=H, affine=True, pads=(0, 0)))
    # at least 4096 rows, but more heads or columns than the batch form compiles in: the row form
    out.append(dict(B=241, S=17, W=1024, H=9, affine=True, pads=(0, 0)))
    out.append(dict(B=241, S=17, W=2048, H=8, affine=True, pads=(0, 0)))
    return out


LN_CASES = _ln_cases()
LN_EPS = 1e-5


def ln_id(c):
    return (f"rows{c['B'] * c['S']} W{c['W']} H{c['H']}" + ("" if c["affine"] else " no affine")
            + (" padded" if any(c["pads"]) else ""))


def ln_inputs(spec, device="cpu"):
    """(x [rows, W], w, b, qk [H, W], ck [H]).  63 rows: kb.layernorm_rows as it is.  A batch: those rows tiled (63 and 16
    are coprime: a copy starts at every offset within the 16-row workgroups and crosses their boundaries), with a whole copy
    as the first and as the last 63 rows."""
    rows, W, H = spec["B"] * spec["S"], spec["W"], spec["H"]
    x, w, b = layernorm_rows(W, H)
    if rows != x.shape[0]:
        x = torch.cat([x.repeat(_up(rows, 63), 1)[:rows - 63], x])
    g = _gen(rows, W, H, "qk")
    qk = torch.randn(H, W, generator=g) * 0.05
    ck = torch.randn(H, generator=g)
    mv = lambda t: t.to(device)
    return mv(x), (mv(w) if spec["affine"] else None), (mv(b) if spec["affine"] else None), mv(qk), mv(ck)


# ---- probe: (W, heads)
PROBE_CASES = [(64, 1), (128, 2), (192, 3), (260, 5), (1280, 16), (1024, 8)]


def probe_inputs(W, heads, device="cpu"):
    g = _gen(W, heads, "probe")
    q = torch.randn(W, generator=g) * (W // heads) ** -0.5
    Wk = torch.randn(W, W, generator=g) * W ** -0.5
    bk = torch.randn(W, generator=g)
    return q.to(device), Wk.to(device), bk.to(device)
