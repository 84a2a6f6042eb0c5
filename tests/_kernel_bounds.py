"""Per-element error bounds of the embed kernels, derived from the rounding each kernel does by design.

For every operation: `reference` (fp64 on the exact bf16 / fp32 inputs the kernel receives), `bound` (elementwise
|kernel - reference| allowed by the kernel's rounding steps), `emulate` (the reference recomputed with those rounding steps)
and `MUTATIONS` (plausible bugs, each a function of the same inputs: the reference with the bug in it).  All torch, on CPU
or GPU tensors.  tests/test_kernel_bounds_teeth.py shows on the CPU that every mutation leaves its bound by a wide margin
while the emulation stays well inside it; tests/test_gpu_kernel_bounds.py holds the kernels to the bounds.

Rounding constants: bf16 keeps 8 significant bits, so round-to-nearest moves a value by at most half an ulp, 2^-8 of its
magnitude at the bottom of a binade (U_BF16); fp32 likewise by 2^-24 (U_F32).  A result rounded once from a value y that is within
d of the exact value r is within ulp(r) + d of r (half an ulp of y, and y's binade is at most one above r's), which is how
every rounded output is bounded below: bf16 outputs by ulp_bf16(r), fp32 ones by ulp_f32(r), plus the error before the
last rounding.

Mutations that a bound cannot separate at some shape are listed in NOT_CAUGHT with the reason; the teeth test checks that
the list is honest (a listed mutation does stay under the required ratio there)."""
import math

import numpy as np
import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634


def ulp(x, bits):
    """One ulp at |x| (fp64) of a format with `bits` significant bits and fp32's exponent range (bf16: 8, fp32: 24):
    2^(floor(log2 |x|) - bits + 1), the subnormal spacing below 2^-126."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)                      # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    # 2^(e - bits) built from its fp64 exponent field: exact (torch.ldexp rounds: it gave 0.0625 as 0.06249999999999999)
    return ((e.to(torch.int64) - bits + 1023) << 52).view(torch.float64)


def bf16_ulp(x):
    return ulp(x, 8)


def f32_ulp(x):
    return ulp(x, 24)


def ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (inf where got is not finite but ref is)."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), err, torch.full_like(err, math.inf))
    return float((err / bound).max())


# ------------------------------------------------------------------ attention ----
# Kernel (attention.hip attn_fwd_kernel): scores s = q.k in fp32 (MFMA, exact bf16 products); p = exp2(s c - m) in fp32 with
# c = fp32(1 / sqrtf(hd)) * fp32(log2 e) and m a running reference; the row sum l adds the fp32 p; P is rounded to bf16
# and O = P.V accumulated in fp32; out = bf16(O * (1 / l)).  With p^ = p / l and eps_j the relative fp32 error of p_j:
#   output rounding                      <= U_BF16 |y|
#   P rounded to bf16                    <= U_BF16 sum_j p^_j |v_j|
#   fp32: O and l summed over S keys     <= 2 S U_F32 sum_j p^_j |v_j|,  1 / l and the product: 2^-21 of the same
#   p's own error (p and l share it)     <= 2 max_j eps_j sum_j p^_j |v_j|,  eps_j = ln 2 (c (hd + 1) U_F32 (|q|.|k_j|)
#                                           + 2^-22 |s_j c|) + 2^-22  (score sum, s c - m, exp2)
# The reference m is not part of the result: p / l is the same softmax against any m.  A move of m (the optimistic softmax's
# rare path) multiplies l and every O by alpha = exp2(m - m_new): alpha's own error is a common factor of l and O and
# cancels in O / l; what stays is one fp32 rounding of each product per move, at most one move per key tile: S / 64 U_F32
# relative, inside the 2 S U_F32 of the summation term (which counts one rounding per KEY and per accumulator).  Terms the
# move scales below fp32's range are lost with a weight below 2^-126 / l.  So the bound needs no term for the moves;
# Attention.emulate_optimistic (the kernel's rule, move by move) stays at <= 0.68 of it on the planted cases below.
def attention_qkv(B, S, H, hd, ld=None, seed=None):
    """The test input: a [B S, ld] bf16 buffer of q | k | v rows (CPU), the seed test_attention uses."""
    W = H * hd
    ld = ld or 3 * W
    g = torch.Generator(device="cpu").manual_seed(seed if seed is not None else S * 31 + H + (ld - 3 * W))
    return torch.randn(B * S, ld, generator=g).bfloat16()


def attention_split(qkv, B, S, H, hd, pairs=None):
    """q, k, v in fp64 as [pairs, S, hd] from a [B S, >= 3W] bf16 buffer; pairs = (image, head) indices b H + h."""
    W = H * hd
    x = qkv[:, :3 * W].double().reshape(B, S, 3, H, hd)
    q, k, v = (x[:, :, i].transpose(1, 2).reshape(B * H, S, hd) for i in range(3))
    if pairs is not None:
        q, k, v = q[pairs], k[pairs], v[pairs]
    return q, k, v


def attention_unsplit(out, B, S, H, hd, pairs=None):
    """A [B S, >= W] output buffer as fp64 [pairs, S, hd]."""
    W = H * hd
    o = out[:, :W].double().reshape(B, S, H, hd).transpose(1, 2).reshape(B * H, S, hd)
    return o if pairs is None else o[pairs]


class Attention:
    @staticmethod
    def reference(q, k, v, scale_mult=1.0):
        p = torch.softmax(q @ k.transpose(-1, -2) * (q.shape[-1] ** -0.5 * scale_mult), dim=-1)
        return p @ v

    @staticmethod
    def bound(q, k, v):
        hd, S = q.shape[-1], k.shape[-2]
        s = q @ k.transpose(-1, -2)
        c = hd ** -0.5 * LOG2E
        p = torch.softmax(s * hd ** -0.5, dim=-1)
        ref = p @ v
        pv = p @ v.abs()
        qk = q.abs() @ k.abs().transpose(-1, -2)
        eps = LN2 * (c * (hd + 1) * U_F32 * qk.amax(-1) + 2.0 ** -22 * (s.abs() * c).amax(-1)) + 2.0 ** -22
        d32 = (2 * S * U_F32 + 2.0 ** -21 + 2 * eps[..., None]) * pv
        return U_BF16 * (ref.abs() + pv) + (1 + U_BF16) * d32

    @staticmethod
    def emulate(q, k, v):
        hd = q.shape[-1]
        c = float(np.float32(np.float32(1.0) / np.sqrt(np.float32(hd))) * np.float32(LOG2E))
        e = (q.float() @ k.float().transpose(-1, -2)) * c
        p = torch.exp2(e - e.amax(-1, keepdim=True))
        l = p.sum(-1, keepdim=True)
        o = p.bfloat16().float() @ v.float()
        return (o * (1.0 / l)).bfloat16().double()

    @staticmethod
    def emulate_optimistic(q, k, v, k_lo, group=32, parts=2, mutate=None):
        """fp32 model of the kernels' optimistic softmax (attention.hip attn_fwd_kernel; parts = 4: attn16_fwd_kernel).

        Key rows [k_lo, S) in 64-key tiles; k_lo = 1: the class-token key as the prelude (m = s_cls c, l = 1, O = v_cls) and
        the query rows in rotated order (1 .. S - 1, 0).  Per tile p = exp2(fma(s, c, -m)) against the running reference m
        with no maximum taken.  A lane sums the keys of the tile it holds -- key i of the tile belongs to part
        (i >> 2) & (parts - 1): the 32 keys (i & 3) + 8 (i >> 2) + 4 hh of each 32-key block pair for the 32x32x16 kernel's
        two halves, the 16 keys 16 mb + 4 lq + i for the 16x16x32 kernel's four lanes -- and a row triggers when a part
        sum is not < 2^80 (inf, NaN and m = -inf included).  The trigger is shared by the `group` rows of a wave (consecutive
        rows in the kernel's row order; both kernels: 32, attn16's two query blocks share one __all).  On a trigger every row
        of the group takes its OWN m_new = max(m, tile max c), alpha = exp2(m - m_new), scales l and O (the P.V of the
        previous tile included) by alpha and redoes the exponentials.  P is rounded to bf16 for P.V; out = bf16(O (1 / l)).

        Returns {"out": fp64 [pairs, S, hd], "moved" / "own" / "overflow": bool [pairs, S, tiles] (the row's reference moved / the row
        itself triggered / the first pass's p was not finite), "alpha": the factor applied (1 where not moved), "m_before":
        m ahead of each tile, "l": l at the end}.  mutate: one of HDR_MUTATION_NAMES, the model with that bug in it."""
        P, S, hd = q.shape
        c = float(np.float32(np.float32(1.0) / np.sqrt(np.float32(hd))) * np.float32(LOG2E))
        dev = q.device
        s = q.float() @ k.float().transpose(-1, -2)                 # [P, S, S], exact bf16 products summed in fp32
        vf = v.float()
        order = torch.arange(S, device=dev)
        if k_lo:
            order = torch.cat([order[1:], order[:1]])
        pos = torch.empty(S, dtype=torch.long, device=dev)
        pos[order] = torch.arange(S, device=dev)
        gid = pos // group                                          # wave group of each sequence row
        ngroups = (S + group - 1) // group
        nt = (S - k_lo + 63) // 64
        m = torch.full((P, S), -math.inf, dtype=torch.float32, device=dev)
        l = torch.zeros(P, S, parts, dtype=torch.float32, device=dev)
        O = torch.zeros(P, S, hd, dtype=torch.float32, device=dev)
        if k_lo:
            m = s[:, :, 0] * c
            l[..., 0] = 1.0
            O = vf[:, :1, :].expand(P, S, hd).clone()
        pending = torch.zeros_like(O)                               # the previous tile's P.V
        moved = torch.zeros(P, S, nt, dtype=torch.bool, device=dev)
        own = torch.zeros_like(moved)
        alphas = torch.ones(P, S, nt, dtype=torch.float32, device=dev)
        m_before = torch.zeros(P, S, nt, dtype=torch.float32, device=dev)
        overflow = torch.zeros_like(moved)                          # the first pass's p held an inf or a NaN
        part_of = (torch.arange(64, device=dev) >> 2) & (parts - 1)

        def exps(sc, m):
            return torch.exp2((sc.double() * c - m.double()[..., None]).float())      # one rounding: v_pk_fma_f32

        def part_sums(p):
            return torch.stack([p[..., part_of == j].sum(-1) for j in range(parts)], dim=-1)

        for t in range(nt):
            k0 = k_lo + 64 * t
            n = min(64, S - k0)
            sc = torch.full((P, S, 64), -math.inf, dtype=torch.float32, device=dev)   # masked past the last key
            sc[..., :n] = s[:, :, k0:k0 + n]
            m_before[..., t] = m
            p = exps(sc, m)
            ps = part_sums(p)
            trig_row = ~((ps < 2.0 ** 80).all(-1))
            trig = torch.zeros(P, ngroups, device=dev).index_add_(1, gid, trig_row.float())[:, gid] > 0
            a_o = torch.ones_like(m)
            a_l = torch.ones_like(m)
            if bool(trig.any()):
                m_new = torch.maximum(m, sc.amax(-1) * c)
                alpha = torch.exp2(m - m_new)                        # 0 when m was -inf
                if mutate == "alpha of the triggering row for the whole wave":
                    first = torch.where(trig_row, pos[None, :].expand(P, S), torch.full((P, S), S, device=dev))
                    for g in range(ngroups):
                        rows = (gid == g).nonzero().flatten()
                        src = order[first[:, rows].amin(1).clamp_max(S - 1)]            # [P] the group's first triggering row
                        alpha[:, rows] = alpha[torch.arange(P, device=dev), src][:, None].expand(P, len(rows))
                elif mutate == "wave mates: m moved, alpha forced to 1":
                    alpha = torch.where(trig_row, alpha, torch.ones_like(alpha))
                elif mutate == "class-token term dropped on the tile-0 move" and k_lo and t == 0:
                    alpha = torch.zeros_like(alpha)
                moved[..., t] = trig
                overflow[..., t] = trig & ~torch.isfinite(p).all(-1)
                own[..., t] = trig_row
                alphas[..., t] = torch.where(trig, alpha, torch.ones_like(alpha))
                m = torch.where(trig, m_new, m)
                if mutate != "O not rescaled on a move":
                    a_o = alphas[..., t]
                if mutate != "l not rescaled on a move":
                    a_l = alphas[..., t]
                if mutate != "exponentials not redone after a move":
                    p = torch.where(trig[..., None], exps(sc, m), p)
                    ps = part_sums(p)
            if mutate == "previous tile's P.V applied after the rescale":
                O = O * a_o[..., None] + pending
            else:
                O = (O + pending) * a_o[..., None]
            l = l * a_l[..., None] + ps
            pending = p[..., :n].bfloat16().float() @ vf[:, k0:k0 + n]
        O = O + pending
        out = (O * (1.0 / l.sum(-1))[..., None]).bfloat16().double()
        return {"out": out, "moved": moved, "own": own, "alpha": alphas, "m_before": m_before, "overflow": overflow,
                "l": l.sum(-1)}


def _drop_key(which):
    def f(q, k, v):
        S = k.shape[-2]
        if S == 1:
            return None                        # (n/a: no other key)
        j = {"first": 0, "last": S - 1, "middle": S // 2}[which]
        keep = torch.cat([torch.arange(0, j), torch.arange(j + 1, S)]).to(k.device)
        return Attention.reference(q, k[..., keep, :], v[..., keep, :])
    return f


def _cls_row_to_row1(q, k, v):
    if q.shape[-2] == 1:
        return None                            # (n/a: no row 1)
    o = Attention.reference(q, k, v)
    o[..., 1, :] = o[..., 0, :]
    return o


def _swap_columns(q, k, v):
    o = Attention.reference(q, k, v)
    return o[..., [1, 0] + list(range(2, o.shape[-1]))]


# (name, mutation, ratio the bound must be exceeded by somewhere); a mutation returns None where it does not apply
Attention.MUTATIONS = [
    ("drop key 0", _drop_key("first"), 3.0),
    ("drop the last key", _drop_key("last"), 3.0),
    ("drop a middle key", _drop_key("middle"), 3.0),
    ("softmax scale x 1.01", lambda q, k, v: Attention.reference(q, k, v, 1.01), 1.5),
    ("class-token query's row written to row 1", _cls_row_to_row1, 3.0),
    ("two output columns swapped", _swap_columns, 3.0),
]


# ------------------------------------------------------------------------ RoPE ----
# Kernel (elementwise.hip rope_kernel): per interleaved pair (x0, x1) of q or k, bf16 -> fp32, y0 = x0 c - x1 s,
# y1 = x1 c + x0 s in fp32 with the fp32 table value (c, s) of the row's position, then one bf16 rounding.  The two
# products and the sum round in fp32 (<= 2 U_F32 (|x0 c| + |x1 s|)); the reference is pe_vit.apply_rope's formula in fp64
# with the same fp32 table, so the table's own rounding is not part of the error.
def rope_table(grid, hd, use_cls, theta=10000.0):
    """The fp32 (cos, sin) table [S, hd / 2, 2] of oracle.pe_vit.rope_angles, as revo_op_rope takes it."""
    from oracle import pe_vit

    class C:
        pass
    c = C()
    c.width, c.heads, c.image_size, c.patch_size, c.use_cls, c.rope_theta = hd, 1, grid, 1, use_cls, theta
    ang = pe_vit.rope_angles(c, torch.float64)
    return torch.stack([ang[:, 0::2].cos(), ang[:, 0::2].sin()], dim=-1).float().contiguous()


def _rope_fp64(x, cs):
    from oracle import pe_vit
    c = cs[..., 0].double().repeat_interleave(2, dim=-1)
    s = cs[..., 1].double().repeat_interleave(2, dim=-1)
    return x * c + pe_vit.rotate_pairs(x) * s


class Rope:
    """x: fp64 [..., S, hd] (the bf16 q or k of each head), cs: fp32 [S, hd / 2, 2]; a mutation also takes cls (row 0 is the
    class token)."""

    @staticmethod
    def reference(x, cs):
        return _rope_fp64(x, cs)

    @staticmethod
    def bound(x, cs):
        from oracle import pe_vit
        c = cs[..., 0].double().abs().repeat_interleave(2, dim=-1)
        s = cs[..., 1].double().abs().repeat_interleave(2, dim=-1)
        return bf16_ulp(_rope_fp64(x, cs)) + 2 * U_F32 * (x.abs() * c + pe_vit.rotate_pairs(x).abs() * s)

    @staticmethod
    def emulate(x, cs):
        x32 = x.float().unflatten(-1, (-1, 2))
        x0, x1 = x32.unbind(-1)
        c, s = cs[..., 0].to(x32.device), cs[..., 1].to(x32.device)
        return torch.stack((x0 * c - x1 * s, x1 * c + x0 * s), dim=-1).flatten(-2).bfloat16().double()


def _rope_rotate_half(x, cs, cls):
    h = x.shape[-1] // 2
    c, s = cs[..., 0].double(), cs[..., 1].double()
    x0, x1 = x[..., :h], x[..., h:]
    return torch.cat((x0 * c - x1 * s, x1 * c + x0 * s), dim=-1)


def _rope_swap_halves(x, cs, cls):
    q = cs.shape[-2] // 2
    return _rope_fp64(x, torch.cat((cs[..., q:, :], cs[..., :q, :]), dim=-2))


def _rope_cls_rotated(x, cs, cls):
    if not cls:
        return None                            # (n/a: no class token)
    return _rope_fp64(x, torch.cat((cs[1:2], cs[1:]), dim=0))


def _rope_sin_flipped(x, cs, cls):
    return _rope_fp64(x, torch.stack((cs[..., 0], -cs[..., 1]), dim=-1))


Rope.MUTATIONS = [
    ("table row shifted by one", lambda x, cs, cls: _rope_fp64(x, torch.roll(cs, 1, dims=0)), 3.0),
    ("x and y halves swapped", _rope_swap_halves, 3.0),
    ("rotate-half pairing instead of interleaved", _rope_rotate_half, 3.0),
    ("class row rotated", _rope_cls_rotated, 3.0),
    ("sin sign flipped", _rope_sin_flipped, 3.0),
]


# ------------------------------------------------------------------- LayerNorm ----
# Kernel (elementwise.hip layernorm_kernel / layernorm8_kernel): fp32, two passes.  mean = (sum x) / W with the sum taken
# 4 or 8 elements per lane, ceil(W / 256) steps per lane, then a 64-lane tree: depth <= n = 9 + ceil(W / 256), so
# |d mean| <= (n + 1) U_F32 mean|x|.  var = sum (x - mean)^2 / W (positive terms: relative n + 2 U_F32 with the squares and the
# subtraction, n + 5 with the division and the sum with eps; half of it passes through the root) and rsqrt's own 2 U_F32.
# y = fma((x - mean) rstd, w, b): two more roundings of z, then the fma's one rounding of y.
#   fp32:  ulp_f32(ref) + |w| |z| ((n + 5) / 2 + 4) U_F32 + |w| rstd |d mean|
#   bf16:  ulp_bf16(ref) + the fp32 bound
def _ln_stats(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return mu, var, 1.0 / torch.sqrt(var + eps)


class LayerNorm:
    """x: fp32 [rows, W], w / b: fp32 [W]; references in fp64."""

    @staticmethod
    def reference(x, w, b, eps):
        xd = x.double()
        mu, _, rstd = _ln_stats(xd, eps)
        return (xd - mu) * rstd * w.double() + b.double()

    @staticmethod
    def bound(x, w, b, eps, out_bf16):
        W = x.shape[-1]
        n = 9 + -(-W // 256)
        xd, wd = x.double(), w.double().abs()
        mu, _, rstd = _ln_stats(xd, eps)
        z = ((xd - mu) * rstd).abs()
        dmu = (n + 1) * U_F32 * xd.abs().mean(-1, keepdim=True)
        ref = LayerNorm.reference(x, w, b, eps)
        d = f32_ulp(ref) + wd * z * (((n + 5) / 2 + 4) * U_F32) + wd * rstd * dmu
        return d + bf16_ulp(ref) if out_bf16 else d

    @staticmethod
    def emulate(x, w, b, eps, out_bf16):
        W = x.shape[-1]
        x = x.float()
        mu = x.sum(-1, keepdim=True) / W
        d = x - mu
        rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / W + np.float32(eps))
        y = d * rstd * w.float() + b.float()
        return (y.bfloat16() if out_bf16 else y).double()


def _ln_with_rstd(rstd_fn):
    def f(x, w, b, eps):
        xd = x.double()
        mu = xd.mean(-1, keepdim=True)
        return (xd - mu) * rstd_fn(xd, mu, eps) * w.double() + b.double()
    return f


def _one_pass_var(xd, mu, eps):
    x32 = xd.float()
    m32 = x32.mean(-1, keepdim=True)
    return torch.rsqrt(((x32 * x32).mean(-1, keepdim=True) - m32 * m32).double() + eps)


LayerNorm.MUTATIONS = [
    ("eps outside the sqrt", _ln_with_rstd(lambda x, mu, eps: 1.0 / (((x - mu) ** 2).mean(-1, keepdim=True).sqrt() + eps)), 3.0),
    ("eps omitted", _ln_with_rstd(lambda x, mu, eps: ((x - mu) ** 2).mean(-1, keepdim=True).rsqrt()), 3.0),
    ("unbiased variance", _ln_with_rstd(lambda x, mu, eps: 1.0 / (x.var(-1, unbiased=True, keepdim=True) + eps).sqrt()), 3.0),
    ("one-pass variance E[x^2] - E[x]^2 in fp32", _ln_with_rstd(_one_pass_var), 3.0),
]


def layernorm_rows(W, seed):
    """The LayerNorm test input, 63 rows (not a multiple of 4): 24 ordinary rows (randn * 3 + 1); 18 rows with std
    1e-3 .. 3e-3, where var is about eps; 18 rows with |mean| / std = 1e3; a constant row; two rows of mean 1e3 and std 1."""
    g = torch.Generator(device="cpu").manual_seed(W * 7 + seed)
    plain = torch.randn(24, W, generator=g) * 3 + 1
    small = torch.randn(18, W, generator=g) * (torch.rand(18, 1, generator=g) * 2e-3 + 1e-3) + torch.randn(18, 1, generator=g)
    std = torch.rand(18, 1, generator=g) * 2 + 0.01
    offset = torch.randn(18, W, generator=g) * std + 1e3 * std * torch.sign(torch.randn(18, 1, generator=g))
    const = torch.full((1, W), -2.75)
    big = torch.randn(2, W, generator=g) + 1e3
    x = torch.cat([plain, small, offset, const, big])
    w = torch.randn(W, generator=g)
    b = torch.randn(W, generator=g)
    return x, w, b


# --------------------------------------------------------------- f32 -> bf16 ----
# Kernel (elementwise.hip f32_to_bf16_kernel): v_cvt_pk_bf16_f32, round to nearest even; expected bit for bit to equal
# torch's .bfloat16() (NaN only as "a NaN": the payload is not part of the contract).  Columns cols .. ld_dst - 1 are zero.
def f32_special_values():
    """Every class the conversion must get right, as fp32 bit patterns (int64 list)."""
    bits = [0x00000000, 0x80000000,                          # +-0
            0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00018000, 0x00408000, 0x007fffff, 0x807fffff,
            0x00010000, 0x0000ffff,                          # fp32 subnormals (ties among them, the largest)
            0x00800000, 0x80800000,                          # smallest normals
            0x7f800000, 0xff800000,                          # +-inf
            0x7fc00000, 0xffc00000, 0x7f800001, 0x7fbfffff, 0x7fc12345,   # NaNs (quiet, signalling, with payloads)
            0x3f808000, 0xbf808000,                          # tie, even below: rounds down
            0x3f818000, 0xbf818000,                          # tie, odd below: rounds up
            0x3f807fff, 0x3f808001, 0x3f81ffff,              # just below / above a tie; up into the next exponent
            0x3fff8000, 0x3fffffff,                          # ties / rounding that carry into the exponent
            0x7f7f0000, 0x7f7f7fff,                          # largest bf16; stays finite
            0x7f7f8000, 0xff7f8000, 0x7f7fffff, 0xff7fffff]  # round up to +-inf (tie at the top; fp32 max)
    return bits


def f32_from_bits(bits):
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.float32))


def bf16_bits(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


# ------------------------------------------------------------ GEMM bf16 epilogues ----
# Kernel (gemm.hip, EPI_BF16 / EPI_BF16_GELU): acc = A.B^T summed in fp32 (MFMA, exact bf16 products, any order:
# <= K U_F32 (|A||B|^T)_ij), + bias in fp32 (U_F32 of |acc| + |bias|), GELU by the erf form of gemm.hip gelu_erf2
# (documented erf error ~2e-6 after its fp32 16th power: 1e-6 |x|; its three fp32 steps: 2^-22 |x|; the accumulated error
# passes through with gelu' <= 1.13), then one bf16 rounding: ulp_bf16(ref) + the fp32 error.
GELU_SLOPE_MAX = 1.13


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


class GemmBf16:
    """a: bf16 [M, K], b: bf16 [N, K], bias fp32 [N]."""

    @staticmethod
    def reference(a, b, bias, gelu):
        x = a.double() @ b.double().T + bias.double()
        return _gelu64(x) if gelu else x

    @staticmethod
    def bound(a, b, bias, gelu):
        K = a.shape[1]
        acc = a.double() @ b.double().T
        d = K * U_F32 * (a.double().abs() @ b.double().abs().T) + U_F32 * (acc.abs() + bias.double().abs())
        x = acc + bias.double()
        if gelu:
            d = GELU_SLOPE_MAX * d + x.abs() * (1e-6 + 2.0 ** -22)
            x = _gelu64(x)
        return bf16_ulp(x) + d

    @staticmethod
    def emulate(a, b, bias, gelu):
        x = a.float() @ b.float().T + bias.float()
        if gelu:
            x = torch.nn.functional.gelu(x)
        return x.bfloat16().double()


GemmBf16.MUTATIONS = [
    ("bias dropped", lambda a, b, bias, gelu: GemmBf16.reference(a, b, torch.zeros_like(bias), gelu), 3.0),
    ("GELU before the bias", lambda a, b, bias, gelu: (_gelu64(a.double() @ b.double().T) + bias.double()) if gelu else None,
     3.0),
    ("tanh-approximate GELU", lambda a, b, bias, gelu: torch.nn.functional.gelu(a.double() @ b.double().T + bias.double(),
                                                                               approximate="tanh") if gelu else None, 3.0),
]


# ------------------------------------------------------------------ not caught ----
# (op, mutation name) -> (predicate on the case, reason).  A predicate gets the case's dict (op-specific keys).
NOT_CAUGHT = {
    ("attention", "softmax scale x 1.01"): (lambda c: c["S"] == 1, "one key: its softmax weight is 1 at any scale"),
    ("gemm", "tanh-approximate GELU"): (lambda c: True, "differs from the erf form by at most ~5e-4 absolute, below one "
                                        "bf16 ulp of the outputs where it is largest (|x| ~ 2-3)"),
}


NOT_CAUGHT.update({
    (op, "split-K planes summed in bf16"): (lambda c: c["K"] >= 3072,
                                            "the fp32 bound of any summation order, K U_F32 (|A||B|^T), grows with K: from "
                                            "K = 3072 it is as large as the bf16 rounding of a partial plane")
    for op in ("gemm f32", "resid", "splitk ln x")})


def not_caught(op, name, case):
    e = NOT_CAUGHT.get((op, name))
    return e is not None and e[0](case)


# ------------------------------------------------------------------ the cases ----
# shared by the CPU teeth test and the GPU test: (label, B, S, H, hd, ld, ldo); ld / ldo None = packed (3W / W)
ATTENTION_CASES = ([(f"S{S} H{H} hd{hd} b{B}", B, S, H, hd, None, None)
                    for hd in (64, 96)
                    for B, S, H in [(2, 577, 2), (1, 197, 3), (3, 17, 2), (1, 64, 1), (1, 65, 1), (2, 128, 2), (1, 129, 1),
                                    (1, 1, 1), (1, 1024, 2), (2, 16, 2)]]
                   + [("L14 b64", 64, 577, 16, 64, None, None),
                      ("B16 b1 (8 + 4 pairs)", 1, 197, 12, 64, None, None),
                      ("B16 b5 (56 + 4 pairs)", 5, 197, 12, 64, None, None),
                      ("G14 b1", 1, 1024, 16, 96, None, None),
                      ("G14 b3", 3, 1024, 16, 96, None, None),
                      ("class-token split hd96", 2, 1025, 4, 96, None, None),
                      ("Tiny-T14", 4, 17, 2, 64, None, None),
                      ("Tiny-N14", 4, 16, 2, 96, None, None),
                      ("wide rows hd64", 3, 197, 3, 64, 3 * 192 + 64, 192 + 40),
                      ("wide rows hd96", 2, 577, 2, 96, 3 * 192 + 40, 192 + 24)])

# (label, grid, heads, head_dim, class token, images); rows = images x S, ld = 3W
ROPE_CASES = [("B16", 14, 12, 64, True, 3), ("L14", 24, 16, 64, True, 2), ("G14", 32, 16, 96, False, 2),
              ("Tiny-T14", 4, 2, 64, True, 5), ("Tiny-N14", 4, 2, 96, False, 5)]

LAYERNORM_WIDTHS = [128, 192, 256, 768, 1024, 1280, 1536]

# the shapes of test_gemm_epilogues and test_gemm_skinny_all_epilogues
GEMM_CASES = [(333, 512, 256), (64, 1024, 1024), (64, 4096, 1024), (64, 1024, 4096), (1, 256, 256), (7, 260, 512),
              (33, 1000, 768), (64, 1024, 1280)]


def rope_qkv(grid, H, hd, cls, B):
    S = grid * grid + (1 if cls else 0)
    g = torch.Generator(device="cpu").manual_seed(S * 13 + hd)
    return torch.randn(B * S, 3 * H * hd, generator=g).bfloat16(), S


def rope_heads(qkv, B, S, H, hd, which):
    """q (which 0) or k (1) of a [B S, 3W] buffer as fp64 [B, H, S, hd]."""
    return qkv.double().reshape(B, S, 3, H, hd)[:, :, which].transpose(1, 2)


def gemm_case(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M * 3 + N * 5 + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = (torch.randn(N, K, generator=g) * 0.1).bfloat16()
    bias = torch.randn(N, generator=g)
    return a, b, bias


# ====================================================================== the GEMM family ====
# The rest of the GEMM's epilogues, one class each, on a `GemmCase` (the exact bf16 / fp32 inputs the kernel receives).
# Common to all of them: acc = A.B^T summed in fp32 in any order -- one K range, split-K partial planes added in a fixed
# order, the eight-wave order of the queued kernel's leftover rows -- is within K U_F32 (|A||B|^T)_ij of the exact sum
# (the bound of a sum tree of depth <= K), so one acc term covers every launch form.
class GemmCase:
    """a: bf16 [M, K], b: bf16 [N, K], bias fp32 [N]; optional: gamma fp32 [N] (residual), x fp32 [M, N] (the old residual
    rows) or hi / lo bf16 [M, N] (the old stream in planes), stats fp32 [M, P, 2] + csum fp32 [N] + eps (folded-LayerNorm
    consumer), cs fp32 [S, hd / 2, 2] + S + hd + rope_cols (RoPE), ksplit (the K parts of a split-K form; 1 = none)."""

    def __init__(self, a, b, bias, **kw):
        self.a, self.b, self.bias = a, b, bias
        self.gamma = self.x = self.hi = self.lo = self.stats = self.csum = self.cs = None
        self.eps, self.S, self.hd, self.rope_cols, self.ksplit, self.epi = 1e-5, 1, 64, 0, 1, "bf16"
        self.row0 = 0                          # index of row 0 in the whole problem (RoPE tokens of a row chunk)
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def K(self):
        return self.a.shape[1]

    def acc(self, k_end=None, dtype=torch.float64):
        k_end = self.K if k_end is None else k_end
        return self.a[:, :k_end].to(dtype) @ self.b[:, :k_end].to(dtype).T

    def acc_abs(self):
        return self.a.double().abs() @ self.b.double().abs().T

    def old(self):
        """the old residual values, fp64: x, or hi + lo as given"""
        if self.hi is not None:
            return self.hi.double() + self.lo.double()
        return self.x.double()

    def rows(self, r0, r1):
        """the sub-problem of rows [r0, r1) (the GPU test's fp64 reference goes in row chunks)"""
        kw = {k: getattr(self, k)[r0:r1] for k in ("a", "x", "hi", "lo", "stats") if getattr(self, k) is not None}
        return self.with_(row0=self.row0 + r0, **kw)

    def with_(self, **kw):
        c = GemmCase(self.a, self.b, self.bias)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c


def _acc_err(c):
    return c.K * U_F32 * c.acc_abs()


def _acc_drop_last_ktile(c):
    return c.acc(c.K - 64)


def _acc_drop_plane(c):
    """split-K: the last of the c.ksplit K ranges never added (one K range: the last K-tile)"""
    S = max(c.ksplit, 1)
    nt = c.K // 64
    return c.acc(c.K - (nt - (S - 1) * (nt // S)) * 64 if S > 1 else c.K - 64)


def _acc_planes_bf16(c):
    """split-K: each partial plane rounded to bf16 before the fixed-order sum (the reduce reading bf16 planes)"""
    S = max(c.ksplit, 2)
    nt = c.K // 64
    edges = [(nt // S) * s * 64 for s in range(S)] + [c.K]
    tot = 0
    for k0, k1 in zip(edges[:-1], edges[1:]):
        tot = tot + (c.a[:, k0:k1].double() @ c.b[:, k0:k1].double().T).float().bfloat16().double()
    return tot


# ------------------------------------------------------------------------ EPI_F32 ----
# C = fp32(acc + bias): the acc error plus the bias add's one rounding (U_F32 of |acc| + |bias|) -- the add IS the output's
# rounding, so there is no separate ulp term.
class GemmF32:
    @staticmethod
    def reference(c, acc=None):
        return (c.acc() if acc is None else acc) + c.bias.double()

    @staticmethod
    def bound(c):
        acc = c.acc()
        return _acc_err(c) + U_F32 * (acc.abs() + c.bias.double().abs())

    @staticmethod
    def emulate(c):
        return (c.acc(dtype=torch.float32) + c.bias.float()).double()


GemmF32.MUTATIONS = [
    ("the last K-tile dropped", lambda c: GemmF32.reference(c, _acc_drop_last_ktile(c)), 3.0),
    ("bias dropped", lambda c: c.acc(), 3.0),
    ("bias added twice", lambda c: c.acc() + 2 * c.bias.double(), 3.0),
    ("split-K planes summed in bf16", lambda c: GemmF32.reference(c, _acc_planes_bf16(c)), 3.0),
]


# ------------------------------------------------------------------ EPI_RESID_F32 ----
# x_new = x_old + gamma (acc + bias): fp32 steps  t = acc + bias (U_F32 (|acc| + |bias|)), t gamma (U_F32 |gamma t|), then
# the add, which is the output's rounding (ulp_f32(ref)).  The old value is x, or hi + lo (exact in fp32: lo is below
# half an ulp of hi).  Planes out: hi = bf16(x_new), lo = bf16(x_new - hi) (the difference is exact), so hi + lo misses
# x_new by half a bf16 ulp of |x_new - hi| <= ulp_bf16(x_new) / 2: at most 2^-9 ulp_bf16(ref) more (x2 for the binade).
class GemmResid:
    @staticmethod
    def reference(c, acc=None, bias_gamma=True, old=None):
        acc = c.acc() if acc is None else acc
        g = c.gamma.double() if c.gamma is not None else 1.0
        t = g * (acc + c.bias.double()) if bias_gamma else g * acc + c.bias.double()
        return (c.old() if old is None else old) + t

    @staticmethod
    def bound(c, planes_out=False):
        acc = c.acc()
        g = c.gamma.double().abs() if c.gamma is not None else 1.0
        t = acc + c.bias.double()
        ref = GemmResid.reference(c)
        d = g * (_acc_err(c) + U_F32 * (acc.abs() + c.bias.double().abs())) + U_F32 * (g * t.abs()) + f32_ulp(ref)
        if planes_out:
            d = d + 2.0 ** -8 * bf16_ulp(ref)
        return d

    @staticmethod
    def emulate(c, planes_out=False):
        t = c.acc(dtype=torch.float32) + c.bias.float()
        if c.gamma is not None:
            t = t * c.gamma.float()
        old = (c.hi.float() + c.lo.float()) if c.hi is not None else c.x.float()
        x = old + t
        if planes_out:
            hi = x.bfloat16()
            return hi.double() + (x - hi.float()).bfloat16().double()
        return x.double()


GemmResid.MUTATIONS = [
    ("the last K-tile dropped", lambda c: GemmResid.reference(c, _acc_drop_last_ktile(c)), 3.0),
    ("one split-K plane dropped", lambda c: GemmResid.reference(c, _acc_drop_plane(c)), 3.0),
    ("split-K planes summed in bf16", lambda c: GemmResid.reference(c, _acc_planes_bf16(c)), 3.0),
    ("gamma not applied to the bias", lambda c: GemmResid.reference(c, bias_gamma=False) if c.gamma is not None else None, 3.0),
    ("lo dropped from the old value", lambda c: GemmResid.reference(c, old=c.hi.double()) if c.hi is not None else None, 3.0),
    ("old value read as bf16(x)", lambda c: GemmResid.reference(c, old=c.x.bfloat16().double()) if c.hi is None else None, 3.0),
]


def planes_ok(hi, lo):
    """the planes' own invariant: |lo| <= ulp_bf16(hi) / 2 (lo is the rounded remainder of hi's rounding)"""
    return bool((lo.double().abs() <= bf16_ulp(hi) / 2).all())


# ------------------------------------------------------------------- fused RoPE ----
# EPI_BF16_ROPE: v = fp32(acc + bias), then -- by design, the same bits on every path -- x0 = bf16(v0), x1 = bf16(v1) for
# each interleaved pair of a rotated column, y = (x0 c - x1 s, x1 c + x0 s) in fp32 with the fp32 table of token row % S,
# and one more bf16 rounding.  Two roundings: x_k is within ulp_bf16(r_k) + d_k of r_k = acc + bias (d_k the fp32 error),
# which the rotation passes on weighted by |c| and |s|; the rotation's fp32 steps add 2 U_F32 (|x0 c| + |x1 s|); then
# ulp_bf16(ref).  Columns at or past rope_cols: GemmBf16's bound (the rotation is the identity there).
def _rope_apply(x, c, cs_rows, swap_sign=False):
    """x fp64 [M, N]; rotate the pairs of the first c.rope_cols columns with table rows cs_rows ([M] token indices)"""
    R, hd = c.rope_cols, c.hd
    y = x.clone()
    if R == 0:
        return y
    cs = c.cs.to(x.device).double()[cs_rows]                     # [M, hd / 2, 2]
    reps = R // hd
    co = cs[..., 0].repeat(1, reps)                               # [M, R / 2]
    si = cs[..., 1].repeat(1, reps)
    x0, x1 = x[:, 0:R:2], x[:, 1:R:2]
    y[:, 0:R:2] = x0 * co - x1 * si
    y[:, 1:R:2] = x1 * co + x0 * si
    return y


def _rope_tokens(c, M, device, shift=0, by_row=False):
    """table row of each output row: row % S; the mutations: shifted by one token, or the row itself (rows past the table
    read its last row)"""
    r = torch.arange(M, device=device) + c.row0
    if by_row:
        return r.clamp_max(c.S - 1)
    return (r % c.S + shift) % c.S


class GemmRope:
    @staticmethod
    def reference(c, acc=None, tokens=None):
        x = (c.acc() if acc is None else acc) + c.bias.double()
        return _rope_apply(x, c, _rope_tokens(c, x.shape[0], x.device) if tokens is None else tokens)

    @staticmethod
    def rotated_bound(c, r, d):
        """bound of the rotated output given the pre-rounding values r (fp64 [M, N]) and their fp32 error d"""
        M, R, hd = r.shape[0], c.rope_cols, c.hd
        ref = _rope_apply(r, c, _rope_tokens(c, M, r.device))
        out = bf16_ulp(ref) + d
        if R:
            cs = c.cs.to(r.device).double()[_rope_tokens(c, M, r.device)]
            co = cs[..., 0].abs().repeat(1, R // hd)
            si = cs[..., 1].abs().repeat(1, R // hd)
            e = bf16_ulp(r[:, :R]) + d[:, :R]                      # |x_k - r_k|
            x0, x1 = r[:, 0:R:2].abs() + e[:, 0::2], r[:, 1:R:2].abs() + e[:, 1::2]
            out[:, 0:R:2] = bf16_ulp(ref[:, 0:R:2]) + co * e[:, 0::2] + si * e[:, 1::2] + 2 * U_F32 * (x0 * co + x1 * si)
            out[:, 1:R:2] = bf16_ulp(ref[:, 1:R:2]) + co * e[:, 1::2] + si * e[:, 0::2] + 2 * U_F32 * (x1 * co + x0 * si)
        return out

    @staticmethod
    def bound(c):
        acc = c.acc()
        d = _acc_err(c) + U_F32 * (acc.abs() + c.bias.double().abs())
        return GemmRope.rotated_bound(c, acc + c.bias.double(), d)

    @staticmethod
    def emulate_rotate(c, v):
        """v fp32 [M, N] (the value before the RoPE's roundings) -> the kernel's bf16 output as fp64"""
        R = c.rope_cols
        y = v.bfloat16().float()
        if R:
            cs = c.cs.to(v.device)[_rope_tokens(c, v.shape[0], v.device)]
            co, si = cs[..., 0].repeat(1, R // c.hd), cs[..., 1].repeat(1, R // c.hd)
            x0, x1 = y[:, 0:R:2].clone(), y[:, 1:R:2].clone()
            y[:, 0:R:2] = x0 * co - x1 * si
            y[:, 1:R:2] = x1 * co + x0 * si
        return y.bfloat16().double()

    @staticmethod
    def emulate(c):
        return GemmRope.emulate_rotate(c, c.acc(dtype=torch.float32) + c.bias.float())


def _rope_mutations(ref_fn):
    """the RoPE mutations of an output function ref_fn(c, tokens=...)"""
    def by_row(c):
        M = c.a.shape[0]
        if M <= c.S or not c.rope_cols:
            return None                                           # (n/a: one image)
        return ref_fn(c, tokens=_rope_tokens(c, M, c.a.device, by_row=True))

    def shifted(c):
        if not c.rope_cols:
            return None
        return ref_fn(c, tokens=_rope_tokens(c, c.a.shape[0], c.a.device, shift=1))
    return [("RoPE indexed by row instead of row % S", by_row, 3.0),
            ("RoPE table shifted by one token", shifted, 3.0)]


GemmRope.MUTATIONS = [
    ("the last K-tile dropped", lambda c: GemmRope.reference(c, _acc_drop_last_ktile(c)), 3.0),
    ("bias dropped", lambda c: GemmRope.reference(c.with_(bias=torch.zeros_like(c.bias))), 3.0),
] + _rope_mutations(lambda c, tokens: GemmRope.reference(c, tokens=tokens))


# ------------------------------------------------- folded LayerNorm: the consumer ----
# out = epi(rstd (acc - mean csum) + bias'), mean / rstd merged from the row's P fp32 slots (mean_i, M2_i) of 256-column
# slices (gemm.hip lnf_merge, and merge_n<4> / merge_n<6> in the same order).  Reference: the fp64 merge of the same slots,
#   mean = sum m_i / P,  var = (sum M2_i + 256 sum (m_i - mean)^2) / (256 P),  rstd = 1 / sqrt(var + eps).
# The kernel's fp32 merge: sm over P slots and the division: dm <= (P + 1) U_F32 mean_i|m_i|; sq = sum M2_i: (P - 1) U_F32 sq;
# d_i = m_i - mean is off by dm + U_F32 |d_i| (e_i), dd = sum d_i^2 by fma: P U_F32 dd + sum (2 |d_i| e_i + e_i^2); the fma
# with 256 and the division: 2 U_F32 var; + eps: U_F32 (var + eps); rsqrtf (v_rsq_f32, 1 ulp): 2 U_F32.  So
#   er = |d rstd| / rstd <= 1.01 (dvar / (2 (var + eps)) + 2 U_F32),   mr = -mean rstd: off by rstd dm + |mean| rstd (er + U_F32).
# The epilogue's fp32 steps (acc rstd, csum mr, + bias', the sum; fma or not): 3 U_F32 (|acc rstd| + |csum mr| + |bias'|).
# The acc error passes through rstd.  Then GELU or RoPE as for the plain epilogues, and one bf16 rounding.
def fold_merge64(stats):
    """fp64 (mean, var) of rows from their fp32 slots [M, P, 2]"""
    s = stats.double()
    P = s.shape[1]
    m = s[..., 0].mean(1)
    var = (s[..., 1].sum(1) + LNF_SLICE * ((s[..., 0] - m[:, None]) ** 2).sum(1)) / (LNF_SLICE * P)
    return m, var


LNF_SLICE = 256


def fold_merge32(stats, eps):
    """the kernel's fp32 merge, in lnf_merge's order: (rstd, mr = -mean rstd)"""
    s = stats.float()
    P = s.shape[1]
    sm = torch.zeros(s.shape[0], dtype=torch.float32, device=s.device)
    sq = torch.zeros_like(sm)
    for i in range(P):
        sm = sm + s[:, i, 0]
        sq = sq + s[:, i, 1]
    mean = sm / P
    dd = torch.zeros_like(sm)
    for i in range(P):
        d = s[:, i, 0] - mean
        dd = (d.double() * d.double() + dd.double()).float()      # fmaf
    var = ((LNF_SLICE * dd.double() + sq.double()).float()) / float(LNF_SLICE * P)
    rstd = torch.rsqrt(var + np.float32(eps))
    return rstd, -mean * rstd


def _fold_err(stats, eps):
    """(mean, rstd, dm, er) per row: the fp64 merge and the fp32 merge's error bounds above"""
    s = stats.double()
    P = s.shape[1]
    m, var = fold_merge64(stats)
    mabs = s[..., 0].abs().mean(1)
    dm = (P + 1) * U_F32 * mabs
    di = (s[..., 0] - m[:, None]).abs()
    e = dm[:, None] + U_F32 * di
    sq = s[..., 1].sum(1)
    dd = (di ** 2).sum(1)
    dvar = ((P - 1) * U_F32 * sq + LNF_SLICE * (P * U_F32 * dd + (2 * di * e + e * e).sum(1))) / (LNF_SLICE * P) \
        + 2 * U_F32 * var + U_F32 * (var + eps)
    er = 1.01 * (dvar / (2 * (var + eps)) + 2 * U_F32)
    return m, 1.0 / torch.sqrt(var + eps), dm, er


class GemmLnIn:
    """c.stats [M, P, 2] fp32, c.csum [N] fp32, c.eps; c.epi in ("bf16", "gelu", "rope")."""

    @staticmethod
    def pre(c, acc=None, stats=None, eps=None, mean_csum=True, between=True):
        """the fp64 value before GELU / RoPE; the keyword arguments are the mutations' handles"""
        acc = c.acc() if acc is None else acc
        s = (c.stats if stats is None else stats).double()
        P = s.shape[1]
        m = s[..., 0].mean(1)
        var = (s[..., 1].sum(1) + (LNF_SLICE * ((s[..., 0] - m[:, None]) ** 2).sum(1) if between else 0)) / (LNF_SLICE * P)
        rstd = 1.0 / torch.sqrt(var + (c.eps if eps is None else eps))
        cm = m[:, None] * c.csum.double()[None, :] if mean_csum else 0
        return rstd[:, None] * (acc - cm) + c.bias.double()

    @staticmethod
    def finish(c, x, tokens=None):
        if c.epi == "gelu":
            return _gelu64(x)
        if c.epi == "rope":
            return _rope_apply(x, c, _rope_tokens(c, x.shape[0], x.device) if tokens is None else tokens)
        return x

    @staticmethod
    def reference(c, tokens=None, **kw):
        return GemmLnIn.finish(c, GemmLnIn.pre(c, **kw), tokens)

    @staticmethod
    def bound(c):
        acc = c.acc()
        m, rstd, dm, er = (t[:, None] for t in _fold_err(c.stats, c.eps))
        cs = c.csum.double()[None, :].abs()
        b = c.bias.double().abs()
        d = (rstd * _acc_err(c) + (acc.abs() + cs * m.abs()) * rstd * er + cs * rstd * dm + cs * (m * rstd).abs() * U_F32
             + 3 * U_F32 * (acc.abs() * rstd + cs * (m * rstd).abs() + b))
        x = GemmLnIn.pre(c)
        if c.epi == "gelu":
            return bf16_ulp(_gelu64(x)) + GELU_SLOPE_MAX * d + x.abs() * (1e-6 + 2.0 ** -22)
        if c.epi == "rope":
            return GemmRope.rotated_bound(c, x, d)
        return bf16_ulp(x) + d

    @staticmethod
    def emulate(c):
        rstd, mr = fold_merge32(c.stats, c.eps)
        v = c.acc(dtype=torch.float32) * rstd[:, None] + (c.csum.float()[None, :] * mr[:, None] + c.bias.float()[None, :])
        if c.epi == "gelu":
            return torch.nn.functional.gelu(v).bfloat16().double()
        if c.epi == "rope":
            return GemmRope.emulate_rotate(c, v)
        return v.bfloat16().double()


def _stats_neighbour_row(c):
    return GemmLnIn.reference(c, stats=torch.roll(c.stats, 1, dims=0))


def _stats_one_slot_twice(c):
    """slot 1 read in place of slot 0 (an off-by-one slot index)"""
    if c.stats.shape[1] < 2:
        return None
    s = c.stats.clone()
    s[:, 0] = s[:, 1]
    return GemmLnIn.reference(c, stats=s)


GemmLnIn.MUTATIONS = [
    ("the last K-tile dropped", lambda c: GemmLnIn.reference(c, acc=_acc_drop_last_ktile(c)), 3.0),
    ("the mean csum term dropped", lambda c: GemmLnIn.reference(c, mean_csum=False), 3.0),
    ("statistics of the neighbouring row", _stats_neighbour_row, 3.0),
    ("statistics slot 1 read for slot 0", _stats_one_slot_twice, 3.0),
    ("the between-slice term LNF_SLICE dd dropped", lambda c: GemmLnIn.reference(c, between=False), 3.0),
    ("eps dropped", lambda c: GemmLnIn.reference(c, eps=0.0), 3.0),
] + _rope_mutations(lambda c, tokens: GemmLnIn.reference(c, tokens=tokens) if c.epi == "rope" else None)


# ------------------------------------------------- folded LayerNorm: the producer ----
# Per row and 256-column slice (one column tile) the residual epilogue writes (mean, M2) of the new values: each of the 4
# waves sums its 64 columns in a tree of depth 6 (dm_w <= 6 U_F32 sum|x| / 64, plus a margin of one level) and sums
# (x - m_w)^2 by fma (depth <= 11 with the lanes' tree; the rounding of d: 2 U_F32); m_w off by dm_w adds exactly 64 dm_w^2
# (sum (x - m_w) = 0).  lnf_store_tile_stats: mean = ((a + b) + (c + d)) / 4 (2 U_F32 of the mean of |m_w|, plus the mean of
# dm_w); M2 = sum q_w + 64 sum (m_w - mean)^2: the q errors, 2 U_F32 sum q_w for the adds, 64 sum (2 |d_w| e_w + e_w^2)
# with e_w = dm_w + dmean + U_F32 |d_w|, 3 U_F32 of the between term, U_F32 M2 for the last add.
# The reference is fp64 statistics of the kernel's own output row (fp32 rows, or hi + lo: the kernel worked on the fp32
# value, which hi + lo misses by <= 2^-8 ulp_bf16: its effect on mean and M2 is added).
class LnStats:
    @staticmethod
    def reference(x):
        """x fp64 [M, N] -> [M, N / 256, 2] (mean, M2)"""
        M, N = x.shape
        s = x.double().reshape(M, N // LNF_SLICE, LNF_SLICE)
        m = s.mean(-1)
        return torch.stack((m, ((s - m[..., None]) ** 2).sum(-1)), dim=-1)

    @staticmethod
    def bound(x, planes=False):
        M, N = x.shape
        s = x.double().reshape(M, N // LNF_SLICE, 4, 64)
        a = s.abs()
        mw = s.mean(-1)
        dmw = 7 * U_F32 * a.mean(-1)
        qw = ((s - mw[..., None]) ** 2).sum(-1)
        dqw = (qw + 64 * dmw ** 2) * (13 * U_F32) + 64 * dmw ** 2
        mean = mw.mean(-1)
        dmean = dmw.mean(-1) + 2 * U_F32 * mw.abs().mean(-1)
        dw = (mw - mean[..., None]).abs()
        ew = dmw + dmean[..., None] + U_F32 * dw
        between = 64 * (dw ** 2).sum(-1)
        m2 = qw.sum(-1) + between
        dm2 = dqw.sum(-1) + 2 * U_F32 * qw.sum(-1) + 64 * (2 * dw * ew + ew * ew).sum(-1) + 3 * U_F32 * between + U_F32 * m2
        if planes:
            delta = 2.0 ** -8 * bf16_ulp(s)
            dmean = dmean + delta.mean((-1, -2))
            dm2 = dm2 + (2 * (s - mean[..., None, None]).abs() * delta + delta ** 2).sum((-1, -2)) \
                + 2 * 256 * delta.mean((-1, -2)) ** 2
        return torch.stack((dmean + f32_ulp(mean), dm2 + f32_ulp(m2)), dim=-1)

    @staticmethod
    def emulate(x):
        M, N = x.shape
        s = x.float().reshape(M, N // LNF_SLICE, 4, 64)
        mw = s.sum(-1) / 64
        qw = ((s - mw[..., None]) ** 2).sum(-1)
        mean = ((mw[..., 0] + mw[..., 1]) + (mw[..., 2] + mw[..., 3])) * 0.25
        d = mw - mean[..., None]
        m2 = ((qw[..., 0] + qw[..., 1]) + (qw[..., 2] + qw[..., 3])) + 64 * (d * d).sum(-1)
        return torch.stack((mean, m2), dim=-1).double()


def _stats_no_between(x):
    M, N = x.shape
    s = x.double().reshape(M, N // LNF_SLICE, 4, 64)
    mw = s.mean(-1)
    return torch.stack((mw.mean(-1), ((s - mw[..., None]) ** 2).sum((-1, -2))), dim=-1)


def _stats_next_slot(x):
    r = LnStats.reference(x)
    if r.shape[1] < 2:
        return None
    return torch.roll(r, 1, dims=1)


def _stats_one_pass(x):
    s = x.float().reshape(x.shape[0], -1, LNF_SLICE)
    m = s.mean(-1)
    return torch.stack((m, (s * s).sum(-1) - LNF_SLICE * m * m), dim=-1).double()


LnStats.MUTATIONS = [
    ("the between-wave term 64 sum (m_w - mean)^2 dropped", _stats_no_between, 3.0),
    ("statistics written to the neighbouring slot", _stats_next_slot, 3.0),
    ("statistics of the neighbouring row", lambda x: torch.roll(LnStats.reference(x), 1, dims=0), 3.0),
    ("one-pass M2 = sum x^2 - 256 mean^2 in fp32", _stats_one_pass, 3.0),
]


# ------------------------------------------- split-K reduce + LayerNorm (one image) ----
# splitk_reduce_resid_ln_kernel: x_new = x + gamma (sum of the fp32 planes + bias), stored (GemmResid's bound), and the same
# registers normalised (w = 1, b = 0, bf16): the LayerNorm bound of the kernel's own x_new -- it normalises exactly the
# values it stores, so the reference for h is the fp64 LayerNorm of the stored x_new.
class SplitkResidLn:
    @staticmethod
    def h_reference(x_new, eps, one_pass=False, eps_on=True):
        xd = x_new.double()
        mu = xd.mean(-1, keepdim=True)
        if one_pass:
            x32 = x_new.float()
            m32 = x32.mean(-1, keepdim=True)
            var = ((x32 * x32).mean(-1, keepdim=True) - m32 * m32).double()
        else:
            var = ((xd - mu) ** 2).mean(-1, keepdim=True)
        return (xd - mu) / torch.sqrt(var + (eps if eps_on else 0.0))

    @staticmethod
    def h_bound(x_new, eps):
        W = x_new.shape[1]
        one = torch.ones(W, dtype=torch.float32, device=x_new.device)
        return LayerNorm.bound(x_new, one, torch.zeros_like(one), eps, True)

    @staticmethod
    def h_emulate(x_new, eps):
        W = x_new.shape[1]
        one = torch.ones(W, dtype=torch.float32, device=x_new.device)
        return LayerNorm.emulate(x_new, one, torch.zeros_like(one), eps, True)


SplitkResidLn.MUTATIONS_H = [
    ("eps dropped", lambda x, eps: SplitkResidLn.h_reference(x, eps, eps_on=False), 3.0),
    ("one-pass variance E[x^2] - mean^2 in fp32", lambda x, eps: SplitkResidLn.h_reference(x, eps, one_pass=True), 3.0),
]


# -------------------------------------------------- rounding direction of bf16 stores ----
# A per-element bound of ulp_bf16 cannot tell round-to-nearest from truncation (both are within one ulp).  Over many
# outputs the mean of sign(ref) (got - ref) / ulp_bf16(ref) can: ~0 for round-to-nearest (the fp32 error is far below an
# ulp and symmetric), about -0.5 for a store that truncates toward zero.
ROUNDING_BIAS_MAX = 0.1
ROUNDING_MIN_OUTPUTS = 10 ** 6


def rounding_bias(got, ref):
    """(mean signed error in ulps, outputs counted) over the outputs of at least 1/64 of the output's rms: below that (the
    GELU's negative tail) the fp32 error before the rounding is not small against an ulp of the output"""
    got, ref = got.double().flatten(), ref.double().flatten()
    keep = (ref.abs() >= ref.pow(2).mean().sqrt() / 64) & torch.isfinite(got)
    r = ref[keep]
    return float((torch.sign(r) * (got[keep] - r) / bf16_ulp(r)).mean()), int(keep.sum())


def bf16_truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (the bug the statistic catches), as fp64"""
    b = x.float().contiguous().view(torch.int32) & -65536
    return b.view(torch.float32).double()




# ------------------------------------------------------------------- test data ----
def fold_rows(M, W, seed, device="cpu"):
    """Residual rows the fold is weak on: per-row offsets 0 .. 33 sigma, 256-column slices with different means, outlier
    channels, every 37th row near-constant (std 1e-3: var below eps = 1e-5, so eps matters).  fp32 [M, W]."""
    g = torch.Generator(device=device).manual_seed(seed)
    sig = torch.rand(M, 1, generator=g, device=device) * 1.5 + 0.25
    x = torch.randn(M, W, generator=g, device=device) * sig
    P = -(-W // LNF_SLICE)
    x += (torch.randn(M, P, generator=g, device=device) * sig).repeat_interleave(LNF_SLICE, dim=1)[:, :W]
    off = torch.linspace(0, 33, M, device=device)[torch.randperm(M, generator=g, device=device)]
    x += (off[:, None] * sig) * torch.sign(torch.randn(M, 1, generator=g, device=device))
    ch = torch.randperm(W, generator=g, device=device)[:4]
    x[:, ch] += 20 * sig
    const = near_constant_rows(M, device)
    x[const] = (torch.randn(len(const), 1, generator=g, device=device) * 3
                + torch.randn(len(const), W, generator=g, device=device) * 1e-3)
    return x


def near_constant_rows(M, device="cpu"):
    return torch.arange(3, max(M, 3), 37, device=device)


def spread(n, seed, lo=-3, hi=1, device="cpu"):
    """n fp32 values of either sign over binades 2^lo .. 2^hi (bias / gamma)"""
    g = torch.Generator(device=device).manual_seed(seed)
    e = torch.randint(lo, hi + 1, (n,), generator=g, device=device).float()
    return torch.sign(torch.randn(n, generator=g, device=device)) * (1 + torch.rand(n, generator=g, device=device)) * torch.exp2(e)


def weights(N, K, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(N, K, generator=g, device=device) * K ** -0.5).bfloat16()


def resid_case(M, N, K, seed, device="cpu", planes_in=False, ksplit=1):
    """a residual GEMM: A = bf16 of GELU-like activations, old rows from fold_rows"""
    g = torch.Generator(device=device).manual_seed(seed + 1)
    a = torch.nn.functional.gelu(torch.randn(M, K, generator=g, device=device) * 2).bfloat16()
    x = fold_rows(M, N, seed, device)
    bias, gamma = spread(N, seed + 3, device=device), spread(N, seed + 4, -6, 0, device)
    # the near-constant rows stay near-constant in x_new: A's row is zero there and x_old holds the row minus gamma bias
    const = near_constant_rows(M, device)
    a[const] = 0
    x[const] -= (gamma * bias).float()
    c = GemmCase(a, weights(N, K, seed + 2, device), bias, gamma=gamma, x=x, ksplit=ksplit)
    if planes_in:
        c.hi = x.bfloat16()
        c.lo = (x - c.hi.float()).bfloat16()
    return c


def ln_in_case(M, N, K, seed, epi, device="cpu", S=577, hd=64, rope_cols=0, cs=None):
    """a folded-LayerNorm consumer: A = bf16(x) of fold_rows, its fp32 slot statistics, W' bf16, csum = fp32 sum of W'"""
    x = fold_rows(M, K, seed, device)
    b = weights(N, K, seed + 2, device)
    st = LnStats.reference(x).float()
    csum = b.double().sum(1).float()
    return GemmCase(x.bfloat16(), b, spread(N, seed + 3, device=device), stats=st, csum=csum, eps=1e-5, epi=epi, S=S, hd=hd,
                    rope_cols=rope_cols, cs=cs)


def plain_case(M, N, K, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    a = (torch.randn(M, K, generator=g, device=device) * 2).bfloat16()
    return GemmCase(a, weights(N, K, seed + 2, device), spread(N, seed + 3, device=device))


# ------------------------------------------------------------------ the cases ----
# Shared by the CPU teeth test (M cut to a few hundred rows) and the GPU module (the towers' M).  S / hd / rope table of
# L14 (grid 24, class token: S 577, hd 64) and G14 (grid 32, no class token: S 1024, hd 96).
TOWERS = {"L14": dict(W=1024, Md=4096, S=577, hd=64, grid=24, cls=True),
          "G14": dict(W=1536, Md=8960, S=1024, hd=96, grid=32, cls=False),
          "B16": dict(W=768, Md=3072, S=197, hd=64, grid=14, cls=True)}

# (label, N, K, parts, epi) of the folded consumer; RoPE rows rotate the first 2W columns (q and k)
LN_IN_CASES = [("L14 qkv rope", 3072, 1024, "rope", "L14"), ("L14 fc1 gelu", 4096, 1024, "gelu", "L14"),
               ("K512 bf16 (lnf_merge, parts 2)", 1024, 512, "bf16", "L14"), ("K768 gelu (lnf_merge, parts 3)", 3072, 768, "gelu", "B16"),
               ("G14 qkv rope (merge_n<6>)", 4608, 1536, "rope", "G14"), ("G14 fc1 gelu", 8960, 1536, "gelu", "G14")]

# (label, N, K, ksplit, planes) of the residual epilogue; ksplit = the K parts of the split-K form the GPU case takes
RESID_CASES = [("L14 out-proj fp32", 1024, 1024, 1, "none"), ("L14 out-proj planes out", 1024, 1024, 1, "out"),
               ("L14 fc2 planes in/out", 1024, 4096, 1, "inout"), ("L14 fc2 planes in, fp32 out", 1024, 4096, 1, "in"),
               ("L14 fc2 split-K 3", 1024, 4096, 3, "none"), ("fc2 split-K 2", 1024, 2048, 2, "none"),
               ("G14 fc2 planes in/out", 1536, 8960, 1, "inout")]

# (label, N, K, ksplit) of the split-K reduce with the LayerNorm (MAXG = ceil(N / 512))
SPLITK_LN_CASES = [("L14 out-proj MAXG 2", 1024, 1024, 3), ("L14 fc2 MAXG 2", 1024, 4096, 3), ("N256 MAXG 1", 256, 1024, 3),
                   ("N1536 MAXG 3", 1536, 1024, 3), ("N2048 MAXG 4", 2048, 1024, 3), ("B16 fc2 MAXG 2", 768, 3072, 3)]


def tower_rope(tower):
    t = TOWERS[tower]
    return rope_table(t["grid"], t["hd"], t["cls"])


# ------------------------------------------------------------ launch forms ----
# The bits of revo_debug_gemm_forms (revers-o_amd/csrc/kernels.h GemmForm), in bit order.
GEMM_FORMS = ["SKINNY_444", "SKINNY_411", "128_128", "128_64", "128R", "256_TILE", "256P", "256P_192", "256Q", "256Q_QTAIL",
              "SPLITK_RING", "SPLITK_RING_LN", "SPLITK_256", "LN_FOLDED", "LN_CONSUMED", "PLANES_IN", "PLANES_OUT"]


def form_bits(names):
    return sum(1 << GEMM_FORMS.index(n) for n in names)


def form_names(bits):
    return sorted(n for i, n in enumerate(GEMM_FORMS) if bits >> i & 1)


# A launch is more than its form bit: the kernel of a step is compiled per epilogue, with or without the folded LayerNorm's
# consumer, the fold and the planes, and a leftover step does pointer arithmetic of its own from row0.  The signature of a
# step of a plan (revo_debug_gemm_plan; tests/test_gemm_plan.py `plan` gives the step dicts):
#   (kernel form, epilogue, consumer, LayerNorm in the reduce, fold, planes mode xp, "main" / "leftover")
GEMM_EPILOGUES = ["bf16", "gelu", "resid", "f32", "patch", "rope"]              # kernels.h, in value order
OFFER_LN, OFFER_FOLD, OFFER_XP_IN, OFFER_XP_OUT, OFFER_CONSUMER = 1, 2, 4, 8, 16  # the offers of revo_debug_gemm_plan
BODY_WS_ELEMS = 16 << 20                                                        # tower.h SPLITK_WS_ELEMS


def gemm_signatures(epi, offers, steps):
    """the signatures of the steps of one planned launch (epi: the epilogue's number)"""
    return [(form_names(s["form"])[0], GEMM_EPILOGUES[epi], bool(offers & OFFER_CONSUMER), bool(s["reduce_ln"]), bool(s["fold"]),
             int(s["xp"]), "leftover" if i else "main") for i, s in enumerate(steps)]


def signature_text(sig):
    form, epi, consumer, reduce_ln, fold, xp, step = sig
    flags = [n for n, on in (("consumer", consumer), ("reduce-LN", reduce_ln), ("fold", fold), (f"xp {xp}", xp)) if on]
    return f"{form} {epi} [{', '.join(flags)}] {step}"


def body_gemm_launches(plan, W, Md, rows, layers, qkv_epi, rope=(0, 0, 0)):
    """The launch_gemm calls of tower.h body_blocks for `layers` blocks over `rows` rows, restated; `plan` plans one
    (tests/test_gemm_plan.py plan, passed in so that importing this module loads no library).  qkv_epi / rope: what the
    tower's qkv_args gives (image: "rope" and (S, head_dim, 2 W); text: "bf16").
    Returns [(launch name, block, epilogue number, N, K, offers, form bits, steps)].

    What is restated: ln_stats and xlo exist when W is one to six 256-column slices (alloc_body); the stream lives in planes
    for the whole run when both residual shapes fold (stream_in_planes: gemm_resid_folds, the bare problem with the fold
    offered); a residual GEMM is offered the fused LayerNorm, the fold and the planes together, the last fc2 none of them
    but the planes it must read; qkv and fc1 consume the statistics exactly when the residual GEMM in front of them folded."""
    parts = W // 256 if W % 256 == 0 and W // 256 <= 6 else 0

    def folds(N, K):
        bits, steps = plan(2, rows, N, K, 0, OFFER_FOLD)
        return bits >= 0 and steps[0]["fold"] == 1
    planes = bool(parts) and folds(W, W) and folds(W, Md)
    out, h_xb, x_planes = [], False, False

    def launch(name, block, epi, N, K, ws=0, offers=0, r=(0, 0, 0)):
        bits, steps = plan(epi, rows, N, K, ws, offers, r)
        assert bits >= 0, f"the plan refuses {name} of block {block}: {rows} x {N} x {K}, offers {offers}"
        out.append((name, block, epi, N, K, offers, bits, steps))
        return steps[0]["fold"] == 1

    def after(offered):
        return (OFFER_LN | (OFFER_FOLD if parts else 0) | (OFFER_XP_OUT if planes else 0)) if offered else 0

    for i in range(layers):
        last = i + 1 >= layers
        launch("qkv", i, GEMM_EPILOGUES.index(qkv_epi), 3 * W, W, 0, OFFER_CONSUMER if h_xb else 0, rope)
        folded = launch("out", i, 2, W, W, BODY_WS_ELEMS, after(True) | (OFFER_XP_IN if x_planes else 0))
        h_xb, x_planes = folded, planes and folded
        launch("fc1", i, 1, Md, W, 0, OFFER_CONSUMER if h_xb else 0)
        folded = launch("fc2", i, 2, W, Md, BODY_WS_ELEMS, after(not last) | (OFFER_XP_IN if x_planes else 0))
        h_xb, x_planes = not last and folded, not last and planes and folded
    return out


# The GPU cases of tests/test_gpu_gemm_bounds.py: (label, kind, M, N, K, options, expected forms on librevo_exp.so).
# kind: "f32" / "bf16" / "gelu" / "resid" (revo_op_gemm), "rope" (revo_op_gemm_rope), "ln_in:bf16" / "ln_in:gelu"
# (revo_op_gemm_ln_in), "ln_in_rope", "resid_ln:<planes>" (revo_op_gemm_resid_ln: none = fp32 rows + bf16 copy, out, inout,
# in), "resid_norm" (revo_op_gemm_resid_norm).  options: tower (RoPE table / S / hd), variant / qstores (forced forms: then
# the experiment library only), pad (NaN margins past N and M), ksplit (the split-K parts the form takes, for the record).
# One case per launch signature (gemm_signatures) the towers reach and no other case of GEMM_FORM_CASES holds, each at the fewest rows
# (then columns, then K) of the domain of tests/test_gemm_form_coverage.py that reach it; that test prints the shape.
# "text B x S": the text tower (plain bf16 qkv epilogue; widths 1024 / 4096 and 1280 / 5120) at B prompts of S positions.
# Where the smallest shape of a main-step signature (256_TILE bf16 at 1537 rows, 256_TILE resid at 4865) is also the
# main step of a two-step case, that case holds it: every case here is the only one of the table with some signature
# (tests/test_gemm_form_coverage.py removes them one at a time).
GEMM_SIGNATURE_CASES = [
    ("text L14 5 x 13 last fc2, ring split-K", "resid", 65, 1024, 4096, dict(ksplit=8), ["SPLITK_RING"]),
    ("text L14 5 x 13 qkv, ring", "bf16", 65, 3072, 1024, {}, ["128R"]),
    ("text L14 5 x 13 fc1 gelu, ring", "gelu", 65, 4096, 1024, {}, ["128R"]),
    ("B16 b1 out-proj, ring", "resid", 197, 768, 768, {}, ["128R"]),
    ("text G14 9 x 57 qkv", "bf16", 513, 3840, 1280, {}, ["128_64"]),
    ("text G14 29 x 53 out-proj", "resid", 1537, 1280, 1280, {}, ["128_64"]),
    ("G14 b2 fc1 gelu + 128 x 64 leftover", "gelu", 2048, 8960, 1536, {}, ["256_TILE", "128_64"]),
    ("B16 b14 qkv rope, 128 x 128", "rope", 2758, 2304, 768, dict(tower="B16"), ["128_128"]),
    ("text G14 73 x 43 fc1 gelu + ring leftover", "gelu", 3139, 5120, 1280, {}, ["256_TILE", "128R"]),
    ("G14 b4 qkv rope, persistent", "rope", 4096, 4608, 1536, dict(tower="G14"), ["256P"]),
    ("text G14 65 x 67 qkv + skinny leftover", "bf16", 4355, 3840, 1280, {}, ["256_TILE", "SKINNY_411"]),
    ("text G14 94 x 47 qkv + ring leftover", "bf16", 4418, 3840, 1280, {}, ["256_TILE", "128R"]),
    ("text G14 139 x 35 qkv + 128 x 64 leftover", "bf16", 4865, 3840, 1280, {}, ["256_TILE", "128_64"]),
    ("text G14 151 x 39 qkv + 128 x 128 leftover", "bf16", 5889, 3840, 1280, {}, ["256_TILE", "128_128"]),
    ("text G14 173 x 37 fc1 gelu, queued stores + 1 fused row", "gelu", 6401, 5120, 1280, {}, ["256Q_QTAIL"]),
    ("text G14 223 x 31 qkv, queued stores", "bf16", 6913, 3840, 1280, {}, ["256Q"]),
    ("text G14 130 x 67 qkv, queued stores + 6 fused rows", "bf16", 8710, 3840, 1280, {}, ["256Q_QTAIL"]),
    ("text G14 184 x 71 out-proj + skinny leftover", "resid", 13064, 1280, 1280, {}, ["256_TILE", "SKINNY_411"]),
    ("text G14 184 x 71 fc2 + fragment skinny leftover", "resid", 13064, 1280, 5120, {}, ["256_TILE", "SKINNY_444"]),
    ("G14 b15 out-proj + 128 x 128 leftover", "resid", 15360, 1536, 1536, {}, ["256_TILE", "128_128"]),
    ("G14 b18 out-proj fold, planes out, 256-row tiles", "resid_ln:out", 18432, 1536, 1536, {}, ["256P", "LN_FOLDED", "PLANES_OUT"]),
    ("G14 b18 last fc2 planes in, fp32 out, 256-row tiles", "resid_ln:in", 18432, 1536, 8960, {}, ["256P", "PLANES_IN"]),
    ("G14 b24 fc1 gelu + fold, 128 x 64 leftover", "ln_in:gelu", 24576, 8960, 1536, {}, ["256Q", "128_64", "LN_CONSUMED"]),
    ("L14 b50 fc1 gelu + fold, ring leftover", "ln_in:gelu", 28850, 4096, 1024, {}, ["256Q", "128R", "LN_CONSUMED"]),
]

_L, _G = 36928, 32768
GEMM_FORM_CASES = [
    # PE-L14 at batch 64: the forward's own launches
    ("L14 b64 qkv rope + fold", "ln_in_rope", _L, 3072, 1024, dict(tower="L14"), ["256P", "LN_CONSUMED"]),
    ("L14 b64 out-proj fold, planes out", "resid_ln:out", _L, 1024, 1024, {}, ["256P_192", "LN_FOLDED", "PLANES_OUT"]),
    ("L14 b64 fc1 gelu + fold", "ln_in:gelu", _L, 4096, 1024, dict(pad=True), ["256Q_QTAIL", "LN_CONSUMED"]),
    ("L14 b64 fc2 planes in/out", "resid_ln:inout", _L, 1024, 4096, {}, ["256P_192", "LN_FOLDED", "PLANES_IN", "PLANES_OUT"]),
    ("L14 b64 last fc2 planes in, fp32 out", "resid_ln:in", _L, 1024, 4096, {}, ["256P_192", "PLANES_IN"]),
    ("L14 b64 out-proj fold, fp32 rows + bf16 copy", "resid_ln:none", _L, 1024, 1024, {}, ["256P_192", "LN_FOLDED"]),
    # PE-L14 at batch 8
    ("L14 b8 qkv rope", "rope", 4616, 3072, 1024, dict(tower="L14"), ["256_TILE"]),
    ("L14 b8 fc2", "resid", 4616, 1024, 4096, {}, ["SPLITK_256"]),
    # PE-L14 at batch 1
    ("L14 b1 out-proj + LayerNorm", "resid_norm", 577, 1024, 1024, dict(ksplit=3), ["SPLITK_RING_LN"]),
    ("L14 b1 fc2 + LayerNorm", "resid_norm", 577, 1024, 4096, dict(ksplit=3), ["SPLITK_RING_LN"]),
    ("L14 b1 fc1 gelu", "gelu", 577, 4096, 1024, {}, ["128_64"]),
    ("L14 b1 qkv rope", "rope", 577, 3072, 1024, dict(tower="L14"), ["128R"]),
    # the consumer's merge at the other slot counts; G14
    ("K512 consumer (parts 2)", "ln_in:bf16", _L, 1024, 512, {}, ["256Q", "128_64", "LN_CONSUMED"]),
    ("K768 consumer gelu (parts 3)", "ln_in:gelu", _L, 3072, 768, dict(tower="B16"), ["256Q", "LN_CONSUMED"]),
    ("G14 qkv rope + fold (parts 6)", "ln_in_rope", _G, 4608, 1536, dict(tower="G14"), ["256P", "LN_CONSUMED"]),
    ("G14 fc1 gelu + fold (parts 6)", "ln_in:gelu", _G, 8960, 1536, {}, ["256Q", "128_128", "LN_CONSUMED"]),
    ("G14 fc2 planes in/out", "resid_ln:inout", _G, 1536, 8960, {}, ["256P", "LN_FOLDED", "PLANES_IN", "PLANES_OUT"]),
    # the split-K reduce with the LayerNorm at the widths the towers do not reach
    ("reduce N256 MAXG 1", "resid_norm", 577, 256, 1024, dict(ksplit=4), ["SPLITK_RING_LN"]),
    ("reduce N1536 MAXG 3", "resid_norm", 577, 1536, 1024, dict(ksplit=2), ["SPLITK_RING_LN"]),
    ("reduce N2048 MAXG 4", "resid_norm", 300, 2048, 1024, dict(ksplit=2), ["SPLITK_RING_LN"]),
    ("reduce B16 fc2 MAXG 2 (partial group)", "resid_norm", 197, 768, 3072, dict(ksplit=8), ["SPLITK_RING_LN"]),
    # the tail split: whole rounds of 256-row tiles + the leftover rows' own launch
    ("tail split resid + ring split-K", "resid", 33000, 1024, 2048, dict(ksplit=4), ["256P", "SPLITK_RING"]),
    ("tail split resid + 256 split-K", "resid", 17000, 2048, 2048, dict(ksplit=4), ["256P", "SPLITK_256"]),
    ("tail split gelu, drained kernel", "gelu", _L, 4096, 1024, dict(qstores=0), ["256P", "SKINNY_411"]),
    # forced forms
    ("forced one workgroup per tile", "gelu", _L, 4096, 1024, dict(variant=1 << 16), ["256_TILE", "SKINNY_411"]),
    ("forced no split-K leftover", "resid", 33000, 1024, 2048, dict(variant=1 << 17), ["256P", "128R"]),
    ("forced no ring", "rope", 577, 3072, 1024, dict(tower="L14", variant=1 << 19), ["128_64"]),
    ("forced no 192-row tiles", "resid", _L, 1024, 1024, dict(variant=1 << 3), ["256P", "128_64"]),
    # Odd numbers of K-tiles (K = 192, 320, 1088, 2112: 3, 5, 17, 33 tiles of 64; no tower has one).  gemm256_mainloop walks K
    # two tiles per trip and peels an odd last tile into a block of its own, with its own DMA requests, wait counts and
    # barriers: these cases run that block in every 256-tile kernel that has one, and the 128-row kernels beside them.  N is
    # chosen for the form (1280 / 1088 columns keep the 192-row plan and the queued stores away), never K.  The leftover
    # rows fused into the queued-stores launch (256Q_QTAIL) need K % 256 == 0 and the folded LayerNorm's consumer reads
    # one statistics slot per 256 columns of K (LnStats): neither exists at an odd tile count.  128_64 and 128R need
    # K >= 512 (gemm_plan.h gemm_plan_128): 1088 is the odd count they can have.
    ("K192 resid, 256-row persistent", "resid", _L, 1280, 192, {}, ["256P"]),
    ("K320 resid, 256-row persistent", "resid", _L, 1280, 320, {}, ["256P"]),
    ("K192 bf16, 256-row persistent", "bf16", _L, 1088, 192, {}, ["256P"]),
    ("K1088 bf16, 256-row persistent", "bf16", _L, 1088, 1088, {}, ["256P"]),
    ("K192 out-proj fold, planes out", "resid_ln:out", _L, 1024, 192, {}, ["256P_192", "LN_FOLDED", "PLANES_OUT"]),
    ("K320 out-proj fold, planes out", "resid_ln:out", _L, 1024, 320, {}, ["256P_192", "LN_FOLDED", "PLANES_OUT"]),
    ("K1088 fc2 planes in/out", "resid_ln:inout", _L, 1024, 1088, {}, ["256P_192", "LN_FOLDED", "PLANES_IN", "PLANES_OUT"]),
    ("K192 gelu, queued stores", "gelu", _G, 4096, 192, {}, ["256Q"]),
    ("K1088 gelu, queued stores", "gelu", _G, 4096, 1088, {}, ["256Q"]),
    ("K320 gelu, queued stores + leftover rows", "gelu", _L, 4096, 320, {}, ["256Q", "128_128"]),
    ("K320 forced one workgroup per tile", "gelu", _G, 4096, 320, dict(variant=1 << 16), ["256_TILE"]),
    ("K1088 forced one workgroup per tile", "gelu", _G, 4096, 1088, dict(variant=1 << 16), ["256_TILE"]),
    ("K2112 b8 fc2, 256-tile split-K", "resid", 4616, 1024, 2112, {}, ["SPLITK_256"]),
    ("K192 b1 f32", "f32", 577, 4096, 192, {}, ["128_128"]),
    ("K192 b1 gelu", "gelu", 577, 4096, 192, {}, ["128_128"]),
    ("K1088 b1 gelu", "gelu", 577, 4096, 1088, {}, ["128_64"]),
    ("K1088 b1 qkv rope", "rope", 577, 3072, 1088, dict(tower="L14"), ["128R"]),
    # the text towers' widths where the signature is held above but the arithmetic differs: one partial 128-row tile on five K
    # parts of four K-tiles (the fewest the plan allows) with a reduce of MAXG 3 whose last group is partial; six parts of an
    # 80-tile K (uneven); the width-1024 out-proj of a few prompts; five column tiles on the 256-tile split-K
    ("text G14 5 x 13 out-proj + LayerNorm (MAXG 3, partial group)", "resid_norm", 65, 1280, 1280, dict(ksplit=5), ["SPLITK_RING_LN"]),
    ("text G14 2 x 72 fc2 + LayerNorm (80 K-tiles in 6 parts)", "resid_norm", 144, 1280, 5120, dict(ksplit=6), ["SPLITK_RING_LN"]),
    ("text L14 5 x 13 out-proj + LayerNorm", "resid_norm", 65, 1024, 1024, dict(ksplit=4), ["SPLITK_RING_LN"]),
    ("text G14 770 rows fc2, 256-tile split-K (5 column tiles)", "resid", 770, 1280, 5120, dict(ksplit=8), ["SPLITK_256"]),
] + GEMM_SIGNATURE_CASES + [(f"{m}x{n}x{k} {e}", e, m, n, k, {}, [f]) for e in ("f32", "resid") for (m, n, k), f in zip(
    GEMM_CASES, ["128_128", "SKINNY_444", "SKINNY_411", "SKINNY_444", "SKINNY_411", "SKINNY_411", "SKINNY_411", "SKINNY_411"])]


# ============================================== attention: planted high dynamic range ====
# The randn cases above move the optimistic softmax's reference once (tile 0, from -inf) or never (class-token prelude).
# These cases plant logit steps so that the reference moves late, more than once, for one row of a wave only (its 31 wave
# mates then rescale accumulators whose every term still counts), or stays put with l near 2^75.  A step goes through one
# coordinate d of a head: q[row, d] = 16 on the boosted query rows, k[key, d] = beta on the planted keys and 0 on every
# other key, so a boosted row's score on a planted key is the randn score of the other coordinates + 16 beta, i.e.
# 16 beta c octaves (c = hd^-0.5 log2 e: 0.1803 at head_dim 64, 0.1472 at 96) over its other scores, which stay within a
# few octaves of 0.  beta = bf16(lag / (16 c)): 8 significant bits, every planted value exact in bf16.  The other query
# rows keep their randn q[row, d] ~ N(0, 1): a planted key moves their score by N(0, 1) beta c, a few octaves either way.
#
# Which branch a case takes is a property of the data, checked on the CPU by Attention.emulate_optimistic
# (tests/test_kernel_bounds_teeth.py: every head's predicted move schedule is the one stated here); the GPU test cannot
# observe the path.
HDR_Q = 16.0
HDR_MUTATION_NAMES = [
    "O not rescaled on a move",
    "l not rescaled on a move",
    "exponentials not redone after a move",
    "alpha of the triggering row for the whole wave",
    "wave mates: m moved, alpha forced to 1",
    "previous tile's P.V applied after the rescale",
    "class-token term dropped on the tile-0 move",
]


def attention_k_lo(S, has_cls=True):
    """launch_attention_ex: the class-token key is split off when that saves a key tile (S = 1 mod 64)"""
    return 1 if (has_cls and S > 1 and (S - 1 + 63) // 64 < (S + 63) // 64) else 0


def attention_row_of_pos(pos, S, k_lo):
    """sequence row at position pos of the kernel's row order (rotated by one when the class-token key is split off)"""
    return (pos + 1) % S if k_lo else pos


def hdr_beta(lag, hd):
    """the planted key value that puts a boosted row's score `lag` octaves up: bf16(lag / (16 c))"""
    return float(torch.tensor(lag / (HDR_Q * hd ** -0.5 * LOG2E)).bfloat16())


def _hdr_mutation(name):
    def f(q, k, v):
        return Attention.emulate_optimistic(q, k, v, attention_k_lo(k.shape[-2]), mutate=name)["out"]
    return f


Attention.HDR_MUTATIONS = [(name, _hdr_mutation(name), 3.0) for name in HDR_MUTATION_NAMES]


def _plant(qpos, keys, moves, coord=0):
    """coordinate `coord`: query positions qpos (kernel row order) boosted; keys = [(key indices counted from k_lo, lag in
    octaves)]; moves = the tiles at which the boosted rows themselves must trigger a move (beyond the first one from -inf)"""
    return dict(coord=coord, qpos=list(qpos), keys=keys, moves=tuple(moves))


def _tile(t, offs=range(64)):
    return [64 * t + o for o in offs]


def _head(name, plants, cls=None, quiet=False, mates=False, others_plain=False):
    """cls: lag in octaves (signed) of the class-token key for the boosted rows, through plants[0]'s coordinate; quiet: no
    row's reference moves at all (beyond the first move from -inf); mates: at least 20 % of the boosted rows' wave mates
    move with 0 < alpha < 1; others_plain: the rows that are not boosted get 0 in the planted coordinates (with many
    coordinates planted their randn values would make every row of the head peaked on the planted keys)"""
    return dict(name=name, plants=plants, cls=cls, quiet=quiet, mates=mates, others_plain=others_plain)


# Every step but the ragged tiles' sits on 8 keys (both halves of a tile, all four lanes of attn16's split).  A row whose
# weight sits on two keys takes P's and the output's bf16 roundings without any averaging, and since U_BF16 is the relative
# half ulp at the bottom of a binade the bound is nearly attained there by construction -- by Attention.emulate with the
# true maximum as much as by the optimistic model (0.77 of the bound on a two-key row of an earlier draft of these cases).
# That is the bound's tightness, not a property of the moves, so the cases keep away from it.
_K8 = (1, 6, 12, 19, 27, 36, 46, 57)


def _every(r0, S):
    return range(r0, S, 32)


def _hdr_cases():
    cases = []

    def add(label, B, S, hd, h0, h1):
        cases.append(dict(label=label, B=B, S=S, H=2, hd=hd, heads=[h0, h1]))

    # ---- S577 hd64: class-token prelude, 9 full tiles, 19 wave groups in 3 workgroups (waves 0-3 and 4-7 both), q_rot
    S = 577
    add("S577 hd64 late rise tile 1 / mates tile 4", 2, S, 64,
        _head("late rise, tile 1 full", [_plant(_every(5, S), [(_tile(1), 96)], [1])], mates=True),
        _head("wave mates, 8 keys of tile 4", [_plant(_every(17, S), [(_tile(4, _K8), 96)], [4])], mates=True))
    add("S577 hd64 late rise tile 4 / staircase", 1, S, 64,
        _head("late rise, middle tile full", [_plant(_every(31, S), [(_tile(4), 96)], [4])], mates=True),
        _head("staircase +60, 112, +200", [_plant(_every(0, S), [(_tile(2, _K8), 60), (_tile(5, _K8), 112),
                                                                   (_tile(7, _K8), 312)], [5, 7])], mates=True))
    add("S577 hd64 late rise last tile / whole group", 1, S, 64,
        _head("late rise, last tile full", [_plant(_every(12, S), [(_tile(8), 96)], [8])], mates=True),
        _head("group 5 boosted, each row in its own tile",
              [_plant([160 + i for i in range(32) if i % 9 == j], [(_tile(j, _K8), 96)], [j], coord=j) for j in range(9)],
              mates=True, others_plain=True))
    add("S577 hd64 just below / class token far above", 1, S, 64,
        _head("just below the trigger", [_plant(_every(9, S), [(_tile(3, range(20, 30)), 72)], [])], quiet=True),
        _head("class token 150 octaves above", [_plant(_every(22, S), [], [])], cls=150, quiet=True))
    add("S577 hd64 class token far below / mates tile 0", 1, S, 64,
        _head("class token 150 octaves below", [_plant(_every(3, S), [], [0])], cls=-150, mates=True),
        _head("wave mates, 8 keys of tile 0", [_plant(_every(26, S), [(_tile(0, _K8), 96)], [0])], mates=True))
    # ---- S197 hd64: no prelude, 4 tiles, 5 keys in the last; 7 wave groups (waves 0-3 and 4-6), the last of 5 rows
    S = 197
    add("S197 hd64 ragged / mates tile 1", 2, S, 64,
        _head("row maximum on the last real key", [_plant(_every(3, S), [([196], 96)], [3])], mates=True),
        _head("wave mates, 8 keys of tile 1", [_plant(_every(20, S), [(_tile(1, _K8), 96)], [1])], mates=True))
    add("S197 hd64 staircase / late rise tile 1", 1, S, 64,
        _head("staircase +60, 112, +200", [_plant(_every(2, S), [(_tile(1, _K8), 63), (_tile(2, _K8), 115),
                                                                   (_tile(3, range(5)), 315)], [2, 3])], mates=True),
        _head("late rise, tile 1 full", [_plant(_every(30, S), [(_tile(1), 99)], [1])], mates=True))
    add("S197 hd64 just below / late rise tile 2", 1, S, 64,
        _head("just below the trigger", [_plant(_every(1, S), [(_tile(2, range(30, 40)), 75)], [])], quiet=True),
        _head("late rise, middle tile full", [_plant(_every(4, S), [(_tile(2), 99)], [2])], mates=True))
    # ---- S257 hd96: prelude, 4 full tiles, 9 wave groups in 2 workgroups
    S = 257
    add("S257 hd96 mates tile 2 / class token far below", 2, S, 96,
        _head("wave mates, 8 keys of tile 2", [_plant(_every(9, S), [(_tile(2, _K8), 96)], [2])], mates=True),
        _head("class token 150 octaves below", [_plant(_every(28, S), [], [0])], cls=-150, mates=True))
    add("S257 hd96 staircase / class token far above", 1, S, 96,
        _head("staircase +60, 112, +200", [_plant(_every(14, S), [(_tile(1, _K8), 60), (_tile(2, _K8), 112),
                                                                    (_tile(3, _K8), 312)], [2, 3])], mates=True),
        _head("class token 150 octaves above", [_plant(_every(6, S), [], [])], cls=150, quiet=True))
    # ---- S130 hd96: no prelude, 3 tiles, 2 keys in the last; 5 wave groups (waves 0-4), the last of 2 rows
    S = 130
    add("S130 hd96 ragged / mates tile 1", 2, S, 96,
        _head("row maximum on the last real key", [_plant(_every(1, S), [([129], 99)], [2])], mates=True),
        _head("wave mates, 8 keys of tile 1", [_plant(_every(0, S), [(_tile(1, _K8), 99)], [1])], mates=True))
    add("S130 hd96 just below / late rise last tile", 1, S, 96,
        _head("just below the trigger", [_plant(_every(0, S), [(_tile(1, range(0, 10)), 75)], [])], quiet=True),
        _head("late rise, last tile full", [_plant(_every(1, S), [(_tile(2, (0, 1)), 99)], [2])], mates=True))
    return cases


ATTENTION_HDR_CASES = _hdr_cases()


def attention_hdr_qkv(case):
    """attention_qkv's randn buffer [B S, 3W] (bf16, CPU) with the case's steps planted; every planted value is exact in bf16"""
    B, S, H, hd = case["B"], case["S"], case["H"], case["hd"]
    k_lo = attention_k_lo(S)
    x = attention_qkv(B, S, H, hd).float().reshape(B, S, 3, H, hd)
    for h, head in enumerate(case["heads"]):
        coords = [p["coord"] for p in head["plants"]]
        x[:, :, 1, h, coords] = 0.0                                  # every key is plain in the planted coordinates ...
        if head["others_plain"]:
            x[:, :, 0, h, coords] = 0.0
        for p in head["plants"]:
            rows = [attention_row_of_pos(pos, S, k_lo) for pos in p["qpos"]]
            for d in coords:
                x[:, rows, 0, h, d] = HDR_Q if d == p["coord"] else 0.0
            for keys, lag in p["keys"]:                              # ... but the planted ones
                assert max(keys) < S - k_lo
                x[:, [k_lo + j for j in keys], 1, h, p["coord"]] = hdr_beta(lag, hd)
        if head["cls"] is not None:
            assert k_lo == 1
            x[:, 0, 1, h, coords[0]] = math.copysign(hdr_beta(abs(head["cls"]), hd), head["cls"])
    qkv = x.reshape(B * S, 3 * H * hd).bfloat16()
    assert torch.equal(qkv.float(), x.reshape(B * S, 3 * H * hd))   # nothing planted was rounded
    return qkv


def attention_hdr_schedule(case, h, em):
    """What Attention.emulate_optimistic (em, on the pairs of head h: one per image) predicts for head h, against what the
    case states.  Returns (facts, failures, text): facts feed NOT_CAUGHT's predicates."""
    S, k_lo = case["S"], attention_k_lo(case["S"])
    head = case["heads"][h]
    start = torch.isfinite(em["m_before"])                          # a move from -inf scales zeros: not a rescale
    moved, own, alpha = em["moved"] & start, em["own"] & start, em["alpha"]
    nt = moved.shape[-1]
    failures, boosted, parts = [], [], []
    for p in head["plants"]:
        rows = [attention_row_of_pos(pos, S, k_lo) for pos in p["qpos"]]
        boosted += rows
        want = torch.zeros(nt, dtype=torch.bool)
        want[list(p["moves"])] = True
        got = own[:, rows]
        if not bool((got == want).all()):
            failures.append(f"boosted rows of coordinate {p['coord']} trigger at tiles "
                            f"{sorted(set(got.nonzero()[:, -1].tolist()))}, stated {list(p['moves'])}")
        parts.append(f"boosted x{len(rows)} move at {list(p['moves'])}")
    others = torch.ones(S, dtype=torch.bool)
    others[boosted] = False
    if bool(own[:, others].any()):
        failures.append("a row that is not boosted triggers a move")
    partial = moved & ~own & (alpha > 0) & (alpha < 1)               # a mate whose earlier terms are scaled, not dropped
    mate_rows = (moved & ~own).any(-1)
    n_mates, n_partial = int(mate_rows.sum()), int(partial.any(-1).sum())
    frac = n_partial / max(n_mates, 1)
    if head["quiet"] and bool(moved.any()):
        failures.append(f"stated quiet, but moves at tiles {sorted(set(moved.nonzero()[:, -1].tolist()))}")
    if head["mates"] and frac < 0.2:
        failures.append(f"only {n_partial} of {n_mates} wave mates move with 0 < alpha < 1")
    weighty = moved & (alpha > 2.0 ** -20)                            # the earlier terms keep weight through the move
    # a mate's partial move still shows at the end only if the row does not move by itself later (that wipes the earlier terms)
    later_own = torch.flip(torch.cumsum(torch.flip(own, [-1]), -1), [-1]) - own.long() > 0
    lasting = bool((partial & ~later_own).any())
    facts = dict(S=S, moves=bool(moved.any()), late_moves=bool(moved[..., 1:].any()), mates=lasting,
                 mates_any=bool((moved & ~own & ~later_own).any()), cls_head=head["cls"] is not None,
                 cls_move=bool(k_lo and (weighty & ~later_own)[..., 0].any()), overflow=bool(em["overflow"].any()))
    text = (f"{head['name']}: " + "; ".join(parts) + f"; mates moved {n_mates}, with 0 < alpha < 1 {n_partial} ({frac:.0%})"
            + f"; l max 2^{float(torch.log2(em['l'].max())):.1f}")
    return facts, failures, text


_NO_MOVE = "no row's reference moves in this head: the model with the bug in it is the model"
NOT_CAUGHT.update({
    ("attention hdr", name): (lambda c: not c["moves"], _NO_MOVE) for name in HDR_MUTATION_NAMES})
NOT_CAUGHT.update({
    ("attention hdr", "alpha of the triggering row for the whole wave"):
        (lambda c: not c["mates_any"], "no row shares another row's trigger and keeps what it held: the boosted rows use their "
                                       "own alpha either way"),
    ("attention hdr", "wave mates: m moved, alpha forced to 1"):
        (lambda c: not c["mates"], "no wave mate moves with 0 < alpha < 1"),
    ("attention hdr", "previous tile's P.V applied after the rescale"):
        (lambda c: not c["late_moves"], "every move is at tile 0, where no earlier tile's P.V is pending"),
    ("attention hdr", "class-token term dropped on the tile-0 move"):
        (lambda c: not c["cls_move"], "no prelude, or no tile-0 move that leaves the class-token term a weight above 2^-20 in a row "
                                      "that does not wipe it by a move of its own later"),
    ("attention hdr", "exponentials not redone after a move"):
        (lambda c: not (c["mates"] or c["overflow"]),
         "p against the old reference is finite for every row that moves and no wave mate keeps a partial move: a boosted row's "
         "stale p is the same softmax against another reference"),
    ("attention hdr", "l not rescaled on a move"):
        (lambda c: not c["moves"] or (c["cls_head"] and not c["late_moves"] and c["S"] >= 512),
         "every move is the tile-0 move over a class token far below: what is not scaled is the prelude's l = 1, one key's "
         "worth against the row sum of 576 plain keys"),
    ("attention hdr", "softmax scale x 1.01"): (lambda c: c["S"] == 1, "one key"),
})


# ---- the data of test_attention_huge_logits and test_attention_peaked_softmax (tests/test_gpu_kernels.py), shared with the
# CPU teeth test that decides which of them the per-element bound can be asked of
HUGE_LOGITS_CASES = [(577, 64, 8.0), (260, 64, 12.0), (257, 96, 8.0), (577, 64, 30.0)]


def attention_huge_logits_qkv(S, hd, scale, B=2, H=2):
    W = H * hd
    g = torch.Generator(device="cpu").manual_seed(S + hd)
    qkv = torch.randn(B * S, 3 * W, generator=g)
    qkv[:, : 2 * W] *= scale
    # ascending scores along the key axis for the first head: the maximum keeps moving
    qkv[:, W:W + hd] += torch.linspace(0, scale, B * S)[:, None] * torch.sign(qkv[0, :hd])[None]
    return qkv.bfloat16()


def attention_peaked_qkv():
    """[577, 3 * 64] bf16, one head: one key dominates per query (key 500 aligned with query 3)"""
    S, hd = 577, 64
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(S, 3, hd, generator=g)
    x[:, 0] *= 0.1
    x[500, 1] = x[:, 0].mean(0) * 0 + 8.0 * torch.sign(x[3, 0])
    return x.reshape(S, 3 * hd).bfloat16()


# whether the per-element bound is asserted on that data (the model stays within 0.75 of it on the CPU: the teeth test)
HUGE_LOGITS_BOUND = {c: True for c in HUGE_LOGITS_CASES}
PEAKED_BOUND = True


# ==================================================== the front end: patch embedding ====
# The stage every other stage reads from: patchify (elementwise.hip patchify_kernel, and patchify_band_u8_kernel writing the
# same bytes), the weight split (head.hip split_hi_lo_hi_kernel), the split-precision patch GEMM with gemm.hip
# gemm_epilogue<EPI_PATCH> (position add, rows remapped past the class token) and the class-token rows (cls_rows_kernel).
#
# Inputs as the library receives them: conv1.weight w fp32 [W, 3, P, P], positional_embedding pos fp32 [S, W], class_embedding
# fp32 [W] or none, images uint8 or fp32 [B, 3, H, H].  Reference, fp64: tok[b, cls + g] = sum_k x_k w[:, k] + pos[cls + g] with
# x = (2 v - 255) / 255 for uint8 pixels v and the given value for fp32 ones, k in (channel, py, px) order; row 0 = cls + pos[0].
#
# What the kernels do, with u_b = U_BF16 and U = U_F32:
#   weights     ws = fl32(w fl32(1 / 255)): two fp32 roundings, |ws - w / 255| <= 2 U |w / 255| (1 + U);
#               hi = bf16(ws), lo = bf16(ws - hi) (the difference is exact): |ws - hi - lo| <= u_b |ws - hi| <= u_b^2 |ws|
#   u8 images   a = 2 v - 255, an odd integer of at most 8 bits: exact in bf16; the row is (a | a) against (hi | lo)
#   f32 images  v = fl32(255 x): one rounding, U |v|; hi = bf16(v), lo = bf16(v - hi): u_b^2 |v|; the row is (hi | hi | lo)
#               against (hi | lo | hi): (a_hi + a_lo)(w_hi + w_lo) less the product a_lo w_lo, which is <= u_b^2 (1 + u_b)^2 |v| |ws|
# so the operands as the MFMA sees them stand for x w up to  c_op (|a| |ws|^T)  with |a| = |2 v - 255| or |fl32(255 x)| and
#   c_op = (u_b^2 + 2 U) (1 + 2^-6) for u8,  (3 u_b^2 + 3 U) (1 + 2^-6) for f32  (1 + 2^-6 covers the cross terms: |w / 255|
#   against |ws|, |a_hi + a_lo| against |v|, (1 + u_b)^2).
# Accumulation: every bf16 product is exact in fp32; the sum over all parts Kp terms, in any order, is _acc_err of the operands
# as the MFMA sees them (zero padding columns counted: an upper bound).  Epilogue: one fp32 add, U (|acc| + |pos|).  A term
# below fp32's normal range may be flushed: parts Kp 2^-126 (only the 1e-30 pixels of the special-value fixture come near it).
# The class row is ONE fp32 add of two inputs: bit-exact, compared with torch.equal, not with a bound.
PATCH_TOWERS = {"T14-56": dict(image=56, P=14, W=128, cls=True), "N14-56": dict(image=56, P=14, W=192, cls=False),
                "B16": dict(image=224, P=16, W=768, cls=True), "L14": dict(image=336, P=14, W=1024, cls=True),
                "G14": dict(image=448, P=14, W=1536, cls=False)}
PATCH_C_OP = {True: (U_BF16 ** 2 + 2 * U_F32) * (1 + 2.0 ** -6), False: (3 * U_BF16 ** 2 + 3 * U_F32) * (1 + 2.0 ** -6)}
PATCH_FIXTURES = ["random", "coherent", "special"]              # special: fp32 images only


def _split_bf16(x32):
    hi = x32.bfloat16()
    return hi, (x32 - hi.float()).bfloat16()


def _pad_cols(t, Kp):
    return torch.nn.functional.pad(t, (0, Kp - t.shape[1]))


class PatchCase:
    """w fp32 [W, 3, P, P], pos fp32 [S, W], cls fp32 [W] or None, images uint8 / fp32 [B, 3, H, H], all on one device."""

    def __init__(self, w, pos, cls, images):
        self.w, self.pos, self.cls, self.images = w, pos, cls, images
        self.W, _, self.P, _ = w.shape
        self.B, self.G = images.shape[0], images.shape[-1] // self.P
        self.G2, self.c = self.G * self.G, 0 if cls is None else 1
        self.S, self.M = self.G2 + self.c, self.B * self.G2
        self.Kreal = 3 * self.P * self.P
        self.Kp = (self.Kreal + 63) // 64 * 64
        self.u8 = images.dtype == torch.uint8
        assert pos.shape == (self.S, self.W) and images.shape[-1] % self.P == 0
        self._cols = self._parts = None

    def cols(self, order="cpyx"):
        """im2col, [M, Kreal] in the images' dtype: k in (channel, py, px) order (the kernel's); "pyxc": the mutation"""
        if order == "cpyx" and self._cols is not None:
            return self._cols
        B, G, P = self.B, self.G, self.P
        x = self.images.reshape(B, 3, G, P, G, P)
        x = x.permute(0, 2, 4, 1, 3, 5) if order == "cpyx" else x.permute(0, 2, 4, 3, 5, 1)
        x = x.reshape(self.M, self.Kreal)
        if order == "cpyx":
            self._cols = x
        return x

    def x64(self, r0=0, r1=None):
        v = self.cols()[r0:r1].double()
        return (2 * v - 255) / 255 if self.u8 else v

    def ws(self, scale=None):
        """the fp32 weights the split sees: fl32(w fl32(1 / 255)), [W, Kreal]"""
        s = torch.tensor(1.0 / 255.0 if scale is None else scale, dtype=torch.float32, device=self.w.device)
        return self.w.reshape(self.W, self.Kreal) * s

    def a32(self, cols, shift=True):
        """the fp32 value patchify rounds to bf16: 2 v - 255 (exact), or fl32(255 x)"""
        if self.u8:
            return 2.0 * cols.float() - 255.0 if shift else cols.float()
        return cols * torch.tensor(255.0, dtype=torch.float32, device=cols.device)

    def gemm(self, r0=0, r1=None, cols=None, ws=None, shift=True):
        """The patch GEMM's operands as the MFMA sees them, a GemmCase (bf16 A [rows, parts Kp], B [W, parts Kp]):
        (a | a) x (hi | lo) for u8 images, (hi | hi | lo) x (hi | lo | hi) for fp32 ones, zero padded to Kp per part."""
        cols = self.cols()[r0:r1] if cols is None else cols[r0:r1]
        hi, lo = (_pad_cols(t, self.Kp) for t in _split_bf16(self.ws() if ws is None else ws))
        a = self.a32(cols, shift)
        if self.u8:
            ah = _pad_cols(a.bfloat16(), self.Kp)
            return GemmCase(torch.cat([ah, ah], 1), torch.cat([hi, lo], 1), None)
        ah, al = (_pad_cols(t, self.Kp) for t in _split_bf16(a))
        return GemmCase(torch.cat([ah, ah, al], 1), torch.cat([hi, lo, hi], 1), None)

    def pos_index(self, r0=0, r1=None):
        m = torch.arange(r0, self.M if r1 is None else r1, device=self.pos.device)
        return self.c + m % self.G2

    def pos_rows(self, r0=0, r1=None, index=None):
        return self.pos[self.pos_index(r0, r1) if index is None else index].double()

    def tokens(self, x):
        """the token rows of a [B, S, W] output in the GEMM's row order: [M, W]"""
        return x.reshape(self.B, self.S, self.W)[:, self.c:, :].reshape(self.M, self.W)

    def part_products(self):
        """fp64 [M, W] per part of the K axis (u8: a.hi, a.lo; f32: a_hi.w_hi, a_hi.w_lo, a_lo.w_hi)"""
        if self._parts is None:
            g, Kp = self.gemm(), self.Kp
            self._parts = [g.a[:, i * Kp:(i + 1) * Kp].double() @ g.b[:, i * Kp:(i + 1) * Kp].double().T
                           for i in range(g.K // Kp)]
        return self._parts


class PatchEmbed:
    """Token rows [r0, r1) of the GEMM's row order m = b G2 + g, i.e. output rows (b, cls + g): fp64 [rows, W]."""

    @staticmethod
    def reference(c, r0=0, r1=None):
        return c.x64(r0, r1) @ c.w.reshape(c.W, c.Kreal).double().T + c.pos_rows(r0, r1)

    @staticmethod
    def bound(c, r0=0, r1=None):
        g = c.gemm(r0, r1)
        pos = c.pos_rows(r0, r1)
        a = c.a32(c.cols()[r0:r1]).double().abs()
        return (_acc_err(g) + U_F32 * (g.acc().abs() + pos.abs()) + PATCH_C_OP[c.u8] * (a @ c.ws().double().abs().T)
                + g.K * 2.0 ** -126)

    @staticmethod
    def emulate(c, r0=0, r1=None):
        return (c.gemm(r0, r1).acc(dtype=torch.float32) + c.pos_rows(r0, r1).float()).double()

    @staticmethod
    def class_rows(c):
        """fp32 [W]: the one fp32 add of cls_rows_kernel (None without a class token)"""
        return None if c.cls is None else c.cls.float() + c.pos[0].float()


def _pe_sum(c, keep):
    p = c.part_products()
    return sum(p[i] for i in keep) + c.pos_rows()


def _pe_stride(c):
    """the GEMM reads patch rows at stride parts Kreal where patchify wrote them at parts Kp: the zero padding is data"""
    if c.Kp == c.Kreal:
        return None                            # (n/a: no padding)
    g = c.gemm()
    parts = g.K // c.Kp
    flat = torch.cat([g.a.double().flatten(), torch.zeros(g.K, dtype=torch.float64, device=g.a.device)])
    idx = torch.arange(c.M, device=g.a.device)[:, None] * (parts * c.Kreal) + torch.arange(g.K, device=g.a.device)[None, :]
    return flat[idx] @ g.b.double().T + c.pos_rows()


def _pe_pos(index_fn, need_cls=False, need_images=1):
    def f(c):
        if (need_cls and not c.c) or c.B < need_images:
            return None
        m = torch.arange(c.M, device=c.pos.device)
        return c.gemm().acc() + c.pos_rows(index=index_fn(c, m))
    return f


def _pe_row_m(c):
    """the token of GEMM row m stored at output row m, not (m / G2) S + cls + m % G2; the class rows are written afterwards
    and what no store reaches is taken as zero"""
    if not c.c:
        return None                            # (n/a: without a class token the two agree)
    out = torch.zeros(c.B * c.S, c.W, dtype=torch.float64, device=c.pos.device)
    out[:c.M] = c.gemm().acc() + c.pos_rows()
    out[::c.S] = PatchEmbed.class_rows(c).double()
    return c.tokens(out)


def _pe_no_shift(c):
    return c.gemm(shift=False).acc() + c.pos_rows() if c.u8 else None


# Asserted on every fixture: wrong rows, wrong order, wrong scale.
PatchEmbed.MUTATIONS = [
    ("Kp padding read as data (patch rows at stride Kreal)", _pe_stride, 3.0),
    ("pos of the neighbouring token", _pe_pos(lambda c, m: c.c + (m % c.G2 + 1) % c.G2), 3.0),
    ("pos row g instead of cls + g", _pe_pos(lambda c, m: m % c.G2, need_cls=True), 3.0),
    ("pos indexed by cls + m % S instead of cls + m % G2", _pe_pos(lambda c, m: (c.c + m % c.S) % c.S, True, 2), 3.0),
    ("output row m instead of the remapped row", _pe_row_m, 3.0),
    ("(c, py, px) order taken as (py, px, c)", lambda c: c.gemm(cols=c.cols("pyxc")).acc() + c.pos_rows(), 3.0),
    ("x = v / 255 without the 2 v - 255 shift", _pe_no_shift, 3.0),
    ("1 / 255 rounded to bf16", lambda c: c.gemm(ws=c.ws(float(torch.tensor(1 / 255.0).bfloat16()))).acc() + c.pos_rows(), 3.0),
]
# A dropped low part is u_b^2-small per term.  With random weights and pixels the dropped terms add incoherently and barely
# clear the rigorous (linear in the term count) accumulation term: about 6 x the bound on P14 / W1024 u8, 2.4 on P16 / W768
# fp32 images.  Asserted on the coherent fixtures, where every dropped term has one sign; printed on the others.
PatchEmbed.PART_MUTATIONS = [
    ("the weights' lo part dropped", lambda c: _pe_sum(c, [0] if c.u8 else [0, 2]), 3.0),
    ("the images' lo part dropped", lambda c: None if c.u8 else _pe_sum(c, [0, 1]), 3.0),
    ("w / 255 rounded to bf16 before the split", lambda c: c.gemm(ws=c.ws().bfloat16().float()).acc() + c.pos_rows(), 3.0),
]


def above_bf16(t, frac=0.45):
    """positive fp32 values moved to `frac` of a bf16 ulp above the bf16 value below them"""
    trunc = (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)
    return (trunc.double() + frac * bf16_ulp(trunc)).float()


def patch_weights(tower, fixture, seed, device="cpu", grid=None):
    """(w, pos, cls) of a tower's front end.  random: the synthetic initialiser's distributions (N(0, 0.02^2) weights,
    N(0, 1 / W) pos and cls).  coherent: positive weights whose w / 255 sits 0.45 of a bf16 ulp above a bf16 value (every
    lo part has one sign).  grid: patches per side when the test cuts the image down (the teeth test)."""
    t = PATCH_TOWERS[tower]
    W, P = t["W"], t["P"]
    G = grid or t["image"] // P
    g = torch.Generator(device=device).manual_seed(seed)
    w = torch.randn(W, 3, P, P, generator=g, device=device) * 0.02
    if fixture == "coherent":
        w = (above_bf16((w.abs() + 1e-3) / 255).double() * 255).float()
    pos = torch.randn(G * G + int(t["cls"]), W, generator=g, device=device) * W ** -0.5
    cls = torch.randn(W, generator=g, device=device) * W ** -0.5 if t["cls"] else None
    return w, pos, cls


def patch_images(tower, fixture, u8, B, seed, device="cpu", grid=None):
    """random: uniform bytes, or uniform fp32 in [-1, 1).  coherent: bytes >= 128 (a > 0), or fp32 pixels whose 255 x sits
    0.45 of a bf16 ulp above a bf16 value in [128, 255].  special (fp32): the uint8 lattice (2 v - 255) / 255 with exact 0,
    +-1, off-lattice values, values outside [-1, 1] and values around 1e-30 mixed in; patch 0 of image 0 all zero, patch 1
    all around 1e-30."""
    t = PATCH_TOWERS[tower]
    P = t["P"]
    side = (grid or t["image"] // P) * P
    g = torch.Generator(device=device).manual_seed(seed + 1)
    shape = (B, 3, side, side)
    if u8:
        assert fixture != "special"
        return torch.randint(128 if fixture == "coherent" else 0, 256, shape, generator=g, device=device, dtype=torch.uint8)
    r = torch.rand(shape, generator=g, device=device)
    if fixture == "random":
        return r * 2 - 1
    if fixture == "coherent":
        return (above_bf16(r * 127 + 128).double() / 255).float()
    v = torch.randint(0, 256, shape, generator=g, device=device).float()
    x = (2 * v - 255) / 255
    kind = torch.randint(0, 8, shape, generator=g, device=device)
    sign = torch.sign(r - 0.5)
    x = torch.where(kind == 1, torch.zeros_like(x), x)
    x = torch.where(kind == 2, sign, x)                              # +-1
    x = torch.where(kind == 3, r * 2 - 1, x)                         # off the lattice
    x = torch.where(kind == 4, sign * (1 + 3 * r), x)                # outside [-1, 1]
    x = torch.where(kind == 5, sign * 1e-30 * (1 + r), x)
    x[0, :, :P, :P] = 0.0
    x[0, :, :P, P:2 * P] = (sign * 1e-30 * (1 + r))[0, :, :P, P:2 * P]
    return x


def patch_case(tower, fixture, u8, B, seed=0, device="cpu", grid=None):
    return PatchCase(*patch_weights(tower, fixture, seed, device, grid), patch_images(tower, fixture, u8, B, seed, device, grid))


# The CPU teeth cases: (tower, patches per side, images) -- the real P, W and Kp with the grid cut to a few hundred rows
# and at least two images.
PATCH_TEETH_CASES = [("T14-56", 4, 12), ("N14-56", 4, 12), ("B16", 10, 3), ("L14", 10, 2), ("G14", 10, 2)]


def patch_gemm_form(M, N, K):
    """The launch form the plan (csrc/gemm_plan.h gemm_plan) gives EPI_PATCH, restated: gemm_use_256 (M >= 1024, N >= 256, at
    least 100 tiles of 256 x 256), then the persistent kernel above 256 tiles; else gemm_plan_128's choice.  No skinny form,
    no tail split, no split-K and no 192-row plan for this epilogue (gemm_plan_rows excludes them; tests/test_gemm_plan.py
    holds the plan to this restatement over its sweep)."""
    up = lambda a, b: -(-a // b)
    t256 = up(M, 256) * up(N, 256)
    if M >= 1024 and N >= 256 and t256 >= 100:
        return "256P" if K >= 128 and t256 > 256 else "256_TILE"
    if up(M, 128) * up(N, 128) <= 384 and K >= 512 and N % 64 == 0:
        return "128R" if up(M, 128) * up(N, 64) <= 256 else "128_64"
    return "128_128"


def patch_band(tower, u8, B, gather=False):
    """whether launch_patchify takes patchify_band_u8_kernel (u8, side % 16 == 0, B G >= 64, not forced off)"""
    t = PATCH_TOWERS[tower]
    return bool(u8 and t["image"] % 16 == 0 and B * (t["image"] // t["P"]) >= 64 and not gather)


# Every kernel launch_gemm can send EPI_PATCH through.  gemm.hip compiles the epilogue into gemm_epilogue (gemm128_kernel at
# 128 x 128 and 128 x 64, gemm128r_kernel) and three 256-row kernels; of those, gemm256pp_kernel (phase groups, time stamps)
# exists in the experiment build only and is entered only when a script sets phase groups or a stamp buffer, so no forward
# reaches it.  The 192-row plan, split-K and the tail split are EPI_RESID_F32's, the queued stores the bf16 epilogues'.
PATCH_FORMS = ["128R", "128_64", "128_128", "256_TILE", "256P"]


def _patch_form_cases():
    """(tower, fixture, u8, B, REVO_PATCHIFY_GATHER, form): the GPU cases of tests/test_gpu_patch_embed.py.  Batches per tower:
    one image; either side of the band-patchify condition B G >= 64 (u8, and the band batch again with the gather form
    forced); the largest batch of each 128-row form and the first of the next; either side of use_256 (B16 43 | 44, L14
    10 | 11, G14 4 | 5); the smallest batch on the persistent kernel, which then walks 264 tiles with 256 workgroups (B16 112:
    86 x 3 tiles, L14 29: 66 x 4, G14 11: 44 x 6) and L14's benchmark batch of 64.  B16 has 196 rows per image and no K
    padding: every tile of every form holds an image boundary.  The Tiny towers (W < 256: ring kernel only) run the gather
    patchify (56 % 16 != 0) with K padded 588 -> 640."""
    u, f = True, False
    rows = {
        "T14-56": [("random", u, 1, "128R"), ("random", u, 5, "128R"), ("random", f, 1, "128R"), ("random", f, 5, "128R"),
                   ("coherent", u, 5, "128R"), ("coherent", f, 5, "128R"), ("special", f, 5, "128R")],
        "N14-56": [("random", u, 1, "128R"), ("random", u, 5, "128R"), ("random", f, 1, "128R"), ("random", f, 5, "128R"),
                   ("coherent", u, 5, "128R"), ("coherent", f, 5, "128R"), ("special", f, 3, "128R")],
        "B16": [("random", u, 1, "128R"), ("random", u, 4, "128R"), ("random", u, 5, "128R"), ("random", u, 5, "128R", True),
                ("random", u, 13, "128R"), ("random", u, 14, "128_64"), ("random", u, 41, "128_64"), ("random", u, 43, "128_128"),
                ("random", u, 44, "256_TILE"), ("random", u, 112, "256P"),
                ("random", f, 1, "128R"), ("random", f, 14, "128_64"), ("random", f, 43, "128_128"),
                ("random", f, 44, "256_TILE"), ("random", f, 112, "256P"),
                ("coherent", u, 5, "128R"), ("coherent", u, 44, "256_TILE"), ("coherent", f, 5, "128R"),
                ("coherent", f, 44, "256_TILE"), ("special", f, 2, "128R")],
        "L14": [("random", u, 1, "128R"), ("random", u, 2, "128R"), ("random", u, 3, "128R"), ("random", u, 3, "128R", True),
                ("random", u, 4, "128_64"), ("random", u, 10, "128_64"), ("random", u, 11, "256_TILE"),
                ("random", u, 29, "256P"), ("random", u, 64, "256P"),
                ("random", f, 1, "128R"), ("random", f, 4, "128_64"), ("random", f, 10, "128_64"),
                ("random", f, 11, "256_TILE"), ("random", f, 29, "256P"),
                ("coherent", u, 3, "128R"), ("coherent", u, 11, "256_TILE"), ("coherent", f, 3, "128R"),
                ("coherent", f, 11, "256_TILE"), ("special", f, 2, "128R")],
        "G14": [("random", u, 1, "128R"), ("random", u, 2, "128_64"), ("random", u, 2, "128_64", True),
                ("random", u, 4, "128_64"), ("random", u, 5, "256_TILE"), ("random", u, 11, "256P"),
                ("random", f, 1, "128R"), ("random", f, 4, "128_64"), ("random", f, 5, "256_TILE"), ("random", f, 11, "256P"),
                ("coherent", u, 2, "128_64"), ("coherent", u, 5, "256_TILE"), ("coherent", f, 2, "128_64"),
                ("coherent", f, 5, "256_TILE"), ("special", f, 1, "128R")],
    }
    return [(tower, r[0], r[1], r[2], len(r) > 4, r[3]) for tower, rs in rows.items() for r in rs]


PATCH_FORM_CASES = _patch_form_cases()


def patch_case_id(case):
    tower, fixture, u8, B, gather, form = case
    return f"{tower} {fixture} {'u8' if u8 else 'f32'} b{B}{' gather' if gather else ''}"
