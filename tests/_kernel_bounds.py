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
    return torch.ldexp(torch.ones_like(a), (e - bits).to(torch.int64))


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

LAYERNORM_WIDTHS = [128, 192, 768, 1024, 1536]

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
