"""fp64 reference of the forward on a rectangular token grid (include/revo.h, GRIDS), composed from the
oracle's own sub-blocks (oracle.pe_vit layer_norm, self_attention, mlp, attn_pool, l2_normalize) with its own angle table and
resampled positions.  At the native grid it is oracle.pe_vit.embed(..., float64) exactly (tests/test_aspect_host.py).

Plain helpers, not a conftest.  Everything runs where the parameters live (CPU, or a device for the larger towers)."""

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pe_vit


def grid_of(cfg, grid):
    g = cfg.image_size // cfg.patch_size
    return (g, g) if grid is None else (int(grid[0]), int(grid[1]))


def rope_angles(cfg, grid=None, swap_axes=False):
    """fp64 angle table [S', head_dim] of a gh x gw grid: oracle.pe_vit.rope_angles with a position range per axis.  Integer
    coordinates from `use_cls` up, not rescaled; x-axis angles fill the first half of head_dim, y-axis the second; the class
    row is zeros.  swap_axes: the WRONG table, x and y exchanged (what the tests must be able to tell apart)."""
    gh, gw = grid_of(cfg, grid)
    hd = cfg.width // cfg.heads
    d = hd // 2
    freqs = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    start = 1 if cfg.use_cls else 0
    angy = ((torch.arange(gh, dtype=torch.float64) + start)[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
    angx = ((torch.arange(gw, dtype=torch.float64) + start)[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
    ay = angy[:, None, :].expand(gh, gw, d)                # row (y) position
    ax = angx[None, :, :].expand(gh, gw, d)                # column (x) position
    tab = torch.cat([ay, ax] if swap_axes else [ax, ay], dim=-1).reshape(gh * gw, hd)
    if cfg.use_cls:
        tab = torch.cat([torch.zeros(1, hd, dtype=torch.float64), tab], dim=0)
    return tab


def rope_cos_sin(cfg, grid=None):
    """What the device table holds, in fp64: [S', head_dim / 2, 2] (cos, sin) of one angle per interleaved pair."""
    ang = rope_angles(cfg, grid)[:, 0::2]
    return torch.stack([ang.cos(), ang.sin()], dim=-1)


def _axis(G, g_out):
    """source index pair and upper weight of every output index along one axis (half-pixel centres, fp64)"""
    o = torch.arange(g_out, dtype=torch.float64)
    s = ((o + 0.5) * G / g_out - 0.5).clamp_(min=0.0)
    i0 = s.floor().long().clamp_(max=G - 1)
    i1 = (i0 + 1).clamp_(max=G - 1)
    return i0, i1, s - i0.to(torch.float64)


def resample_positions(cfg, pos, grid=None, nearest=False):
    """fp64 [S', W] position table of a gh x gw grid from the native [S, W]: the class row kept, the G x G patch rows
    resampled bilinearly with half-pixel centres (F.interpolate(mode="bilinear", align_corners=False), no antialiasing).
    Returns (table, max|corner| per element) -- the second is what the device's rounding bound scales with.  At (G, G) the
    native table itself."""
    G = cfg.image_size // cfg.patch_size
    gh, gw = grid_of(cfg, grid)
    pos = pos.to(torch.float64)
    first = 1 if cfg.use_cls else 0
    if (gh, gw) == (G, G):
        return pos, pos.abs()
    p = pos[first:].reshape(G, G, -1)
    y0, y1, ly = _axis(G, gh)
    x0, x1, lx = _axis(G, gw)
    if nearest:
        yy, xx = torch.where(ly > 0.5, y1, y0), torch.where(lx > 0.5, x1, x0)
        out = p[yy][:, xx]
        corner = out.abs()
    else:
        ly, lx = ly[:, None, None], lx[None, :, None]
        p00, p01, p10, p11 = p[y0][:, x0], p[y0][:, x1], p[y1][:, x0], p[y1][:, x1]
        out = (1 - ly) * (1 - lx) * p00 + (1 - ly) * lx * p01 + ly * (1 - lx) * p10 + ly * lx * p11
        corner = torch.stack([p00.abs(), p01.abs(), p10.abs(), p11.abs()]).amax(0)
    out, corner = out.reshape(gh * gw, -1), corner.reshape(gh * gw, -1)
    if first:
        out, corner = torch.cat([pos[:1], out]), torch.cat([pos[:1].abs(), corner])
    return out, corner


@torch.no_grad()
def encode_image(params, cfg, images, grid=None, taps=None, swap_axes=False, nearest=False):
    """oracle.pe_vit.encode_image on [B, 3, gh * P, gw * P] images: un-normalised [B, out_dim] in fp64."""
    p = {k: v.to(torch.float64) for k, v in params.items()}
    images = images.to(torch.float64)
    B, P, W = images.shape[0], cfg.patch_size, cfg.width
    gh, gw = grid_of(cfg, grid)
    assert images.shape[2:] == (gh * P, gw * P), (images.shape, grid)

    def tap(name, t):
        if taps is not None:
            taps[name] = t.detach().clone()

    x = F.conv2d(images, p["visual.conv1.weight"], None, stride=P)       # [B,W,gh,gw]
    x = x.flatten(2).transpose(1, 2)                                      # [B,gh*gw,W]: patch (gy, gx) is row gy * gw + gx
    if cfg.use_cls:
        cls = p["visual.class_embedding"].reshape(1, 1, W).expand(B, 1, W)
        x = torch.cat([cls, x], dim=1)
    pos = resample_positions(cfg, p["visual.positional_embedding"].cpu(), grid, nearest=nearest)[0].to(images.device)
    x = x + pos[None]
    tap("embed", x)
    x = pe_vit.layer_norm(x, p["visual.ln_pre.weight"], p["visual.ln_pre.bias"], cfg.ln_eps)
    tap("ln_pre", x)
    ang = rope_angles(cfg, grid, swap_axes=swap_axes).to(images.device)
    for i in range(cfg.layers):
        pre = f"visual.transformer.resblocks.{i}."
        h = pe_vit.layer_norm(x, p[pre + "ln_1.weight"], p[pre + "ln_1.bias"], cfg.ln_eps)
        a = pe_vit.self_attention(h, p, cfg, pre, ang)
        if cfg.use_ls:
            a = a * p[pre + "ls_1.gamma"]
        x = x + a
        h = pe_vit.layer_norm(x, p[pre + "ln_2.weight"], p[pre + "ln_2.bias"], cfg.ln_eps)
        m = pe_vit.mlp(h, p, pre + "mlp.")
        if cfg.use_ls:
            m = m * p[pre + "ls_2.gamma"]
        x = x + m
        tap(f"block{i}", x)
    x = pe_vit.layer_norm(x, p["visual.ln_post.weight"], p["visual.ln_post.bias"], cfg.ln_eps)
    tap("ln_post", x)
    pooled = pe_vit.attn_pool(x, p, cfg)
    tap("pooled", pooled)
    out = pooled @ p["visual.proj"]
    tap("proj", out)
    return out


def embed(params, cfg, images, grid=None, **kw):
    """L2-normalised fp64 [B, out_dim]"""
    return pe_vit.l2_normalize(encode_image(params, cfg, images, grid, **kw))


def non_native_menu(cfg):
    from reverso_amd import config
    g = cfg.image_size // cfg.patch_size
    return [s for s in config.aspect_grids(cfg) if s != (g, g)]


def random_u8(n, cfg, grid, seed):
    gh, gw = grid_of(cfg, grid)
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 3, gh * cfg.patch_size, gw * cfg.patch_size),
                                                                 dtype=np.uint8))


ROPE_BOUND = 2.0 ** -24 + 1e-12          # one rounding of a value in [-1, 1] to fp32, and the host's libm against torch's
POS_BOUND = 6 * 2.0 ** -24                # times max|corner|: four weight roundings and the fma chain (include/revo.h)
