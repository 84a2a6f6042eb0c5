"""The row normaliser (elementwise.hip l2norm_rows_kernel, through revo_op_l2norm_rows) against fp64 with the bounds of
tests/_norm_bounds.py, and the rounding norms it measures -- the only inputs of the exactness certificate -- against the
fp64 norms of the rows it returned.  |got - ref| <= bound everywhere, the largest ratio of each case printed; the bf16 row
is the round-to-nearest-even of the fp32 row bit for bit; cert_eps on the kernel's numbers is at least the formula on the
exact norms; and the kernel's other duties hold exactly: one row's bits whatever the batch, the form, the scale or the row
map; normalize = 0 a bit copy; the counters cleared to the last word; NaN / Inf rows out of the maxima; the maxima
maximised across calls.  tests/test_norm_bounds_teeth.py shows on the CPU that each of these checks has teeth."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

import _norm_bounds as nb
import reverso_amd  # noqa: F401
from _kernel_bounds import ratio
from reverso_amd import _lib, engine

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SENTINEL_BF16 = 0x7777
SENTINEL_WORD = 0x5A5A5A5A


def _report(what, label, r):
    print(f"[{what} {label}] max |got - ref| / bound = {r:.3f}")
    assert r <= 1.0, (what, label, r)


def _run(lib, dev, x, normalize, outs="both", pads=(0, 0, 0), initial=(0.0, 0.0), stats=True, dst_rows=None, n_dst=None,
         zero=(0, 0)):
    """One launch on x [rows, D] (CPU fp32): the source in a stride of D + pads[0] with NaN in the padding, every output
    between guard rows (and with padding columns) of a sentinel.  Returns y [n_dst, D] fp32 / yb [n_dst, D] int16 (None when
    not asked for), stats [rows, 2], maxima [2] (started from `initial`), za / zb (the cleared arrays) and `untouched`."""
    rows, D = x.shape
    n_dst = rows if n_dst is None else n_dst
    src = torch.full((rows, D + pads[0]), math.nan)
    src[:, :D] = x
    src = src.to(dev)
    f32 = torch.full((n_dst + 2, D + pads[1]), SENTINEL, device=dev) if outs in ("both", "f32") else None
    b16 = torch.full((n_dst + 2, D + pads[2]), SENTINEL_BF16, dtype=torch.int16, device=dev) if outs in ("both", "bf16") else None
    st = torch.full((rows + 2, 2), SENTINEL, device=dev) if stats else None
    mx = torch.tensor([SENTINEL, initial[0], initial[1], SENTINEL], device=dev) if stats else None
    zs = [torch.full((n + 8,), SENTINEL_WORD, dtype=torch.int32, device=dev) for n in zero]
    m = None if dst_rows is None else dst_rows.to(dev)
    assert m is None or (int(m.min()) >= 0 and int(m.max()) < n_dst)
    _lib.check(lib.revo_op_l2norm_rows(
        _lib.ptr(src), D + pads[0], None if f32 is None else _lib.ptr(f32[1:]), D + pads[1],
        None if b16 is None else _lib.ptr(b16[1:]), D + pads[2], rows, D, normalize, None if st is None else _lib.ptr(st[1:]),
        None if mx is None else _lib.ptr(mx[1:]), _lib.ptr(zs[0][4:]) if zero[0] else None, zero[0],
        _lib.ptr(zs[1][4:]) if zero[1] else None, zero[1], _lib.ptr(m), _lib.current_stream()), "revo_op_l2norm_rows")
    torch.cuda.synchronize()
    ok = True
    for buf, sent in ((f32, SENTINEL), (b16, SENTINEL_BF16)):
        if buf is not None:
            ok &= bool((buf[0] == sent).all() and (buf[-1] == sent).all() and (buf[1:-1, D:] == sent).all())
    if stats:
        ok &= bool((st[0] == SENTINEL).all() and (st[-1] == SENTINEL).all() and mx[0] == SENTINEL and mx[3] == SENTINEL)
    for z in zs:
        ok &= bool((z[:4] == SENTINEL_WORD).all() and (z[-4:] == SENTINEL_WORD).all())
    return SimpleNamespace(y=None if f32 is None else f32[1:-1, :D].cpu(), yb=None if b16 is None else b16[1:-1, :D].cpu(),
                           stats=None if st is None else st[1:-1].cpu(), maxima=None if mx is None else mx[1:3].cpu(),
                           za=zs[0][4:-4].cpu(), zb=zs[1][4:-4].cpu(), untouched=ok)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bf16_bits(y):
    return y.bfloat16().view(torch.int16)


# ------------------------------------------------------------------ every case against its bounds ----
@pytest.mark.parametrize("spec", nb.CASES, ids=nb.case_id)
def test_rows_and_stats_within_bounds(lib, dev, spec):
    x, D, normalize, label = nb.case_rows(spec), spec["D"], nb.normalize_of(spec), nb.case_id(spec)
    good = nb.finite_rows(x)
    base = _run(lib, dev, x, normalize)
    assert base.untouched
    y, xg = base.y[good], x[good]
    # the rows
    if normalize:
        _report("norm rows", label, ratio(y, nb.Rows.reference(xg), nb.Rows.bound(xg)))
    else:
        assert _same_bits(y, xg), "normalize = 0 is a bit copy"
    if spec["fixture"] == "zero row":
        z = spec["rows"] // 2
        assert not base.y[z].any() and not base.stats[z].any()
    if spec["fixture"] == "one-hot":
        assert (y.abs().sum(-1) == 1).all() and (y.abs().max(-1).values == 1).all() and (base.stats[:, 0] == 0).all()
    # the bf16 row: round to nearest even of the fp32 row as returned
    assert torch.equal(base.yb[good], _bf16_bits(y))
    # the statistics, against the fp64 norms of what was returned
    S = nb.Stats
    ref, bound = S.reference(y), S.bound(y)
    _report("norm stats", label, ratio(base.stats[good], ref[:, :2], bound[:, :2]))
    m_ref = nb.maxima(ref)
    _report("norm maxima", label, ratio(base.maxima, m_ref, m_ref * S.sigma(D) + nb.SUB))
    if good.any():
        assert _bits(base.maxima[1:]) == _bits(base.stats[good][:, 0].max().reshape(1)), "max_stats[1] is the largest row_stats[:, 0]"
    # the certificate's direction
    ok, r = nb.direction_holds(base.stats[good], base.maxima, ref, D)
    print(f"[direction {label}] smallest eps32 / eps64 = {r:.6f}")
    assert ok, r
    # the case's own strides and outputs: the same bits, padding and guards untouched
    if spec["outs"] != "both" or any(spec["pads"]):
        v = _run(lib, dev, x, normalize, outs=spec["outs"], pads=spec["pads"])
        assert v.untouched
        assert v.y is None or _same_bits(v.y[good], y)
        assert v.yb is None or torch.equal(v.yb[good], base.yb[good])
        assert _same_bits(v.stats[good], base.stats[good]) and _same_bits(v.maxima, base.maxima)
    # NaN / Inf rows: their neighbours' bits are those of a batch without them, and the maxima those of the good rows alone
    if spec["fixture"] == "nan inf":
        assert not good.all()
        clean = x.clone()
        clean[~good] = 1.0
        c = _run(lib, dev, clean, normalize)
        assert _same_bits(c.y[good], y) and _same_bits(c.stats[good], base.stats[good])
        alone = _run(lib, dev, xg, normalize)
        assert _same_bits(alone.maxima, base.maxima)


# ------------------------------------------------------------------ bit-for-bit contracts ----
@pytest.mark.parametrize("D", [65, 1024, 2048, 2049, 4160])
def test_a_row_does_not_depend_on_the_batch(lib, dev, D):
    x = torch.randn(67, D, generator=nb._gen(D, "batch"))
    whole = _run(lib, dev, x, 1)
    for r in (0, 1, 2, 3, 4, 66):
        one = _run(lib, dev, x[r:r + 1], 1)
        assert _same_bits(one.y[0], whole.y[r]) and torch.equal(one.yb[0], whole.yb[r]) and _same_bits(one.stats[0], whole.stats[r])
    for r0 in (1, 2, 3):                          # the same rows at every other position of the four-row workgroup
        part = _run(lib, dev, x[r0:r0 + 9], 1)
        assert _same_bits(part.y, whole.y[r0:r0 + 9]) and _same_bits(part.stats, whole.stats[r0:r0 + 9])


@pytest.mark.parametrize("normalize", [1, 0])
def test_register_form_and_loop_form_give_the_same_bits(lib, dev, normalize):
    x = torch.randn(7, 2048, generator=nb._gen(normalize, "forms"))
    reg = _run(lib, dev, x, normalize)
    loop = _run(lib, dev, torch.cat([x, torch.zeros(7, 64)], dim=1), normalize)
    assert _same_bits(loop.y[:, :2048], reg.y) and not loop.y[:, 2048:].any()
    assert torch.equal(loop.yb[:, :2048], reg.yb)
    assert _same_bits(loop.stats, reg.stats) and _same_bits(loop.maxima, reg.maxima)


@pytest.mark.parametrize("D", [128, 2112])
def test_a_power_of_two_scale_changes_no_bit(lib, dev, D):
    x = torch.randn(5, D, generator=nb._gen(D, "scale"))
    one = _run(lib, dev, x, 1)
    for k in (-40, -10, 10, 40):
        s = _run(lib, dev, x * 2.0 ** k, 1)
        assert _same_bits(s.y, one.y) and torch.equal(s.yb, one.yb)
        assert _same_bits(s.stats, one.stats) and _same_bits(s.maxima, one.maxima)
        # and stored as given, the measured norms scale with the rows exactly: the sums are taken on the scaled row
        g = _run(lib, dev, one.y * 2.0 ** k, 0)
        assert _same_bits(g.stats, one.stats * 2.0 ** k) and _same_bits(g.maxima, one.maxima * 2.0 ** k)


@pytest.mark.parametrize("rows,n_dst,D", [(3, 9, 128), (5, 5, 2112), (67, 300, 192)])
def test_row_map_scatters_the_same_bits(lib, dev, rows, n_dst, D):
    x = torch.randn(rows, D, generator=nb._gen(rows, D, "mapped")) * torch.arange(1, rows + 1)[:, None]
    m = nb.row_map(rows, n_dst)
    for normalize in (1, 0):
        direct = _run(lib, dev, x, normalize)
        mapped = _run(lib, dev, x, normalize, dst_rows=m, n_dst=n_dst, pads=(0, 4, 8))
        assert mapped.untouched
        assert _same_bits(mapped.y[m], direct.y) and torch.equal(mapped.yb[m], direct.yb)
        other = torch.ones(n_dst, dtype=torch.bool)
        other[m] = False
        assert (mapped.y[other] == SENTINEL).all() and (mapped.yb[other] == SENTINEL_BF16).all()
        assert _same_bits(mapped.stats, direct.stats) and _same_bits(mapped.maxima, direct.maxima)     # by source row


def test_maxima_are_maximised_across_calls(lib, dev):
    big = torch.randn(5, 128, generator=nb._gen("two calls")) * 3
    small = torch.randn(5, 128, generator=nb._gen("second"))
    a, b = _run(lib, dev, big, 0), _run(lib, dev, small, 0)
    assert (a.maxima > b.maxima).all()
    for first, second in ((a, small), (b, big)):
        both = _run(lib, dev, second, 0, initial=tuple(first.maxima.tolist()))
        assert _same_bits(both.maxima, torch.maximum(a.maxima, b.maxima))
    # a call with stats but nothing else to write
    only = _run(lib, dev, big, 0, outs="none")
    assert _same_bits(only.stats, a.stats) and _same_bits(only.maxima, a.maxima)


@pytest.mark.parametrize("rows", nb.CLEAR_ROWS)
def test_counter_arrays_are_cleared_to_the_last_word(lib, dev, rows):
    x = torch.randn(rows, 128, generator=nb._gen(rows, "clear"))
    counts = nb.CLEAR_COUNTS
    for na, nz in zip(counts, counts[::-1]):
        r = _run(lib, dev, x, 1, zero=(na, nz))
        assert r.untouched, (na, nz)
        assert len(r.za) == na and len(r.zb) == nz and not r.za.any() and not r.zb.any(), (na, nz)


def test_refusals_come_before_the_device(lib, dev):
    t = torch.zeros(64, device=dev)
    w = torch.zeros(4, dtype=torch.int32, device=dev)
    p, st = _lib.ptr, _lib.current_stream()
    f = lib.revo_op_l2norm_rows
    assert f(None, 8, p(t), 8, None, 0, 1, 8, 1, None, None, None, 0, None, 0, None, st) == -2
    assert f(p(t), 8, p(t), 8, None, 0, -1, 8, 1, None, None, None, 0, None, 0, None, st) == -2
    assert f(p(t), 8, p(t), 8, None, 0, 1, 0, 1, None, None, None, 0, None, 0, None, st) == -2
    assert f(p(t), 7, p(t), 8, None, 0, 1, 8, 1, None, None, None, 0, None, 0, None, st) == -2 and b"stride" in lib.revo_last_error()
    assert f(p(t), 8, p(t), 7, None, 0, 1, 8, 1, None, None, None, 0, None, 0, None, st) == -2
    assert f(p(t), 8, None, 0, p(t), 7, 1, 8, 1, None, None, None, 0, None, 0, None, st) == -2
    assert f(p(t), 8, p(t), 8, None, 0, 1, 8, 1, None, None, None, 1, None, 0, None, st) == -2
    assert f(p(t), 8, p(t), 8, None, 0, 1, 8, 1, None, None, p(w), 4, None, 1, None, st) == -2
    assert f(p(t), 8, p(t), 8, None, 0, 0, 8, 1, None, None, None, 0, None, 0, None, st) == 0          # no rows: nothing to do
    assert lib.revo_op_gallery_cert_stats(None, (C.c_float * 2)(), st) == -2


# ------------------------------------------------------------------ the range of normalize = 1 ----
def _unit64(rows, D, key):
    u = torch.randn(rows, D, generator=nb._gen(D, key)).double()
    return u / u.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("D", [128, 2112])
def test_normalise_holds_its_bound_to_both_edges_of_its_range(lib, dev, D):
    """The bound holds wherever the fp32 sum of squares neither overflows nor vanishes.  Just below NORM_HI it holds by its
    relative part alone; past NORM_HI the sum is +inf and the row comes out as zeros.  At NORM_LO, where the sum is still a
    normal number, and further down, where it is subnormal and the absolute term takes over, the row still comes out near unit
    length, inside the bound; with every x^2 rounding to 0 the row is left unscaled."""
    u = _unit64(4, D, "edges")
    inside = torch.cat([u[:2] * nb.NORM_LO * (1 + 2.0 ** -8), u[2:] * nb.NORM_HI * (1 - 2.0 ** -8)]).float()
    r = _run(lib, dev, inside, 1)
    R = nb.Rows
    rel_only = R.reference(inside).abs() * (nb.chain_roundings(D, False) / 2 + 3) * nb.U_F32 * nb.SECOND + nb.SUB
    _report("norm rows", f"D{D} at the edges", ratio(r.y, R.reference(inside), R.bound(inside)))
    assert ratio(r.y[2:], R.reference(inside)[2:], rel_only[2:]) <= 1.0
    over = (u[:2] * nb.NORM_HI * (1 + 2.0 ** -8)).float()
    assert torch.isfinite(over).all()
    z = _run(lib, dev, over, 1)
    assert (z.y == 0).all() and (z.stats == 0).all() and (z.maxima == 0).all()
    vanished = (u[:2] * 2.0 ** -76).float()                        # every |x| <= 2^-76: x^2 <= 2^-152 rounds to 0
    v = _run(lib, dev, vanished, 1)
    assert _same_bits(v.y, vanished)
    between = (u[:2] * math.sqrt(D) * 2.0 ** -70).float()          # the sum is subnormal: the absolute term, 2^-11 of |y| here
    b = _run(lib, dev, between, 1)
    assert torch.isfinite(R.bound(between)).all() and (R.bound(between) <= 2.0 ** -10 * R.reference(between).abs() + nb.SUB).all()
    _report("norm rows", f"D{D} with a subnormal sum", ratio(b.y, R.reference(between), R.bound(between)))


# ------------------------------------------------------------------ the gallery keeps what the kernel measured ----
def _exact_maxima(rows):
    s = nb.Stats.reference(rows.cpu())
    return float(s[:, 2].max()), float(s[:, 0].max())


def _holds(got, rows, tight):
    G, Eg = _exact_maxima(rows)
    sig = nb.Stats.sigma(rows.shape[1])
    print(f"[gallery maxima] got {got}, exact ({G:.9g}, {Eg:.9g})")
    assert got[0] >= G * (1 - sig) - nb.SUB and got[1] >= Eg * (1 - sig) - nb.SUB, (got, G, Eg)
    if tight:
        assert got[0] <= G * (1 + sig) + nb.SUB and got[1] <= Eg * (1 + sig) + nb.SUB, (got, G, Eg)


def test_gallery_maxima_bound_the_rows_present(dev):
    D = 128
    g = nb._gen(D, "gallery")
    a = torch.randn(200, D, generator=g)
    b = torch.randn(150, D, generator=g) * (0.5 + 1.5 * torch.rand(150, 1, generator=g)) / math.sqrt(D)      # norms 0.5 .. 2
    upd = torch.randn(10, D, generator=g) / math.sqrt(D)
    upd[3] *= 5.0                                                   # larger than any row before
    idx = torch.tensor([0, 5, 199, 200, 349, 17, 18, 19, 300, 301])
    G1, G0 = engine.Gallery(D, 1024, device=0), engine.Gallery(D, 1024, device=0, keep_f32=False)
    try:
        assert G1.cert_stats() == (0.0, 0.0)
        for G in (G1, G0):
            G.add(a, normalize=True)                                # from host memory
        _holds(G1.cert_stats(), G1.read(), True)
        assert G0.cert_stats() == G1.cert_stats()
        for G in (G1, G0):
            G.add(b.to(dev), normalize=False)                       # from device memory, stored as given
        _holds(G1.cert_stats(), G1.read(), True)
        assert G0.cert_stats() == G1.cert_stats()
        for G in (G1, G0):
            G.update(idx, upd.to(dev), normalize=False)
        _holds(G1.cert_stats(), G1.read(), False)
        assert G1.cert_stats()[0] >= float(upd[3].double().norm()) * (1 - 1e-6)
        assert G0.cert_stats() == G1.cert_stats()
        gone = torch.zeros(350, dtype=torch.bool)
        gone[::3] = True
        gone[200] = True                                            # the largest row leaves: the maxima stay upper bounds
        for G in (G1, G0):
            assert G.remove(gone) == int(gone.sum())
        _holds(G1.cert_stats(), G1.read(), False)
        assert G0.cert_stats() == G1.cert_stats()
        fresh = torch.cat([torch.randn(40, D, generator=g) * 7.0, a[:30]])      # new rows, and copies of rows still present
        _, _, kept = G1.add_unique(fresh.to(dev), 0.98, normalize=True)
        assert 40 <= int(kept.sum()) < 70
        _holds(G1.cert_stats(), G1.read(), False)
        for G in (G1, G0):
            assert G.remove(torch.ones(len(G), dtype=torch.bool)) > 0 and len(G) == 0
            assert G.cert_stats() == (0.0, 0.0)
            G.add(b, normalize=False)
            assert G.cert_stats()[0] > 0
            G.clear()
            assert G.cert_stats() == (0.0, 0.0)
    finally:
        G1.close()
        G0.close()


# ------------------------------------------------------------------ the two holes, end to end ----
@pytest.mark.parametrize("exponent", [67, -66], ids=["rows of norm 1.5e20", "rows of norm 1.4e-20"])
def test_scan_error_stays_under_eps_from_the_librarys_own_stats(lib, dev, exponent):
    """test_certificate_error_bound_is_rigorous' construction on a tiny gallery stored as given: unit rows moved to just above
    bf16 midpoints, queried by themselves.  exponent 67: eight of them times 2^67 among unit rows (squares past fp32's range:
    plain fp32 sums left them out of max ||g||); exponent -66: every row times 2^-66 (squared errors underflow: Eg was 0).
    eps is built from the gallery's own maxima and the normaliser's own query stats, and every measured
    |scan score - fp32 score| stays under it."""
    D, N, Q, k = 128, 512, 16, 16
    gal = nb.midpoint_rows(_unit64(N, D, "holes").float())
    queries = gal[:Q].clone()                            # (before the scaling: unit length)
    if exponent > 0:
        gal[:8] *= 2.0 ** exponent
    else:
        gal *= 2.0 ** exponent
    Gs = engine.Gallery(D, N, device=0, keep_f32=False)
    try:
        Gs.add(gal.to(dev), normalize=False)
        ss, si, _ = Gs.search(queries.to(dev), k)
        gstat = Gs.cert_stats()
    finally:
        Gs.close()
    ss, si = ss.cpu(), si.cpu()
    G, Eg = _exact_maxima(gal)
    sig = nb.Stats.sigma(D)
    assert gstat[0] >= G * (1 - sig) and gstat[1] >= Eg * (1 - sig), (gstat, G, Eg)
    q = _run(lib, dev, queries, 1)
    eps = nb.cert_eps32(q.stats[:, 0], q.stats[:, 1], gstat[0], gstat[1], D).double()
    exact = torch.einsum("qd,qkd->qk", q.y.double(), gal[si].double())
    err = (ss.double() - exact).abs().max(dim=1).values
    print(f"[holes 2^{exponent}] max err / eps = {float((err / eps).max()):.3f}, gstat {gstat}")
    assert (err <= eps).all(), (err / eps).max()
    assert float((err / eps).max()) >= 0.25            # the construction does come near the bound
    assert torch.equal(si[:8, 0], torch.arange(8))
