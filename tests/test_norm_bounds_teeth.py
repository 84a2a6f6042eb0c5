"""The bounds of the row normaliser and of the certificate's rounding norms (tests/_norm_bounds.py) have teeth (CPU only).

On every case the GPU tier (tests/test_gpu_norm_bounds.py) runs: the fp32 emulation of the kernel stays at or below
EMULATION_MAX of the bounds and meets the certificate's direction; every planted error leaves a bound by 3 x, or is listed
in NOT_CAUGHT with the reason and stays under 3 x there.  The 1.001 of cert_eps covers the statistics' bound and its own
roundings up to the largest D a launcher accepts.  And the sums of squares taken in plain fp32, as the kernel took them
before it scaled the row, miss the direction on rows of norm 1e20 and 1e-20: the scaled sums do not, and agree with the
plain ones in every bit on the rest of the case list."""
import math

import pytest
import torch

import _norm_bounds as nb
from _kernel_bounds import ratio
from test_kernel_bounds_teeth import EMULATION_MAX, _check  # noqa: F401

NORMALISED = [c for c in nb.CASES if nb.normalize_of(c)]


def _returned(spec):
    """(the finite source rows, the rows the emulated kernel returns for them)"""
    x = nb.case_rows(spec)
    x = x[nb.finite_rows(x)]
    return x, (nb.Rows.emulate(x) if nb.normalize_of(spec) else x.clone())


@pytest.mark.parametrize("spec", NORMALISED, ids=nb.case_id)
def test_rows_bound_has_teeth(spec):
    x, y = _returned(spec)
    R = nb.Rows
    _check("norm rows", nb.case_id(spec), nb.facts(spec, y), R.reference(x), R.bound(x), y.double(),
           [(name, f(x), need) for name, f, need in R.MUTATIONS])


def _with_maxima(s):
    return torch.cat([s.reshape(-1), nb.maxima(s)])


@pytest.mark.parametrize("spec", nb.CASES, ids=nb.case_id)
def test_stats_bound_has_teeth(spec):
    x, y = _returned(spec)
    S = nb.Stats
    ref, bound, em = S.reference(y), S.bound(y), S.emulate(y).double()
    muts = []
    for name, f, need in S.MUTATIONS:
        m = f(y)
        muts.append((name, None if m is None else _with_maxima(m), need))
    if spec["D"] > 64 * nb.NV:
        muts.append(("maxima skipped in the loop form", torch.cat([ref.reshape(-1), torch.zeros(2, dtype=torch.float64)]), 3.0))
    _check("norm stats", nb.case_id(spec), nb.facts(spec, y), _with_maxima(ref), _with_maxima(bound), _with_maxima(em), muts)
    ok, r = nb.direction_holds(em[:, :2].float(), nb.maxima(em).float(), ref, spec["D"])
    print(f"[direction {nb.case_id(spec)}] smallest eps32 / eps64 = {r:.6f}")
    assert ok, r
    # max_stats[1] is the largest row_stats[:, 0] in bits; and scaling by a power of two changed no bit of a row whose
    # squares fit fp32
    if spec["fixture"] not in ("huge", "tiny"):
        assert torch.equal(S.emulate(y), S.emulate(y, scaled=False)), nb.case_id(spec)


def _plain_maxima(em):
    """the maxima as the kernel kept them before: a row whose ||y|| or error norm is not below +inf is left out"""
    ny, ne = em[:, 2], em[:, 0]
    return torch.stack([ny[ny < math.inf].max(), ne[ne < math.inf].max()])


@pytest.mark.parametrize("spec", [c for c in nb.CASES if c["fixture"] in ("huge", "tiny")], ids=nb.case_id)
def test_plain_fp32_sums_miss_the_direction_on_huge_and_tiny_rows(spec):
    """The two holes, on the emulation: a finite row of norm 1e20 among unit rows squares to +inf and left the maxima (G = 1,
    not 1e20); rows of norm 1e-20 have every squared rounding error underflow (Eg = 0).  Scaled sums measure both."""
    x, y = _returned(spec)
    S, D = nb.Stats, spec["D"]
    ref = S.reference(y)
    plain = S.emulate(y, scaled=False)
    ok, r = nb.direction_holds(plain[:, :2], _plain_maxima(plain), ref, D)
    print(f"[plain sums {nb.case_id(spec)}] smallest eps32 / eps64 = {r:.3g}")
    assert not ok and r < 0.75
    if spec["fixture"] == "huge":
        assert plain[1, 2] == math.inf and _plain_maxima(plain)[0] < 2.0
    else:
        assert (plain[:, 0] == 0).all()
    em = S.emulate(y)
    ok, r = nb.direction_holds(em[:, :2], nb.maxima(em), ref, D)
    assert ok and ratio(em, ref, S.bound(y)) <= EMULATION_MAX


def test_slack_of_cert_eps_covers_the_bounds_to_the_longest_row():
    assert nb.D_MAX % 64 == 0 and 256 * nb.D_MAX * 2 < 2 ** 31 <= 256 * (nb.D_MAX + 64) * 2
    for D in nb.DIMS + [8192, 65536, nb.D_MAX]:
        assert nb.slack_covers(D), D
    # one chain of D / 64 steps per lane would not have: the loop form's runs are what keeps the longest rows covered
    assert not nb.slack_covers(nb.D_MAX, runs=False) and nb.slack_covers(2 ** 20, runs=False)
    # and cert_eps in fp32 loses no more than its CERT_ROUNDINGS roundings against the formula on the same numbers
    g = torch.Generator().manual_seed(5)
    for D in (64, 1024, nb.D_MAX):
        e_q, n_qb, G, Eg = (torch.rand(4096, generator=g) * s for s in (2.0 ** -9, 1.0, 3.0, 2.0 ** -8))
        got = nb.cert_eps32(e_q, n_qb, G, Eg, D).double()
        want = nb.cert_eps64(e_q.double(), n_qb.double(), G.double(), Eg.double(), D)
        assert (got >= want * 1.001 * (1 - nb.U_F32) ** nb.CERT_ROUNDINGS).all()
        assert (got <= want * 1.0011 + 2e-30).all()


def test_case_list_reaches_every_form_and_position():
    Ds, Rs = {c["D"] for c in nb.CASES}, {c["rows"] for c in nb.CASES}
    assert Ds == set(nb.DIMS) and Rs == set(nb.ROWS)
    assert any(c["D"] <= 64 * nb.NV for c in nb.CASES) and any(c["D"] > 64 * nb.NV for c in nb.CASES)
    assert {c["outs"] for c in nb.CASES} == set(nb.OUTS) and any(any(c["pads"]) for c in nb.CASES)
    assert {c["fixture"] for c in nb.CASES} == set(nb.FIXTURES)
    for f in nb.FIXTURES:
        assert {c["D"] > 64 * nb.NV for c in nb.CASES if c["fixture"] == f} == {True, False}, f
    for spec in nb.CASES:
        if spec["fixture"] == "nan inf":
            bad = ~nb.finite_rows(nb.case_rows(spec))
            assert bad[:4].sum() == 2 and not bad[0] and not bad[3]
    assert nb.chain_roundings(2048, True) == 38 and nb.chain_roundings(2112, True) == 32 + 1 + 6
    assert nb.chain_roundings(nb.D_MAX, True) == 32 + 2047 + 6 and nb.chain_roundings(nb.D_MAX, False) == 65535 + 6


def test_midpoint_rows_have_the_largest_error_norm():
    spec = next(c for c in nb.CASES if c["fixture"] == "midpoint")
    s = nb.Stats.reference(nb.case_rows(spec))
    # (half a bf16 ulp is 2^-9 of the binade's lower end: between 2^-9 |y| and 2^-8 |y| per element)
    assert ((s[:, 0] / s[:, 2]) > 2.0 ** -9).all() and ((s[:, 0] / s[:, 2]) <= 2.0 ** -8).all()
    onehot = nb.Stats.reference(nb.case_rows(next(c for c in nb.CASES if c["fixture"] == "one-hot")))
    assert (onehot[:, 0] == 0).all()


# ------------------------------------------------------------------ the other duties ----
def test_maxima_overwritten_across_calls_is_caught():
    big, small = torch.randn(5, 128, generator=nb._gen("two calls")) * 3, torch.randn(5, 128, generator=nb._gen("second"))
    S = nb.Stats
    first, second = S.reference(big), S.reference(small)
    ref = nb.maxima(second, initial=tuple(nb.maxima(first).tolist()))
    bound = ref * S.sigma(128) + nb.SUB
    assert ratio(nb.maxima(second), ref, bound) >= 3.0
    em = nb.maxima(S.emulate(small).double(), initial=tuple(nb.maxima(S.emulate(big).double()).tolist()))
    assert ratio(em, ref, bound) <= EMULATION_MAX


@pytest.mark.parametrize("rows,n_dst", [(3, 9), (5, 5), (67, 300)])
def test_stats_at_the_destination_row_is_caught(rows, n_dst):
    y = nb.Rows.emulate(torch.randn(rows, 128, generator=nb._gen(rows, "mapped")) * torch.arange(1, rows + 1)[:, None])
    ref = nb.Stats.reference(y)
    m = nb.row_map(rows, n_dst)
    assert len(set(m.tolist())) == rows and int(m.max()) < n_dst and not torch.equal(m, torch.arange(rows))
    assert ratio(nb.stats_at_destination(ref, m), ref, nb.Stats.bound(y)) >= 3.0


@pytest.mark.parametrize("words", nb.CLEAR_COUNTS)
def test_clearing_only_whole_blocks_is_caught(words):
    full, planted = nb.cleared(words), nb.cleared(words, whole_blocks_only=True)
    assert not full.any()
    if words % 256 == 0:
        assert torch.equal(full, planted)          # not caught: the mutation is the identity where the count is a multiple of 256
    else:
        assert planted.any()
    assert {w % 256 == 0 for w in nb.CLEAR_COUNTS} == {True, False}
