"""Teeth of the scan-sum bound (tests/_scan_bounds.py) on the CPU: at every admitted width of tests/test_gpu_search_widths.py
and on its data, a main loop that leaves the last K-tile out, adds it twice or multiplies it against the previous tile's
gallery columns (a stale LDS stage) breaks the bound for EVERY query -- on the scores a top-k search would return -- while
a strict left-to-right fp32 accumulation of the bf16 products, the slowest-converging order an fp32 accumulator can take,
stays inside it."""
import pytest
import torch

import _scan_bounds as sb

Q, K = 12, 10


@pytest.fixture(scope="module", params=sb.W, ids=[f"D{d}" for d in sb.W])
def data(request):
    D = request.param
    x, q = sb.rows(sb.N_SMALL, D), sb.queries(D, Q=Q)
    gb = sb.bf16_round(torch.nn.functional.normalize(x, dim=1))
    qb = sb.bf16_round(torch.nn.functional.normalize(q, dim=1))
    return D, qb, gb, sb.reference(qb, gb), sb.bound(qb, gb)


def test_fp32_chain_stays_inside_the_bound(data):
    D, qb, gb, ref, bnd = data
    s = sb.emulate(qb, gb, "chain")
    every = float(((s.double() - ref).abs() / bnd).max())
    s_top, i_top = torch.sort(s, dim=1, descending=True, stable=True)
    ratios = sb.check_topk(s_top[:, :K].contiguous(), i_top[:, :K].contiguous(), torch.full((Q,), K), ref, bnd, K)
    print(f"[scan bound teeth D={D}] fp32 chain: max ratio {every:.3f} over all {Q} x {sb.N_SMALL} scores, "
          f"{float(ratios.max()):.3f} over the top {K}")
    assert every <= 1.0


@pytest.mark.parametrize("what", sb.PLANTED)
def test_planted_main_loop_errors_break_the_bound(data, what):
    D, qb, gb, ref, bnd = data
    s = sb.emulate(qb, gb, what)
    ratios = sb.topk_ratio(s, K, ref, bnd)
    print(f"[scan bound teeth D={D}] {what}: ratio per query min {float(ratios.min()):.1f}, max {float(ratios.max()):.1f}")
    assert bool((ratios > 1.0).all()), ratios
    s_top, i_top = torch.sort(s, dim=1, descending=True, stable=True)
    with pytest.raises(AssertionError):
        sb.check_topk(s_top[:, :K].contiguous(), i_top[:, :K].contiguous(), torch.full((Q,), K), ref, bnd, K)
