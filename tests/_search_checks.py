"""Checks of a GPU search result against the fp64 CPU oracle, shared by the search test modules (tests/test_gpu_search.py,
tests/test_gpu_filtered_kernels.py)."""
import numpy as np


def _check(out, ref, atol=1e-3, near_tie=0.0):
    """near_tie > 0: two neighbours whose oracle scores differ by less than that may come out swapped
    (the GPU re-scores with an fp32 fma chain, the oracle rounds an fp64 sum once: ~1e-7 apart)."""
    s, i, c = (t.cpu().numpy() for t in out)
    rs, ri, rc = ref
    assert np.array_equal(c, rc)
    if near_tie > 0.0 and not np.array_equal(i, ri):
        for q in np.where((i != ri).any(1))[0]:
            assert sorted(i[q].tolist()) == sorted(ri[q].tolist()), q
            for j in np.where(i[q] != ri[q])[0]:
                jj = int(np.where(ri[q] == i[q][j])[0][0])
                assert abs(jj - j) == 1 and abs(rs[q][jj] - rs[q][j]) <= near_tie, (q, j)
    else:
        assert np.array_equal(i, ri)
    fin = np.isfinite(rs)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.abs(s[fin] - rs[fin]).max(initial=0.0) <= atol
    return np.abs(s[fin] - rs[fin]).max(initial=0.0)


def _assert_indices_equal_up_to_fp32_ties(i, ri, rs, gal, qr, tie=3e-7):
    """Index equality with the fp64 oracle, except where fp32 cannot tell two rows apart: a differing position must hold
    a row whose true (fp64) score is within `tie` of the oracle's score at that position (the GPU's exact scores are
    fp32 fma chains, the oracle rounds an fp64 sum once: ~1e-7 apart).  Returns the number of queries whose index SETS
    differ (a tie exactly at the k-th place; swaps of neighbours inside the list are not counted)."""
    bad = np.where((i != ri).any(1))[0]
    if bad.size == 0:
        return 0
    g64 = None if callable(gal) else gal.astype(np.float64)       # callable: row index -> fp32 row (a gallery too large to copy)
    for q in bad:
        qv = qr[q].astype(np.float64)
        qv /= np.linalg.norm(qv)
        for j in np.where(i[q] != ri[q])[0]:
            row = gal(int(i[q, j])).astype(np.float64) if g64 is None else g64[i[q, j]]
            true = float(row @ qv / np.linalg.norm(row))
            assert abs(true - float(rs[q, j])) <= tie, (q, j, true, rs[q, j])
    return sum(sorted(i[q].tolist()) != sorted(ri[q].tolist()) for q in bad)      # queries whose index SETS differ


OFFSETS_PAST_2_31 = (2 ** 31 + 5, 2 ** 40 + 3)


def _assert_offset_moves_the_indices_only(call, index_positions, offsets=OFFSETS_PAST_2_31):
    """call(index_offset) -> the result tensors of one search.  The int64 contract of index_offset at and above 2^31: the
    tensors at index_positions are the offset-0 row indices plus the offset (padding stays -1), in int64; every other
    tensor (scores, counts, offsets, group ids) is byte-identical to the offset-0 result."""
    import torch
    base = call(0)
    assert any(bool((base[p] >= 0).any()) for p in index_positions)
    for off in offsets:
        got = call(off)
        assert len(got) == len(base)
        for p, (a, b) in enumerate(zip(base, got)):
            a, b = torch.as_tensor(a), torch.as_tensor(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (off, p)
            if p in index_positions:
                assert b.dtype == torch.int64 and torch.equal(b, torch.where(a >= 0, a + off, a)), (off, p)
            elif a.dtype == torch.float32:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (off, p)
            else:
                assert torch.equal(a, b), (off, p)
