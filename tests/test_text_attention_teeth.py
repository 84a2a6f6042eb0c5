"""CPU: the causal attention's per-element bound (tests/_text_reference.CausalAttention.bound) has teeth.  On the GPU test's
own seeded inputs at S = 33 every wrong reference -- no mask, the mask shifted by one in either direction, the mask applied
after the row maximum -- leaves the bound, while the fp32 emulation of the kernel's rounding steps stays well inside it, at
every sequence length the GPU test runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_bounds as kb  # noqa: E402
import _text_reference as tr  # noqa: E402

EMULATION_MAX = 0.75        # the emulation's share of the bound at most
MUTATION_MIN = 3.0          # a wrong reference exceeds the bound at least this many times


@pytest.mark.parametrize("B,H", tr.ATT_BH)
def test_wrong_references_leave_the_bound_at_33(B, H):
    S = 33
    q, k, v = tr.attention_split(tr.attention_qkv(B, S, H), B, S, H)
    A = tr.CausalAttention
    ref, bound = A.reference(q, k, v), A.bound(q, k, v)
    em = kb.ratio(A.emulate(q, k, v), ref, bound)
    print(f"[causal S{S} B{B} H{H}] emulation / bound max {em:.3f}")
    assert em <= EMULATION_MAX, em
    for label, fn in A.MUTATIONS:
        r = kb.ratio(getattr(A, fn)(q, k, v), ref, bound)
        print(f"    {label}: {r:.3g} x the bound")
        assert r >= MUTATION_MIN, (label, r)


@pytest.mark.parametrize("S", tr.ATT_SEQS)
def test_emulation_stays_inside_the_bound(S):
    A = tr.CausalAttention
    for B, H in tr.ATT_BH:
        q, k, v = tr.attention_split(tr.attention_qkv(B, S, H), B, S, H)
        r = kb.ratio(A.emulate(q, k, v), A.reference(q, k, v), A.bound(q, k, v))
        assert r <= EMULATION_MAX, (S, B, H, r)


def test_row_i_of_the_reference_sees_rows_up_to_i_only():
    B, S, H = 2, 77, 2
    q, k, v = tr.attention_split(tr.attention_qkv(B, S, H), B, S, H)
    base = tr.CausalAttention.reference(q, k, v)
    for cut in (1, 31, 32, 33, 64):
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        for t in (q2, k2, v2):
            t[:, cut + 1:] *= 1024.0
        assert torch.equal(tr.CausalAttention.reference(q2, k2, v2)[:, :cut + 1], base[:, :cut + 1])
