"""Every stream-taking entry point on a side stream whose inputs arrive behind a sleep, byte for byte against the same calls on
the default stream (tests/_stream_cases.py has the method and the cases, DESIGN.md section 2e the numbers).  First the
harness itself is held to three stand-ins for a library that breaks the contract: if it cannot see those, the sleep is too
short or the poison does not reach the inputs, and the real cases would prove nothing."""
import os
import sys

import pytest
import torch

import reverso_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- 1. teeth ------------------------------------------------------------------------------------------------------------------
def test_side_streams_run_beside_the_default_stream(dev):
    s1, s2 = sc.side_streams()
    assert s1 != s2 and s1 != torch.cuda.default_stream() and s2 != torch.cuda.default_stream()
    print("cycles per ms:", sc.cycles_per_ms())
    assert sc.cycles_per_ms() > 0


def test_a_fake_that_keeps_the_contract_passes(dev):
    rep = sc.compare("fake, correct", sc.fake_that_keeps_the_contract)
    print(rep)
    assert rep.ok, str(rep)


def test_a_counter_zeroed_on_the_default_stream_is_caught(dev):
    rep = sc.compare("fake, memset on stream 0", sc.fake_zeroes_a_counter_on_the_default_stream)
    print(rep)
    assert rep.mismatches and not rep.failed, str(rep)


def test_a_middle_step_on_the_default_stream_is_caught(dev):
    rep = sc.compare("fake, kernel on stream 0", sc.fake_launches_its_middle_step_on_the_default_stream)
    print(rep)
    assert rep.mismatches and not rep.failed, str(rep)


def test_a_synchronisation_inside_an_asynchronous_call_is_caught(dev):
    rep = sc.compare("fake, hidden synchronisation", sc.fake_synchronises_inside_an_asynchronous_call)
    print(rep)
    assert not rep.mismatches, str(rep)                     # (ordered, merely not asynchronous)
    assert len(rep.failed) == 1 and rep.failed[0].startswith("fake call: returned"), str(rep)


def test_poison_reaches_the_inputs(dev):
    """a late run that never feeds its inputs computes on NaN and on 0x5A5A5A5A"""
    seen = {}

    def fn(r):
        x, w = r.dev(sc.rows(2, 300)), r.dev(sc.bitmap(100, 301))
        if r.late:
            r._pending = []                                  # the copies never come
        r.arm()
        seen[r.late] = (x.clone(), w.clone())
        r.out("x", x)
        r.out("w", w)
    rep = sc.compare("never fed", fn)
    assert len(rep.mismatches) == 2, str(rep)
    assert bool(torch.isnan(seen[True][0]).all()) and bool((seen[True][1] == sc.POISON_WORD).all())
    assert not bool(torch.isnan(seen[False][0]).any())


# ---- 2. the library ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_late_inputs_on_a_side_stream(dev, name):
    rep = sc.compare(name, sc.CASES[name].fn)
    print(rep)
    assert not rep.failed, str(rep)
    assert not rep.mismatches, str(rep)
    assert rep.late.enqueue_ms < sc.SLEEP_MS / 2, str(rep)   # (the sleep is at least twice what any call needed)


def test_clear_leaves_the_maxima_of_a_fresh_gallery(dev):
    """rows of norm 2^20 -> clear -> unit rows: on either stream the certificate's maxima are those of a gallery that only
    ever held the unit rows (a maximum that survives the clear makes every bound 2^20 times too wide; a clear that lands
    after the next append makes it too small, which no search test can see)"""
    fresh = sc.fresh_unit_gallery_cert_stats()
    fn = sc.CASES["sequence_clear_between_two_appends"].fn
    for run in (sc.run_default, sc.run_late):
        r, got = run(fn)
        import json
        cert = json.loads(got["cert"])
        print(run.__name__, "cert_stats", cert, "fresh", fresh)
        assert cert == fresh, (run.__name__, cert, fresh)
        assert not r.failed, r.failed


def test_cert_stats_of_an_emptied_gallery_are_zero(dev):
    G = sc._engine().Gallery(sc.D, 100, device=0)
    try:
        G.add(sc.rows(100, 302).to(sc.DEV) * 7.0, normalize=False)
        assert G.cert_stats()[0] > 1.0
        G.clear()
        assert G.cert_stats() == (0.0, 0.0)
        G.add(sc.unit_rows()[:100].to(sc.DEV), normalize=False)
        g, e = G.cert_stats()
        # unit rows; bf16 keeps 8 significant bits: |bf16(x) - x| <= half an ulp <= 2^-8 |x| per element, so for the norms too
        assert abs(g - 1.0) <= 1e-6 and 0.0 < e <= 2.0 ** -8 * g * (1 + 1e-6), (g, e)
    finally:
        G.close()
