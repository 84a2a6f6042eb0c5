"""The late-input case of the boosted search (revo_search_boosted; DESIGN.md section 2e, tests/_stream_cases.py): the query, the
multipliers and the biases arrive on a side stream behind a sleep, and the call's outputs must have the default-stream run's
bytes.  The case is registered in the harness's own table from here, a file of its own, so that the header's coverage
(tests/test_stream_cases_host.py: every entry point that takes a stream has a case) counts it; this module sorts before
tests/test_gpu_streams.py, whose parametrised test then runs the case as well.  test_stream_cases_host.py reads the table when
its tests run, which is after every module of a session has been imported; run on its own, without this module, it reports
revo_search_boosted as uncovered."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_cases as sc  # noqa: E402


@sc.case("revo_search_boosted")
def boosted(r):
    G = sc.gallery(r, sc.rows(sc.N_ROWS, 66))
    g = torch.Generator().manual_seed(67)
    q = r.dev(sc.rows(1, 68)[0])
    m, b = r.dev(4 * torch.rand(sc.N_ROWS, generator=g)), r.dev(2 * torch.rand(sc.N_ROWS, generator=g) - 1)
    r.arm()
    r.out("boosted", G.search_boosted(q, m, b, k=50, min_similarity=-0.05))
    r.synchronous("boosted")
    sc._stats(r, G, "stats")


def test_the_case_is_in_the_table_and_the_header_is_covered():
    """CPU: with this module imported, no stream-taking declaration of include/revo.h is left without a case."""
    import re
    assert sc.CASES["boosted"].abi == ("revo_search_boosted",)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "revo.h")
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]
    assert "revo_search_boosted" in names
    claimed = {n for c in sc.CASES.values() for n in c.abi}
    assert [n for n in names if n not in claimed and n not in sc.NOT_RUN and not (n in sc.VIA and sc.VIA[n] in claimed)] == []


@pytest.mark.gpu
def test_boosted_search_with_late_inputs_on_a_side_stream():
    rep = sc.compare("boosted", sc.CASES["boosted"].fn)
    print(rep)
    assert not rep.failed, str(rep)
    assert not rep.mismatches, str(rep)
    assert rep.late.enqueue_ms < sc.SLEEP_MS / 2, str(rep)
