"""Coverage of tests/_stream_cases.py, checked without a GPU: every declaration of include/revo.h that takes a `void* stream`
is reached by a case of the late-input harness (tests/test_gpu_streams.py), directly or through the entry point that calls the
same launcher, or is listed as not run with a reason.  An entry point added later without a case fails here."""
import os
import re
import sys

import reverso_amd  # noqa: F401
from reverso_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _stream_cases as sc  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "revo.h")


def stream_declarations(text):
    """names of the functions declared with a `void* stream` parameter (comments stripped; both builds of the header)"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]


def uncovered(names, cases=None, via=None, not_run=None):
    cases = sc.CASES if cases is None else cases
    via = sc.VIA if via is None else via
    not_run = sc.NOT_RUN if not_run is None else not_run
    claimed = {n for c in cases.values() for n in c.abi}
    return [n for n in names if n not in claimed and n not in not_run and not (n in via and via[n] in claimed)]


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_parser_finds_the_declarations():
    names = stream_declarations(_header())
    assert len(names) == len(set(names)) >= 63
    for n in ("revo_sync", "revo_search_topk", "revo_vit_forward_regions", "revo_preprocess_crop_resize", "revo_probe_gridbar",
              "revo_op_gemm_resid_ln", "revo_search_stats"):
        assert n in names, n
    for n in ("revo_gallery_clear", "revo_gallery_read", "revo_gallery_pairs_read", "revo_version", "revo_search_set_total_rows"):
        assert n not in names, n


def test_every_stream_taking_entry_point_has_a_case_or_a_reason():
    names = stream_declarations(_header())
    assert uncovered(names) == []


def test_a_new_declaration_without_a_case_is_noticed():
    text = _header().replace("#ifdef __cplusplus\n}\n#endif",
                             "int32_t revo_made_up(revo_gallery* g, const float* x,\n        void* stream);\n#ifdef __cplusplus\n}\n#endif")
    assert uncovered(stream_declarations(text)) == ["revo_made_up"]


def test_a_claim_that_is_removed_is_noticed():
    names = stream_declarations(_header())
    for victim in ("sequence_clear_between_two_appends", "detect", "crop_resize_on_two_streams", "search_k10", "two_shards"):
        cases = {k: v for k, v in sc.CASES.items() if k != victim}
        if victim == "sequence_clear_between_two_appends":
            assert uncovered(names, cases) == []          # (append, search and cert_stats have other cases as well)
        else:
            assert uncovered(names, cases) != [], victim
    # the forward's claim carries the launchers named through it
    cases = {k: sc.Case(k, v.fn, [n for n in v.abi if n != "revo_vit_forward"]) for k, v in sc.CASES.items()}
    missing = uncovered(names, cases)
    assert "revo_vit_forward" in missing and "revo_op_gemm" in missing and "revo_op_attention" in missing


def test_claims_and_tables_name_real_entry_points():
    names = set(stream_declarations(_header()))
    table = set(_lib.BASE_SIGNATURES) | set(_lib.EXPERIMENT_SIGNATURES)
    for c in sc.CASES.values():
        assert c.abi, c.name
        for n in c.abi:
            assert n in table, (c.name, n)
            assert n in names, (c.name, n, "takes no stream")
    for n, entry in sc.VIA.items():
        assert n in table and n in names and entry in table and entry in names, (n, entry)
        assert n.startswith("revo_op_"), n                # only the thin launchers are claimed through another entry point
    for n, why in sc.NOT_RUN.items():
        assert n in table and n in names and len(why) > 20, n
    assert not (set(sc.NOT_RUN) & {n for c in sc.CASES.values() for n in c.abi})
    assert not (set(sc.NOT_RUN) & set(sc.VIA))
    assert len(sc.NOT_RUN) <= 8
