"""The facade's reports, whole: every text, every item and every question to the store of the cases in _facade_cases.py
against the table recorded at the parent of the commit that gathered the report path into shared helpers
(tests/golden/facade_reports_parent.json, scripts/facade_reports_record.py)."""
import ast
import inspect
import json
import os
import sys
import textwrap

import pytest

import _facade_cases as fc
from reverso_amd import core_system
from reverso_amd.core_system import SimpleReverso

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "facade_reports_parent.json")
# functions of the range whose returns the table does not claim: the thumbnail (a decoded one is not portable) and the
# text tower's loader, which needs a device
NOT_REPORTS = {"thumbnail", "load_text_model", "embed_text", "visualize_detections"}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def replay():
    """(the table's results, the lines of core_system.py that ran on this thread meanwhile)"""
    path, lines = core_system.__file__, set()

    def tracer(frame, event, arg):
        if frame.f_code.co_filename != path:
            return None
        if event == "line":
            lines.add(frame.f_lineno)
        return tracer

    old = sys.gettrace()
    sys.settrace(tracer)
    try:
        rows = fc.run_table()
    finally:
        sys.settrace(old)
    return json.loads(json.dumps(rows)), lines


def test_reports_equal_the_parent_commits(golden, replay):
    rows, _ = replay
    assert [(r["method"], r["outcome"]) for r in rows] == [(g["method"], g["outcome"]) for g in golden]
    for n, (r, g) in enumerate(zip(rows, golden)):
        where = f"case {n}: {g['method']} / {g['outcome']}"
        assert r["text"] == g["text"], where
        assert r["items"] == g["items"], where
        assert r["calls"] == g["calls"], where


def test_every_return_of_every_method_is_a_case(replay):
    rows, _ = replay
    seen = {}
    for r in rows:
        seen.setdefault(r["method"], []).append(r["outcome"])
    assert list(seen) == list(fc.RETURNS)
    for method, outcomes in fc.RETURNS.items():
        assert sorted(set(seen[method])) == sorted(outcomes), method
    # the table's methods are the public ones from search_similar to summarize_database (and delete_images)
    first = inspect.getsourcelines(SimpleReverso.search_similar)[1]
    last = inspect.getsourcelines(SimpleReverso.summarize_database)[1]
    public = [n for n, f in vars(SimpleReverso).items() if inspect.isfunction(f) and not n.startswith("_")
              and first <= inspect.getsourcelines(f)[1] <= last and n not in NOT_REPORTS]
    assert sorted(public + ["delete_images"]) == sorted(fc.RETURNS)


def test_no_return_is_left_unvisited(replay):
    """Every ``return`` statement of the class from ``search_similar`` on ran during the replay, those of NOT_REPORTS apart."""
    _, lines = replay
    src, start = inspect.getsourcelines(SimpleReverso)
    tree = ast.parse(textwrap.dedent("".join(src)))
    first = inspect.getsourcelines(SimpleReverso.search_similar)[1]
    missed = []

    def walk(node, skip):
        for child in ast.iter_child_nodes(node):
            inside = skip or (isinstance(child, ast.FunctionDef) and child.name in NOT_REPORTS)
            if isinstance(child, ast.Return) and not inside:
                a, b = child.lineno + start - 1, child.end_lineno + start - 1
                if a >= first and not lines.intersection(range(a, b + 1)):
                    missed.append(a)
            walk(child, inside)

    walk(tree, False)
    assert missed == [], f"core_system.py: no case reaches the return at line(s) {missed}"
