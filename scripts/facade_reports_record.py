"""Record every report of the facade over the stub store of tests/_facade_cases.py: tests/golden/facade_reports_parent.json.

    python scripts/facade_reports_record.py OUT.json          (no GPU needed)

The table is the reference of tests/test_facade_reports.py (CPU tier): ``SimpleReverso`` must return, case for case, the text
and the items recorded here, after asking the store the questions recorded here.  The committed table was recorded with
core_system.py and store.py of the commit BEFORE the report path was gathered into shared helpers; regenerate it only from a
tree whose reports are known good, never to make a failing test pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reverso_amd  # noqa: E402,F401
import _facade_cases as fc  # noqa: E402


def main(out_path):
    rows = fc.run_table()
    with open(out_path, "w", encoding="utf-8") as f:
        f.write('{"cases": [\n')
        f.write(",\n".join(json.dumps(r, ensure_ascii=False) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
