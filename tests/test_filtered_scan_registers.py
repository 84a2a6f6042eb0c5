"""CPU: the filtered forms of the 256 x 256 scan (topk_scan256_kernel<KSEL, ROWS, MARGIN, FILTER = true>, every ksel / rows /
margin form that is built) from hipcc's resource report: at or below the spill numbers pinned for the plain forms
(tests/test_kernel_register_budget.py), and no scratch traffic inside the tile loop beyond what the plain forms have.  The
report and the listing are the ones the plain forms' tests read (tests/_hipcc_report.py compiles topk256.hip once for each)."""
import re

import pytest

from _hipcc_report import listing as _listing, scratch_in_loops as _scratch_in_loops, usage as _usage

# (ksel, rows, margin) -> spilled VGPRs allowed: the plain forms' pinned numbers (the 256-row margin form is not built
# filtered: filtered searches of more than 128 queries scan without the margin)
PINNED = {(32, 0, 0): 1, (32, 64, 0): 0, (32, 128, 0): 0, (32, 192, 0): 5,
          (64, 0, 0): 1, (64, 64, 0): 0, (64, 128, 0): 0, (64, 192, 0): 2,
          (64, 64, 1): 0, (64, 128, 1): 2}
# the plain forms: the eight without the margin, and the margin with 64 candidates at 64, 128 and 256 rows
PLAIN = {(ksel, rows, 0) for ksel in (32, 64) for rows in (0, 64, 128, 192)} | {(64, 0, 1), (64, 64, 1), (64, 128, 1)}


@pytest.fixture(scope="module")
def usage():
    return _usage("topk256.hip")


def test_filtered_scan_forms_spill_no_more_than_the_plain_forms(usage):
    forms = {0: set(), 1: set()}                   # FILTER -> the (ksel, rows, margin) that are instantiated
    for name, u in usage.items():
        m = re.search(r"19topk_scan256_kernelILi(\d+)ELi(\d+)ELb(\d)ELb(\d)E", name)
        if not m:
            continue
        form = tuple(int(x) for x in m.groups()[:3])
        forms[int(m.group(4))].add(form)
        if int(m.group(4)):
            assert form in PINNED, form
            assert u["VGPRs"] <= 256 and u["VGPRs Spill"] <= PINNED[form], (form, u)
    # exactly the 11 plain and the 10 filtered forms the launcher selects, and no other symbol that carries the scan's name
    assert forms[1] == set(PINNED), (sorted(set(PINNED) - forms[1]), sorted(forms[1] - set(PINNED)))
    assert forms[0] == PLAIN and len(PLAIN) == 11, (sorted(PLAIN - forms[0]), sorted(forms[0] - PLAIN))
    assert len([k for k in usage if "topk_scan256" in k]) == 21, [k for k in usage if "topk_scan256" in k]
    # ... so none of: a filtered 256-row margin form, a 192-row margin form, a 32-candidate margin form
    assert (64, 0, 1) not in forms[1]
    # the collect pass: <ROWS, FILTER>, three row forms each
    collect = {tuple(int(x) for x in m.groups()) for m in (re.search(r"22topk_collect256_kernelILi(\d+)ELb(\d)E", k) for k in usage) if m}
    assert collect == {(rows, flt) for rows in (0, 64, 128) for flt in (0, 1)}, sorted(collect)
    assert len([k for k in usage if "topk_collect256" in k]) == 6
    for flt in (0, 1):
        assert not [f for f in forms[flt] if f[2] and f[1] == 192], forms[flt]
        assert not [f for f in forms[flt] if f[2] and f[0] == 32], forms[flt]


def test_filtered_scans_keep_scratch_out_of_the_hot_loops():
    seen = 0
    for m, hot in _scratch_in_loops(_listing("topk256.hip"),
                                    r"_ZN4revo19topk_scan256_kernelILi(\d+)ELi(\d+)ELb(\d)ELb1EEEvNS_11Scan256ArgsE"):
        seen += 1
        assert not [h for h in hot if h[0] >= 2], (m.group(1), hot)
        allowed = 1 if (int(m.group(3)) == 192 or int(m.group(4))) else 0
        if int(m.group(3)) == 192 and int(m.group(2)) == 32:
            allowed = 12
        assert len(hot) <= allowed, (m.group(1), hot)
    assert seen == 10, seen
