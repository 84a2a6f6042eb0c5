"""CPU: the host side of the grouped search (revo_search_groups) -- Qdrant's group_by as dense ids over the payload
index, argument checks that return before the device is touched, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reverso_amd  # noqa: F401
from reverso_amd import _lib, filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"]


# ---- PayloadIndex.group_ids ---------------------------------------------------------------------------------------------
def test_group_ids_str_and_int_values():
    pl = [{"img": "a"}, {"img": "b"}, {"img": "a"}, {"img": 7}, {"img": "7"}, {"img": 7}, {"other": 1}, {}]
    ids, values = filters.PayloadIndex().sync(list(range(len(pl))), pl).group_ids("img")
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 0, 2, 3, 2, -1, -1]
    assert values == ["a", "b", 7, "7"]
    assert type(values[2]) is int


def test_group_ids_other_scalars_are_in_no_group():
    pl = [{"k": True}, {"k": False}, {"k": 1.5}, {"k": None}, {"k": {"x": 1}}, {"k": 2}, {"k": np.int64(2)}, "not a dict"]
    ids, values = filters.PayloadIndex().sync(list(range(len(pl))), pl).group_ids("k")
    assert ids.tolist() == [-1, -1, -1, -1, -1, 0, 0, -1]
    assert values == [2]
    ids, values = filters.PayloadIndex().sync(list(range(len(pl))), pl).group_ids("missing")
    assert ids.tolist() == [-1] * len(pl) and values == []


def test_group_ids_refuses_list_values():
    pl = [{"tags": "a"}, {"tags": ["a", "b"]}]
    with pytest.raises(ValueError, match="group_by over a list-valued key is not supported"):
        filters.PayloadIndex().sync([0, 1], pl).group_ids("tags")
    pl = [{"tags": "a"}, {"tags": []}]
    with pytest.raises(ValueError, match="list-valued"):
        filters.PayloadIndex().sync([0, 1], pl).group_ids("tags")


def test_group_ids_follow_appends():
    ids_, pl = [0, 1], [{"img": "x"}, {"img": "y"}]
    ix = filters.PayloadIndex().sync(ids_, pl)
    assert ix.group_ids("img")[0].tolist() == [0, 1]
    ids_ += [2, 3, 4]
    pl += [{"img": "y"}, {"img": "z"}, {"img": False}]
    ids, values = ix.sync(ids_, pl).group_ids("img")
    assert ids.tolist() == [0, 1, 1, 2, -1] and values == ["x", "y", "z"]
    # a list appended later is refused from then on
    ids_.append(5)
    pl.append({"img": ["x"]})
    with pytest.raises(ValueError):
        ix.sync(ids_, pl).group_ids("img")


# ---- argument checks (no device) ----------------------------------------------------------------------------------------
def _groups_call(lib, h, limit, group_size, Q=1):
    f = C.c_void_p(8)                                        # never dereferenced: every call below fails its checks first
    return lib.revo_search_groups(h, f, Q, limit, group_size, 0, 0.0, 0, f, f, f, f, f, None)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    assert _groups_call(lib, None, 5, 1) == -2
    assert b"null handle" in lib.revo_last_error()
    for limit, gs in ((10, 6), (0, 1), (1, 0), (51, 1), (1, 51), (7, 8)):
        assert _groups_call(lib, None, limit, gs) == -2, (limit, gs)
        assert b"limit * group_size <= 50" in lib.revo_last_error(), (limit, gs)
    assert _groups_call(lib, None, 5, 1, Q=-1) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_search_set_groups(None, None, 0, 0, None) == -2 and b"null handle" in lib.revo_last_error()


def test_binding_declares_the_grouped_entry_points():
    for n in ("revo_search_set_groups", "revo_search_groups"):
        assert n in _lib.SIGNATURES
        assert hasattr(_lib.load(), n)


# ---- register budget ------------------------------------------------------------------------------------------------------
GROUP_KERNELS = ("topk_group_select_kernel", "topk_group_final_kernel", "topk_group_bruteforce_kernel",
                 "topk_group_bruteforce_filtered_kernel")


def test_grouped_kernels_do_not_spill():
    out = subprocess.run([HIPCC, *FLAGS, "-c", "topk_exact.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    cur, d = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        for key, pat in (("VGPRs", r" VGPRs: (\d+)"), ("VGPRs Spill", r"VGPRs Spill: (\d+)"),
                         ("SGPRs Spill", r"SGPRs Spill: (\d+)"), ("Scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                d[cur][key] = int(m.group(1))
    seen = set()
    for name, u in d.items():
        for k in GROUP_KERNELS:
            if re.search(rf"\d{k}E", name):
                assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["Scratch"] == 0, (k, u)
                # (the brute-force forms keep the plain forms' occupancy: 16 waves of 1024 threads per workgroup)
                assert u["VGPRs"] <= 128, (k, u)
                seen.add(k)
    assert seen == set(GROUP_KERNELS), sorted(set(GROUP_KERNELS) - seen)
