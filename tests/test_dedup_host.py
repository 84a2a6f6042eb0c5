"""CPU: what the deduplicating append must do without a device -- the refusals of revo_gallery_append_unique (they return before
the device is touched, with nothing written), its binding and export by both libraries, the register allocation of dedup.hip's
kernels (hipcc's own resource report: hipcc cross-compiles for gfx950 without a GPU), the tile-pair walk of its join as host
code (csrc/dedup_plan.h, `make dedup_plan_check`), the numpy statement of the greedy selection on hand-made score matrices,
and the argument handling of GalleryStore.upsert(skip_duplicates=...) and SimpleReverso(skip_duplicates=...)."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store
from reverso_amd.core_system import SimpleReverso

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill  # noqa: E402
import _dedup_checks as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")


def _fake_handle(capacity=0, keep_f32=0):
    """a stand-in for a handle, zero-filled but for the fields the checks read: D, device, keep_f32 (three ints), then
    capacity and size (two int64)"""
    buf = C.create_string_buffer(1 << 16)
    C.memmove(buf, (C.c_int32 * 3)(64, 0, keep_f32), 12)
    C.memmove(C.byref(buf, 16), (C.c_int64 * 2)(capacity, 0), 16)
    return buf


def test_refusals_without_a_device():
    lib = _lib.load()
    vecs = C.cast(C.create_string_buffer(4 * 64 * 4), C.c_void_p)
    rows_b = C.create_string_buffer(b"\x5a" * 64, 64)
    scores_b = C.create_string_buffer(b"\x5a" * 32, 32)
    rows, scores = C.cast(rows_b, C.c_void_p), C.cast(scores_b, C.c_void_p)
    kept = C.c_int64(-5)
    fake = _fake_handle(capacity=3, keep_f32=1)
    g0 = C.cast(fake, C.c_void_p)

    def call(g=g0, v=vecs, n=2, t=0.9, r=rows, s=scores, k=C.byref(kept)):
        return lib.revo_gallery_append_unique(g, v, n, 1, 0, t, r, s, 0, k, None)

    assert call(g=None) == -2 and b"null" in lib.revo_last_error()
    assert call(v=None) == -2 and b"null" in lib.revo_last_error()
    assert call(r=None) == -2 and b"null" in lib.revo_last_error()
    assert call(s=None) == -2 and b"null" in lib.revo_last_error()
    assert call(k=None) == -2 and b"null" in lib.revo_last_error()
    assert call(n=-1) == -2 and b"negative" in lib.revo_last_error()
    assert call(n=16385) == -2 and b"16384" in lib.revo_last_error()
    assert call(t=float("nan")) == -2 and b"NaN" in lib.revo_last_error()
    assert call(n=4) == -2 and b"capacity" in lib.revo_last_error()             # room for 3 rows
    nof32 = C.cast(_fake_handle(capacity=3, keep_f32=0), C.c_void_p)
    assert call(g=nof32) == -2 and b"keep_f32" in lib.revo_last_error()
    assert call(g=nof32, v=None, n=0) == -2 and b"keep_f32" in lib.revo_last_error()
    assert kept.value == -5 and rows_b.raw == b"\x5a" * 64 and scores_b.raw == b"\x5a" * 32
    assert C.cast(C.byref(fake, 24), C.POINTER(C.c_int64))[0] == 0              # the size
    # n = 0 on a handle with fp32 rows: nothing to do, no device needed (vecs may be null)
    assert call(v=None, n=0) == 0 and kept.value == 0
    assert rows_b.raw == b"\x5a" * 64 and scores_b.raw == b"\x5a" * 32


def test_binding_and_export():
    name = "revo_gallery_append_unique"
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)
    with open(os.path.join(ROOT, "include", "revo.h")) as f:
        header = f.read()
    m = re.search(r"int32_t revo_gallery_append_unique\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == 11


def test_dedup_kernels_do_not_spill():
    """Every kernel of dedup.hip: no VGPR spills and no scratch (the join holds the 256 x 256 tile's 128 accumulators per lane
    through its epilogue, as the clusters join does)."""
    assert_no_spill("dedup.hip", "dedup_", 5)              # join, rescore, select, scores, bits


def test_tile_pair_walk_on_the_host():
    subprocess.run(["make", "-C", CSRC, "dedup_plan_check"], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "dedup_plan_check")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for N0 in (0, 255, 256, 257):
        for n in (1, 256, 257):
            assert f"N0 {N0} n {n}: " in r.stdout


def _sym(n, entries):
    s = np.zeros((n, n), dtype=np.float32)
    for (i, j), v in entries.items():
        s[i, j] = s[j, i] = np.float32(v)
    np.fill_diagonal(s, np.nan)                            # never read
    return s


def test_greedy_on_hand_made_matrices():
    t = np.float32(0.9)
    # a chain a - b - c: s(a, b), s(b, c) >= t, s(a, c) < t.  b is dropped, so it does not suppress c: c is kept
    S = _sym(3, {(0, 1): 0.95, (1, 2): 0.95, (0, 2): 0.5})
    kept, rep, score = dc.greedy_dense(S, 0, t)
    assert kept.tolist() == [True, False, True] and rep.tolist() == [-1, 0, -1]
    assert score[1] == np.float32(0.95) and score[0] == -np.inf and score[2] == -np.inf
    assert dc.final_rows(0, kept, rep).tolist() == [0, 0, 1]
    assert dc.teeth(S, 0, t, kept, rep) == (1, 0)
    # the same chain with a as a gallery row: b's representative is the gallery row, c becomes row N
    kept, rep, _ = dc.greedy_dense(S, 1, t)
    assert kept.tolist() == [False, True] and rep.tolist() == [0, -1] and dc.final_rows(1, kept, rep).tolist() == [0, 1]
    # first seen wins: the best-scoring neighbour of row 3 is row 2, its representative the lowest one, row 0 -- and a
    # gallery row comes before every batch row, whatever the scores
    S = _sym(4, {(0, 3): 0.91, (2, 3): 0.99, (0, 2): 0.1, (1, 3): 0.2})
    kept, rep, score = dc.greedy_dense(S, 0, t)
    assert kept.tolist() == [True, True, True, False] and rep[3] == 0 and score[3] == np.float32(0.91)
    assert dc.teeth(S, 0, t, kept, rep) == (0, 1)
    kept, rep, score = dc.greedy_dense(S, 2, t)                              # rows 0, 1: the gallery
    assert kept.tolist() == [True, False] and rep.tolist() == [-1, 0] and dc.final_rows(2, kept, rep).tolist() == [2, 0]
    # exact hits of t count; the next fp32 below does not
    below = np.nextafter(t, np.float32(0))
    S = _sym(3, {(0, 1): t, (0, 2): below, (1, 2): below})
    kept, rep, score = dc.greedy_dense(S, 0, t)
    assert kept.tolist() == [True, False, True] and score[1] == t
    # a dropped row's representative is a KEPT row even when a dropped one in between scores higher
    S = _sym(4, {(0, 1): 0.95, (1, 3): 0.99, (0, 3): 0.92, (2, 3): 0.1})
    kept, rep, _ = dc.greedy_dense(S, 0, t)
    assert kept.tolist() == [True, False, True, False] and rep.tolist() == [-1, 0, -1, 0]
    assert dc.final_rows(0, kept, rep).tolist() == [0, 0, 1, 0]
    # the edge-list form gives the same
    pairs = np.array([[0, 1], [0, 3], [1, 3]])
    k2, r2, s2 = dc.greedy_pairs(0, 4, pairs, np.array([0.95, 0.92, 0.99], dtype=np.float32))
    assert k2.tolist() == kept.tolist() and r2.tolist() == rep.tolist() and s2[3] == np.float32(0.92)
    # nothing at all
    kept, rep, _ = dc.greedy_dense(np.zeros((2, 2), dtype=np.float32), 2, t)
    assert kept.shape == (0,) and dc.final_rows(2, kept, rep).shape == (0,)


class _StubGallery:
    """Gallery.add_unique of a gallery of 2 rows: batch rows 0 and 2 are kept, 1 is a copy of gallery row 1, 3 of batch row 0"""
    device = torch.device("cpu")
    capacity = 100

    def __init__(self):
        self.calls = []

    def add_unique(self, vectors, threshold, normalize=True):
        self.calls.append((tuple(vectors.shape), threshold))
        return (torch.tensor([2, 1, 3, 2]), torch.tensor([-np.inf, 0.97, -np.inf, 1.0], dtype=torch.float32),
                torch.tensor([True, False, True, False]))

    def add(self, vectors, normalize=True):
        self.calls.append("add")


def _stub_store():
    st = object.__new__(store.GalleryStore)
    st.ids, st.payloads = ["g0", "g1"], [{"k": 0}, {"k": 1}]
    st.gallery = _StubGallery()
    st.dim, st._files_pending, st.complete = 8, [], True
    return st


def test_store_upsert_argument_handling():
    st = _stub_store()
    v = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="replace_existing"):
        st.upsert(v, list("abcd"), [{}] * 4, replace_existing=True, skip_duplicates=0.9)
    with pytest.raises(ValueError, match="NaN"):
        st.upsert(v, list("abcd"), [{}] * 4, skip_duplicates=float("nan"))
    assert st.gallery.calls == [] and st.ids == ["g0", "g1"]
    rep = st.upsert(v, list("abcd"), [{"k": c} for c in "abcd"], files=["f.jpg"], skip_duplicates=0.9)
    assert st.gallery.calls == [((4, 8), 0.9)]
    assert rep["kept"] == 2 and st.ids == ["g0", "g1", "a", "c"] and [p["k"] for p in st.payloads] == [0, 1, "a", "c"]
    assert [(a, b) for a, b, _ in rep["dropped"]] == [("b", "g1"), ("d", "a")]
    assert rep["dropped"][0][2] == pytest.approx(0.97) and rep["dropped"][1][2] == 1.0
    assert st._files_pending == ["f.jpg"] and st.complete is False
    # without the argument: the plain append, and no report
    assert st.upsert(v[:1], ["e"], [{}]) is None and st.gallery.calls[-1] == "add" and st.ids[-1] == "e"
    # an empty call still records its files
    rep = st.upsert(torch.zeros((0, 8)), [], [], files=["g.jpg"], skip_duplicates=0.9)
    assert rep == {"kept": 0, "dropped": []} and st._files_pending == ["f.jpg", "g.jpg"]


def test_facade_argument_handling(tmp_path):
    r = object.__new__(SimpleReverso)                      # no device: only the host-side checks are exercised
    r._building_lock, r._building_names = threading.Lock(), set()
    r.skip_duplicates, r.region_mode, r.db_root = 0.95, "global", str(tmp_path / "db")
    seen = []
    out = r.create_database(str(tmp_path), "x", use_direct_pe=False, progress_callback=lambda m, v=None: seen.append(m))
    assert out.startswith("❌ skip_duplicates") and seen == [out] and not os.path.exists(r.db_root)
    assert r._building_names == set()
    import inspect
    sig = inspect.signature(SimpleReverso.__init__).parameters
    assert sig["skip_duplicates"].default is None
    assert list(inspect.signature(SimpleReverso.create_database).parameters) == [
        "self", "folder_path", "database_name", "text_prompt", "use_direct_pe", "progress_callback", "resume_from_checkpoint",
        "include_subfolders"]                              # the reference's signature stays


def test_build_info_carries_the_threshold():
    class _Cfg:
        name, use_ls = "m", False

    class _Model:
        cfg = _Cfg()
    r = object.__new__(SimpleReverso)
    r.pe_model, r.region_mode, r.skip_duplicates = _Model(), "global", None
    a = r._build_info("/f", True, False)
    r.skip_duplicates = 0.95
    b = r._build_info("/f", True, False)
    assert a["skip_duplicates"] is None and b["skip_duplicates"] == 0.95
    old_header = {k: v for k, v in a.items() if k != "skip_duplicates"}          # a manifest written before the argument existed
    assert [k for k in a if old_header.get(k) != a[k]] == []                     # ... equals None: the resume goes on
    assert [k for k in b if old_header.get(k) != b[k]] == ["skip_duplicates"]    # ... and a threshold starts fresh
