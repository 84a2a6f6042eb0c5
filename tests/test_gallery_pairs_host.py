"""CPU: the near-duplicate pair search's argument checks (they return before the device is touched), the host-side grouping of
pairs into near-duplicate groups (store.connected_groups), and the register allocation of its kernels (pairs.hip, from
hipcc's own resource report: hipcc cross-compiles for gfx950 without a GPU)."""
import ctypes as C
import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store

from _hipcc_report import assert_no_spill


def _fake_handle():
    """a zero-filled stand-in for a handle: no result, no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_pairs_argument_checks_without_a_device():
    lib = _lib.load()
    n = C.c_int64(-5)
    assert lib.revo_gallery_pairs(None, 0.9, C.byref(n), None) == -2 and b"null" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_pairs(fake, 0.9, None, None) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_gallery_pairs(fake, float("nan"), C.byref(n), None) == -2 and b"NaN" in lib.revo_last_error()
    assert lib.revo_gallery_pairs(fake, 0.9, C.byref(n), None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert n.value == -5


def test_pairs_read_argument_checks_without_a_device():
    lib = _lib.load()
    pairs = C.create_string_buffer(16 * 8)
    scores = C.create_string_buffer(4 * 8)
    pp, sp = C.cast(pairs, C.c_void_p), C.cast(scores, C.c_void_p)
    assert lib.revo_gallery_pairs_read(None, 0, 1, pp, sp, 0) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_pairs_read(fake, -1, 1, pp, sp, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_pairs_read(fake, 0, -1, pp, sp, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_pairs_read(fake, 0, 1, None, sp, 0) == -2 and b"null argument" in lib.revo_last_error()
    assert lib.revo_gallery_pairs_read(fake, 0, 1, pp, None, 0) == -2 and b"null argument" in lib.revo_last_error()
    # a handle without a result: every read fails, past the (absent) result or not
    assert lib.revo_gallery_pairs_read(fake, 0, 1, pp, sp, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_gallery_pairs_read(fake, 0, 0, None, None, 0) == -2 and b"no result" in lib.revo_last_error()


def test_binding_and_export():
    for name in ("revo_gallery_pairs", "revo_gallery_pairs_read"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)


def _components_reference(pairs, n):
    """components of size >= 2 by breadth-first search"""
    adj = {r: set() for r in range(n)}
    for a, b in pairs:
        adj[a].add(b)
        adj[b].add(a)
    seen, out = set(), []
    for r in range(n):
        if r in seen or not adj[r]:
            continue
        comp, todo = set(), [r]
        while todo:
            x = todo.pop()
            if x in comp:
                continue
            comp.add(x)
            todo.extend(adj[x] - comp)
        seen |= comp
        out.append(sorted(comp))
    return sorted(out)


def test_connected_groups_on_synthetic_pair_lists():
    assert store.connected_groups(np.zeros((0, 2), np.int64), 10) == []
    assert store.connected_groups([[3, 7]], 10) == [[3, 7]]
    # a chain joined from its far end, and two groups whose first rows interleave
    assert store.connected_groups([[5, 9], [1, 9], [0, 4], [2, 6], [4, 8], [6, 7]], 10) == [[0, 4, 8], [1, 5, 9], [2, 6, 7]]
    rng = np.random.default_rng(0)
    for n, m in ((20, 5), (200, 150), (1000, 900), (500, 2000)):
        a = rng.integers(0, n, m)
        b = rng.integers(0, n, m)
        keep = a != b
        pairs = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)[keep]
        got = store.connected_groups(pairs, n)
        assert got == _components_reference(pairs.tolist(), n)
        assert [g[0] for g in got] == sorted(g[0] for g in got)          # groups ordered by their first row
        assert all(g == sorted(g) and len(g) >= 2 for g in got)


def test_pair_kernels_do_not_spill():
    """Every kernel of pairs.hip: no VGPR spills and no scratch (the join runs the 256 x 256 main loop at up to 256 VGPRs;
    a spill inside its tile loop would wait for the next tile's operand DMA)."""
    assert_no_spill("pairs.hip", "pairs_", 3)            # join, rescore, emit


def test_sort_kernels_do_not_spill():
    """Every kernel of radix_sort.hip (the sort step of the pairs, range and recommend searches, and the range offsets): no
    VGPR spills and no scratch."""
    assert_no_spill("radix_sort.hip", "_kernel", 4)       # radix hist / scatter, prefix sum (u32 exclusive, u64 inclusive)
