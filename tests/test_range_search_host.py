"""CPU: the range search's argument checks (they return before the device is touched), its binding and export by both
libraries, and the register allocation of its kernels (range.hip, from hipcc's own resource report: hipcc cross-compiles for
gfx950 without a GPU)."""
import ctypes as C
import reverso_amd  # noqa: F401
from reverso_amd import _lib

from _hipcc_report import assert_no_spill


def _fake_handle():
    """a zero-filled stand-in for a handle: no result, no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_range_argument_checks_without_a_device():
    lib = _lib.load()
    q = C.cast(C.create_string_buffer(4 * 64), C.c_void_p)
    n = C.c_int64(-5)
    assert lib.revo_search_range(None, q, 1, 0.9, 0, C.byref(n), None) == -2 and b"null" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_search_range(fake, q, 1, 0.9, 0, None, None) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_search_range(fake, None, 1, 0.9, 0, C.byref(n), None) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_search_range(fake, q, -1, 0.9, 0, C.byref(n), None) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_search_range(fake, q, 1, float("nan"), 0, C.byref(n), None) == -2 and b"NaN" in lib.revo_last_error()
    assert lib.revo_search_range(fake, q, 1, 0.9, 0, C.byref(n), None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert n.value == -5


def test_range_read_argument_checks_without_a_device():
    lib = _lib.load()
    idx = C.cast(C.create_string_buffer(8 * 8), C.c_void_p)
    sc = C.cast(C.create_string_buffer(4 * 8), C.c_void_p)
    off = C.cast(C.create_string_buffer(8 * 8), C.c_void_p)
    assert lib.revo_search_range_read(None, off, 0, 1, idx, sc, 0) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_search_range_read(fake, off, -1, 1, idx, sc, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_search_range_read(fake, off, 0, -1, idx, sc, 0) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_search_range_read(fake, off, 0, 1, None, sc, 0) == -2 and b"null argument" in lib.revo_last_error()
    assert lib.revo_search_range_read(fake, off, 0, 1, idx, None, 0) == -2 and b"null argument" in lib.revo_last_error()
    # a handle without a result: every read fails, offsets only or not
    assert lib.revo_search_range_read(fake, off, 0, 1, idx, sc, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_search_range_read(fake, off, 0, 0, None, None, 0) == -2 and b"no result" in lib.revo_last_error()
    assert lib.revo_search_range_read(fake, None, 0, 0, None, None, 0) == -2 and b"no result" in lib.revo_last_error()


def test_binding_and_export():
    for name in ("revo_search_range", "revo_search_range_read"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)


def test_range_kernels_do_not_spill():
    """Every kernel of range.hip: no VGPR spills and no scratch (the candidate pass runs the 256 x 256 main loop at up to 256
    VGPRs in five forms; a spill inside its tile loop would wait for the next tile's operand DMA)."""
    assert_no_spill("range.hip", "range_", 7)            # join (64, 128, 192, 256 rows; 256 with default-policy DMA), rescore, emit
