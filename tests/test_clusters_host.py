"""CPU: what the duplicate clusters must do without a device -- the argument checks of revo_gallery_clusters and
revo_gallery_clusters_read (they return before the device is touched), the binding, the CSR-to-lists step, the `largest_first`
order, and the id mapping of GalleryStore.duplicate_clusters / SimpleReverso.find_duplicate_clusters over a stub gallery."""
import ctypes as C
import threading

import numpy as np
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store
from reverso_amd.core_system import SimpleReverso


def _fake_handle():
    """a zero-filled stand-in for a handle: no result, no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def test_clusters_argument_checks_without_a_device():
    lib = _lib.load()
    nc, nm = C.c_int64(-5), C.c_int64(-6)
    assert lib.revo_gallery_clusters(None, 0.9, C.byref(nc), C.byref(nm), None) == -2 and b"null" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_clusters(fake, 0.9, None, C.byref(nm), None) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_gallery_clusters(fake, 0.9, C.byref(nc), None, None) == -2 and b"null" in lib.revo_last_error()
    assert lib.revo_gallery_clusters(fake, float("nan"), C.byref(nc), C.byref(nm), None) == -2
    assert b"NaN" in lib.revo_last_error()
    assert lib.revo_gallery_clusters(fake, 0.9, C.byref(nc), C.byref(nm), None) == -2 and b"keep_f32" in lib.revo_last_error()
    assert (nc.value, nm.value) == (-5, -6)


def test_clusters_read_argument_checks_without_a_device():
    lib = _lib.load()
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.revo_gallery_clusters_read(None, buf, buf, buf, 0) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    # a handle without a result: every read fails, whatever it asks for
    for args in ((buf, buf, buf), (None, None, None), (buf, None, None), (None, buf, None), (None, None, buf)):
        assert lib.revo_gallery_clusters_read(fake, *args, 0) == -2 and b"no result" in lib.revo_last_error()


def test_binding_and_export():
    for name in ("revo_gallery_clusters", "revo_gallery_clusters_read"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)


def test_csr_to_lists_and_largest_first():
    assert store.split_clusters([0], []) == []
    groups = store.split_clusters([0, 2, 5, 7, 10], [4, 9, 0, 1, 8, 2, 3, 5, 6, 7])
    assert groups == [[4, 9], [0, 1, 8], [2, 3], [5, 6, 7]]
    # size descending; equal sizes by their first row, ascending
    assert store.largest_first(groups) == [[0, 1, 8], [5, 6, 7], [2, 3], [4, 9]]
    assert store.largest_first([]) == []
    assert groups == [[4, 9], [0, 1, 8], [2, 3], [5, 6, 7]]              # (the argument is left as it was)


class _StubGallery:
    """Gallery.clusters of a gallery whose clusters are {1, 4, 5}, {2, 3} and, without a filter, {0, 6}"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def clusters(self, threshold, allow=None):
        self.calls.append((threshold, allow))
        if allow is None:
            labels, off, mem = [0, 1, 2, 2, 1, 1, 0, 7], [0, 2, 5, 7], [0, 6, 1, 4, 5, 2, 3]
        else:
            labels, off, mem = [-1, 1, 2, 2, 1, 1, -1, 7], [0, 3, 5], [1, 4, 5, 2, 3]
        return tuple(torch.tensor(a, dtype=torch.int64) for a in (labels, off, mem))


def _stub_store():
    st = object.__new__(store.GalleryStore)
    st.ids = [f"id-{r}" for r in range(8)]
    st.payloads = [{"filename": f"f{r}.jpg", "image_source": f"/src/f{r}.jpg", "bbox": [r, 0, 1, 1]} for r in range(8)]
    st.gallery = _StubGallery()
    st._allow_bits = lambda flt: ("bits-of", flt)
    return st


def test_duplicate_clusters_map_rows_to_ids():
    st = _stub_store()
    assert st.duplicate_row_clusters(0.9) == [[0, 6], [1, 4, 5], [2, 3]]
    assert st.duplicate_clusters(0.9) == [["id-0", "id-6"], ["id-1", "id-4", "id-5"], ["id-2", "id-3"]]
    assert st.duplicate_clusters(0.75, query_filter="F") == [["id-1", "id-4", "id-5"], ["id-2", "id-3"]]
    assert st.gallery.calls == [(0.9, None), (0.9, None), (0.75, ("bits-of", "F"))]


def test_find_duplicate_clusters_formats_and_orders():
    r = object.__new__(SimpleReverso)            # no device: only the host-side methods are exercised
    r._lock = threading.RLock()
    r.vector_db = None
    r.current_database = None
    text, groups = r.find_duplicate_clusters()
    assert text.startswith("❌") and groups == []
    r.vector_db = _stub_store()
    r.current_database = "stub"
    text, groups = r.find_duplicate_clusters(0.9)
    assert [[m["id"] for m in g] for g in groups] == [["id-1", "id-4", "id-5"], ["id-0", "id-6"], ["id-2", "id-3"]]
    assert all(set(m) == {"filename", "image_source", "bbox", "id"} for g in groups for m in g)
    assert text.startswith("🎯 Found 3 groups") and "1. 3 regions" in text and "f4.jpg  (Source: /src/f4.jpg)" in text
    text, groups = r.find_duplicate_clusters(0.9, largest_first=False)
    assert [[m["id"] for m in g] for g in groups] == [["id-0", "id-6"], ["id-1", "id-4", "id-5"], ["id-2", "id-3"]]

    class _Empty(_StubGallery):
        def clusters(self, threshold, allow=None):
            return tuple(torch.tensor(a, dtype=torch.int64) for a in ([0, 1], [0], []))
    r.vector_db.gallery = _Empty()
    text, groups = r.find_duplicate_clusters(0.99)
    assert groups == [] and "No near-duplicates" in text
