"""CPU: the host side of removing and overwriting gallery rows -- the manifest replay (pure host code), the argument checks
of revo_gallery_remove / revo_gallery_update that return before the device is touched, and the export of the new symbols."""
import ctypes as C
import json

import pytest

import reverso_amd  # noqa: F401
from reverso_amd import _lib, store as st

from _hipcc_report import assert_no_spill


def _fake_handle():
    """a zero-filled stand-in for a handle: size 0, no rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def _shard(i, ids, files_done=()):
    return {"shard": i, "file": f"vectors.{i:05d}.f32.npy", "rows": len(ids), "ids": list(ids),
            "payloads": [{"n": f"{pid}@{i}"} for pid in ids], "files_done": list(files_done)}


# ---- the manifest replay ---------------------------------------------------------------------------------------------------
def test_replay_of_an_old_format_manifest_is_the_shards_in_order():
    recs = [_shard(0, ["a", "b", "c"]), {"shard": 1, "file": None, "rows": 0, "ids": [], "payloads": [], "files_done": ["x"]},
            _shard(2, ["d", "a"])]
    pts = st.replay_manifest(recs)
    assert [p[0] for p in pts] == ["a", "b", "c", "d", "a"]                  # (an id may occur twice: appended, not replaced)
    assert [p[2] for p in pts] == [("vectors.00000.f32.npy", 0), ("vectors.00000.f32.npy", 1), ("vectors.00000.f32.npy", 2),
                                   ("vectors.00002.f32.npy", 0), ("vectors.00002.f32.npy", 1)]
    assert pts[4][1] == {"n": "a@2"} and pts[0][1] == {"n": "a@0"}


def test_replay_append_update_delete_and_reappend_in_mixed_order():
    recs = [
        _shard(0, ["a", "b", "c", "d"]),
        {"op": "update", "file": "vectors.00001.f32.npy", "rows": 2, "ids": ["c", "a"], "payloads": [{"n": "c2"}, {"n": "a2"}]},
        {"op": "delete", "ids": ["b", "nobody"]},
        _shard(3, ["e", "b"]),                                                # b again: a new point at the end
        {"op": "update", "file": None, "rows": 1, "ids": ["d"], "payloads": [{"n": "d-payload-only"}]},
        {"op": "delete", "ids": ["a"]},
        {"op": "update", "file": "vectors.00006.f32.npy", "rows": 1, "ids": ["b"], "payloads": [{"n": "b3"}]},
    ]
    pts = st.replay_manifest(recs)
    assert pts == [
        ("c", {"n": "c2"}, ("vectors.00001.f32.npy", 0)),
        ("d", {"n": "d-payload-only"}, ("vectors.00000.f32.npy", 3)),
        ("e", {"n": "e@3"}, ("vectors.00003.f32.npy", 0)),
        ("b", {"n": "b3"}, ("vectors.00006.f32.npy", 0)),
    ]
    # every prefix replays too (a database is valid after each line)
    assert [p[0] for p in st.replay_manifest(recs[:3])] == ["a", "c", "d"]
    assert st.replay_manifest(recs[:2])[0] == ("a", {"n": "a2"}, ("vectors.00001.f32.npy", 1))
    assert st.replay_manifest([]) == []


def test_replay_rejects_what_it_does_not_understand():
    with pytest.raises(KeyError):
        st.replay_manifest([_shard(0, ["a"]), {"op": "update", "file": None, "rows": 1, "ids": ["zz"], "payloads": [{}]}])
    with pytest.raises(ValueError, match="unknown op"):
        st.replay_manifest([_shard(0, ["a"]), {"op": "merge", "ids": ["a"]}])
    with pytest.raises(ValueError, match="rows"):
        st.replay_manifest([{"shard": 0, "file": "f", "rows": 2, "ids": ["a"], "payloads": [{}]}])


def test_read_manifest_accepts_op_lines_and_a_torn_last_line(tmp_path):
    man = tmp_path / st.MANIFEST
    lines = [{"format": 2, "collection": "c", "dim": 64}, _shard(0, ["a", "b", "c"]), {"complete": True, "rows": 3},
             {"op": "delete", "ids": ["b"]},
             {"op": "update", "file": None, "rows": 1, "ids": ["c"], "payloads": [{"k": 1}]}]
    whole = "".join(json.dumps(x) + "\n" for x in lines)
    man.write_text(whole + '{"op": "delete", "ids": ["a"')                  # the process died while appending
    header, recs, complete, good = st.read_manifest(str(man))
    assert header["dim"] == 64 and len(recs) == 3 and good == len(whole.encode())
    assert complete is False                                                  # changed after the last save
    assert st.replay_manifest(recs) == [("a", {"n": "a@0"}, ("vectors.00000.f32.npy", 0)),
                                        ("c", {"k": 1}, ("vectors.00000.f32.npy", 2))]
    man.write_text(whole + json.dumps({"complete": True, "rows": 2}) + "\n")
    assert st.read_manifest(str(man))[2] is True


# ---- argument checks that return before the device is touched ---------------------------------------------------------------
def test_remove_argument_checks_without_a_device():
    lib = _lib.load()
    bits = C.cast(C.create_string_buffer(64), C.c_void_p)
    n = C.c_int64(-5)
    assert lib.revo_gallery_remove(None, bits, 0, 0, C.byref(n), None) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_remove(fake, bits, 0, 0, None, None) == -2 and b"n_removed" in lib.revo_last_error()
    assert lib.revo_gallery_remove(fake, bits, -1, 0, C.byref(n), None) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_remove(fake, None, 7, 0, C.byref(n), None) == -2 and b"remove_bits" in lib.revo_last_error()
    assert lib.revo_gallery_remove(fake, bits, 7, 0, C.byref(n), None) == -2 and b"revo_gallery_size" in lib.revo_last_error()
    assert n.value == -5                                                      # outputs untouched
    # an empty gallery: nothing to remove, no device needed
    assert lib.revo_gallery_remove(fake, bits, 0, 0, C.byref(n), None) == 0 and n.value == 0


def test_update_argument_checks_without_a_device():
    lib = _lib.load()
    idx = (C.c_int64 * 3)(0, 1, 2)
    vec = C.cast(C.create_string_buffer(3 * 64 * 4), C.c_void_p)
    pidx = C.cast(idx, C.c_void_p)
    assert lib.revo_gallery_update(None, pidx, vec, 3, 1, 0, None) == -2 and b"null handle" in lib.revo_last_error()
    fake = _fake_handle()
    assert lib.revo_gallery_update(fake, pidx, vec, -1, 1, 0, None) == -2 and b"negative" in lib.revo_last_error()
    assert lib.revo_gallery_update(fake, None, vec, 3, 1, 0, None) == -2 and b"row_idx" in lib.revo_last_error()
    assert lib.revo_gallery_update(fake, pidx, None, 3, 1, 0, None) == -2 and b"vecs" in lib.revo_last_error()
    # size 0: every index is outside the gallery
    assert lib.revo_gallery_update(fake, pidx, vec, 3, 1, 0, None) == -2 and b"outside the gallery" in lib.revo_last_error()
    assert lib.revo_gallery_update(fake, None, None, 0, 1, 0, None) == 0      # n = 0: nothing to do


def test_binding_and_export():
    for name in ("revo_gallery_remove", "revo_gallery_update"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)
    assert "revo_debug_set_remove_chunk" in _lib.EXPERIMENT_SIGNATURES
    assert hasattr(_lib.load_exp(), "revo_debug_set_remove_chunk")
    assert not hasattr(_lib.load(), "revo_debug_set_remove_chunk")


def test_remove_kernels_do_not_spill():
    """the count and gather kernels of gallery_edit.hip: no VGPR spills and no scratch (the gather is HBM-bound row movement)"""
    assert_no_spill("gallery_edit.hip", "remove_", 2)
