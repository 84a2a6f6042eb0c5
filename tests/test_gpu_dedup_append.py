"""The deduplicating append (revo_gallery_append_unique, include/revo.h DEDUP; Gallery.add_unique, GalleryStore.upsert(
skip_duplicates=t), SimpleReverso(skip_duplicates=t)).  Two oracles, neither the code under test: (1) the edges and score bits
of revo_gallery_pairs on a gallery that received every row by a plain add, fed to the numpy greedy of _dedup_checks.py -- rows,
scores and kept flags must be equal bit for bit; (2) the same greedy over fp64 scores of the master rows, under the condition
that no pair lies within the fp32 chain's band of the threshold.  After the call the gallery must answer every search, byte
for byte, like a fresh gallery that received only the kept vectors."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dedup_checks as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = [(1500, 700, 256), (300, 1000, 64), (0, 600, 128), (2000, 300, 1024), (515, 1, 320), (257, 255, 64)]
SEEDS = {s: 11 + i for i, s in enumerate(SHAPES)}
THRESHOLDS = [0.8, 0.9, 0.95]
# where the join's walk over the tile pairs (csrc/tile_walk.h, dedup_plan.h) can go wrong, (old rows, batch rows, D): N0 + n = 1,
# 255, 256, 257 and 513 rows (one tile; the diagonal tile only; a partial last tile; the next column), N0 = 100 and 300 inside a
# tile (it straddles old and new rows), and 23 row tiles = 276 tile pairs, more than the one workgroup per CU
WALK_SHAPES = [(0, 1, 64), (0, 255, 64), (0, 256, 64), (100, 157, 64), (300, 213, 64), (100, 5789, 64)]
SEEDS.update({s: 31 + i for i, s in enumerate(WALK_SHAPES)})


def _delta(D):
    """the fp32 chain's band: 3e-7 at D = 1024, scaled with D, never below that (test_gpu_gallery_pairs.py)"""
    return 3e-7 * max(1.0, D / 1024)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gallery(x, capacity, keep_f32=True):
    G = engine.Gallery(x.shape[1], max(1, capacity), device=0, keep_f32=keep_f32)
    if x.shape[0]:
        G.add(torch.tensor(x).to(DEV))
    return G


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    N, n, D = shape
    g, b = dc.video_like(N, n, D, SEEDS[shape])
    g.setflags(write=False)
    b.setflags(write=False)
    return g, b


@functools.lru_cache(maxsize=None)
def _reference(shape, t):
    """computed once per case, shared, left unchanged: the master rows of all N + n rows (plain add), the pairs oracle
    (kept, rep, rep_score, rows) and the pairs at t among the first N rows"""
    N, n, D = shape
    g, b = _inputs(shape)
    H = _gallery(np.concatenate([g, b]), N + n)
    master = H.read().cpu().numpy()
    pairs, scores = H.pairs(t)
    pairs, scores = pairs.cpu().numpy(), scores.cpu().numpy()
    H.close()
    kept, rep, rep_score = dc.greedy_pairs(N, n, pairs, scores)
    old = pairs[:, 1] < N
    return dict(master=master, kept=kept, rep=rep, score=rep_score.astype(np.float32), rows=dc.final_rows(N, kept, rep),
                old_pairs=pairs[old], old_scores=scores[old])


def _expect(got, ref):
    rows, scores, kept = (a.cpu().numpy() for a in got)
    assert np.array_equal(kept, ref["kept"])
    assert np.array_equal(rows, ref["rows"])
    assert np.array_equal(scores.view(np.uint32), ref["score"].view(np.uint32))


# ---- 1, 2, 4: the pairs oracle bit for bit, the fp64 oracle, the pairs invariant -------------------------------------------
@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-n%d-D%d" % s)
def test_matches_the_pairs_oracle_and_fp64(shape, t):
    N, n, D = shape
    g, b = _inputs(shape)
    ref = _reference(shape, t)
    G = _gallery(g, N + n)
    got = G.add_unique(torch.tensor(b).to(DEV), t)
    st = G.search_stats()
    _expect(got, ref)
    n_kept = int(ref["kept"].sum())
    assert len(G) == N + n_kept
    assert st["join_passes"] >= 1 and all(st[k] == 0 for k in st if k not in ("join_passes", "collected_rows"))
    # the gallery: the old rows and the kept rows' master bits, in order
    want = np.concatenate([ref["master"][:N], ref["master"][N:][ref["kept"]]])
    assert G.read().cpu().numpy().tobytes() == want.tobytes()
    # 4. pairs(t) afterwards = pairs(t) of the old rows: no pair with an end >= N
    p, s = G.pairs(t)
    assert np.array_equal(p.cpu().numpy(), ref["old_pairs"])
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref["old_scores"].view(np.uint32))
    assert p.numel() == 0 or int(p.max()) < N
    G.close()
    # two calls give identical bytes
    G2 = _gallery(g, N + n)
    again = G2.add_unique(torch.tensor(b).to(DEV), t)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(got, again))
    assert G2.read().cpu().numpy().tobytes() == want.tobytes()
    G2.close()
    # 2. fp64 scores of the master rows, independent of the library
    X = ref["master"].astype(np.float64)
    S = X @ X.T
    t32 = float(np.float32(t))
    iu = np.triu_indices(N + n, 1)
    gap = float(np.abs(S[iu] - t32).min())
    print(f"shape {shape} t {t}: min |s - t| = {gap:.3g}, band {_delta(D):.3g}")
    assert gap > _delta(D), "a pair lies inside the fp32 band of the threshold: choose another seed or threshold"
    kept, rep, _ = dc.greedy_dense(S, N, t32)
    naive, notbest = dc.teeth(S, N, t32, kept, rep)
    print(f"kept {int(kept.sum())} of {n}; kept despite an earlier dropped neighbour {naive}; representative not the best {notbest}")
    if shape in ((1500, 700, 256), (300, 1000, 64)):
        assert naive >= 5
    if shape == (300, 1000, 64):
        assert notbest >= 1
    assert np.array_equal(kept, ref["kept"]) and np.array_equal(rep, ref["rep"])
    d = ~kept
    assert np.abs(S[N + np.flatnonzero(d), rep[d]] - ref["score"][d]).max(initial=0.0) <= _delta(D)


@pytest.mark.parametrize("shape", WALK_SHAPES, ids=lambda s: "N%d-n%d-D%d" % s)
def test_matches_the_pairs_oracle_where_the_tile_walk_turns(shape):
    N, n, D = shape
    t = 0.9
    g, b = _inputs(shape)
    ref = _reference(shape, t)
    G = _gallery(g, N + n)
    got = G.add_unique(torch.tensor(b).to(DEV), t)
    _expect(got, ref)
    assert len(G) == N + int(ref["kept"].sum())
    if n > 1:
        assert 0 < int(ref["kept"].sum()) < n                             # some rows are dropped and some are kept
    want = np.concatenate([ref["master"][:N], ref["master"][N:][ref["kept"]]])
    assert G.read().cpu().numpy().tobytes() == want.tobytes()
    p, s = G.pairs(t)                                                     # no pair with an end among the new rows is left
    assert np.array_equal(p.cpu().numpy(), ref["old_pairs"])
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref["old_scores"].view(np.uint32))
    G.close()


# ---- 3. the gallery afterwards equals a fresh one of the old and the kept vectors ---------------------------------------------
def _battery(G, q, t):
    out = []
    out += list(G.search(q, k=10))
    out += list(G.search(q, k=10, score_threshold=0.5))
    out += list(G.search(q, k=200))
    out += list(G.search_range(q, 0.6))
    out += list(G.pairs(t))
    out += list(G.pairs(0.7))
    out += list(G.recommend(q[:3], q[3:5], k=10))
    out += list(G.search_mmr(q, k=10, candidates=50, diversity=0.5))
    return [o.cpu().numpy().tobytes() for o in out]


@pytest.mark.parametrize("shape,t", [(SHAPES[0], 0.9), (SHAPES[1], 0.8), (SHAPES[2], 0.95), (SHAPES[3], 0.9), (SHAPES[4], 0.9),
                                     (SHAPES[5], 0.8)], ids=lambda v: "N%d-n%d-D%d" % v if isinstance(v, tuple) else str(v))
def test_gallery_equals_a_fresh_one_of_the_kept_vectors(shape, t):
    N, n, D = shape
    g, b = _inputs(shape)
    G = _gallery(g, N + n)
    _, _, kept = G.add_unique(torch.tensor(b).to(DEV), t)
    F = _gallery(g, N + n)
    kb = b[kept.cpu().numpy()]
    if kb.shape[0]:
        F.add(torch.tensor(kb).to(DEV))
    assert len(G) == len(F)
    rng = np.random.default_rng(5)
    q = torch.tensor(np.concatenate([b[rng.integers(0, n, size=5)], rng.standard_normal((3, D)).astype(np.float32)])).to(DEV)
    for x, y in zip(_battery(G, q, t), _battery(F, q, t)):
        assert x == y
    assert G.read().cpu().numpy().tobytes() == F.read().cpu().numpy().tobytes()
    G.close()
    F.close()


# ---- 5. composition: one call = calls of 64 rows = calls of one row ------------------------------------------------------------
@pytest.mark.parametrize("n,step", [(700, 64), (60, 1)])
def test_split_calls_give_the_same(n, step):
    shape = (300, 1000, 64)
    N, _, D = shape
    g, b = _inputs(shape)
    b = b[200:200 + n]                                      # (a stretch with repeats, chains and gallery copies)
    t = 0.9
    A = _gallery(g, N + n)
    ra = A.add_unique(torch.tensor(b).to(DEV), t)
    assert 0 < int(ra[2].sum()) < n
    B = _gallery(g, N + n)
    parts = [B.add_unique(torch.tensor(b[a:a + step]).to(DEV), t) for a in range(0, n, step)]
    rb = [torch.cat([p[i] for p in parts]) for i in range(3)]
    assert torch.equal(ra[0], rb[0]) and torch.equal(_bits(ra[1]), _bits(rb[1])) and torch.equal(ra[2], rb[2])
    assert A.read().cpu().numpy().tobytes() == B.read().cpu().numpy().tobytes()
    A.close()
    B.close()


# ---- 6. idempotence ------------------------------------------------------------------------------------------------------------
def test_the_same_batch_again_keeps_nothing():
    shape, t = (1500, 700, 256), 0.9
    N, n, D = shape
    g, b = _inputs(shape)
    G = _gallery(g, N + 2 * n)
    bd = torch.tensor(b).to(DEV)
    r1 = G.add_unique(bd, t)
    size = len(G)
    rows1 = G.read().cpu().numpy()
    # the oracle of test 1 for the second call: every row of the gallery as it is now, then the batch, by a plain add
    H = engine.Gallery(D, size + n, device=0)
    H.add(torch.tensor(rows1).to(DEV), normalize=False)                                     # (the master bits as they are)
    H.add(bd)
    pairs, scores = H.pairs(t)
    H.close()
    kept, rep, rep_score = dc.greedy_pairs(size, n, pairs.cpu().numpy(), scores.cpu().numpy())
    r2 = G.add_unique(bd, t)
    assert len(G) == size and not bool(r2[2].any()) and not kept.any()
    assert torch.equal(r2[0], r1[0])                        # every row's earlier answer: its own row, or its representative's
    assert np.array_equal(r2[0].cpu().numpy(), dc.final_rows(size, kept, rep))
    assert np.array_equal(r2[1].cpu().numpy().view(np.uint32), rep_score.astype(np.float32).view(np.uint32))
    # a row kept the first time now meets its exact copy: the self-score bits, those of every other exact copy
    was_kept = r1[2].cpu().numpy()
    self_bits = r2[1].cpu().numpy().view(np.uint32)[was_kept]
    assert np.all(np.abs(self_bits.view(np.float32) - 1.0) <= 1e-6)
    d = ~was_kept
    assert np.array_equal(r2[1].cpu().numpy().view(np.uint32)[d], r1[1].cpu().numpy().view(np.uint32)[d])
    assert G.read().cpu().numpy().tobytes() == rows1.tobytes()
    G.close()


# ---- 7. a block of identical rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gallery", [False, True])
def test_sixteen_thousand_identical_rows(with_gallery):
    D, n = 64, 16384
    rng = np.random.default_rng(21)
    v = rng.standard_normal(D).astype(np.float32)
    N = 300 if with_gallery else 0
    g = rng.standard_normal((N, D)).astype(np.float32)
    if with_gallery:
        g[37] = v
    G = _gallery(g, N + n)
    rows = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    scores = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    kept = C.c_int64(-5)
    vd = torch.tensor(np.repeat(v[None], n, 0)).to(DEV)
    rc = G._lib.revo_gallery_append_unique(G._h, _lib.ptr(vd), n, 1, 1, 0.9, _lib.ptr(rows), _lib.ptr(scores), 1, C.byref(kept),
                                           _lib.current_stream())
    assert rc == 0, G._lib.revo_last_error()
    st = G.search_stats()
    assert st["collected_rows"] < n and st["join_passes"] == 1           # (1.3e8 duplicate pairs, none of them stored)
    s = scores.cpu().numpy()
    if with_gallery:
        assert kept.value == 0 and len(G) == N
        assert bool((rows == 37).all())
        assert (s.view(np.uint32) == s.view(np.uint32)[0]).all() and abs(float(s[0]) - 1.0) <= 1e-6
    else:
        assert kept.value == 1 and len(G) == 1
        assert bool((rows == 0).all())
        assert s[0] == -np.inf and (s[1:].view(np.uint32) == s[1:].view(np.uint32)[0]).all() and abs(float(s[1]) - 1.0) <= 1e-6
    G.close()


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------
def _raw(G, v, t, n=None):
    n = v.shape[0] if n is None else n
    rows = torch.full((max(n, 1),), -7, dtype=torch.int64, device=DEV)
    scores = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=DEV)
    kept = C.c_int64(-5)
    rc = G._lib.revo_gallery_append_unique(G._h, _lib.ptr(v), n, 1, 1, t, _lib.ptr(rows), _lib.ptr(scores), 1, C.byref(kept),
                                           _lib.current_stream())
    return rc, rows, scores, kept.value


def test_edge_cases():
    shape, t = (300, 1000, 64), 0.9
    N, _, D = shape
    g, b = _inputs(shape)
    bd = torch.tensor(b).to(DEV)
    G = _gallery(g, N + 100)
    # n = 0
    r, s, k = G.add_unique(bd[:0], t)
    assert r.shape == (0,) and s.shape == (0,) and k.shape == (0,) and len(G) == N
    rc, rows, _, kept = _raw(G, bd, t, n=0)
    assert rc == 0 and kept == 0 and int(rows[0]) == -7
    # one row short of N + n: refused, nothing written, the size unchanged -- however few rows would be kept
    rc, rows, scores, kept = _raw(G, bd[:101], t)
    assert rc == -2 and b"capacity" in G._lib.revo_last_error()
    assert kept == -5 and bool((rows == -7).all()) and bool((scores == -7.0).all()) and len(G) == N
    # a held pairs result and a filter sized for N
    G.pairs(t)
    bits = G.allow_bits(torch.ones(N, dtype=torch.bool, device=DEV))
    assert G._lib.revo_search_set_filter(G._h, _lib.ptr(bits), N, 1, _lib.current_stream()) == 0
    # capacity exactly N + n
    rc, rows, scores, kept = _raw(G, bd[:100], t)
    assert rc == 0 and 0 < kept < 100 and len(G) == N + kept
    ref = dc.final_rows(N, *_reference_slice(g, b[:100], t)[:2])
    assert np.array_equal(rows.cpu().numpy(), ref)
    pr = torch.empty((1, 2), dtype=torch.int64, device=DEV)
    ps = torch.empty((1,), dtype=torch.float32, device=DEV)
    assert G._lib.revo_gallery_pairs_read(G._h, 0, 1, _lib.ptr(pr), _lib.ptr(ps), 1) == -2
    assert b"no result" in G._lib.revo_last_error()
    with pytest.raises(_lib.RevoError, match="set it again after appending"):
        G.search(bd[:2], k=3)
    G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    G.close()
    # more rows than one call takes
    big = engine.Gallery(D, 20000, device=0)
    v = torch.zeros((16385, D), dtype=torch.float32, device=DEV)
    rc, _, _, kept = _raw(big, v, t)
    assert rc == -2 and b"16384" in big._lib.revo_last_error() and kept == -5 and len(big) == 0
    big.close()
    # no fp32 master rows
    K = _gallery(g, N + 10, keep_f32=False)
    rc, _, _, kept = _raw(K, bd[:10], t)
    assert rc == -2 and b"keep_f32" in K._lib.revo_last_error() and kept == -5 and len(K) == N
    with pytest.raises(_lib.RevoError):
        K.add_unique(bd[:10], t)
    K.close()


def _reference_slice(g, b, t):
    N, n = g.shape[0], b.shape[0]
    H = _gallery(np.concatenate([g, b]), N + n)
    pairs, scores = H.pairs(t)
    H.close()
    return dc.greedy_pairs(N, n, pairs.cpu().numpy(), scores.cpu().numpy())


def test_twenty_thousand_rows_are_chunked_inside():
    N, n, D, t = 300, 20000, 64, 0.9
    g, b = dc.video_like(N, n, D, 31)
    kept, rep, rep_score = _reference_slice(g, b, t)
    G = _gallery(g, N + n)
    rows, scores, k = G.add_unique(torch.tensor(b), t)                     # (a host source)
    assert rows.is_cuda and scores.is_cuda and k.is_cuda
    assert np.array_equal(k.cpu().numpy(), kept) and 0 < int(kept[16384:].sum()) < n - 16384
    assert np.array_equal(rows.cpu().numpy(), dc.final_rows(N, kept, rep))
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), rep_score.astype(np.float32).view(np.uint32))
    assert len(G) == N + int(kept.sum())
    G.close()


# ---- 9. the store ---------------------------------------------------------------------------------------------------------------
def test_store_upsert_skips_duplicates(tmp_path):
    from reverso_amd import store
    shape, t = (300, 1000, 64), 0.9
    N, n, D = shape
    g, b = _inputs(shape)
    ref = _reference(shape, t)
    st = store.GalleryStore(D, device=0, capacity=64, path=str(tmp_path / "db"))          # (a small capacity: the store regrows)
    gid, bid = [f"g-{i}" for i in range(N)], [f"b-{j}" for j in range(n)]
    assert st.upsert(torch.tensor(g.copy()), gid, [{"k": i} for i in range(N)], files=["old.jpg"]) is None
    with pytest.raises(ValueError, match="replace_existing"):
        st.upsert(torch.tensor(b.copy()), bid, [{} for _ in bid], replace_existing=True, skip_duplicates=t)
    rep = st.upsert(torch.tensor(b.copy()).to(DEV), bid, [{"k": N + j} for j in range(n)], files=["new.jpg"], skip_duplicates=t)
    kept = ref["kept"]
    want_ids = gid + [bid[j] for j in np.flatnonzero(kept)]
    assert rep["kept"] == int(kept.sum()) and st.ids == want_ids and len(st) == len(st.gallery) == len(want_ids)
    assert [p["k"] for p in st.payloads] == list(range(N)) + [N + int(j) for j in np.flatnonzero(kept)]
    all_ids = gid + bid
    assert [(a, r) for a, r, _ in rep["dropped"]] == [(bid[j], all_ids[ref["rep"][j]]) for j in np.flatnonzero(~kept)]
    assert np.array_equal(np.asarray([s for _, _, s in rep["dropped"]], dtype=np.float32).view(np.uint32),
                          ref["score"][~kept].view(np.uint32))
    # ids and payloads are aligned with the rows: a kept point's own vector finds it first
    for j in np.flatnonzero(kept)[::7]:
        hit = st.search(torch.tensor(b[j].copy()), limit=1)[0]
        assert hit.id == bid[j] and hit.payload == {"k": N + int(j)}
    # a file whose rows were all dropped still counts as done
    rep2 = st.upsert(torch.tensor(b[:5].copy()), [f"again-{j}" for j in range(5)], [{} for _ in range(5)], files=["dup.jpg"],
                     skip_duplicates=t)
    assert rep2["kept"] == 0 and len(rep2["dropped"]) == 5 and st.ids == want_ids
    q = torch.tensor(b[::50].copy()).to(DEV)
    before = [a.cpu().numpy().tobytes() for a in st.gallery.search(q, k=10)]
    st.save()
    assert {"old.jpg", "new.jpg", "dup.jpg"} <= st.files_done
    st.close()
    ld = store.GalleryStore.load(str(tmp_path / "db"), device=0)
    assert ld.ids == want_ids and {"old.jpg", "new.jpg", "dup.jpg"} <= ld.files_done
    assert [a.cpu().numpy().tobytes() for a in ld.gallery.search(q, k=10)] == before
    ld.close()


# ---- 10. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_skips_byte_copies(tmp_path):
    import shutil
    from PIL import Image
    from reverso_amd.core_system import SimpleReverso
    folder = tmp_path / "frames"
    folder.mkdir()
    rng = np.random.default_rng(3)
    originals = {}
    for i in (0, 1, 3, 4, 6, 8, 10):                                     # 7 different frames ...
        arr = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8).repeat(20, 0).repeat(20, 1)
        Image.fromarray(arr).save(str(folder / f"f_{i:02d}.jpg"), quality=90)
        originals[i] = f"f_{i:02d}.jpg"
    for i, src in ((2, 0), (5, 4), (7, 1), (9, 8), (11, 0)):             # ... and 5 byte copies of earlier ones
        shutil.copyfile(str(folder / f"f_{src:02d}.jpg"), str(folder / f"f_{i:02d}.jpg"))
    want = sorted(originals.values())

    def system(name, skip):
        return SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / name), max_batch=4, skip_duplicates=skip,
                             checkpoint_interval_s=0.0)

    def stopped_build(r):
        """three batches of four files; a stop requested while the first is stored leaves the last one for the resume"""
        msg = r.create_database(str(folder), "frames", use_direct_pe=True,
                                progress_callback=lambda m, v=None: r.request_stop() if m.startswith("🔄 Processing 1/") else None)
        assert "⏸️ Processing stopped" in msg

    r = system("a", 0.999)
    msg = r.create_database(str(folder), "frames", use_direct_pe=True)
    assert "ready for searching" in msg and len(r.vector_db) == 7
    assert sorted(p["filename"] for p in r.vector_db.payloads) == want
    assert r.last_ingest_stats["duplicates_skipped"] == 5
    assert sum(int(line.split()[2]) for line in msg.splitlines() if line.startswith("♻️ Skipped")) == 5
    rows_a = r.vector_db.gallery.read().cpu().numpy().tobytes()
    r.vector_db.close()
    # a stop, then a resume: the same 7 (a copy of an earlier batch's file is dropped against the rows the checkpoint brought back)
    r = system("b", 0.999)
    stopped_build(r)
    msg = r.create_database(str(folder), "frames", use_direct_pe=True, resume_from_checkpoint=True)
    assert "📋 Resuming from checkpoint" in msg and "ready for searching" in msg and len(r.vector_db) == 7
    assert sorted(p["filename"] for p in r.vector_db.payloads) == want
    assert r.vector_db.gallery.read().cpu().numpy().tobytes() == rows_a
    r.vector_db.close()
    # a resume with another value starts fresh; without the argument all 12 are stored
    stopped_build(system("c", 0.999))
    r = system("c", None)
    msg = r.create_database(str(folder), "frames", use_direct_pe=True, resume_from_checkpoint=True)
    assert "different skip_duplicates" in msg and "Starting fresh" in msg and "ready for searching" in msg
    assert len(r.vector_db) == 12 and "♻️" not in msg and r.last_ingest_stats["duplicates_skipped"] == 0
    r.vector_db.close()
    # the detector in region_mode "global": every region would share its image's vector -- refused before any work
    out = system("d", 0.9).create_database(str(folder), "frames", use_direct_pe=False)
    assert out.startswith("❌ skip_duplicates") and not os.path.exists(str(tmp_path / "d"))
