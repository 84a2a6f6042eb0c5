"""CPU: the argument checks of the hybrid queries (revo_search_fusion and revo_topk_fuse return before the device is touched),
their binding and export by both libraries, the register allocation of their kernels (fusion.hip, from hipcc's own resource
report: hipcc cross-compiles for gfx950 without a GPU), the numpy statement of the contract on hand-made lists -- with the
wrong readings it must tell apart -- and the same refusals from a stand-alone program under the host sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

import reverso_amd  # noqa: F401
from reverso_amd import _lib, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hipcc_report import assert_no_spill, usage  # noqa: E402
import _fusion_checks  # noqa: E402
from _fusion_checks import bits, dbsf_stats, fuse, fuse_many  # noqa: E402

RRF, DBSF = engine.FUSION_METHODS["rrf"], engine.FUSION_METHODS["dbsf"]       # the method codes of the C ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = float("inf")


def _fake_handle():
    """a zero-filled stand-in for a handle: no fp32 rows (checks that read only these fields)"""
    return C.cast(C.create_string_buffer(1 << 16), C.c_void_p)


def _floats(*v):
    return (C.c_float * len(v))(*v)


def test_search_fusion_argument_checks_without_a_device():
    lib = _lib.load()
    qv = C.cast(C.create_string_buffer(4 * 64 * 4), C.c_void_p)
    bufs = [C.create_string_buffer(b"\x5a" * 256, 256) for _ in range(5)]
    s, i, c, r, ls = (C.cast(b, C.c_void_p) for b in bufs)
    fake = _fake_handle()

    def call(g=fake, q=qv, n=1, m=2, lim=8, method=0, rk=60.0, w=None, t=None, k=5, has=0, thr=0.0, s=s, i=i, c=c, r=r, ls=ls):
        return lib.revo_search_fusion(g, q, n, m, lim, method, rk, w, t, k, has, thr, 0, s, i, c, r, ls, None)

    err = lib.revo_last_error
    assert call(g=None) == -2 and b"null" in err()
    assert call(q=None) == -2 and b"null" in err()
    assert call(s=None) == -2 and b"null" in err()
    assert call(i=None) == -2 and b"null" in err()
    assert call(c=None) == -2 and b"null" in err()
    assert call(n=-1) == -2 and b"negative" in err()
    assert call(m=0) == -2 and b"[1, 64]" in err()
    assert call(m=65, lim=1) == -2 and b"[1, 64]" in err()
    assert call(lim=0) == -2 and b"[1, 1024]" in err()
    assert call(lim=1025) == -2 and b"[1, 1024]" in err()
    assert call(m=9, lim=1024) == -2 and b"8192" in err()
    assert call(m=64, lim=129) == -2 and b"8192" in err()
    assert call(m=3, lim=2731) == -2
    assert call(k=0) == -2 and b"k must" in err()
    assert call(k=1025) == -2 and b"k must" in err()
    assert call(method=2) == -2 and b"method" in err()
    assert call(method=-1) == -2 and b"method" in err()
    assert call(rk=-0.5) == -2 and b"rrf_k" in err()
    assert call(rk=INF) == -2 and b"rrf_k" in err()
    assert call(rk=float("nan")) == -2 and b"rrf_k" in err()
    assert call(w=_floats(1.0, -1.0)) == -2 and b"weight" in err()
    assert call(w=_floats(INF, 1.0)) == -2 and b"weight" in err()
    assert call(w=_floats(1.0, float("nan"))) == -2 and b"weight" in err()
    assert call(t=_floats(0.0, float("nan"))) == -2 and b"list threshold" in err()
    assert call(has=1, thr=float("nan")) == -2 and b"NaN" in err()
    # every argument valid, the boundary values included: the handle has no fp32 master rows
    assert call() == -2 and b"keep_f32" in err()
    assert call(r=None, ls=None) == -2 and b"keep_f32" in err()                # ranks and list_scores may be NULL
    assert call(q=None, n=0) == -2 and b"keep_f32" in err()                    # queries may be NULL at n = 0
    assert call(m=1, lim=1, k=1, rk=0.0, method=1) == -2 and b"keep_f32" in err()
    assert call(m=8, lim=1024, k=1024) == -2 and b"keep_f32" in err()
    assert call(m=64, lim=128, w=_floats(*([0.0] * 64)), t=_floats(*([-INF] * 63 + [INF]))) == -2 and b"keep_f32" in err()
    assert call(has=1, thr=-INF) == -2 and b"keep_f32" in err()
    assert call(has=0, thr=float("nan")) == -2 and b"keep_f32" in err()        # an unused threshold is not looked at
    assert all(b.raw == b"\x5a" * 256 for b in bufs)


def test_topk_fuse_argument_checks_without_a_device():
    lib = _lib.load()
    ins = [C.create_string_buffer(b"\x00" * 256, 256) for _ in range(3)]
    outs = [C.create_string_buffer(b"\x5a" * 256, 256) for _ in range(4)]
    a, b, c = (C.cast(x, C.c_void_p) for x in ins)
    s, i, n_out, r = (C.cast(x, C.c_void_p) for x in outs)

    def call(a=a, b=b, c=c, n=1, m=2, lim=8, method=0, rk=60.0, w=None, t=None, k=5, has=0, thr=0.0, s=s, i=i, n_out=n_out, r=r):
        return lib.revo_topk_fuse(a, b, c, n, m, lim, method, rk, w, t, k, has, thr, s, i, n_out, r, None)

    err = lib.revo_last_error
    for kw in ({"a": None}, {"b": None}, {"c": None}, {"s": None}, {"i": None}, {"n_out": None}):
        assert call(**kw) == -2 and b"null" in err(), kw
    assert call(n=-1) == -2 and b"negative" in err()
    assert call(m=0) == -2 and call(m=65, lim=1) == -2 and b"[1, 64]" in err()
    assert call(lim=0) == -2 and call(lim=1025) == -2 and b"[1, 1024]" in err()
    assert call(m=9, lim=1024) == -2 and b"8192" in err()
    assert call(k=0) == -2 and call(k=1025) == -2 and b"k must" in err()
    assert call(method=2) == -2 and b"method" in err()
    assert call(rk=-1.0) == -2 and call(rk=INF) == -2 and call(rk=float("nan")) == -2 and b"rrf_k" in err()
    assert call(w=_floats(-1.0, 1.0)) == -2 and b"weight" in err()
    assert call(t=_floats(float("nan"), 0.0)) == -2 and b"list threshold" in err()
    assert call(has=1, thr=float("nan")) == -2 and b"NaN" in err()
    # no fused search: status 0, nothing launched, the inputs may be NULL
    assert call(a=None, b=None, c=None, n=0, m=64, lim=128, k=1024, rk=0.0, method=1) == 0
    assert all(x.raw == b"\x5a" * 256 for x in outs)


def test_binding_and_export():
    with open(os.path.join(ROOT, "include", "revo.h")) as f:
        header = f.read()
    for name, n_args in (("revo_search_fusion", 19), ("revo_topk_fuse", 18)):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_exp(), name)
        m = re.search(r"int32_t " + name + r"\(([^;]*)\);", header)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == n_args
    assert "FUSION." in header
    assert (RRF, DBSF) == (_fusion_checks.RRF, _fusion_checks.DBSF) == (0, 1)


def test_fusion_kernels_do_not_spill():
    """Both kernels of fusion.hip: no VGPR spills and no scratch (the weights and list thresholds arrive by value, 512 bytes
    of kernel arguments indexed by the list: they must be read where they lie, not copied to scratch); the fuse kernel's
    static LDS and its two dynamic arrays of 8192 keys fit the 160 KiB of a CU."""
    assert_no_spill("fusion.hip", "fusion_", 2)
    fuse_k = [v for k, v in usage("fusion.hip").items() if "fusion_fuse_kernel" in k]
    assert len(fuse_k) == 1 and fuse_k[0]["LDS Size"] + 2 * 8192 * 8 <= 160 * 1024


# ------------------------------------------------------------------ the statement ----
def _one(lists, **kw):
    """lists: [[(row, score), ...], ...] -> fuse() on padded arrays"""
    m, C = len(lists), max(1, max(len(x) for x in lists))
    s = np.full((m, C), np.nan, dtype=f32)
    i = np.full((m, C), -5, dtype=np.int64)
    for j, entries in enumerate(lists):
        for p, (row, score) in enumerate(entries):
            i[j, p], s[j, p] = row, score
    return fuse(s, i, [len(x) for x in lists], **kw)


TIES = [[(5, 0.9), (3, 0.8)], [(3, 0.5), (5, 0.4)]]                      # rows 3 and 5 hold ranks {1, 2} in different lists
ORDER = [[(7, 0.9)], [(7, 0.8)], [(7, 0.7)]]                             # one row, three contributions: 1, 2^-24, 2^-24
ORDER_W = [61.0, 61.0 * 2.0 ** -24, 61.0 * 2.0 ** -24]
CUT = [[(4, 0.1), (9, 0.8), (2, 0.7)], [(2, 0.6)]]                       # unsorted; t_0 = 0.5 drops the first entry
# nine equal scores and one below: the low one lies exactly 3 sd under the mean in real arithmetic, so its v is nothing but the
# rounding of the operations before it -- any other rounding sequence gives other bits
NINE_ONE = [[(r, 0.55827516) for r in range(9)] + [(9, 0.27065924)]]


def test_rrf_statement_on_hand_made_lists():
    F, rows, n, ranks = _one(TIES, k=4, method=RRF)
    c1, c2 = f32(1.0) / f32(f32(60.0) + f32(1.0)), f32(1.0) / f32(f32(60.0) + f32(2.0))
    # equal fused scores (fp32 addition commutes): the lower row first
    assert n == 2 and rows.tolist() == [3, 5, -1, -1] and ranks[:2].tolist() == [[2, 1], [1, 2]]
    assert np.array_equal(bits(F[:2]), bits([f32(c2 + c1), f32(c1 + c2)])) and F[0] == F[1]
    assert np.all(np.isneginf(F[2:])) and ranks[2:].tolist() == [[0, 0], [0, 0]]
    # each operation rounded where the contract says: rrf_k + r is an fp32 sum (2^24 + 1 is not an fp32 number) ...
    F, _, _, _ = _one([[(1, 0.5)]], k=1, method=RRF, rrf_k=16777216.0)
    assert F[0] == f32(2.0 ** -24) and F[0] != f32(1.0 / 16777217.0)
    # ... the weight is the fp32 weight, and the division is one correctly rounded fp32 operation
    F, _, _, _ = _one([[(1, 0.5), (2, 0.4), (3, 0.3)]], k=3, method=RRF, rrf_k=2.0, weights=[0.1])
    assert np.array_equal(bits(F), bits([f32(0.1) / f32(3.0), f32(0.1) / f32(4.0), f32(0.1) / f32(5.0)]))
    # the sum runs over the lists in ascending order, from the first contribution present: (1 + 2^-24) + 2^-24 = 1
    F, _, _, _ = _one(ORDER, k=1, method=RRF, weights=ORDER_W)
    assert F[0] == f32(1.0)
    # a weight-0 list: its rows are candidates with F = 0, behind every positive row, by row; a row of both keeps its ranks
    F, rows, n, ranks = _one([[(8, 0.9), (1, 0.8)], [(6, 0.7), (1, 0.6)]], k=5, method=RRF, weights=[0.0, 1.0])
    assert n == 3 and rows[:3].tolist() == [6, 1, 8] and F[2] == 0 and ranks[:3].tolist() == [[0, 1], [2, 2], [1, 0]]
    assert np.array_equal(bits(F[:2]), bits([c1, f32(f32(0.0) + c2)]))
    # a list emptied by its threshold, per-entry cut of an unsorted list: positions are those of the UNCUT list
    F, rows, n, ranks = _one(CUT, k=4, method=RRF, list_thresholds=[0.5, INF])
    assert n == 2 and rows[:2].tolist() == [9, 2] and ranks[:2].tolist() == [[2, 0], [3, 0]]
    assert np.array_equal(bits(F[:2]), bits([c2, f32(1.0) / f32(f32(60.0) + f32(3.0))]))
    # the fused threshold cuts F < t (a score equal to it stays); fewer candidates than k; k cuts
    F, rows, n, _ = _one(TIES + [[(8, 0.3)]], k=4, method=RRF, threshold=float(c1))
    assert n == 3 and rows[:3].tolist() == [3, 5, 8]
    assert _one(TIES + [[(8, 0.3)]], k=4, method=RRF, threshold=float(np.nextafter(c1, f32(1))))[2] == 2
    assert _one(TIES, k=1, method=RRF)[1].tolist() == [3]
    # a row twice in one list: once per occurrence in position order, the first position reported; entries past the count ignored
    F, rows, n, ranks = _one([[(4, 0.9), (4, 0.8), (2, 0.7)]], k=3, method=RRF)
    assert n == 2 and rows[:2].tolist() == [4, 2] and ranks[:2].tolist() == [[1], [3]] and F[0] == f32(c1 + c2)
    s = np.array([[0.9, 0.8, 0.7]], dtype=f32)
    assert fuse(s, np.array([[1, 2, 3]]), [2], 3, RRF)[1].tolist() == [1, 2, -1]
    assert fuse(s, np.array([[1, 2, 3]]), [0], 3, RRF)[2] == 0


def test_dbsf_statement_on_hand_made_lists():
    # a list of one member, and all-equal scores: sd = 0, v = 0.5
    F, rows, n, _ = _one([[(3, 0.2)], [(4, 0.7), (5, 0.7), (6, 0.7)]], k=4, method=DBSF, weights=[1.0, 0.3])
    assert n == 4 and rows.tolist() == [3, 4, 5, 6]
    assert np.array_equal(bits(F), bits([0.5] + [f32(0.3) * f32(0.5)] * 3))
    # two members: z = +-1, v = 0.5 +- 1/6 through the fp64 operations of the contract, one rounding to fp32 at the end
    F, rows, _, _ = _one([[(1, 0.75), (2, 0.25)]], k=2, method=DBSF)
    mu, sd = dbsf_stats([f32(0.75), f32(0.25)])
    assert (mu, sd) == (0.5, 0.25)
    assert np.array_equal(bits(F), bits([(0.75 - (0.5 - 3.0 * 0.25)) / (6.0 * 0.25), (0.25 - (0.5 - 3.0 * 0.25)) / (6.0 * 0.25)]))
    # ... fp64 throughout: the same formula in fp32 gives other bits for these scores
    sc = [f32(0.8123), f32(0.3377), f32(0.3011)]
    F, _, _, _ = _one([[(1, sc[0]), (2, sc[1]), (3, sc[2])]], k=3, method=DBSF)
    mu32 = f32(f32(f32(sc[0] + sc[1]) + sc[2]) / f32(3))
    sd32 = np.sqrt(f32(f32(f32(f32((sc[0] - mu32) ** 2) + f32((sc[1] - mu32) ** 2)) + f32((sc[2] - mu32) ** 2)) / f32(3)))
    F32 = [f32(f32(s - f32(mu32 - f32(3) * sd32)) / f32(f32(6) * sd32)) for s in sc]
    assert not np.array_equal(bits(F), bits(F32)) and np.allclose(F, F32, rtol=1e-5)
    # a v outside [0, 1] is not clamped: ten equal scores and one far below (z = -sqrt(10) < -3), then one far above
    F, rows, _, _ = _one([[(r, 0.9) for r in range(10)] + [(10, 0.1)]], k=11, method=DBSF)
    assert rows[-1] == 10 and F[-1] < 0 and math.isclose(F[-1], 0.5 - math.sqrt(10) / 6, rel_tol=1e-5)
    F, rows, _, _ = _one([[(0, 0.9)] + [(r, 0.1) for r in range(1, 11)]], k=11, method=DBSF)
    assert rows[0] == 0 and F[0] > 1
    # -0 = +0: weight 0 times a negative v is -0; it ties with the +0 of the other rows, the row decides, the sign is kept
    low_first = [[(r, 0.9) for r in range(5, 15)] + [(2, 0.1)]]
    F, rows, _, _ = _one(low_first, k=11, method=DBSF, weights=[0.0])
    assert rows.tolist() == [2] + list(range(5, 15)) and np.signbit(F).tolist() == [True] + [False] * 10
    low_last = [[(r, 0.9) for r in range(5, 15)] + [(20, 0.1)]]
    F, rows, _, _ = _one(low_last, k=11, method=DBSF, weights=[0.0])
    assert rows.tolist() == list(range(5, 15)) + [20] and np.signbit(F).tolist() == [False] * 10 + [True]
    # the statistics run over the kept entries only, in position order
    F, rows, _, ranks = _one(CUT, k=3, method=DBSF, list_thresholds=[0.5, -INF])
    mu, sd = dbsf_stats([f32(0.8), f32(0.7)])
    v9 = f32((float(f32(0.8)) - (mu - 3.0 * sd)) / (6.0 * sd))
    v2 = f32((float(f32(0.7)) - (mu - 3.0 * sd)) / (6.0 * sd))
    assert rows[:2].tolist() == [2, 9] and np.array_equal(bits(F[:2]), bits([f32(v2 + f32(0.5)), v9]))
    assert ranks[:2].tolist() == [[3, 1], [2, 0]]
    # the noise fixture: pinned, so that a change of the statement's own rounding sequence shows
    F, rows, _, _ = _one(NINE_ONE, k=10, method=DBSF)
    assert rows[-1] == 9 and bits(F[-1:])[0] == bits([-1.0722469e-16])[0] and F[0] == f32(0.5555556)


def test_wrong_readings_differ_from_the_contract():
    def differs(lists, variant, **kw):
        a, b = _one(lists, **kw), _one(lists, variant=variant, **kw)
        return not all(np.array_equal(x, y) if x.dtype != f32 else np.array_equal(bits(x), bits(y))
                       for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))

    assert differs(ORDER, "lists_desc", k=1, method=RRF, weights=ORDER_W)          # (2^-24 + 2^-24) + 1 = 1 + 2^-23
    assert _one(ORDER, variant="lists_desc", k=1, method=RRF, weights=ORDER_W)[0][0] == f32(1.0) + f32(2.0 ** -23)
    assert differs(NINE_ONE, "fma", k=10, method=DBSF)
    assert differs(CUT, "renumber", k=4, method=RRF, list_thresholds=[0.5, INF])
    assert differs(TIES, "row_desc", k=4, method=RRF)
    # and each fixture is indifferent to the readings it is not about (so the four fixtures are four separate checks)
    assert not differs(TIES, "lists_desc", k=4, method=RRF) and not differs(TIES, "renumber", k=4, method=RRF)
    assert not differs(ORDER, "row_desc", k=1, method=RRF, weights=ORDER_W)
    assert not differs(NINE_ONE, "lists_desc", k=10, method=DBSF) and not differs(NINE_ONE, "renumber", k=10, method=DBSF)


def test_array_form_equals_the_statement():
    """fuse_many (array operations, for the large GPU cases) against fuse, bit for bit: random lists with overlap, duplicates
    inside a list, counts of 0, 1 and C, thresholds, a zero weight."""
    rng = np.random.default_rng(5)
    for trial in range(24):
        m, C = [(1, 1), (2, 7), (3, 16), (5, 40), (64, 4), (8, 33)][trial % 6]
        n = 3
        idx = rng.integers(0, max(2, m * C // 2), size=(n, m, C)).astype(np.int64)
        if trial % 4 == 3:
            idx += (1 << 47) - 1 - int(idx.max())
        sc = rng.uniform(-0.2, 0.9, size=(n, m, C)).astype(f32)
        if trial % 5 == 0:
            sc[:, 0] = f32(0.25)
        counts = rng.choice([0, 1, C, max(1, C // 2)], size=(n, m)).astype(np.int32)
        w = rng.uniform(0.1, 2.0, size=m).astype(f32).tolist()
        w[-1] = 0.0 if trial % 2 else w[-1]
        t = [(-INF, 0.1, INF)[(trial + j) % 3] for j in range(m)] if trial % 3 == 0 else None
        thr = None if trial % 2 else 0.01
        for method in (RRF, DBSF):
            k = (1, 10, 50)[trial % 3]
            got = fuse_many(sc, idx, counts, k, method, rrf_k=(0.0, 2.0, 60.0)[trial % 3], weights=w, list_thresholds=t,
                            threshold=thr)
            for i in range(n):
                want = fuse(sc[i], idx[i], counts[i], k, method, rrf_k=(0.0, 2.0, 60.0)[trial % 3], weights=w,
                            list_thresholds=t, threshold=thr)
                assert np.array_equal(bits(got[0][i]), bits(want[0])), (trial, method, i)
                assert np.array_equal(got[1][i], want[1]) and got[2][i] == want[2] and np.array_equal(got[3][i], want[3])


def test_fusion_entry_points_under_address_and_ub_sanitizers():
    """tests/native/fusion_host_check.cpp: the same refusals from a stand-alone program whose host code (the translation units
    of the C ABI) is compiled with -fsanitize=address,undefined, the weight and threshold arrays exactly m long; no device is
    touched."""
    csrc = os.path.join(ROOT, "revers-o_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "4", "all", "fusion_check"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "fusion_host_check")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("search_fusion: null arguments", "search_fusion: domains", "topk_fuse: domains",
                 "topk_fuse: null arguments and the empty call"):
        assert case in r.stdout
