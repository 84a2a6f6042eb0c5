"""CPU: the phases of the scan launch (topk256.hip scan256_plan, host logic) through the experiment library's
revo_debug_scan_plan -- no device needed.

With 8 query tiles and more, query tiles are pinned to XCDs and the slices of an XCD's query tiles have to line up, so the
launch takes them in phases of 8 a query tiles (a = 1, 2, 4 ... 32 per XCD, 32 / a slices each: 256 workgroups, every CU
busy), largest first, then the < 8 left over with the slices of a small launch.  Checked here: every query tile is in
exactly one phase, pinned phases start at a multiple of 8 blocks and fill an XCD's 32 CUs exactly, the segment-slot count
is the largest slice count, the block count adds up; plus the cases DESIGN.md quotes (8 192 and 9 984 queries)."""
import ctypes as C

import pytest

from reverso_amd import _lib


def _plan(Q, rows):
    lib = _lib.load_exp()
    out = (C.c_int64 * 64)()
    blocks = lib.revo_debug_scan_plan(Q, rows, out, 64)
    assert blocks > 0, (Q, rows)
    nph, splits = int(out[0]), int(out[1])
    phases = [tuple(int(out[2 + 4 * i + j]) for j in range(4)) for i in range(nph)]     # first block, q0, qn, ns
    return int(blocks), splits, phases


@pytest.mark.parametrize("rows", [16384, 60000, 116808, 991808, 10_000_000])
@pytest.mark.parametrize("Q", [1, 64, 255, 256, 257, 1000, 1792, 2048, 2049, 2304, 4096, 8192, 9984, 10000, 10240, 65536,
                               65537, 100_000, 1_000_000])
def test_phases_cover_every_query_tile_once(Q, rows):
    blocks, splits, phases = _plan(Q, rows)
    qtiles, tiles = (Q + 255) // 256, (rows + 255) // 256
    assert 1 <= len(phases) <= 8
    nxt, used = 0, 0
    for i, (first, q0, qn, ns) in enumerate(phases):
        assert q0 == nxt and qn >= 1 and 1 <= ns <= max(tiles, 1), (i, phases)
        assert first == used, (i, phases)                       # phases follow each other (padded to 8 blocks in between)
        nxt += qn
        used += qn * ns
        last = i == len(phases) - 1
        if not last:
            assert first % 8 == 0 and qn % 8 == 0, phases       # pinned: block b of the phase -> XCD b % 8 = its query tile % 8
            used = (used + 7) // 8 * 8
        if qtiles >= 8 and qn % 8 == 0 and (not last or qn >= 8):
            per_xcd = qn // 8 if qn <= 256 else 32              # query tiles an XCD holds at a time
            assert per_xcd in (1, 2, 4, 8, 16, 32), phases
            assert per_xcd * ns <= 32, phases                   # ... times their slices: at most its 32 CUs
            if tiles >= 3 * 32:
                assert per_xcd * ns == 32, phases               # and exactly 32 once the gallery has tiles to slice
    assert nxt == qtiles and used == blocks
    assert splits == max(p[3] for p in phases)
    if qtiles < 8:
        assert len(phases) == 1


def test_the_cases_the_design_quotes():
    tiles_rows = 991808                                         # 1 M rows minus the 8192-row pre-pass
    blocks, splits, phases = _plan(8192, tiles_rows)            # 32 query tiles: four per XCD x eight slices, nothing left over
    assert phases == [(0, 0, 32, 8)] and blocks == 256 and splits == 8
    blocks, splits, phases = _plan(9984, tiles_rows)            # 39 = 32 + 7
    assert phases[0] == (0, 0, 32, 8) and phases[1][1:3] == (32, 7) and len(phases) == 2
    assert 7 * phases[1][3] <= 256 and splits == phases[1][3]
    blocks, splits, phases = _plan(2048, tiles_rows)            # eight query tiles: one per XCD x 32 slices
    assert phases == [(0, 0, 8, 32)]
    blocks, splits, phases = _plan(64, tiles_rows)              # one query tile: a small launch, one round of workgroups
    assert len(phases) == 1 and phases[0][2] == 1 and 128 <= phases[0][3] <= 256


def test_the_two_phase_launch_of_the_small_gpu_cases():
    """The phase table has one author (scan256_phase_table, scan_plan.h) and two users; the GPU suite launches more than one
    phase through both.  The range join scans the whole gallery: tests/test_gpu_range_search.py runs 2304 queries x 1024 rows.
    The top-k scan skips the pre-pass rows (8192 at these sizes; N < 16 384 takes the small scan and has no phases at all):
    tests/test_gpu_search.py's test_phases_of_query_tiles_vs_oracle runs 2300 x 70 003, 3000 x 33 000 and 2560 x 300 000."""
    blocks, splits, phases = _plan(2304, 1024)                  # 9 query tiles x 4 gallery tiles: too few tiles to slice
    assert phases == [(0, 0, 8, 1), (8, 8, 1, 1)] and blocks == 9 and splits == 1
    for Q, rows, qn in ((2300, 70_003 - 8192, (8, 1)), (3000, 33_000 - 8192, (8, 4)), (2560, 300_000 - 8192, (8, 2))):
        blocks, splits, phases = _plan(Q, rows)
        assert tuple(p[2] for p in phases) == qn and phases[1][0] == 8 * phases[0][3], (Q, rows, phases)


# ---- galleries past 2^24 rows: the scan's 24-bit relative row index (topk256.hip key packing; launch_topk_scan256 refuses a
# slice of more than 2^24 rows) --------------------------------------------------------------------------------------------
_SLICE_LIMIT = 1 << 24
# The first query count at which a phase's slice passes 2^24 rows (None: never, the whole gallery fits one slice).  Pinned
# phases give each query tile 32 / a slices, a = 1, 2 .. 32 query tiles per XCD: one slice from 256 query tiles on (65 281
# queries), two from 128 (32 513), four from 64 (16 129) -- so a gallery of more than 2^26 rows is refused from 16 129
# queries on, one of more than 2^25 from 32 513, any of more than 2^24 from 65 281.
_FIRST_REFUSED = {2 ** 24 - 1: None, 2 ** 24: None, 2 ** 24 + 300: 65_281, 2 ** 25 + 1: 32_513, 10 ** 8: 16_129, 2 ** 27: 16_129}


def _largest_slice(Q, rows):
    """Rows of the longest slice of any phase.  revo_debug_scan_plan reports only the slice COUNT of a phase; the split into
    slices is made in launch_topk_scan256 (per = ceil(tiles / ns), slice i = tiles [i per, (i + 1) per) clipped to the
    gallery), and the lines below MIRROR that formula: they say what the launch does with the count (contiguous slices, the
    last ends at the last tile, trailing slices may be empty) and check the count's sanity, not the launch's own arithmetic."""
    _, _, phases = _plan(Q, rows)
    tiles = (rows + 255) // 256
    worst = 0
    for _, _, _, ns in phases:
        per = (tiles + ns - 1) // ns                                  # launch_topk_scan256: slice i = tiles [i per, (i + 1) per)
        ends = [min((i + 1) * per, tiles) for i in range(ns)]
        starts = [min(i * per, tiles) for i in range(ns)]
        assert 1 <= ns <= tiles and starts[0] == 0 and ends[-1] == tiles and starts[1:] == ends[:-1], (Q, rows, ns)
        worst = max(worst, per * 256)
    return worst


@pytest.mark.parametrize("rows", sorted(_FIRST_REFUSED))
def test_slices_of_galleries_past_2_24_rows(rows):
    first = _FIRST_REFUSED[rows]
    # every query-tile count up to 520 (133 120 queries), at both ends of the tile
    counts = sorted({1, 2, 255} | {256 * t + d for t in range(1, 521) for d in (0, 1)})
    over = [Q for Q in counts if _largest_slice(Q, rows) > _SLICE_LIMIT]
    assert (over[0] if over else None) == first, (rows, over[:3])
    for Q in counts:
        if Q <= 16_384 and (first is None or Q < first):
            assert _largest_slice(Q, rows) <= _SLICE_LIMIT, (Q, rows)
    if first is not None:
        assert _largest_slice(first - 1, rows) <= _SLICE_LIMIT
        assert all(Q in over for Q in counts if first <= Q <= 65_536), "refused from there on, up to 65 536 queries"
