"""The late-input cases of native-aspect embedding (revo_vit_set_grid, revo_preprocess_crop_resize_hw and the experiment
library's revo_vit_read_grid_tables; DESIGN.md sections 2e and 4aa, tests/_stream_cases.py): the images arrive on a side stream
behind a sleep, and the outputs must have the default-stream run's bytes.  The cases are registered in the harness's own table
from here, a file of its own, so that the header's coverage (tests/test_stream_cases_host.py: every entry point that takes a
stream has a case) counts them; this module sorts before tests/test_gpu_streams.py, whose parametrised test then runs the cases
as well.  test_stream_cases_host.py reads the table when its tests run, which is after every module of a session has been
imported; run on its own, without this module, it reports the three entry points as uncovered."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_cases as sc  # noqa: E402

NEW = ("revo_vit_set_grid", "revo_preprocess_crop_resize_hw", "revo_vit_read_grid_tables")


def _u8(n, grid, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 3, grid[0] * 14, grid[1] * 14), dtype=np.uint8))


@sc.case("revo_vit_set_grid")
def embed_on_a_grid(r):
    """(2, 8) is built before the inputs exist: set_grid is then a lookup and the forward asynchronous.  (5, 3) is built by
    the late call itself: its tables are made on the side stream, behind the sleep, and the call waits for them as
    documented."""
    eng = sc._vit(r)
    eng.embed(_u8(1, (2, 8), 1).to(sc.DEV), grid=(2, 8))
    torch.cuda.synchronize()
    wide, tall = r.dev(_u8(5, (2, 8), 90)), r.dev(_u8(3, (5, 3), 91))
    native = r.dev(sc.images_u8(2, 92))
    bits = r.host(np.array([[0x1ff], [0x1fe00], [0x1ffff]], dtype=np.uint32))
    r.arm()
    r.out("wide", eng.embed(wide, grid=(2, 8)))
    r.asynchronous("embed(grid=(2, 8)), a cached shape")
    r.out("wide tokens", eng.embed_tokens(wide, grid=(2, 8)))
    r.asynchronous("embed_tokens(grid=(2, 8))")
    r.out("native between", eng.embed(native))
    r.asynchronous("embed() between two grids")
    r.out("wide regions", eng.embed_regions(wide, [0, 4, 2], bits, grid=(2, 8)))
    r.noted("embed_regions(grid=(2, 8))")                     # host bitmaps: the pinned buffer
    r.scribble(bits)
    r.out("tall", eng.embed(tall, grid=(5, 3)))
    r.noted("embed(grid=(5, 3)), a new shape")                # documented: the first set_grid of a shape waits for its tables
    r.out("native after", eng.embed(native))


@sc.case("revo_vit_read_grid_tables", "revo_vit_set_grid")
def grid_tables_hook(r):
    from reverso_amd import _lib
    eng = r.closing(sc._engine().VitEngine.synthetic(sc.TOWER, seed=3, device=0, max_batch=2, randomize_affine=True,
                                                    experiments=True))
    torch.cuda.synchronize()
    dummy = r.dev(_u8(1, (3, 5), 93))
    r.arm()
    S = 3 * 5 + (1 if eng.cfg.use_cls else 0)
    pos = torch.zeros((S, eng.cfg.width), device=sc.DEV)
    rope = torch.zeros((S, eng.cfg.head_dim // 2, 2), device=sc.DEV)
    with eng._grid_frame((3, 5)) as st:
        eng._call("revo_vit_read_grid_tables", _lib.ptr(pos), _lib.ptr(rope), st)
    r.noted("read_grid_tables after the shape's first set_grid")
    r.out("positions", pos)
    r.out("rope", rope)
    r.out("forward", eng.embed(dummy, grid=(3, 5)))


@sc.case("revo_preprocess_crop_resize_hw")
def crop_resize_to_rectangles(r):
    from reverso_amd import preprocess as pp
    rng = np.random.default_rng(94)
    frames = [r.dev(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))) for h, w in ((97, 131), (240, 135))]
    boxes = []
    for i in range(30):
        f = i % 2
        h, w = frames[f].shape[:2]
        x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
        boxes.append((f, x0, y0, int(rng.integers(x0 + 4, w + 1)), int(rng.integers(y0 + 4, h + 1))))
    r.arm()
    r.out("wide", pp.crop_resize_device(frames, boxes, (28, 112)))
    r.asynchronous("crop_resize to 28 x 112")
    r.out("tall", pp.crop_resize_device(frames, boxes[:11], (112, 28)))
    r.asynchronous("crop_resize to 112 x 28")
    r.out("square", pp.crop_resize_device(frames, boxes[3:], 56))
    r.asynchronous("crop_resize to 56 x 56 after two rectangles")


def test_the_cases_are_in_the_table_and_the_header_is_covered():
    """CPU: with this module imported, no stream-taking declaration of include/revo.h is left without a case."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "revo.h")
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]
    claimed = {n for c in sc.CASES.values() for n in c.abi}
    for n in NEW:
        assert n in names and n in claimed, n
    if "boosted" in sc.CASES:        # (registered by its own module, as these are: present when the suite runs as a whole)
        assert [n for n in names if n not in claimed and n not in sc.NOT_RUN and not (n in sc.VIA and sc.VIA[n] in claimed)] == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["embed_on_a_grid", "grid_tables_hook", "crop_resize_to_rectangles"])
def test_grids_with_late_inputs_on_a_side_stream(dev, name):
    rep = sc.compare(name, sc.CASES[name].fn)
    print(rep)
    assert not rep.failed, str(rep)
    assert not rep.mismatches, str(rep)
    assert rep.late.enqueue_ms < sc.SLEEP_MS / 2, str(rep)
