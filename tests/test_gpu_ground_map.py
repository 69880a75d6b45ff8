"""emf_hip_groundColumns, emf_hip_groundCells and emf_hip_groundClasses (include/emf_hip.h "Ground map", DESIGN.md
5.24) against tests/ground_reference.py, byte for byte: every box shape of the restatement's fixtures -- the tile edges
and the ragged 16-byte rows -- under every frame (the six axis-aligned ups at cells of 1, 2 and 3 voxels, two tilted
ups, a frame that maps every voxel outside the map, a frame with a NaN entry), all contents, 1 / 63 / 64 / 65 / 256
bins, robots of 1, 5 and B bins, steps of 0 and 2; outputs poisoned beforehand, a second call into the dirty buffers,
inputs only read; the contraction build gives the same bytes; every rejected argument leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import ground_reference as rf
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
CASES = rf.kernel_cases()
_expected = {}


def ident(case):
    shape, content, spec, bins, robot, step = case
    return f'{"x".join(str(v) for v in shape)}-{content}-{"_".join(str(v) for v in spec)}-B{bins}-R{robot}-S{step}'


def expected(case):
    """(classes, G, W, H, B, occ, fre, cells, classes2d) of the restatement, computed once and shared."""
    if case not in _expected:
        shape, content, spec, bins, robot, step = case
        v = rf.volume(shape, content)
        G, W, H, B = rf.spec_frame(shape, spec, bins)
        out = (v, G, W, H, B) + rf.ground_map(v, G, W, H, B, robot, step)
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[case] = out
    return _expected[case]


def poisoned(shape, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray(shape, dtype).fill_bytes_(POISON)


def run_case(case, lib=None):
    """The three entries on poisoned outputs, twice into the same buffers; with lib, through that library's entries."""
    from emfusion_amd import ops
    v, G, W, H, B, occ, fre, cells, classes2d = expected(case)
    robot, step = case[4], case[5]
    frame = ops.ground_frame(G, (W, H), B)
    d_v = to_dev(v)
    words = rf.words_of(B)
    d_occ, d_fre = poisoned((H, W, words), np.uint64), poisoned((H, W, words), np.uint64)
    d_cells, d_classes = poisoned((H, W), rf.CELL_DTYPE), poisoned((1, H, W), np.uint8)
    for again in (False, True):
        if lib is None:
            assert ops.ground_columns(d_v, frame, out=(d_occ, d_fre)) == (d_occ, d_fre)
            assert ops.ground_cells(d_occ, d_fre, B, robot, out=d_cells) is d_cells
            assert ops.ground_classes(d_cells, step, out=d_classes) is d_classes
        else:
            p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
            size, map_ = (C.c_int32 * 3)(*v.shape[::-1]), (C.c_int32 * 2)(W, H)
            assert lib.emf_hip_groundColumns(p(d_v), size, frame, p(d_occ), p(d_fre), None) == 0
            assert lib.emf_hip_groundCells(p(d_occ), p(d_fre), map_, B, robot, p(d_cells), None) == 0
            assert lib.emf_hip_groundClasses(p(d_cells), map_, step, p(d_classes), None) == 0
        got = d_occ.numpy(), d_fre.numpy(), d_cells.numpy(), d_classes.numpy()
        assert got[0].tobytes() == occ.tobytes(), (ident(case), again, "occ", np.argwhere(got[0] != occ)[:4])
        assert got[1].tobytes() == fre.tobytes(), (ident(case), again, "fre", np.argwhere(got[1] != fre)[:4])
        assert got[2].tobytes() == cells.tobytes(), (ident(case), again, "cells", np.argwhere(got[2] != cells)[:4])
        assert got[3].tobytes() == classes2d.tobytes(), (ident(case), again, "classes", np.argwhere(got[3] != classes2d)[:4])
    assert d_v.numpy().tobytes() == v.tobytes()  # only read


def test_the_cases_cover_what_the_issue_lists():
    seen = {(c[0], c[2]) for c in CASES}
    assert all((shape, spec) in seen for shape in rf.SHAPES for spec in rf.FRAME_SPECS)
    assert {c[1] for c in CASES} == set(rf.CONTENTS) and {c[3] for c in CASES} == set(rf.BINS)
    assert {c[5] for c in CASES} == {0, 2} and {1, 5} <= {c[4] for c in CASES} and any(c[4] == c[3] > 5 for c in CASES)
    for shape in rf.SHAPES:
        assert {c[1] for c in CASES if c[0] == shape} == set(rf.CONTENTS)


@pytest.mark.parametrize("shape", rf.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("content", rf.CONTENTS)
def test_the_three_entries_are_exact(dev, shape, content):
    mine = [c for c in CASES if c[0] == shape and c[1] == content]
    assert len(mine) >= 4
    for case in mine:
        run_case(case)


def test_the_scene_has_floors_tables_and_a_pole(dev):
    """What the scene cases hold, so that their exactness means something: floors, two storeys under the high table, a
    low table that a tall robot does not fit under, and the one-voxel pole that turns its cell of 3 voxels into an
    obstacle."""
    shape = (70, 21, 19)
    by = {(c[2], c[4]): expected(c) for c in CASES if c[0] == shape and c[1] == "scene" and c[2][0] == "axis" and c[2][1:3] == (2, 1)}
    one, tall = by[(("axis", 2, 1, 1), 1)], by[(("axis", 2, 1, 1), 5)]
    cells1, cells5 = one[7], tall[7]
    assert (cells1["floor"] >= 0).sum() > 1000 and (cells1["levels"] > 1).sum() > 100
    low = (slice(21 // 2, 21), slice(70 // 2, 3 * 70 // 4))         # under the low table: 3 free voxels
    assert (cells1["floor"][low] == 1).all() and (cells1["clear"][low] == 3).all()
    assert (cells5["floor"][low] == 5).all()                        # the tall robot stands on the plate, not under it
    assert cells1["floor"][4, 7] == -1 and cells1["top"][4, 7] >= 2  # the pole at cell size 1
    coarse = by[(("axis", 2, 1, 3), 1)]
    assert coarse[7]["top"][1, 2] == 5 and coarse[7]["floor"][1, 2] == -1 and coarse[8][0, 1, 2] == rf.OCCUPIED  # ... in its cell of 3


def test_the_contraction_build_gives_the_same_bytes(dev):
    from emfusion_amd import _lib
    fma = _lib.load_variant("_fma")
    tilted = [c for c in CASES if c[2][0] in ("tilt20", "generic") and c[1] in ("random", "scene", "bytes_above_2")]
    assert len(tilted) >= 8
    for case in tilted:
        run_case(case, lib=fma)


def test_the_plain_return_values(dev):
    from emfusion_amd import ops
    case = next(c for c in CASES if c[0] == (70, 21, 19) and c[1] == "scene" and c[2] == ("tilt20", 2))
    v, G, W, H, B, occ, fre, cells, classes2d = expected(case)
    frame = ops.ground_frame(G, (W, H), B)
    d_occ, d_fre = ops.ground_columns(to_dev(v), frame)
    assert d_occ.shape == (H, W, rf.words_of(B)) and d_occ.numpy().tobytes() == occ.tobytes() and d_fre.numpy().tobytes() == fre.tobytes()
    d_cells, d_classes = ops.ground_map(to_dev(v), frame, case[4], case[5])
    assert d_cells.shape == (H, W) and d_cells.dtype == rf.CELL_DTYPE and d_cells.numpy().tobytes() == cells.tobytes()
    assert d_classes.shape == (1, H, W) and d_classes.numpy().tobytes() == classes2d.tobytes()
    # the 2-D classes are a valid input of the class-volume entries
    d2 = ops.distance_transform(d_classes, site_mask=2).numpy()
    assert d2.shape == (1, H, W) and ((d2 == 0) == (classes2d == rf.OCCUPIED)).all()


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    lib = _lib.load()
    p = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
    case = next(c for c in CASES if c[0] == (33, 9, 8) and c[2][0] == "axis" and c[3] == 65)
    v, G, W, H, B, occ, fre, cells, classes2d = expected(case)
    words = rf.words_of(B)
    d_v = to_dev(v)
    d_occ, d_fre = poisoned((H, W, words), np.uint64), poisoned((H, W, words), np.uint64)
    d_cells, d_classes = poisoned((H, W), rf.CELL_DTYPE), poisoned((1, H, W), np.uint8)
    i3 = lambda *a: (C.c_int32 * len(a))(*a)  # noqa: E731
    size, map_ = i3(*v.shape[::-1]), i3(W, H)

    def frame(W=W, H=H, B=B):
        f = ops.ground_frame(G, (1, 1), 1)
        f.map[:] = [W, H]
        f.bins = B
        return f

    def columns(classes=d_v, size=size, frame=frame(), occ=d_occ, fre=d_fre):
        return lib.emf_hip_groundColumns(p(classes), size, frame, p(occ), p(fre), None)

    class Off:  # a plane that is not 8-byte aligned
        ptr = d_occ.ptr + 4

    for bad, code in ((dict(classes=None), E_ARG), (dict(size=None), E_ARG), (dict(occ=None), E_ARG), (dict(fre=None), E_ARG),
                      (dict(fre=d_occ), E_ARG), (dict(occ=Off), E_ARG), (dict(size=i3(0, 9, 8)), E_ARG), (dict(size=i3(33, -1, 8)), E_ARG),
                      (dict(size=i3(2049, 1, 1)), E_LIMIT), (dict(size=i3(2048, 2048, 512)), E_LIMIT),
                      (dict(frame=frame(W=0)), E_ARG), (dict(frame=frame(H=-3)), E_ARG), (dict(frame=frame(W=2049)), E_LIMIT),
                      (dict(frame=frame(H=2049)), E_LIMIT), (dict(frame=frame(B=0)), E_ARG), (dict(frame=frame(B=257)), E_LIMIT)):
        assert columns(**bad) == code, bad

    def cells_(occ=d_occ, fre=d_fre, map_=map_, bins=B, robot=1, out=d_cells):
        return lib.emf_hip_groundCells(p(occ), p(fre), map_, bins, robot, p(out), None)

    for bad, code in ((dict(occ=None), E_ARG), (dict(fre=None), E_ARG), (dict(out=None), E_ARG), (dict(map_=None), E_ARG),
                      (dict(map_=i3(0, H)), E_ARG), (dict(map_=i3(W, 2049)), E_LIMIT), (dict(bins=0), E_ARG), (dict(bins=257), E_LIMIT),
                      (dict(robot=0), E_ARG), (dict(robot=-1), E_ARG), (dict(occ=Off), E_ARG)):
        assert cells_(**bad) == code, bad

    def classes_(cells=d_cells, map_=map_, step=0, out=d_classes):
        return lib.emf_hip_groundClasses(p(cells), map_, step, p(out), None)

    for bad, code in ((dict(cells=None), E_ARG), (dict(out=None), E_ARG), (dict(map_=None), E_ARG), (dict(map_=i3(W, 0)), E_ARG),
                      (dict(map_=i3(2049, H)), E_LIMIT), (dict(step=-1), E_ARG)):
        assert classes_(**bad) == code, bad
    for a in (d_occ, d_fre, d_cells, d_classes):  # nothing was enqueued
        assert (a.numpy().view(np.uint8) == POISON).all()
    # ... and what is taken: a robot taller than the band, a very large step
    assert columns() == 0 and cells_(robot=1000) == 0 and classes_(step=2 ** 31 - 1) == 0
    assert d_occ.numpy().tobytes() == occ.tobytes() and d_fre.numpy().tobytes() == fre.tobytes()
    got = d_cells.numpy()
    assert (got["floor"] == -1).all() and (got["levels"] == 0).all() and (got["top"] == cells["top"]).all()
    with pytest.raises(Exception):
        ops.ground_cells(d_occ, d_fre, B, 0)
    with pytest.raises(Exception):
        ops.ground_classes(d_cells, -1)
