"""CPU checks of what the world-query tests stand on (tests/world_queries_reference.py): the restated
tile occupancy holds what the device tests need it to hold, the virtual-background description of a world box gives
the stamping arithmetic the same bits, and emf_hip_occupancyTiles refuses malformed tables and boxes without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import world_queries_reference as wq
from tests import world_reference as wr
from tests import world_volumes as wv

RES = (64, 48, 40)
OFFSET = (-1, -3, 2)


def margin_box(tiles):
    """The assembled extent plus one tile of margin on every side (test 1a of test_gpu_occupancy_tiles.py)."""
    lo, size = wq.extent_of(tiles)
    return tuple(a - t for a, t in zip(lo, wr.TILE)), tuple(s + 2 * t for s, t in zip(size, wr.TILE))


def third_removed(n):
    keep = np.ones(n, bool)
    keep[1::3] = False
    return keep


@pytest.fixture(scope="module")
def fused(oracle):
    t, w, vox = wv.fused(oracle, RES)
    t, w = wq.planted(t, w)
    return t, w, vox, wr.cut(t, w, offset=OFFSET)


def test_the_reference_over_the_margin_box_holds_what_the_device_tests_lean_on(fused):
    t, w, _, tiles = fused
    assert len(tiles["coords"]) == 60
    box = margin_box(tiles)
    assert box == ((-64, -32, 8), (128, 64, 56))
    ref = wq.classes_of_tiles(tiles, RES, box)
    assert ref.shape == (56, 64, 128)
    assert set(np.unique(ref)) == {dr.FREE, dr.OCCUPIED, dr.UNKNOWN}
    # inside the extent it is the dense volume's classes, outside all unknown
    assert ref[8:48, 8:56, 32:96].tobytes() == dr.classes_of(t, w).tobytes()
    outside = np.ones(ref.shape, bool)
    outside[8:48, 8:56, 32:96] = False
    assert (ref[outside] == dr.UNKNOWN).all()
    # literal, repeated-word and all-zero arrays all occur among tsdf and weights; absent tiles are the margin
    k = tiles["classes"][:, :2]
    assert (k == 2).any() and (k == 1).any() and (k == 0).any()
    assert sorted(tuple(int(v) for v in r) for r in np.unique(k, axis=0)) == [(0, 0), (0, 2), (1, 0), (1, 1), (2, 1), (2, 2)]
    # a listed tile whose weights are one repeated word of 0: the whole tile reads unknown whatever its tsdf says
    whole = np.flatnonzero((k[:, 0] == 1) & (k[:, 1] == 0))
    assert len(whole) == 1
    c = tiles["coords"][whole[0]] - np.array(OFFSET)
    assert (dr.classes_of(t, w)[wr.sr.tile_slices(tuple(int(v) for v in c))] == dr.UNKNOWN).all()
    # tiles decided once and tiles read voxel by voxel both occur
    uniform = (k < 2).all(axis=1)
    assert uniform.any() and (~uniform).any()


def test_a_third_of_the_tiles_removed_turns_voxels_unknown(fused):
    t, w, _, tiles = fused
    keep = third_removed(60)
    fewer = wr.cut(t, w, offset=OFFSET, keep=keep)
    assert len(fewer["coords"]) == 40
    box = margin_box(tiles)
    full, cut = wq.classes_of_tiles(tiles, RES, box), wq.classes_of_tiles(fewer, RES, box)
    changed = full != cut
    assert changed.any() and (cut[changed] == dr.UNKNOWN).all()
    # the same set by dropping entries from the full table
    again = wq.classes_of_tiles(wq.without(tiles, np.flatnonzero(~keep)), RES, box)
    assert again.tobytes() == cut.tobytes()


def test_boxes_that_leave_everything_and_boxes_of_one_voxel(fused):
    t, w, _, tiles = fused
    first = tuple(o * e for o, e in zip(OFFSET, wr.TILE))
    lo = (first[0] - 29, first[1] - 19, first[2] + 17)
    got = wq.classes_of_tiles(tiles, RES, (lo, (61, 21, 23)))
    want = np.full((23, 21, 61), dr.UNKNOWN, np.uint8)
    want[:, 19:, 29:] = dr.classes_of(t, w)[17:40, 0:2, 0:32]
    assert got.tobytes() == want.tobytes() and len(np.unique(got)) == 3
    one = wq.classes_of_tiles(tiles, RES, ((first[0] + 40, first[1] + 20, first[2] + 20), (1, 1, 1)))
    assert one.shape == (1, 1, 1) and one[0, 0, 0] == dr.classes_of(t, w)[20, 20, 40]
    far = wq.classes_of_tiles(tiles, RES, ((1000, -500, 77), (5, 6, 7)))
    assert far.shape == (7, 6, 5) and (far == dr.UNKNOWN).all()
    assert (wq.classes_of_tiles(wq.without(tiles, range(60)), RES, margin_box(tiles)) == dr.UNKNOWN).all()


def test_coordinate_maps():
    assert wq.lattice_of((-3, 5, 7), (32, 0, -8)) == (29, 5, -1)
    assert wq.volume_of(wq.lattice_of((-3, 5, 7), (32, 0, -8)), (32, 0, -8)) == (-3, 5, 7)
    box = ((-32, 4, 90), (128, 8, 20))
    assert wq.pad_of(box, (96, 96, 96)) == (32, 0, 14)
    assert wq.virtual_of(box, (96, 96, 96)) == ((160, 96, 124), ((0, 4, 104), (128, 8, 20)))
    assert wq.pad_of(((0, 0, 0), (96, 96, 96)), (96, 96, 96)) == (0, 0, 0)


@pytest.mark.parametrize("pad", [32, 40, 2048])
def test_virtual_volume_identity_of_the_stamping_coordinate(pad):
    """float(v + pad) - (res + 2 pad - 1) / 2.f has the bits of float(v) - (res - 1) / 2.f: operands and results are
    half-integers far below 2^23, so both expressions are exact."""
    v = np.arange(-2048, 4096, dtype=np.int64)
    for res in (40, 48, 64, 96, 512, 2047):
        real = wq.stamping_coordinate(v, res)
        virtual = wq.stamping_coordinate(v + pad, res + 2 * pad)
        assert real.dtype == np.float32 and real.tobytes() == virtual.tobytes(), (res, pad)
        # ... and in double, as QueryBox::worldPoint / voxelAt compute it
        assert ((v + pad) - (res + 2 * pad - 1) / 2.0).tobytes() == (v - (res - 1) / 2.0).tobytes()


def test_stamp_gives_the_same_bytes_in_both_descriptions(fused):
    t, w, vox, _ = fused
    classes = dr.classes_of(t, w)
    # a 16^3 ball, turned a little, near the middle of the volume
    g = np.arange(16, dtype=np.float32) - np.float32(7.5)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    ot = (np.sqrt(x * x + y * y + z * z) - np.float32(5.3)).astype(np.float32)
    ow = np.ones_like(ot)
    a = np.float32(0.3)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    obj = (ot, ow, None, np.float32(vox), R, np.array([0.013, -0.021, 0.017], np.float32))
    box = ((5, 3, 2), (40, 30, 20))
    want = dr.stamp(dr.crop(classes, box), RES, vox, box, [obj])
    assert (want != dr.crop(classes, box)).sum() > 100                 # the ball lands in the box
    for pad in ((32, 40, 2048), (1, 0, 7), (2048, 2048, 2048)):
        vres, vbox = wq.virtual_of(box, RES, pad)
        got = dr.stamp(dr.crop(classes, box), vres, vox, vbox, [obj])
        assert got.tobytes() == want.tobytes(), pad


# ---- the entry refuses what the host can see, without a device -------------------------------------------------------

def table_of(coords, classes=None):
    from emfusion_amd import ops
    n = len(coords)
    classes = np.ones((n, 3), np.uint8) if classes is None else classes
    return ops.mesh_tile_table(coords, classes, np.ones((n, 4), np.uint32), np.zeros((n, 3), np.uint64),
                               np.full((n, 7), -77, np.int32))     # (neighbours are neither used nor checked)


def occupancy(table, n, src=None, dev=16, host=True, lo=(0, 0, 0), size=(4, 4, 4), out=16):
    from emfusion_amd import _lib
    L = _lib.load()
    src = _lib.EmfMeshTilesSource() if src is None else src
    i3 = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    return L.emf_hip_occupancyTiles(C.c_void_p(dev), C.cast(table, C.c_void_p) if host else None, n, C.byref(src),
                                    i3(lo), i3(size), C.c_void_p(out), None)


def test_the_entry_refuses_null_and_malformed_arguments_before_any_launch():
    from emfusion_amd import _lib
    L = _lib.load()
    NULL, ARG, LIMIT = -1, -4, -5
    good = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    t = table_of(good)
    err = L.emf_hip_last_error_string
    assert occupancy(t, 3, dev=0) == NULL and b"tiles_dev is NULL" in err()
    assert occupancy(t, 3, host=False) == NULL
    assert L.emf_hip_occupancyTiles(C.c_void_p(16), C.cast(t, C.c_void_p), 3, None, (C.c_int32 * 3)(), (C.c_int32 * 3)(4, 4, 4),
                                    C.c_void_p(16), None) == NULL
    assert occupancy(t, (1 << 17) + 1) == LIMIT
    # the table rules of the tile mesher, with its codes
    k = np.ones((3, 3), np.uint8)
    k[1, 2] = 4
    assert occupancy(table_of(good, classes=k), 3) == ARG and b"class 4 of tile 1" in err()
    k[1, 2] = 2
    assert occupancy(table_of(good, classes=k), 3) == NULL
    k[1, 2] = 3
    assert occupancy(table_of(good, classes=k), 3) == NULL
    assert occupancy(table_of([(1, 0, 0), (0, 0, 0)]), 2) == ARG
    assert occupancy(table_of([(0, 1, 0), (5, 0, 0)]), 2) == ARG
    assert occupancy(table_of([(0, 0, 0), (0, 0, 0)]), 2) == ARG and b"not after" in err()
    src = _lib.EmfMeshTilesSource(arena=4096 + 8, arena_units=4)
    assert occupancy(t, 3, src) == ARG and b"arena" in err()
    src = _lib.EmfMeshTilesSource(tsdf=4096, weights=4096 + 4, volume_elements=1 << 20, row_stride=64, plane_stride=4096)
    assert occupancy(t, 3, src) == ARG
    src = _lib.EmfMeshTilesSource(tsdf=4096, weights=8192, volume_elements=1 << 20, row_stride=66, plane_stride=4096)
    assert occupancy(t, 3, src) == ARG and b"strides" in err()
    for axis, ext in enumerate((32, 8, 8)):
        for tile in ((1 << 19) // ext, -(1 << 19) // ext - 1):
            c = [0, 0, 0]
            c[axis] = tile
            assert occupancy(table_of([tuple(c)]), 1) == LIMIT, (axis, tile)
    # the box: the limits and codes of emf_hip_occupancyClasses, on the lattice
    assert occupancy(t, 3, out=0) == ARG and b"classes is NULL" in err()
    assert occupancy(t, 3, lo=None) == ARG
    assert occupancy(t, 3, size=None) == ARG
    assert occupancy(t, 3, size=(4, 0, 4)) == ARG and b"axis 1" in err()
    assert occupancy(t, 3, size=(4, 4, -1)) == ARG
    assert occupancy(t, 3, size=(2049, 1, 1)) == LIMIT and b"axis 0" in err()
    assert occupancy(t, 3, size=(2048, 2048, 512)) == LIMIT and b"2^31 - 1" in err()
    assert occupancy(t, 3, lo=(-(1 << 19) - 1, 0, 0)) == LIMIT and b"lattice" in err()
    assert occupancy(t, 3, lo=(0, (1 << 19) - 3, 0)) == LIMIT
    assert occupancy(t, 3, lo=(0, 0, (1 << 19) - 4), size=(4, 4, 5)) == LIMIT
