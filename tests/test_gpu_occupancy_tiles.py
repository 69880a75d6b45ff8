"""emf_hip_occupancyTiles (ops.occupancy_tiles; include/emf_hip.h "Occupancy of a set of tiles"): the
occupancy classes of a box of the lattice from a sparse set of tiles, against tests/world_queries_reference.py and
against the dense pass.  Bytes against numpy, no tolerance.  Shapes chosen where the pass can go wrong: a 64 x 48 x 40
volume of 2 x 6 x 5 tiles under a negative lattice offset, boxes that are not aligned to a tile, to four voxels or to
anything, absent tiles on every face, tiles decided once next to tiles read voxel by voxel."""
import numpy as np
import pytest

from tests import distance_reference as dr
from tests import world_queries_reference as wq
from tests import world_reference as wr
from tests import world_volumes as wv
from tests.test_world_queries_reference_cpu import OFFSET, RES, margin_box, third_removed

pytestmark = pytest.mark.gpu
FIRST = tuple(o * e for o, e in zip(OFFSET, wr.TILE))      # the first tile's corner, lattice voxels
UNALIGNED = ((FIRST[0] - 29, FIRST[1] - 19, FIRST[2] + 17), (61, 21, 23))


@pytest.fixture(scope="module")
def vol(oracle):
    t, w, vox = wv.fused(oracle, RES)
    t, w = wq.planted(t, w)
    return t, w, vox


def check(tiles, box, want=None, what=""):
    from emfusion_amd import ops
    want = wq.classes_of_tiles(tiles, RES, box) if want is None else want
    got = ops.occupancy_tiles(tiles, box)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))
    return got


@pytest.mark.parametrize("mode", ["literal", "inplace", "mixed"])
def test_the_60_tiles_in_every_representation(dev, vol, mode):
    t, w, _ = vol
    tiles = wr.cut(t, w, offset=OFFSET, mode=mode, seed=3)
    if mode == "mixed":
        assert {2, 3} <= set(np.unique(tiles["classes"][:, 0]))
    a = check(tiles, margin_box(tiles), what="margin")                       # absent tiles on every face
    assert len(np.unique(a)) == 3
    b = check(tiles, UNALIGNED, what="unaligned")    # x start no multiple of 4, rows cut inside a tile on both ends
    assert len(np.unique(b)) == 3
    check(tiles, ((FIRST[0] + 40, FIRST[1] + 20, FIRST[2] + 20), (1, 1, 1)), what="one voxel")
    far = check(tiles, ((1000, -500, 77), (5, 6, 7)), what="absent space")
    assert (far == dr.UNKNOWN).all()
    # rows of the box that start at every x modulo 4, and rows whose length is no multiple of 4
    for dx in range(1, 4):
        check(tiles, ((FIRST[0] + dx, FIRST[1] + 1, FIRST[2] + 3), (64 - dx, 9, 7)), what=f"x + {dx}")


def test_all_tiles_in_place_at_offset_0_equal_the_dense_pass(dev, vol):
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    t, w, _ = vol
    tiles = wr.cut(t, w, mode="inplace")
    d_t, d_w = DeviceArray.from_numpy(t), DeviceArray.from_numpy(w)
    whole = ops.occupancy_classes(d_t, d_w).numpy()
    assert whole.tobytes() == dr.classes_of(t, w).tobytes()
    assert ops.occupancy_tiles(tiles, ((0, 0, 0), RES)).tobytes() == whole.tobytes()
    box = ((3, 5, 17), (61, 21, 23))                                         # UNALIGNED's shape, inside the volume
    assert ops.occupancy_tiles(tiles, box).tobytes() == ops.occupancy_classes(d_t, d_w, box=box).numpy().tobytes()


def test_stamping_through_the_virtual_resolution(dev, vol):
    """One 16^3 ball across the face x = 0 of the volume: the box leaves the volume, emf_hip_occupancyStampObjects gets
    it as a box of the virtual background, and the bytes are those of the restatement in REAL volume coordinates."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    t, w, vox = vol
    f = np.float32
    g = np.arange(16, dtype=f) - f(7.5)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    ot = (np.sqrt(x * x + y * y + z * z) - f(5.3)).astype(f)
    ow = np.ones_like(ot)
    a = f(0.3)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], f)
    centre = (np.array([0, 24, 20], f) - np.array([(n - 1) / 2 for n in RES], f)) * f(vox)
    tr = (-(R @ centre)).astype(f)
    tiles = wr.cut(t, w, mode="inplace")
    box = ((-16, -8, -8), (96, 64, 56))
    base = wq.classes_of_tiles(tiles, RES, box)
    want = dr.stamp(base, RES, vox, box, [(ot, ow, None, f(vox), R, tr)])
    changed = want != base
    assert changed[:, :, :16].any() and changed[:, :, 16:].any()               # on both sides of the face
    vres, vbox = wq.virtual_of(box, RES)
    assert vres == (96, 64, 56) and vbox[0] == (0, 0, 0)
    d_obj = (DeviceArray.from_numpy(ot), DeviceArray.from_numpy(ow), None, float(vox), R, tr)
    got = DeviceArray.from_numpy(ops.occupancy_tiles(tiles, box))
    ops.stamp_objects(got, vres, vox, [d_obj], box=vbox)
    assert got.numpy().tobytes() == want.tobytes()
    # a larger padding than needed describes the same box
    vres, vbox = wq.virtual_of(box, RES, (40, 32, 2048))
    again = DeviceArray.from_numpy(base)
    ops.stamp_objects(again, vres, vox, [d_obj], box=vbox)
    assert again.numpy().tobytes() == want.tobytes()
    # inside the volume it is the dense pass with the object stamped in the volume's own description
    dense = ops.occupancy_classes(DeviceArray.from_numpy(t), DeviceArray.from_numpy(w), objects=[d_obj], voxel_size=vox).numpy()
    assert want[8:48, 8:56, 16:80].tobytes() == dense.tobytes()


def test_a_third_of_the_tiles_removed_and_an_empty_table(dev, vol):
    t, w, _ = vol
    tiles = wr.cut(t, w, offset=OFFSET)
    box = margin_box(tiles)
    for mode in ("literal", "mixed"):
        fewer = wr.cut(t, w, offset=OFFSET, mode=mode, seed=5, keep=third_removed(60))
        got = check(fewer, box, what=mode)
        assert (got != wq.classes_of_tiles(tiles, RES, box)).any()
    none = wr.cut(t, w, offset=OFFSET, keep=np.zeros(60, bool))
    assert len(none["coords"]) == 0
    got = check(none, box, what="empty")
    assert (got == dr.UNKNOWN).all()
    check(none, UNALIGNED, what="empty, unaligned")


@pytest.mark.parametrize("mode", ["literal", "inplace"])
def test_nan_negative_zero_and_bad_weights(dev, vol, mode):
    t, w, _ = vol
    t, w = t.copy(), w.copy()
    rng = np.random.default_rng(11)
    sl = wr.sr.tile_slices((1, 3, 2))                                         # one literal tile
    tt, ww = t[sl].copy(), w[sl].copy()
    pick = rng.integers(0, 8, tt.shape)
    tt[pick == 0], tt[pick == 1] = np.nan, -0.0
    ww[pick == 2], ww[pick == 3], ww[pick == 4] = np.nan, -1.0, -0.0
    ww[pick < 2] = 1.0
    t[sl], w[sl] = tt, ww
    for tile, tv, wv_ in (((0, 1, 1), np.nan, 1.0), ((1, 0, 2), -0.0, 1.0), ((0, 2, 3), 0.5, np.nan), ((1, 5, 0), 0.5, -1.0),
                          ((0, 4, 1), 0.5, -0.0)):                            # the repeated word of class-1 tiles
        s2 = wr.sr.tile_slices(tile)
        t[s2], w[s2] = np.float32(tv), np.float32(wv_)
    tiles = wr.cut(t, w, offset=OFFSET, mode=mode)
    if mode == "literal":
        k = {tuple(int(v) for v in c - np.array(OFFSET)): tuple(int(v) for v in cl[:2]) for c, cl in zip(tiles["coords"], tiles["classes"])}
        assert k[(0, 1, 1)] == k[(1, 0, 2)] == k[(0, 2, 3)] == k[(1, 5, 0)] == k[(0, 4, 1)] == (1, 1) and k[(1, 3, 2)] == (2, 2)
    want = wq.classes_of_tiles(tiles, RES, margin_box(tiles))
    inner = want[8:48, 8:56, 32:96]
    assert (inner[wr.sr.tile_slices((0, 1, 1))] == dr.OCCUPIED).all() and (inner[wr.sr.tile_slices((1, 0, 2))] == dr.OCCUPIED).all()
    for tile in ((0, 2, 3), (1, 5, 0), (0, 4, 1)):
        assert (inner[wr.sr.tile_slices(tile)] == dr.UNKNOWN).all()
    lit = inner[sl]
    assert (lit[pick < 2] == dr.OCCUPIED).all() and (lit[(pick >= 2) & (pick <= 4)] == dr.UNKNOWN).all()
    check(tiles, margin_box(tiles), want, what="planted values")
    check(tiles, UNALIGNED, what="planted values, unaligned")


def test_what_only_the_device_sees_skips_the_tile(dev, vol):
    t, w, _ = vol
    # a literal outside the arena
    tiles = wr.cut(t, w, offset=OFFSET)
    i = int(np.flatnonzero((tiles["classes"][:, :2] == 2).all(axis=1))[7])
    for array, beyond in ((0, len(tiles["arena"])), (1, 1 << 40)):
        bad = dict(tiles, at=tiles["at"].copy())
        bad["at"][i, array] = beyond
        got = check(bad, margin_box(tiles), wq.classes_of_tiles(wq.without(tiles, [i]), RES, margin_box(tiles)), what="arena")
        cell = tuple(slice(s.start + 8 if k < 2 else s.start + 32, s.stop + 8 if k < 2 else s.stop + 32)
                     for k, s in enumerate(wr.sr.tile_slices(tuple(int(v) for v in tiles["coords"][i] - np.array(OFFSET)))))
        assert (got[cell] == dr.UNKNOWN).all()
    # an in-place tile that does not lie inside volume_elements, and one at an offset that is no multiple of 4
    tiles = wr.cut(t, w, offset=OFFSET, mode="inplace")
    for array, at in ((0, t.size - 64), (1, t.size), (0, int(tiles["at"][9, 0]) + 2)):
        bad = dict(tiles, at=tiles["at"].copy())
        bad["at"][9, array] = at
        check(bad, margin_box(tiles), wq.classes_of_tiles(wq.without(tiles, [9]), RES, margin_box(tiles)), what="volume")
    # the colour class counts for the skip rule alone: a colour literal outside the arena removes the tile
    tiles = wr.cut(t, w, offset=OFFSET)
    bad = dict(tiles, classes=tiles["classes"].copy(), at=tiles["at"].copy())
    bad["classes"][i, 2], bad["at"][i, 2] = 2, len(tiles["arena"]) - 1        # two units are needed, one is left
    check(bad, margin_box(tiles), wq.classes_of_tiles(wq.without(tiles, [i]), RES, margin_box(tiles)), what="colour")
    bad["at"][i, 2] = 0                                                        # inside: read by nobody, the tile counts
    check(bad, margin_box(tiles), wq.classes_of_tiles(tiles, RES, margin_box(tiles)), what="colour inside")
