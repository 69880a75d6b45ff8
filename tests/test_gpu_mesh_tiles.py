"""Marching cubes over a set of tiles on the device (include/emf_hip.h "Meshing a set of tiles"):
emf_hip_meshTilesCount / ...Emit / ...Colors / ...EdgeKeys through ops.mesh_tiles against the oracle's soup of the
dense box the tiles stand for, permuted into the canonical order (tests/world_reference.py).  Everything is compared
as bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import world_reference as wr
from tests import world_volumes as wv
from tests.weld_reference import weld

pytestmark = pytest.mark.gpu

RES = (64, 48, 40)
OFFSET = (-1, -3, 2)   # negative coordinates and seams across zero
_cache = {}


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k)


def fused_case(oracle, mode, colour=False, keep=None, tag=""):
    """(tiles, reference, voxel size) of the fused volume cut into tiles -- the reference computed once per set."""
    key = (mode, colour, tag)
    if key not in _cache:
        t, w, vox = wv.fused(oracle, RES)
        col = wv.colours(t.shape) if colour else None
        tiles = wr.cut(t, w, col, offset=OFFSET, mode=mode, seed=3, keep=keep)
        _cache[key] = (tiles, wr.reference(oracle, tiles, RES, vox, with_color=colour), vox)
    return _cache[key]


def check_all(ops, tiles, ref, vox, res, what, colour=False):
    """Soup, keys, welded and (with colour) coloured, each as bytes against the canonical oracle soup."""
    half = wr.half_of(res)
    soup, keys = ref["soup"], ref["keys"]
    got = ops.mesh_tiles(tiles, vox, half, keys=True)
    same(got[:3], soup, what)
    assert got[3].dtype == np.uint64 and np.array_equal(got[3], keys), what
    welded = ops.mesh_tiles(tiles, vox, half, weld=True)
    same(welded, weld(*soup, keys), what + " welded")
    assert len(welded[0]) == len(np.unique(keys))
    if colour:
        c = ops.mesh_tiles(tiles, vox, half, colors=True)
        same(c, soup + (ref["colours"],), what + " colours")
        same(ops.mesh_tiles(tiles, vox, half, weld=True, colors=True), weld(*soup, keys, ref["colours"]),
             what + " welded colours")


@pytest.mark.parametrize("mode", ["literal", "inplace", "mixed"])
def test_fused_volume_cut_into_its_tiles(oracle, ops, mode):
    tiles, ref, vox = fused_case(oracle, mode)
    assert len(tiles["coords"]) == 60 and len(ref["soup"][0]) == 18119
    if mode == "mixed":
        assert 20 < (tiles["classes"][:, 0] == 3).sum() < 40
    check_all(ops, tiles, ref, vox, RES, mode)


@pytest.mark.parametrize("mode", ["literal", "inplace", "mixed"])
def test_fused_volume_with_colours(oracle, ops, mode):
    tiles, ref, vox = fused_case(oracle, mode, colour=True)
    assert len(np.unique(ref["colours"], axis=0)) > 20
    check_all(ops, tiles, ref, vox, RES, mode + " colour", colour=True)


def test_a_tile_without_a_colour_array_counts_as_uncoloured(oracle, ops):
    """Class 0 colour on a seeded half of the tiles: their voxels are uncoloured, so a vertex on a seam takes the
    coloured endpoint's colour and one between two such tiles is black."""
    key = "half_coloured"
    if key not in _cache:
        t, w, vox = wv.fused(oracle, RES)
        col = wv.colours(t.shape).copy()
        bare = np.random.default_rng(5).integers(0, 2, 60).astype(bool)
        i = 0
        for z in range(5):
            for y in range(6):
                for x in range(2):
                    if bare[i]:
                        col[wr.sr.tile_slices((x, y, z))] = 0
                    i += 1
        tiles = wr.cut(t, w, col, offset=OFFSET, mode="mixed", seed=4)
        tiles["classes"][bare & (tiles["classes"][:, 2] == 3), 2] = 0   # absent, not "in place and zero"
        _cache[key] = (tiles, wr.reference(oracle, tiles, RES, vox, with_color=True), vox, bare)
    tiles, ref, vox, bare = _cache[key]
    assert (tiles["classes"][bare, 2] == 0).all() and (tiles["classes"][~bare, 2] != 0).all()
    assert (ref["colours"] == 0).all(axis=1).sum() > 1000 and len(np.unique(ref["colours"], axis=0)) > 20
    check_all(ops, tiles, ref, vox, RES, key, colour=True)


def test_a_third_of_the_tiles_removed(oracle, ops):
    keep = np.random.default_rng(11).integers(0, 3, 60) != 0
    assert 15 <= (~keep).sum() <= 25
    tiles, ref, vox = fused_case(oracle, "mixed", keep=keep, tag="holes")
    full = fused_case(oracle, "mixed")[1]
    # on the reference: cubes at the new rim are invalid, so triangles go, and enough stay to test something
    assert 1000 < len(ref["soup"][2]) < len(full["soup"][2]) - 500
    check_all(ops, tiles, ref, vox, RES, "holes")


def test_random_signs_the_densest_tiles(oracle, ops):
    if "random" not in _cache:
        t, w, vox = wv.random_sign()
        tiles = wr.cut(t, w, wv.colours(t.shape, seed=9), mode="literal")
        _cache["random"] = (tiles, wr.reference(oracle, tiles, (64, 16, 16), vox, with_color=True), vox)
    tiles, ref, vox = _cache["random"]
    assert (tiles["classes"][:, 1] == 1).all() and len(tiles["coords"]) == 8      # weights: one repeated element
    tc, la = ref["cubes"]
    cub, per = np.unique(np.concatenate([tc, la], 1), axis=0), None
    per = np.unique(cub[:, :3], axis=0, return_counts=True)[1]
    assert len(ref["soup"][0]) == 85481 and per.max() == 2030
    assert ((cub[:, :3] == 0).all(axis=1) & (cub[:, 3] == 31) & (cub[:, 4] == 7) & (cub[:, 5] == 7)).sum() == 1
    check_all(ops, tiles, ref, vox, (64, 16, 16), "random", colour=True)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_repeated_element_tiles_meet_at_the_surface(oracle, ops, axis):
    """tsdf -0.5 beside +0.5, weights 1, no literal anywhere: the surface lies exactly on the seam."""
    second = [0, 0, 0]
    second[axis] = 1
    word = lambda v: int(np.float32(v).view(np.uint32))
    # colour: one repeated voxel in the first tile (R, G | B, Wc), none in the second -- its side takes the first's
    tiles = dict(coords=np.array([(0, 0, 0), tuple(second)], np.int32), classes=np.array([(1, 1, 1), (1, 1, 0)], np.uint8),
                 words=np.array([(word(-0.5), word(1.0), 0x40002000, 0x00806000), (word(0.5), word(1.0), 0, 0)], np.uint32),
                 at=np.zeros((2, 3), np.uint64), arena=None, volume=None)
    res = (64, 16, 16)
    ref = wr.reference(oracle, tiles, res, 0.02, with_color=True)
    assert (ref["colours"] == (0x20, 0x40, 0x60)).all()
    ext = [32, 8, 8]
    del ext[axis]
    assert len(ref["soup"][2]) == 2 * ext[0] * ext[1] - 2 * (ext[0] + ext[1]) + 2  # two triangles per seam cube
    check_all(ops, tiles, ref, 0.02, res, f"seam {axis}", colour=True)
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in tiles.items()}
    got = ops.mesh_tiles(one, 0.02, wr.half_of(res))
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 4)
    assert got[0].dtype == np.float32 and got[2].dtype == np.int32


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_zeros_on_a_tile_face(oracle, ops, axis):
    """weld_volumes.zero_plane across a seam on each axis: the first plane of the second tile is exactly 0, and half of
    the last plane of the first, so vertexInterp's |v| < 1e-5 branches return corners on both sides of the seam -- in
    y and z the corner comes out of the halo rows."""
    shape = [8, 8, 32]                          # (z, y, x) of one tile
    a = 2 - axis                                # numpy axis of the seam
    ext = shape[a]
    shape[a] *= 2
    t = np.full(shape, -0.5, np.float32)
    along = [slice(None)] * 3
    along[a] = slice(ext + 1, None)
    t[tuple(along)] = 0.5
    along[a] = ext
    t[tuple(along)] = 0.0
    along[a] = ext - 1
    other = (a + 1) % 3
    along[other] = slice(shape[other] // 2, None)
    t[tuple(along)] = 0.0
    w = np.ones_like(t)
    res = tuple(shape[::-1])
    tiles = wr.cut(t, w, mode="mixed", seed=1)
    assert sorted(tiles["classes"][:, 0]) == [2, 3]
    ref = wr.reference(oracle, tiles, res, 0.02)
    assert len(ref["soup"][2]) > 40
    check_all(ops, tiles, ref, 0.02, res, f"zeros {axis}")


def test_an_empty_table(ops):
    tiles = dict(coords=np.zeros((0, 3), np.int32), classes=np.zeros((0, 3), np.uint8), words=np.zeros((0, 4), np.uint32),
                 at=np.zeros((0, 3), np.uint64), arena=None, volume=None)
    for kw in ({}, dict(weld=True), dict(colors=True), dict(weld=True, colors=True, min_triangles=5)):
        got = ops.mesh_tiles(tiles, 0.01, (0.0, 0.0, 0.0), **kw)
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 4)
        assert len(got) == (4 if kw.get("colors") else 3)


def test_component_filter_on_the_welded_tiles(oracle, ops):
    from tests import components_reference as cr
    keep = np.random.default_rng(11).integers(0, 3, 60) != 0
    tiles, ref, vox = fused_case(oracle, "mixed", keep=keep, tag="holes")
    welded = weld(*ref["soup"], ref["keys"])
    want = cr.filter_mesh(*welded, min_triangles=40)
    assert 0 < len(want[2]) < len(welded[2])
    same(ops.mesh_tiles(tiles, vox, wr.half_of(RES), weld=True, min_triangles=40), want)


def test_refusals_with_device_memory(oracle, ops):
    """Every refusal the host can see, this time with real device pointers, and EMF_E_LIMIT at coordinate 2^19."""
    from emfusion_amd import _lib
    tiles, ref, vox = fused_case(oracle, "literal")
    half = wr.half_of(RES)

    def code(**change):
        t = dict(tiles, **change)
        with pytest.raises(_lib.EmfHipError) as e:
            ops.mesh_tiles(t, vox, half)
        return e.value.code

    k = tiles["classes"].copy()
    k[7, 1] = 4
    assert code(classes=k) == -4
    c = tiles["coords"].copy()
    c[[3, 4]] = c[[4, 3]]
    assert code(coords=c) == -4                                   # unsorted
    c = tiles["coords"].copy()
    c[4] = c[3]
    assert code(coords=c) == -4                                   # repeated
    nb = np.full((60, 7), -1, np.int32)
    nb[59, 6] = 60
    assert code(neighbours=nb) == -4                              # a neighbour index >= n
    assert code(arena=None) == -1                                 # literals without an arena
    c = tiles["coords"].copy()
    c[:, 0] += (1 << 19) // 32                                    # the last tile in x starts at voxel 2^19
    assert code(coords=c) == -5
    c[:, 0] -= 1                                                  # one tile less: inside, and the same mesh elsewhere
    got = ops.mesh_tiles(dict(tiles, coords=c), vox, half)
    assert got[2].tobytes() == ref["soup"][2].tobytes() and len(got[0]) == len(ref["soup"][0])
    # a misaligned arena: the entry itself, with the uploaded arena's address moved by 8 bytes
    L = _lib.load()
    arena = ops.DeviceArray.from_numpy(tiles["arena"])
    table = ops.mesh_tile_table(tiles["coords"], tiles["classes"], tiles["words"], tiles["at"])
    d_table = ops.DeviceArray.from_numpy(np.frombuffer(table, np.uint8).copy())
    scratch = ops.DeviceArray.zeros((3 * 61,), np.uint32)
    src = _lib.EmfMeshTilesSource(arena=arena.ptr + 8, arena_units=arena.nbytes // 8192 - 1)
    assert L.emf_hip_meshTilesCount(C.c_void_p(d_table.ptr), C.cast(table, C.c_void_p), 60, C.byref(src),
                                    C.c_void_p(scratch.ptr), C.c_void_p(scratch.ptr), None) == -4


def test_a_literal_outside_the_arena_skips_its_tile(oracle, ops):
    """What only the device sees: the tile is skipped by the bounds compare -- as an owner and as a neighbour -- and
    the mesh is that of the set without it."""
    tiles, ref, vox = fused_case(oracle, "literal")
    units = len(tiles["arena"])
    victim = int(np.flatnonzero(tiles["classes"][:, 0] == 2)[20])
    at = tiles["at"].copy()
    at[victim, 0] = units                                          # one past the end
    keep = np.ones(60, bool)
    keep[victim] = False
    t, w, _ = wv.fused(oracle, RES)
    without = wr.cut(t, w, offset=OFFSET, mode="literal", keep=keep)
    want = wr.reference(oracle, without, RES, vox)
    assert 0 < len(want["soup"][2]) < len(ref["soup"][2])
    got = ops.mesh_tiles(dict(tiles, at=at), vox, wr.half_of(RES), keys=True)
    same(got[:3], want["soup"], "skipped")
    assert np.array_equal(got[3], want["keys"])
    # the same for an in-place tile whose offset leaves the volume
    tiles3, _, _ = fused_case(oracle, "inplace")
    at = tiles3["at"].copy()
    at[victim] = t.size - 7 * 64 * 48 - 7 * 64 - 28                # its last voxels lie past the end
    got = ops.mesh_tiles(dict(tiles3, at=at), vox, wr.half_of(RES), keys=True)
    same(got[:3], want["soup"], "skipped in place")
