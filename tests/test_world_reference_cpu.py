"""CPU checks of what the world-mesh tests stand on (tests/world_reference.py): the canonical order is
a permutation of the oracle's soup, symmetric padding leaves the oracle's positions and triangles byte-identical, the
lattice keys are one per grid edge, and the new entries refuse malformed tables without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import world_reference as wr
from tests import world_volumes as wv

RES = (64, 48, 40)
OFFSET = (-1, -3, 2)


@pytest.fixture(scope="module")
def fused_ref(oracle):
    t, w, vox = wv.fused(oracle, RES)
    tiles = wr.cut(t, w, offset=OFFSET)
    return t, w, vox, tiles, wr.reference(oracle, tiles, RES, vox)


def rows(a):
    """The rows of a 2-d array as a sorted multiset of byte strings."""
    return sorted(np.ascontiguousarray(r).tobytes() for r in a)


def test_canonical_is_a_permutation_of_the_oracle_soup(oracle, fused_ref):
    t, w, vox, tiles, ref = fused_ref
    bt, bw, _ = ref["box"]
    v, n, tr = oracle.marching_cubes(bt, bw, vox)
    cv, cn, ct = ref["soup"]
    assert len(cv) == 18119 and len(ct) == 9051
    assert rows(np.concatenate([v, n], 1)) == rows(np.concatenate([cv, cn], 1))
    assert ct.shape == tr.shape and (ct[:, 0] == 3).all()
    # every triangle still refers to the same positions, and the triangles are the oracle's as a multiset
    assert rows(v[tr[:, 1:]].reshape(len(tr), 9)) == rows(cv[ct[:, 1:]].reshape(len(ct), 9))
    # the order is the canonical one: tiles ascending in (z, y, x), anchors ascending inside a tile
    tc, la = ref["cubes"]
    key = np.concatenate([tc[:, ::-1], la[:, ::-1]], 1)
    assert all(tuple(a) <= tuple(b) for a, b in zip(key[:-1], key[1:]))
    # a cube's triangles refer to the cube's own vertices
    assert np.array_equal(key[ct[:, 1]], key[ct[:, 2]]) and np.array_equal(key[ct[:, 1]], key[ct[:, 3]])
    # the figures the GPU tests rely on: surface cubes, and those that straddle a tile face / a y-z tile edge
    cub = np.unique(np.concatenate([tc, la], 1), axis=0)
    assert len(cub) == 4533
    assert ((cub[:, 3] == 31).sum(), (cub[:, 4] == 7).sum(), (cub[:, 5] == 7).sum()) == (74, 492, 460)
    assert ((cub[:, 4] == 7) & (cub[:, 5] == 7)).sum() == 56


@pytest.mark.parametrize("name, changed", [("fused_64x48x40", 41), ("fused_96x40x32", 129), ("random_sign", 8192)])
def test_symmetric_padding_leaves_positions_and_triangles_identical(oracle, name, changed):
    if name == "random_sign":
        t, w, vox = wv.random_sign()
    else:
        t, w, vox = wv.fused(oracle, tuple(int(s) for s in name[6:].split("x")))
    v, n, tr = oracle.marching_cubes(t, w, vox)
    pad = ((8, 8), (8, 8), (32, 32))
    pv, pn, ptr = oracle.marching_cubes(np.pad(t, pad), np.pad(w, pad), vox)
    assert v.tobytes() == pv.tobytes() and tr.tobytes() == ptr.tobytes()
    # the normals change only where the unpadded volume's forward differences were cut off: at its last planes
    differ = (n != pn).any(axis=1)
    assert differ.sum() == changed
    z, y, x, e = wr.soup_cubes(t, w)
    lo = np.array([np.maximum(wr.CORNERS[a], wr.CORNERS[b]) for a, b in wr.EDGES])
    last = (x + lo[e, 0] == t.shape[2] - 1) | (y + lo[e, 1] == t.shape[1] - 1) | (z + lo[e, 2] == t.shape[0] - 1)
    assert not (differ & ~last).any()


def test_lattice_keys_are_one_per_grid_edge(oracle, fused_ref):
    t, w, vox, tiles, ref = fused_ref
    bt, bw, _ = ref["box"]
    cubes = wr.soup_cubes(bt, bw)
    keys = wr.lattice_keys(cubes, ref["pad"])
    assert keys.dtype == np.uint64 and not (keys == np.uint64(0xffffffffffffffff)).any() and keys.max() < 1 << 62
    # the same partition of the soup as the dense volume's keys of the box, and negative coordinates occur
    from tests.weld_reference import edge_keys
    dense = edge_keys(bt, bw)
    _, a = np.unique(keys, return_inverse=True)
    _, b = np.unique(dense, return_inverse=True)
    assert len(np.unique(keys)) == len(np.unique(dense)) == len(np.unique(np.stack([a.ravel(), b.ravel()], 1), axis=0))
    x = (keys // np.uint64(3)) & np.uint64((1 << 20) - 1)
    assert (x < wr.BIAS).any() and (x >= wr.BIAS).any()
    assert np.array_equal(np.sort(ref["keys"]), np.sort(keys))


# ---- the entries refuse what the host can see, without a device ------------------------------------------------------

def table_of(coords, classes=None, at=None, neighbours=None):
    from emfusion_amd import ops
    n = len(coords)
    classes = np.ones((n, 3), np.uint8) if classes is None else classes
    return ops.mesh_tile_table(coords, classes, np.ones((n, 4), np.uint32), np.zeros((n, 3), np.uint64) if at is None else at,
                               neighbours)


def count(table, n, src=None, dev=16, host=True, scratch=16, counts=16):
    from emfusion_amd import _lib
    L = _lib.load()
    src = _lib.EmfMeshTilesSource() if src is None else src
    return L.emf_hip_meshTilesCount(C.c_void_p(dev), C.cast(table, C.c_void_p) if host else None, n, C.byref(src),
                                    C.c_void_p(scratch), C.c_void_p(counts), None)


def test_entries_refuse_null_and_malformed_tables_before_any_launch():
    from emfusion_amd import _lib
    L = _lib.load()
    NULL, ARG, LIMIT = -1, -4, -5
    good = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    t = table_of(good)
    assert L.emf_hip_meshTilesScratchBytes(3) == 44 and L.emf_hip_meshTilesScratchBytes((1 << 17) + 1) == 0
    assert count(t, 3, dev=0) == NULL and b"tiles_dev is NULL" in L.emf_hip_last_error_string()
    assert count(t, 3, host=False) == NULL
    assert count(t, 3, scratch=0) == NULL
    assert count(t, 3, counts=0) == NULL
    assert L.emf_hip_meshTilesCount(C.c_void_p(16), C.cast(t, C.c_void_p), 3, None, C.c_void_p(16), C.c_void_p(16),
                                    None) == NULL
    assert count(t, (1 << 17) + 1) == LIMIT
    # a class above 3
    k = np.ones((3, 3), np.uint8)
    k[1, 2] = 4
    assert count(table_of(good, classes=k), 3) == ARG and b"class 4 of tile 1" in L.emf_hip_last_error_string()
    # literals without an arena, in-place tiles without a volume
    k[1, 2] = 2
    assert count(table_of(good, classes=k), 3) == NULL
    k[1, 2] = 3
    assert count(table_of(good, classes=k), 3) == NULL
    # an unsorted and a repeated coordinate
    assert count(table_of([(1, 0, 0), (0, 0, 0)]), 2) == ARG
    assert count(table_of([(0, 1, 0), (5, 0, 0)]), 2) == ARG
    assert count(table_of([(0, 0, 0), (0, 0, 0)]), 2) == ARG and b"not after" in L.emf_hip_last_error_string()
    # a neighbour index outside the table, and one that names a tile somewhere else
    nb = np.full((3, 7), -1, np.int32)
    nb[0, 0] = 3
    assert count(table_of(good, neighbours=nb), 3) == ARG
    nb[0, 0] = -2
    assert count(table_of(good, neighbours=nb), 3) == ARG
    nb[0, 0] = 2
    assert count(table_of(good, neighbours=nb), 3) == ARG and b"another coordinate" in L.emf_hip_last_error_string()
    # a misaligned arena, volume or stride
    src = _lib.EmfMeshTilesSource(arena=4096 + 8, arena_units=4)
    assert count(t, 3, src) == ARG and b"arena" in L.emf_hip_last_error_string()
    src = _lib.EmfMeshTilesSource(tsdf=4096, weights=4096 + 4, volume_elements=1 << 20, row_stride=64, plane_stride=4096)
    assert count(t, 3, src) == ARG
    src = _lib.EmfMeshTilesSource(tsdf=4096, weights=8192, volume_elements=1 << 20, row_stride=66, plane_stride=4096)
    assert count(t, 3, src) == ARG and b"strides" in L.emf_hip_last_error_string()
    # lattice voxel coordinates outside +-2^19: the first tile beyond on every axis, the last one inside is accepted
    # as far as the host checks go (nothing is launched here: the next refusal is the one that answers)
    for axis, ext in enumerate((32, 8, 8)):
        for tile in ((1 << 19) // ext, -(1 << 19) // ext - 1):
            c = [0, 0, 0]
            c[axis] = tile
            assert count(table_of([tuple(c)]), 1) == LIMIT, (axis, tile)
    # the other entries check their pointers too
    s = _lib.EmfMeshTilesSource()
    p = C.c_void_p(16)
    half = (C.c_float * 3)(0, 0, 0)
    assert L.emf_hip_meshTilesEmit(p, 3, C.byref(s), half, 0.01, p, None, p, p, None) == NULL
    assert L.emf_hip_meshTilesEmit(p, 3, C.byref(s), None, 0.01, p, p, p, p, None) == NULL
    assert L.emf_hip_meshTilesEmit(p, 3, C.byref(s), half, 0.0, p, p, p, p, None) == ARG
    assert L.emf_hip_meshTilesColors(p, 3, C.byref(s), p, None, None) == NULL
    assert L.emf_hip_meshTilesEdgeKeys(p, 3, C.byref(s), None, p, None) == NULL
    assert L.emf_hip_meshTilesEdgeKeys(None, 3, C.byref(s), p, p, None) == NULL
