"""The inputs of tests/test_gpu_mesh_shapes.py, checked without a GPU: the shapes take the branches of meshing.hip they
are listed for (plan()'s arithmetic restated in tests/mesh_volumes.py), and the fills leave no chunk and no counting
workgroup without surface -- a kernel that skips, shifts or misplaces any of them then writes a different mesh.  The
oracle and the numpy restatements agree on what the soup of these volumes is."""
import numpy as np
import pytest

from tests import mesh_volumes as MV
from tests.mesh_color_reference import vertex_colours
from tests.weld_reference import edge_keys

BIG_DENSE = [s for s in MV.DENSE if s[0] * s[1] * s[2] >= 10 ** 5]


def ids(shapes):
    return [MV.name_of(s) for s in shapes]


def test_shapes_take_the_branches_they_are_listed_for():
    L = {s: MV.layout(s) for s in MV.DENSE + MV.SPARSE}
    assert all(L[s]["per"] == 8 for s in MV.DENSE + [MV.SPARSE[0], MV.SPARSE[3]])
    assert all(L[s]["per"] == 32 for s in MV.SPARSE[1:3])
    assert 256 * 256 * 256 == MV.LARGE_VOXELS and 256 * 256 * 255 < MV.LARGE_VOXELS      # the threshold and its neighbour
    assert 273 * 241 * 255 == MV.LARGE_VOXELS - 1                                        # one voxel below it
    assert all(s[0] < 6 and L[s]["wpp"] == 1 for s in MV.THIN)                           # rows of 1 - 4 cubes
    assert [L[s]["wpp"] for s in MV.SLABS] == [1, 1, 6]                                  # (a plane of 130 x 9 is below a span)
    assert [s[0] for s in MV.ROWS] == [63, 64, 65, MV.CHUNK, MV.CHUNK + 1]
    a, b, c = (L[s] for s in MV.BANDS)
    assert (a["wpp"], a["nblocks"], a["nblocks"] % a["wpp"]) == (2, 41, 1)               # a short last row
    assert (b["wpp"], b["band"]) == (3, 1) and 74 % 4 != 0                               # five idle XCD columns
    assert (c["wpp"], c["band"], c["nblocks"]) == (9, 2, 271) and c["grid"] > c["nblocks"]
    d = L[MV.CARRY]
    assert (d["nblocks"], d["scan_passes"], d["chunks"], d["wpp"]) == (1057, 2, 8456, 10) and d["chunks"] > 4096
    e, f, g = (L[s] for s in MV.SPARSE[:3])
    assert (e["nblocks"], e["scan_passes"], e["wpp"], e["band"]) == (8290, 9, 32, 4) and e["chunks"] > 4096
    assert (f["wpp"], f["band"], f["scan_passes"]) == (8, 1, 3)
    assert (g["wpp"], g["band"]) == (11, 2)
    assert max(L[s]["wpp"] for s in MV.DENSE_SMALL) == 9
    # the table of the GPU test: 8- and 32-chunk models in one launch
    assert {L[s]["per"] for s in MV.DENSE_SMALL + [MV.SPARSE[2]]} == {8, 32}


def test_surface_cubes_on_a_known_volume():
    t = np.ones((3, 3, 4), np.float32)
    t[1, 1, 1] = -1                                  # the centre voxel of the 8 cubes around it
    w = np.ones_like(t)
    s = MV.surface_cubes(t, w)
    assert s.shape == t.shape and s[:2, :2, :2].all() and s.sum() == 8
    w[0, 0, 0] = 0                                   # one cube loses a corner
    assert MV.surface_cubes(t, w).sum() == 7
    w[0, 0, 0] = 1e-40                               # a positive denormal is observed
    assert MV.surface_cubes(t, w).sum() == 8
    fg = np.full(t.shape, 2, np.uint8)
    fg[2, 2, 3] = 0                                  # a corner of no cube with both signs
    assert MV.surface_cubes(t, w, fg).sum() == 8
    fg[2, 2, 2] = 0
    assert MV.surface_cubes(t, w, fg).sum() == 7
    t[1, 1, 1] = -0.0                                # -0.0 is not negative
    assert MV.surface_cubes(t, w).sum() == 0
    assert MV.vertices_per_chunk(np.where(t == 0, np.float32(-1), t), w).tolist() == [24]


def check_groups(surface, shape, size):
    """Every run of `size` positions in which a cube is anchored holds a surface cube -- the first and the last too."""
    anchored = MV.per_group(MV.anchors(shape), size) > 0
    have = MV.per_group(surface, size) > 0
    assert anchored[0] and have[0], "the first"
    last = np.flatnonzero(anchored)[-1]
    assert have[last], "the last that holds a cube"
    assert not (anchored & ~have).any(), np.flatnonzero(anchored & ~have)[:8]
    return int(anchored.sum())


@pytest.mark.parametrize("shape", MV.DENSE, ids=ids(MV.DENSE))
def test_dense_fill_leaves_no_chunk_without_surface(shape):
    t, w, fg, vox = MV.dense(shape)
    nx, ny, nz = shape
    assert t.shape == w.shape == fg.shape == (nz, ny, nx) and t.dtype == w.dtype == np.float32 and fg.dtype == np.uint8
    assert not np.isnan(t).any() and np.abs(t).max() <= 1
    for mask in (None, fg):                          # the plain variant and the foreground variant
        n = check_groups(MV.surface_cubes(t, w, mask), shape, MV.CHUNK)
        assert shape != MV.CARRY or n > 4096         # more surface chunks than the emit grid has workgroups
    # the hostile values are there
    if t.size >= 2000:
        bits = t.view(np.uint32)
        for v in (0.0, -0.0, 1e-40, -1e-40, 5e-6, -5e-6, 1.0, -1.0):
            assert (bits == np.float32(v).view(np.uint32)).any(), v
        assert (t[:, :, 1:] == t[:, :, :-1]).sum() > t.size // 1000        # both ends of an x edge equal
        wbits = w.view(np.uint32)
        for v in (0.0, -0.0, -1.0, 1e-40):
            assert (wbits == np.float32(v).view(np.uint32)).any(), v
        assert 0.85 < (w > 0).mean() < 0.95 and w.max() <= 64
        assert set(np.unique(fg).tolist()) == {0, 1, 2, 128, 255} and 0.04 < (fg == 0).mean() < 0.09


@pytest.mark.parametrize("shape", BIG_DENSE, ids=ids(BIG_DENSE))
def test_big_dense_fill_shows_every_class_and_a_full_chunk(shape):
    t, w, fg, vox = MV.dense(shape)
    for mask in (None, fg):
        complete, cls = MV.cube_classes(t, w, mask)
        seen = np.unique(cls[complete])
        assert len(np.setdiff1d(np.arange(1, 255), seen)) == 0           # all 254 classes that carry surface
        per_chunk = MV.vertices_per_chunk(t, w, mask)
        assert 1500 < per_chunk.max() <= 3024                            # half of what the packed fields must hold


@pytest.mark.parametrize("shape", MV.SPARSE, ids=ids(MV.SPARSE))
def test_sparse_fill_leaves_no_workgroup_without_surface(shape):
    t, w, fg, vox = MV.sparse(shape)
    nx, ny, nz = shape
    assert fg is None and t[0, 0, 0] < 0 and t[nz - 2, ny - 2, nx - 2] < 0
    flat = t.reshape(-1)
    assert (flat[::1009] < 0).all() and (flat < 0).sum() <= len(flat[::1009]) + 1 and (flat[flat > 0] == 0.5).all()
    surface = MV.surface_cubes(t, w)
    check_groups(surface, shape, MV.layout(shape)["span"])
    assert surface[0, 0, 0] and surface[nz - 2, ny - 2, nx - 2]            # the first cube and the last
    assert 10 ** 5 < MV.vertices_per_chunk(t, w).sum() < 10 ** 6


@pytest.mark.parametrize("shape", MV.DENSE_SMALL, ids=ids(MV.DENSE_SMALL))
def test_oracle_and_restatement_agree_on_the_soup(oracle, shape):
    t, w, fg, vox = MV.dense(shape)
    for mask in (None, fg):
        kw = {} if mask is None else dict(fg=mask)
        v, n, tri = oracle.marching_cubes(t, w, vox, **kw)
        assert len(v) == len(edge_keys(t, w, mask)) == MV.vertices_per_chunk(t, w, mask).sum() > 0
        assert tri[:, 1:].min() == 0 and tri[:, 1:].max() == len(v) - 1


def test_colour_restatement_on_known_volumes():
    t, w, fg, vox = MV.dense((5, 3, 70))
    n = len(edge_keys(t, w, fg))
    col = np.zeros(t.shape + (4,), np.uint16)
    col[...] = (200 * 256 + 77, 3 * 256 + 128, 255 * 256, 1)              # 200.3 -> 200, 3.5 -> 4 (half to even), 255
    c = vertex_colours(t, w, col, fg)
    assert c.shape == (n, 3) and c.dtype == np.uint8 and (c == np.array([200, 4, 255], np.uint8)).all()
    assert not vertex_colours(t, w, None, fg).any() and len(vertex_colours(t, w, None, fg)) == n
    # every other x plane uncoloured: an edge with one coloured end takes that end's colour, one with none is black
    col[:, :, 0::2, 3] = 0
    col[:, :, 0::2, :3] = 999                                             # must not leak
    kinds = {tuple(r) for r in np.unique(vertex_colours(t, w, col, fg), axis=0).tolist()}
    assert kinds == {(200, 4, 255), (0, 0, 0)}
    # between two coloured ends: a single cube, the vertex a quarter of the way from 0 to 100 levels
    t = np.array([[[-1, 3], [1, 1]], [[1, 1], [1, 1]]], np.float32)
    col = np.zeros((2, 2, 2, 4), np.uint16)
    col[..., 3] = 1
    col[0, 0, 1, :3] = 100 * 256
    c = vertex_colours(t, np.ones_like(t), col)
    assert c.tolist() == [[25, 25, 25], [0, 0, 0], [0, 0, 0]]
    col[0, 0, 0, 3] = 0                                                   # the negative corner uncoloured
    assert vertex_colours(t, np.ones_like(t), col).tolist() == [[100, 100, 100], [0, 0, 0], [0, 0, 0]]
