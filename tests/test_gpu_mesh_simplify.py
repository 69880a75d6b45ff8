"""Simplified meshes on the device (include/emf_hip.h "Simplified meshes"): ops.simplify_mesh and the
simplify= keyword of ops.extract_mesh / extract_meshes / mesh_tiles, byte for byte against the numpy restatement
(tests/simplify_reference.py), at the smallest shapes at which the table, the run aggregation of the accumulate kernel,
the three scans and the refusals can go wrong.  The switch through Fusion, the result files and the two apps:
tests/test_gpu_simplify_pipeline.py."""
import numpy as np
import pytest

from tests import mesh_volumes as MV
from tests.components_reference import filter_mesh, welded_case
from tests.parity_util import to_dev
from tests.simplify_reference import Refused, simplify, simplify_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k)


def check(ops, v, n, t, c=None, what="", **kw):
    """ops.simplify_mesh against the restatement, arrays and counts; returns the restatement's (arrays, stats)."""
    want, wst = simplify(v, n, t, c, stats=True, **kw)
    got, gst = ops.simplify_mesh(v, n, t, colors=c, stats=True, **kw)
    same(got, want, what)
    for key in ("vertices_in", "triangles_in", "vertices_out", "triangles_out", "clusters"):
        assert gst[key].tolist() == [wst[key]], (what, key, gst[key], wst[key])
    return want, wst


def tris_of(corners):
    c = np.asarray(corners, np.int64).reshape(-1, 3)
    return np.concatenate([np.full((len(c), 1), 3), c], axis=1).astype(np.int32)


def strip(nv):
    """nv vertices on a folded 512 x 512 lattice of 1 cm with a seeded jitter, nv - 2 triangles (i, i + 1, i + 2), random
    normals (a few hostile) and colours."""
    rng = np.random.default_rng([7, nv])
    i = np.arange(nv)
    v = np.stack([i % 512, (i // 512) % 512, i // 262144], axis=1) * 0.01 + rng.uniform(-0.004, 0.004, (nv, 3)) - 1.3
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    n[rng.uniform(size=(nv, 3)) < 0.01] = np.float32(np.nan)
    n[rng.uniform(size=(nv, 3)) < 0.01] = np.float32(1e30)
    c = rng.integers(0, 256, (nv, 3), dtype=np.uint8)
    k = np.arange(max(nv - 2, 0))
    return v.astype(np.float32), n, tris_of(np.stack([k, k + 1, k + 2], axis=1)), c


# ---- the shapes that steer the kernels ------------------------------------------------------------------------------

def test_nothing_in_nothing_out(ops):
    e3, e4 = np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32)
    (sv, sn, st), stats = ops.simplify_mesh(e3, e3, e4, cell=0.1, stats=True)
    assert sv.shape == (0, 3) and sn.shape == (0, 3) and st.shape == (0, 4) and st.dtype == np.int32
    assert stats["vertices_out"].tolist() == [0] and stats["clusters"].tolist() == [0]
    out = ops.simplify_mesh(e3, e3, e4, colors=np.zeros((0, 3), np.uint8), cell=0.1)
    assert len(out) == 4 and out[3].shape == (0, 3) and out[3].dtype == np.uint8
    # vertices no triangle uses: clusters met, none referenced; a pass-through keeps them
    v, n, _, c = strip(300)
    want, wst = check(ops, v, n, e4, c, cell=0.025)
    assert want[0].shape == (0, 3) and want[2].shape == (0, 4) and 100 < wst["clusters"] < 300
    same(ops.simplify_mesh(v, n, e4, colors=c, cell=0.0), (v, n, e4, c))


def test_a_single_triangle(ops):
    v = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.6, 0.1]], np.float32)
    t = tris_of([(2, 0, 1)])
    same(check(ops, v, -v, t, cell=0.25)[0], (v, -v, t))
    assert check(ops, v, -v, t, cell=0.5)[0][2].shape == (0, 4)      # two corners share a cell: the triangle collapses
    assert check(ops, v, -v, t, cell=1.0)[0][0].shape == (0, 3)


def test_all_vertices_in_one_cell(ops):
    """Maximal contention on one table slot and one set of accumulators: 20 000 members of one cluster.  Alone they
    collapse to nothing; with two vertices outside, the triangles that reach them keep the cluster's mean."""
    rng = np.random.default_rng(20_000)
    nv = 20_000
    v = rng.uniform(0.01, 0.99, (nv, 3)).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    c = rng.integers(0, 256, (nv, 3), dtype=np.uint8)
    k = np.arange(nv - 2)
    t = tris_of(np.stack([k, k + 1, k + 2], axis=1))
    want, wst = check(ops, v, n, t, c, cell=1.0)
    assert want[0].shape == (0, 3) and want[2].shape == (0, 4) and wst["clusters"] == 1
    v2 = np.concatenate([v, [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]]).astype(np.float32)
    n2, c2 = np.concatenate([n, n[:2]]), np.concatenate([c, c[:2]])
    t2 = np.concatenate([t, tris_of(np.stack([k, np.full(nv - 2, nv), np.full(nv - 2, nv + 1)], axis=1))])
    want, wst = check(ops, v2, n2, t2, c2, cell=1.0)
    assert len(want[0]) == 3 and len(want[2]) == nv - 2 and wst["clusters"] == 3
    assert np.all(np.abs(want[0][0] - 0.5) < 0.02)                    # the mean of 20 000 uniform positions
    # the members in another order: the same sums
    order = rng.permutation(nv)
    back = np.argsort(order)
    t3 = t2.copy()
    t3[:, 1:] = np.where(t2[:, 1:] < nv, back[np.minimum(t2[:, 1:], nv - 1)], t2[:, 1:])
    v3, n3, c3 = (np.concatenate([a[order], a[nv:]]) for a in (v2, n2, c2))
    again, _ = check(ops, v3, n3, t3, c3, cell=1.0)
    same(again, want)


def test_one_vertex_per_cell_is_the_identity(ops):
    g = np.stack(np.meshgrid(np.arange(-9, 9), np.arange(-9, 9), np.arange(-3, 3), indexing="ij"), axis=-1).reshape(-1, 3)
    v = ((g + 0.5) * 0.125).astype(np.float32)
    rng = np.random.default_rng(3)
    v = v[rng.permutation(len(v))]
    n = rng.standard_normal(v.shape).astype(np.float32)
    n[5] = [np.nan, np.inf, 1e30]                                      # kept bit for bit: a cluster of one sums nothing
    c = rng.integers(0, 256, v.shape, dtype=np.uint8)
    k = rng.permutation(len(v) - 2)
    t = tris_of(np.stack([k, k + 1, k + 2], axis=1))
    same(check(ops, v, n, t, c, cell=0.125)[0], (v, n, t, c))


@pytest.mark.parametrize("nv", [255, 256, 257, 258, 259, 262_145, 262_147])
def test_counts_around_the_scan_blocks(ops, nv):
    """Vertex counts and (two less) triangle counts of 255, 256, 257 -- the flag / rank workgroup -- and of 262 145: one
    past what the first round of the 1024-thread sums workgroup covers."""
    v, n, t, c = strip(nv)
    want, wst = check(ops, v, n, t, c, cell=0.025, what=nv)
    assert 0 < len(want[0]) < nv and 0 < len(want[2]) < len(t)
    assert wst["clusters"] >= len(want[0])
    if nv <= 259:
        check(ops, v, n, t, cell=0.0151, origin=(0.3, 0.3, 0.3), what=nv)                      # no colours
        same(check(ops, v, n, t, c, cell=0.001, what=nv)[0], (v, n, t, c))                     # every vertex alone


def test_negative_coordinates_cell_faces_and_an_origin(ops):
    """Vertices exactly on cell faces (multiples of the cell, both signs, -0.0 among them) belong to the cell above;
    negative coordinates floor; a non-zero origin moves the faces."""
    k = np.arange(-8, 9)
    g = np.stack(np.meshgrid(k, k, [-1, 0, 1], indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(4)
    on = (g * 0.25).astype(np.float32)
    on[rng.uniform(size=on.shape) < 0.2] *= np.float32(-1.0)           # also -0.0
    off = (on + rng.choice(np.array([-2.0 ** -20, 2.0 ** -20, 0.1], np.float32), on.shape)).astype(np.float32)
    v = np.concatenate([on, off])
    v = v[rng.permutation(len(v))]
    n = rng.standard_normal(v.shape).astype(np.float32)
    c = rng.integers(0, 256, v.shape, dtype=np.uint8)
    t = tris_of(rng.integers(0, len(v), (3000, 3)))
    for cell, origin in ((0.25, (0, 0, 0)), (0.5, (0, 0, 0)), (0.5, (0.1, -0.2, 0.3)), (0.3, (-7.0, 5.5, 0.25)),
                         (0.25, (0.25, -0.25, 1024.0))):
        want, wst = check(ops, v, n, t, c, cell=cell, origin=origin, what=(cell, origin))
        assert 0 < len(want[2]) < len(t) and 8 <= wst["clusters"] < len(v)
    a = simplify(v, n, t, c, cell=0.5)
    b = simplify(v, n, t, c, cell=0.5, origin=(0.1, -0.2, 0.3))
    assert len(a[0]) != len(b[0]) or a[0].tobytes() != b[0].tobytes()


def test_hostile_normals_count_as_zero(ops):
    v, n, t, c = strip(4000)
    n[::3, 0] = np.nan
    n[1::3, 1] = 1e30
    n[2::3, 2] = -np.inf
    n[5::7] = [1023.9999, -1024.0, 1024.0]
    want, _ = check(ops, v, n, t, c, cell=0.03)
    assert len(want[0]) > 100


def test_a_table_of_three_models_two_equal_one_empty(ops):
    v, n, t, c = strip(700)
    tb, vb = [0, len(t), len(t), 2 * len(t)], [0, 700, 700, 1400]
    V, N, T, Cc = np.concatenate([v, v]), np.concatenate([n, n]), np.concatenate([t, t]), np.concatenate([c, c])
    for colours in (Cc, None):
        for cells in (0.025, [0.025, 0.05, 0.0], [0.0, 0.0, 0.06], [-1.0, 1.0, 0.0]):
            got, st = ops.simplify_mesh(V, N, T, colors=colours, cell=cells, tri_bases=tb, vertex_bases=vb, stats=True)
            want = simplify_table(V, N, T, colours, cells=cells, tri_bases=tb, vertex_bases=vb)
            assert len(got) == 3
            for k in range(3):
                same(got[k], want[k], (cells, k))
            assert got[1][0].shape == (0, 3) and got[1][2].shape == (0, 4)
            assert st["vertices_out"].tolist() == [len(w[0]) for w in want]
            assert st["triangles_out"].tolist() == [len(w[2]) for w in want]
            assert st["vertices_in"].tolist() == [700, 0, 700] and st["clusters"][1] == 0
    got = ops.simplify_mesh(V, N, T, colors=Cc, cell=0.025, tri_bases=tb, vertex_bases=vb)
    same(got[0], got[2])                                               # equal arrays, equal slices, neither merged
    same(got[0], simplify(v, n, t, c, cell=0.025))
    same(ops.simplify_mesh(V, N, T, colors=Cc, cell=[0.0, 0.0, 0.0], tri_bases=tb, vertex_bases=vb)[2], (v, n, t, c))


def test_two_runs_give_equal_bytes(ops):
    v, n, t, c = strip(50_000)
    a = ops.simplify_mesh(v, n, t, colors=c, cell=0.035)
    b = ops.simplify_mesh(v, n, t, colors=c, cell=0.035)
    same(a, b)
    assert 1000 < len(a[0]) < 10_000


# ---- refusals -------------------------------------------------------------------------------------------------------

def refused(ops, *args, **kw):
    from emfusion_amd import _lib
    with pytest.raises(_lib.EmfHipError) as e:
        ops.simplify_mesh(*args, **kw)
    return e.value


def test_refusals_report_their_codes(ops):
    v, n, t, c = strip(1000)
    assert refused(ops, v, n, t, cell=1e-5).code == -5                 # a cell coordinate beyond 2^15
    assert refused(ops, v, n, t, cell=1.0, origin=(0, 40000.0, 0)).code == -5
    for bad in (np.nan, np.inf, 1024.0, -1024.0):
        w = v.copy()
        w[777, 1] = bad
        assert refused(ops, w, n, t, cell=0.025).code == -5, bad
        with pytest.raises(Refused) as e:
            simplify(w, n, t, cell=0.025)
        assert e.value.code == -5
        same(ops.simplify_mesh(w, n, t, cell=0.0), (w, n, t))           # a pass-through looks at no position
    w = v.copy()
    w[777, 1] = 1023.9999
    check(ops, w, n, t, c, cell=0.05)


def test_a_triangle_index_out_of_range_is_dropped_and_reported(ops):
    v, n, t, c = strip(1000)
    for bad in (-1, 1000, 2 ** 31 - 1, -2 ** 31):
        u = t.copy()
        u[[0, 500, 997], [1, 2, 3]] = bad
        for cell in (0.025, 0.0):
            err = refused(ops, v, n, u, colors=c, cell=cell)
            assert err.code == -4, (bad, cell)
            with pytest.raises(Refused) as e:
                simplify(v, n, u, c, cell=cell)
            assert e.value.code == -4
            same(err.partial, e.value.partial, (bad, cell))
            same(err.partial, simplify(v, n, np.delete(u, [0, 500, 997], axis=0), c, cell=cell))
    # in a table the range is the model's own: an index that another model would hold is out of range too
    tb, vb = [0, len(t), 2 * len(t)], [0, 1000, 2000]
    u = np.concatenate([t, t])
    u[3, 2] = 1000
    err = refused(ops, np.concatenate([v, v]), np.concatenate([n, n]), u, cell=0.025, tri_bases=tb, vertex_bases=vb)
    assert err.code == -4
    same(err.partial[1], simplify(v, n, t, cell=0.025))
    same(err.partial[0], simplify(v, n, np.delete(t, 3, axis=0), cell=0.025))


def test_aliased_output_is_rejected_before_any_launch(ops):
    import ctypes as C

    from emfusion_amd import _lib
    L = _lib.load()
    a, b = to_dev(np.zeros(8192, np.uint64)), to_dev(np.zeros(8192, np.uint64))
    p, q = C.c_void_p(a.ptr), C.c_void_p(b.ptr)
    emit = lambda *args: L.emf_hip_meshSimplifyEmit(p, 8, 1, None, None, 1, *args, None)
    assert emit(q, q, None, q, q, p, None, p) == -4
    assert emit(q, q, None, q, p, q, None, p) == -4
    assert emit(q, q, None, q, p, p, None, q) == -4
    assert emit(q, q, q, q, p, p, q, p) == -4
    assert emit(q, q, q, q, p, p, None, p) == -1
    assert not a.numpy().any() and not b.numpy().any()


# ---- through the extractors -----------------------------------------------------------------------------------------

def dev_or_none(a):
    return None if a is None else to_dev(a)


@pytest.mark.parametrize("voxels", [2.0, 3.5])
def test_three_noisy_frames_sphere_through_extract_mesh(oracle, ops, voxels):
    t, w, fg, vox, ref = welded_case(oracle, "fused")
    cell = np.float32(voxels * vox)
    args = (to_dev(t), to_dev(w), vox)
    got = ops.extract_mesh(*args, weld=True, simplify=cell)
    want = simplify(*ref, cell=cell)
    same(got, want, voxels)
    assert 0 < len(want[0]) < len(ref[0]) / 3
    same(ops.simplify_mesh(*ref, cell=cell), want, voxels)
    filtered = filter_mesh(*ref, min_triangles=8)
    got = ops.extract_mesh(*args, weld=True, min_triangles=8, simplify=cell)
    same(got, simplify(*filtered, cell=cell), (voxels, "filtered"))
    assert len(filtered[0]) < len(ref[0]) and len(got[0]) <= len(want[0])
    same(ops.extract_mesh(*args, weld=True, simplify=0.0), ref)        # off: the welded mesh
    with pytest.raises(ValueError):
        ops.extract_mesh(*args, simplify=cell)


def test_coloured_masked_volume_through_extract_mesh(oracle, ops):
    t, w, fg, vox, ref = welded_case(oracle, "fused_masked")
    rng = np.random.default_rng(8)
    col = rng.integers(0, 65281, t.shape + (4,), dtype=np.uint16)
    col[..., 3] = rng.integers(0, 3, t.shape) * 128
    args = (to_dev(t), to_dev(w), vox)
    welded = ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col), weld=True)
    same(welded[:3], ref)
    for voxels in (2.0, 3.5):
        cell = np.float32(voxels * vox)
        got = ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col), weld=True, simplify=cell)
        same(got, simplify(*welded[:3], welded[3], cell=cell), voxels)
        assert len(np.unique(got[3], axis=0)) > 20


DENSE_AND_SPARSE = [("dense", (74, 90, 66), False), ("dense", (9, 96, 130), True), ("sparse", (256, 256, 255), False)]


@pytest.mark.parametrize("case", DENSE_AND_SPARSE, ids=lambda c: f"{c[0]}-{MV.name_of(c[1])}{'-masked' if c[2] else ''}")
def test_dense_and_sparse_volumes_through_extract_mesh(ops, case):
    """The restatement on the device's own welded (and filtered) mesh, which tests/test_gpu_mesh_shapes.py holds to the
    oracle: hundreds of thousands of vertices, tens of thousands of fragments."""
    kind, shape, masked = case
    t, w, fg, vox = MV.dense(shape) if kind == "dense" else MV.sparse(shape)
    args = (to_dev(t), to_dev(w), vox)
    kw = dict(fg_mask=to_dev(fg) if masked else None, weld=True)
    for mn in (0, 8):
        welded = ops.extract_mesh(*args, min_triangles=mn, **kw)
        assert len(welded[0]) > 1000
        for voxels in (2.0, 3.5):
            cell = np.float32(voxels * vox)
            want = simplify(*welded, cell=cell)
            same(ops.extract_mesh(*args, min_triangles=mn, simplify=cell, **kw), want, (mn, voxels))
            assert len(want[0]) < len(welded[0]) / 2


def test_table_through_extract_meshes(oracle, ops):
    names = ["sphere", "fused", "random_sign", "fused"]
    cases = [welded_case(oracle, name) for name in names]
    vols = [dict(tsdf=to_dev(c[0]), weights=to_dev(c[1]), voxel_size=c[3], fg_mask=dev_or_none(c[2])) for c in cases]
    e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32))
    z = np.zeros((8, 8, 8), np.float32)
    vols.insert(2, dict(tsdf=to_dev(z), weights=to_dev(z), voxel_size=0.01, fg_mask=None))
    refs = [c[4] for c in cases]
    refs.insert(2, e)
    cells = [0.1, 0.032, 0.02, 0.0, 0.056]
    got = ops.extract_meshes(vols, weld=True, simplify=cells)
    for k in range(5):
        same(got[k], simplify(*refs[k], cell=cells[k]), k)
    same(got[3], refs[3])
    got = ops.extract_meshes(vols, weld=True, simplify=0.04, min_triangles=8)
    for k in range(5):
        same(got[k], simplify(*filter_mesh(*refs[k], min_triangles=8), cell=0.04), (k, "filtered"))
    same(got[1], got[4])
    plain = ops.extract_meshes(vols, weld=True, simplify=0.0)
    for k in range(5):
        same(plain[k], refs[k], (k, "off"))
    with pytest.raises(ValueError):
        ops.extract_meshes(vols, simplify=0.04)


def test_tiles_through_mesh_tiles(oracle, ops):
    from tests import world_reference as wr
    from tests import world_volumes as wv
    from tests.weld_reference import weld
    res = (64, 48, 40)
    t, w, vox = wv.fused(oracle, res)
    col = wv.colours(t.shape)
    tiles = wr.cut(t, w, col, offset=(-1, -3, 2), mode="mixed", seed=3)
    ref = wr.reference(oracle, tiles, res, vox, with_color=True)
    welded = weld(*ref["soup"], ref["keys"], ref["colours"])
    half = wr.half_of(res)
    cell = np.float32(2.5 * vox)
    want = simplify(*welded[:3], welded[3], cell=cell)
    same(ops.mesh_tiles(tiles, vox, half, weld=True, colors=True, simplify=cell), want)
    assert 0 < len(want[0]) < len(welded[0]) / 3
    same(ops.mesh_tiles(tiles, vox, half, weld=True, simplify=cell), simplify(*welded[:3], cell=cell))
    same(ops.mesh_tiles(tiles, vox, half, weld=True, min_triangles=40, simplify=cell),
         simplify(*filter_mesh(*welded[:3], min_triangles=40), cell=cell))
    with pytest.raises(ValueError):
        ops.mesh_tiles(tiles, vox, half, simplify=cell)
