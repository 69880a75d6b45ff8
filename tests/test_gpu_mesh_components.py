"""Mesh components on the device (include/emf_hip.h "Mesh components"): labels, sizes and the component filter through
ops.extract_mesh / extract_meshes / mesh_components / filter_mesh, byte for byte against the restatement
(tests/components_reference.py) applied to the oracle's welded soup and to synthetic index buffers -- the smallest
shapes at which the union-find, the aggregated count and the scans can go wrong.  The switch through Fusion, the result
files and the two apps: tests/test_gpu_components_pipeline.py.  No test feeds out-of-range indices: that guard is read,
not provoked."""
import numpy as np
import pytest

from tests import weld_volumes as WV
from tests.components_reference import components, filter_mesh, welded_case
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

VOLUMES = ["sphere", "masked_sphere", "zero_plane", "random_sign", "single_cube", "fused", "fused_masked"]
CRITERIA = [(1, False), (8, False), (10 ** 6, False), (0, True), (8, True)]


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def dev_or_none(a):
    return None if a is None else to_dev(a)


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k)


def volume(t, w, fg, vox):
    return dict(tsdf=to_dev(t), weights=to_dev(w), voxel_size=vox, fg_mask=dev_or_none(fg))


@pytest.mark.parametrize("name", VOLUMES)
def test_labels_and_sizes_of_the_welded_volume(oracle, ops, name):
    t, w, fg, vox, ref = welded_case(oracle, name)
    got = ops.extract_mesh(to_dev(t), to_dev(w), vox, fg_mask=dev_or_none(fg), weld=True)
    same(got, ref, name)
    labels, sizes = ops.mesh_components(got[2], len(got[0]))
    same((labels, sizes), components(ref[2], len(ref[0])), name)
    assert sizes.min() >= 1


@pytest.mark.parametrize("name", VOLUMES)
def test_filtered_volume_equals_the_filtered_welded_oracle_soup(oracle, ops, name):
    t, w, fg, vox, ref = welded_case(oracle, name)
    args = (to_dev(t), to_dev(w), vox)
    differs = False
    for mn, largest in CRITERIA:
        want = filter_mesh(*ref, min_triangles=mn, largest_only=largest)
        got = ops.extract_mesh(*args, fg_mask=dev_or_none(fg), weld=True, min_triangles=mn, largest_only=largest)
        same(got, want, (name, mn, largest))
        differs |= len(want[0]) != len(ref[0])
        if mn == 1 and not largest:
            same(got, ref, name)                                     # the identity
        if mn == 10 ** 6:
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 4)
    assert differs
    # filter_mesh on the welded arrays is the same thing
    same(ops.filter_mesh(*ref, min_triangles=8), filter_mesh(*ref, min_triangles=8), name)


def test_filtered_colours(oracle, ops):
    t, w, fg, vox, ref = welded_case(oracle, "fused_masked")
    rng = np.random.default_rng(8)
    col = rng.integers(0, 65281, t.shape + (4,), dtype=np.uint16)
    col[..., 3] = rng.integers(0, 3, t.shape) * 128  # a third of the voxels uncoloured
    args = (to_dev(t), to_dev(w), vox)
    welded = ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col), weld=True)
    same(welded[:3], ref)
    assert len(np.unique(welded[3], axis=0)) > 20
    for mn, largest in ((8, False), (0, True)):
        got = ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col), weld=True, min_triangles=mn,
                               largest_only=largest)
        want = filter_mesh(*welded[:3], c=welded[3], min_triangles=mn, largest_only=largest)
        same(got, want, (mn, largest))
        assert 0 < len(got[0]) < len(welded[0]) and got[3].any()


TABLE = ["sphere", "masked_sphere", "empty_0", "single_cube", "random_sign", "fused_masked", "random_sign"]


def table_case(oracle, name):
    if name == "empty_0":
        t, w, fg, vox = WV.empties()[0]
        e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32))
        return t, w, fg, vox, e
    return welded_case(oracle, name)


def test_table_slices_equal_the_volumes_alone(oracle, ops):
    cases = [table_case(oracle, name) for name in TABLE]
    vols = [volume(*c[:4]) for c in cases]
    # one criterion for all: the two equal volumes give equal slices, neither merged into the other
    got = ops.extract_meshes(vols, weld=True, min_triangles=8)
    for k, c in enumerate(cases):
        same(got[k], filter_mesh(*c[4], min_triangles=8), (k, TABLE[k]))
    same(got[4], got[6])
    assert len(got[4][0]) == 2866 and got[2][0].shape == (0, 3) and got[3][2].shape == (0, 4)
    # criteria that differ within the table
    mins = [1, 8, 8, 1, 20, 8, 8]
    largest = [False, True, False, True, False, False, True]
    got = ops.extract_meshes(vols, weld=True, min_triangles=mins, largest_only=largest)
    for k, c in enumerate(cases):
        same(got[k], filter_mesh(*c[4], min_triangles=mins[k], largest_only=largest[k]), (k, TABLE[k]))
    assert len(got[3][0]) == 3 and len(got[4][0]) != len(got[6][0]) and len(got[6][2]) == 4615
    # the filter off: the welded table as it was
    plain = ops.extract_meshes(vols, weld=True)
    for k, c in enumerate(cases):
        same(plain[k], c[4], (k, TABLE[k]))


def test_two_runs_give_the_same_bytes(oracle, ops):
    t, w, fg, vox, ref = welded_case(oracle, "random_sign")
    a = ops.extract_mesh(to_dev(t), to_dev(w), vox, weld=True, min_triangles=8)
    b = ops.extract_mesh(to_dev(t), to_dev(w), vox, weld=True, min_triangles=8)
    same(a, b)
    assert len(a[0]) == 2866
    la = ops.mesh_components(ref[2], len(ref[0]))
    lb = ops.mesh_components(ref[2], len(ref[0]))
    same(la, lb)


# ---- synthetic index buffers ----------------------------------------------------------------------------------------

def tris_of(corners):
    c = np.asarray(corners, np.int64).reshape(-1, 3)
    return np.concatenate([np.full((len(c), 1), 3), c], axis=1).astype(np.int32)


def strip(n, first=0):
    k = np.arange(n) + first
    return np.stack([k, k + 1, k + 2], axis=1)


def attributes(nv, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, 3)).astype(np.float32), rng.standard_normal((nv, 3)).astype(np.float32)


def check_buffer(ops, tri, nv, criteria, expect_labels=None, expect_sizes=None):
    """Labels, sizes and each filter against the restatement; returns the restatement's (labels, sizes)."""
    want = components(tri, nv)
    same(ops.mesh_components(tri, nv), want)
    if expect_labels is not None:
        assert np.array_equal(want[0], expect_labels) and np.array_equal(want[1], expect_sizes)
    v, n = attributes(nv)
    for mn, largest in criteria:
        same(ops.filter_mesh(v, n, tri, min_triangles=mn, largest_only=largest),
             filter_mesh(v, n, tri, min_triangles=mn, largest_only=largest), (mn, largest))
    return want


def test_long_strip_in_random_numbering(ops):
    """(a) 70 000 triangles (more than 65 536, many workgroups): vertex numbers a fixed random permutation with vertex 0
    at one end, triangles in reverse order."""
    n = 70_000
    perm = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(n + 1)])
    tri = tris_of(perm[strip(n)][::-1])
    check_buffer(ops, tri, n + 2, [(n, False), (n + 1, False), (0, True)], np.zeros(n + 2, np.int32),
                 np.full(n + 2, n, np.uint32))


def test_fan_around_the_highest_index(ops):
    """(b) 5 000 triangles that share the vertex with the highest index."""
    n = 5_000
    k = np.arange(n)
    tri = tris_of(np.stack([np.full(n, n + 1), k, k + 1], axis=1))
    check_buffer(ops, tri, n + 2, [(n, False), (n + 1, False)], np.zeros(n + 2, np.int32), np.full(n + 2, n, np.uint32))


def test_isolated_triangles(ops):
    """(c) 20 000 components of one triangle: largest_only is a 20 000-way tie that label 0 wins."""
    n = 20_000
    tri = tris_of(np.arange(3 * n).reshape(n, 3))
    check_buffer(ops, tri, 3 * n, [(1, False), (2, False), (0, True)], 3 * (np.arange(3 * n, dtype=np.int32) // 3),
                 np.ones(3 * n, np.uint32))
    v, nrm = attributes(3 * n)
    assert len(ops.filter_mesh(v, nrm, tri, largest_only=True)[0]) == 3


def test_interleaved_strips_take_the_per_lane_count(ops):
    """(d) two strips of 4 096 triangles interleaved triangle by triangle: no wave is label-uniform."""
    n = 4_096
    both = np.empty((2 * n, 3), np.int64)
    both[0::2] = strip(n)
    both[1::2] = strip(n, n + 2)
    labels = np.repeat(np.array([0, n + 2], np.int32), n + 2)
    check_buffer(ops, tris_of(both), 2 * n + 4, [(n, False), (0, True), (n + 1, False)], labels,
                 np.full(2 * n + 4, n, np.uint32))


def test_ordered_strip_takes_the_aggregated_count(ops):
    """(e) one strip in natural numbering and order: every wave is label-uniform, every workgroup merges its waves."""
    n = 5_000
    check_buffer(ops, tris_of(strip(n)), n + 2, [(n, False), (0, True)], np.zeros(n + 2, np.int32),
                 np.full(n + 2, n, np.uint32))


def fans(sizes):
    corners, nv = [], 0
    for size in sizes:
        corners += [(nv, nv + k + 1, nv + k + 2) for k in range(size)]
        nv += size + 2
    return tris_of(corners), nv


def test_tie_goes_to_the_smaller_label_and_the_winner_is_not_label_0(ops):
    """(f) components of 5, 9 and 9 triangles, the size-5 one holding vertex 0: the first size-9 one wins."""
    tri, nv = fans((5, 9, 9))
    labels, sizes = check_buffer(ops, tri, nv, [(0, True), (6, False), (9, True), (10, True)])
    assert sorted(set(labels.tolist())) == [0, 7, 18]
    v, n = attributes(nv)
    fv, fn, ft = ops.filter_mesh(v, n, tri, largest_only=True)
    assert fv.tobytes() == v[7:18].tobytes() and len(ft) == 9 and ft[:, 1:].min() == 0 and ft[:, 1:].max() == 10
    (_, _, _), st = ops.filter_mesh(v, n, tri, largest_only=True, stats=True)
    assert st["components"].tolist() == [3] and st["kept_components"].tolist() == [1]


def test_nothing_in_nothing_out(ops):
    """(g) nt = 0 and nv = 0: no launch, zero counts."""
    labels, sizes = ops.mesh_components(np.zeros((0, 4), np.int32), 0)
    assert labels.shape == (0,) and labels.dtype == np.int32 and sizes.shape == (0,) and sizes.dtype == np.uint32
    e3, e4 = np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32)
    (fv, fn, ft), st = ops.filter_mesh(e3, e3, e4, min_triangles=8, stats=True)
    assert fv.shape == (0, 3) and fn.shape == (0, 3) and ft.shape == (0, 4)
    assert st["components"].tolist() == [0] and st["kept_components"].tolist() == [0]
    # vertices no triangle uses: components of size 0, kept by nothing but the identity
    v, n = attributes(5)
    same(ops.mesh_components(e4, 5), (np.arange(5, dtype=np.int32), np.zeros(5, np.uint32)))
    same(ops.filter_mesh(v, n, e4, min_triangles=1), (v, n, e4))
    assert ops.filter_mesh(v, n, e4, min_triangles=2)[0].shape == (0, 3)


def test_table_of_index_buffers_keeps_models_apart(ops):
    """The fans and the interleaved strips as two models of one launch plus an empty model between them: labels are
    model-local and no component crosses a model."""
    fan_tri, fan_nv = fans((5, 9, 9))
    n = 300
    both = np.empty((2 * n, 3), np.int64)
    both[0::2] = strip(n)
    both[1::2] = strip(n, n + 2)
    strip_tri, strip_nv = tris_of(both), 2 * n + 4
    tri = np.concatenate([fan_tri, strip_tri])
    tb = [0, len(fan_tri), len(fan_tri), len(tri)]
    vb = [0, fan_nv, fan_nv, fan_nv + strip_nv]
    labels, sizes = ops.mesh_components(tri, fan_nv + strip_nv, tri_bases=tb, vertex_bases=vb)
    lf, sf = components(fan_tri, fan_nv)
    ls, ss = components(strip_tri, strip_nv)
    same((labels, sizes), (np.concatenate([lf, ls]), np.concatenate([sf, ss])))
    v, nrm = attributes(fan_nv + strip_nv)
    got, st = ops.filter_mesh(v, nrm, tri, min_triangles=[6, 0, 0], largest_only=[False, True, True], tri_bases=tb,
                              vertex_bases=vb, stats=True)
    same(got[0], filter_mesh(v[:fan_nv], nrm[:fan_nv], fan_tri, min_triangles=6))
    assert got[1][0].shape == (0, 3) and got[1][2].shape == (0, 4)
    same(got[2], filter_mesh(v[fan_nv:], nrm[fan_nv:], strip_tri, largest_only=True))
    assert st["components"].tolist() == [3, 0, 2] and st["kept_components"].tolist() == [2, 0, 1]


def test_entries_check_their_arguments(ops):
    import ctypes as C

    from emfusion_amd import _lib
    L = _lib.load()
    dummy = to_dev(np.zeros(8192, np.uint64))
    other = to_dev(np.zeros(8192, np.uint64))
    p, q = C.c_void_p(dummy.ptr), C.c_void_p(other.ptr)
    assert L.emf_hip_meshComponentsLabel(p, 8, 1, None, None, None, None) == -1                   # EMF_E_NULL: scratch
    assert L.emf_hip_meshComponentsLabel(None, 8, 1, p, None, None, None) == -1                   # triangles
    assert L.emf_hip_meshComponentsLabel(p, (1 << 30) + 1, 1, p, None, None, None) == -5          # EMF_E_LIMIT
    assert L.emf_hip_meshComponentsLabel(p, 8, 1 << 31, p, None, None, None) == -5
    assert L.emf_hip_meshComponentsLabel(p, 0, 1, p, None, None, None) == -4                      # triangles, no vertex
    assert L.emf_hip_meshComponentsLabelBatched(p, 8, 1, None, p, 1, p, None, None, None) == -1
    assert L.emf_hip_meshComponentsLabelBatched(p, 8, 1, p, p, 0, p, None, None, None) == -5
    assert L.emf_hip_meshComponentsFilterCount(p, 8, 1, p, None, None, None, None, None, None) == -1   # kept_counts
    assert L.emf_hip_meshComponentsEmit(p, 8, 1, q, q, None, q, q, p, None, p, None) == -4        # vertices alias
    assert L.emf_hip_meshComponentsEmit(p, 8, 1, q, q, None, q, p, p, None, q, None) == -4        # triangles alias
    assert L.emf_hip_meshComponentsEmit(p, 8, 1, q, q, q, q, p, p, None, p, None) == -1           # colours in, none out
    assert L.emf_hip_meshComponentsEmit(None, 0, 0, None, None, None, None, None, None, None, None, None) == 0
    assert L.emf_hip_meshComponentsStatus(None, 8, 1, None) == -1
