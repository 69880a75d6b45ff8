"""Mesh components without a GPU: the new entries are declared, exported and typed, the scratch honours the bound the
header declares, and the numpy restatement (tests/components_reference.py) gives, on the oracle's welded soup of the
welded-mesh test volumes, the components measured when the feature was proposed (union-find, cross-checked with
scipy.sparse.csgraph.connected_components at the time; neither is on the test path)."""
import numpy as np
import pytest

from tests.components_reference import components, filter_mesh, kept_labels, summary, welded_case

ENTRIES = ["emf_hip_meshComponentsScratchBytes", "emf_hip_meshComponentsLabel", "emf_hip_meshComponentsLabelBatched",
           "emf_hip_meshComponentsFilterCount", "emf_hip_meshComponentsFilterCountBatched",
           "emf_hip_meshComponentsStatus", "emf_hip_meshComponentsEmit", "emf_hip_meshComponentsEmitBatched"]


def test_entries_are_declared_exported_and_typed():
    import ctypes as C

    from emfusion_amd import _lib, pipeline
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name], name
    assert lib.emf_hip_meshComponentsScratchBytes.restype is C.c_size_t
    assert "emf_fusion_set_mesh_filter" in pipeline.declared_symbols()
    assert hasattr(pipeline.load(), "emf_fusion_set_mesh_filter")


def test_scratch_is_linear_in_vertices_plus_triangles():
    """include/emf_hip.h: under 13 bytes per welded vertex + 5 per triangle + 6 KiB, 0 beyond the limits."""
    from emfusion_amd import _lib
    lib = _lib.load()
    for nv, nt in ((0, 0), (1, 0), (3, 1), (255, 256), (256, 257), (1032, 2060), (123_000, 231_000), (1 << 20, 1 << 21),
                   (1 << 30, (1 << 31) - 1)):
        b = lib.emf_hip_meshComponentsScratchBytes(nv, nt)
        assert 12 * nv + 4 * nt < b <= 13 * nv + 5 * nt + 6144, (nv, nt, b)
    assert lib.emf_hip_meshComponentsScratchBytes((1 << 30) + 1, 8) == 0
    assert lib.emf_hip_meshComponentsScratchBytes(8, 1 << 31) == 0


def welded(oracle, name):
    return welded_case(oracle, name)[4]


# volume -> (welded vertices, triangles, components, the largest's (vertices, triangles), what ">= 8 triangles" leaves:
# (vertices, triangles, components))
TABLE = {
    "sphere": (1032, 2060, 1, (1032, 2060), (1032, 2060, 1)),
    "masked_sphere": (745, 860, 7, (701, 830), (724, 847, 3)),
    "zero_plane": (36, 50, 1, (36, 50), (36, 50, 1)),
    "random_sign": (3012, 4935, 44, (2706, 4615), (2866, 4827, 15)),
    "single_cube": (3, 1, 1, (3, 1), (0, 0, 0)),
    "fused": (2568, 4716, 23, (2462, 4650), (2491, 4678, 3)),
    "fused_masked": (2045, 2625, 35, (1857, 2503), (1936, 2573, 6)),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_gives_the_measured_components(oracle, name):
    v, n, t = welded(oracle, name)
    nv, nt, ncomp, largest, ge8 = TABLE[name]
    assert (len(v), len(t)) == (nv, nt)
    got = summary(t, len(v), 8)
    assert (got[0], got[2], got[3]) == (ncomp, largest, ge8), got
    if name == "masked_sphere":
        assert got[1] == [830, 9, 8, 7, 3, 2, 1]
    labels, sizes = components(t, len(v))
    assert labels.dtype == np.int32 and sizes.dtype == np.uint32
    assert sizes.min() >= 1                                    # every welded vertex lies in at least one triangle
    # labels are fixed points, the smallest index of their component, and constant over every triangle
    assert np.array_equal(labels[labels], labels) and np.all(labels <= np.arange(len(v)))
    assert np.all(labels[t[:, 1]] == labels[t[:, 2]]) and np.all(labels[t[:, 1]] == labels[t[:, 3]])
    fv, fn, ft = filter_mesh(v, n, t, min_triangles=8)
    assert (len(fv), len(ft)) == ge8[:2]
    lv, ln, lt = filter_mesh(v, n, t, largest_only=True)
    assert (len(lv), len(lt)) == largest


@pytest.mark.parametrize("name", ["masked_sphere", "random_sign", "fused_masked", "single_cube"])
def test_filter_properties(oracle, name):
    v, n, t = welded(oracle, name)
    same = lambda a, b: all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))
    assert same(filter_mesh(v, n, t, min_triangles=1), (v, n, t))          # the identity
    assert same(filter_mesh(v, n, t, min_triangles=0), (v, n, t))
    for kw in (dict(min_triangles=8), dict(largest_only=True), dict(min_triangles=8, largest_only=True),
               dict(min_triangles=10 ** 6)):
        once = filter_mesh(v, n, t, **kw)
        assert same(filter_mesh(*once, **kw), once), kw                     # idempotent
        fv, fn, ft = once
        assert fv.shape[1:] == (3,) and ft.shape[1:] == (4,)
        if len(ft):
            assert np.all(ft[:, 0] == 3) and ft[:, 1:].min() >= 0 and ft[:, 1:].max() < len(fv)  # only kept vertices
        assert len(np.unique(ft[:, 1:])) == len(fv)                         # every kept vertex is used
        labels, _ = components(ft, len(fv))
        assert np.array_equal(labels[labels], labels) and np.all(labels <= np.arange(len(fv)))
    assert len(filter_mesh(v, n, t, min_triangles=10 ** 6)[0]) == 0


def test_largest_only_ties_go_to_the_smaller_label():
    """Three components of 5, 9 and 9 triangles (fans), the size-5 one holding vertex 0."""
    tri, nv = [], 0
    for size in (5, 9, 9):
        tri += [(3, nv, nv + k + 1, nv + k + 2) for k in range(size)]
        nv += size + 2
    tri = np.array(tri, np.int32)
    labels, sizes = components(tri, nv)
    assert sorted(set(labels.tolist())) == [0, 7, 18]
    assert kept_labels(labels, sizes, 0, True).tolist() == [7]
    v = np.arange(3 * nv, dtype=np.float32).reshape(nv, 3)
    fv, fn, ft = filter_mesh(v, -v, tri, largest_only=True)
    assert fv.tobytes() == v[7:18].tobytes() and len(ft) == 9 and ft[:, 1:].min() == 0 and ft[:, 1:].max() == 10
    assert len(filter_mesh(v, -v, tri, min_triangles=10, largest_only=True)[0]) == 0
