"""Simplified meshes without a GPU: the new entries are declared, exported and typed, the scratch honours the bound the
header declares, and the numpy restatement (tests/simplify_reference.py) has, on the oracle's welded soup of the
welded-mesh test volumes, the properties include/emf_hip.h "Simplified meshes" promises -- and the counts measured when
the feature was proposed."""
import numpy as np
import pytest

from tests.components_reference import welded_case
from tests.simplify_reference import E_ARG, E_LIMIT, Refused, cluster_keys, simplify, simplify_table

ENTRIES = ["emf_hip_meshSimplifyScratchBytes", "emf_hip_meshSimplifyCount", "emf_hip_meshSimplifyStatus",
           "emf_hip_meshSimplifyEmit"]


def test_entries_are_declared_exported_and_typed():
    import ctypes as C
    import re

    from emfusion_amd import _lib
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name], name
    assert lib.emf_hip_meshSimplifyScratchBytes.restype is C.c_size_t
    assert int(re.search(r"#define\s+EMF_HIP_ABI_VERSION\s+(\d+)", _lib.HEADER_PATH.read_text()).group(1)) == 8


def test_scratch_is_linear_in_vertices_plus_triangles():
    """include/emf_hip.h: under 137 bytes per vertex + 5 per triangle + 8 KiB, 0 beyond the limits."""
    from emfusion_amd import _lib
    lib = _lib.load()
    for nv, nt in ((0, 0), (1, 0), (3, 1), (255, 256), (256, 257), (1032, 2060), (123_000, 231_000), (1 << 20, 1 << 21),
                   (1 << 30, (1 << 31) - 1)):
        b = lib.emf_hip_meshSimplifyScratchBytes(nv, nt)
        assert 112 * nv + 4 * nt < b <= 137 * nv + 5 * nt + 8192, (nv, nt, b)
    assert lib.emf_hip_meshSimplifyScratchBytes((1 << 30) + 1, 8) == 0
    assert lib.emf_hip_meshSimplifyScratchBytes(8, 1 << 31) == 0


def test_entries_reject_bad_arguments_before_any_launch():
    """What needs no device: NULL pointers, sizes beyond the limits, models without bases, cells that are not finite."""
    import ctypes as C

    from emfusion_amd import _lib
    L = _lib.load()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    cell = (C.c_float * 2)(0.1, 0.1)
    nan = (C.c_float * 1)(float("nan"))
    count = lambda nv, nt, tb, vb, n, cells, scratch, kc: L.emf_hip_meshSimplifyCount(
        p, p, None, p, nv, nt, tb, vb, n, cells, None, scratch, kc, None, None, None)
    assert count(8, 1, None, None, 1, cell, None, p) == -1                  # EMF_E_NULL: scratch
    assert count(8, 1, None, None, 1, cell, p, None) == -1                  # kept_counts
    assert count(8, 1, None, None, 1, None, p, p) == -1                     # cells
    assert count(8, 1, p, None, 1, cell, p, p) == -1                        # one of the two bases
    assert count((1 << 30) + 1, 1, None, None, 1, cell, p, p) == -5         # EMF_E_LIMIT
    assert count(8, 1 << 31, None, None, 1, cell, p, p) == -5
    assert count(8, 1, p, p, 257, cell, p, p) == -5
    assert count(0, 1, None, None, 1, cell, p, p) == -4                     # EMF_E_ARG: triangles over no vertex
    assert count(8, 1, None, None, 2, cell, p, p) == -4                     # two models, no bases
    assert count(8, 1, None, None, 1, nan, p, p) == -4                      # a cell that is not finite
    assert L.emf_hip_meshSimplifyStatus(None, 8, 1, None) == -1
    emit = lambda *a: L.emf_hip_meshSimplifyEmit(p, 8, 1, None, None, 1, *a, None)
    q = C.cast((C.c_uint64 * 64)(), C.c_void_p)
    assert emit(q, q, None, q, q, p, None, p) == -4                         # vertices alias
    assert emit(q, q, None, q, p, q, None, p) == -4                         # normals alias
    assert emit(q, q, None, q, p, p, None, q) == -4                         # triangles alias
    assert emit(q, q, q, q, p, p, q, p) == -4                               # colours alias
    assert emit(q, q, q, q, p, p, None, p) == -1                            # colours in, none out
    assert L.emf_hip_meshSimplifyEmit(None, 0, 0, None, None, 1, None, None, None, None, None, None, None, None, None) == 0


def welded(oracle, name):
    return welded_case(oracle, name)


# volume -> (welded vertices, triangles) in, and at a cell of two voxels (vertices, triangles, clusters) out
TABLE = {
    "sphere": ((1032, 2060), (168, 332, 168)),
    "masked_sphere": ((745, 860), (158, 155, 166)),
    "zero_plane": ((36, 50), (16, 18, 16)),
    "random_sign": ((3012, 4935), (392, 1109, 393)),
    "single_cube": ((3, 1), (3, 1, 3)),
    "fused": ((2568, 4716), (474, 857, 507)),
    "fused_masked": ((2045, 2625), (442, 477, 479)),
}


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_gives_the_measured_counts(oracle, name):
    _, _, _, vox, (v, n, t) = welded(oracle, name)
    (nv, nt), out2 = TABLE[name]
    assert (len(v), len(t)) == (nv, nt)
    (sv, sn, st), stats = simplify(v, n, t, cell=np.float32(2 * vox), stats=True)
    assert (len(sv), len(st), stats["clusters"]) == out2, (len(sv), len(st), stats["clusters"])
    assert (stats["vertices_in"], stats["triangles_in"], stats["vertices_out"], stats["triangles_out"]) == \
        (nv, nt, out2[0], out2[1])
    assert sv.dtype == np.float32 and sn.dtype == np.float32 and st.dtype == np.int32


@pytest.mark.parametrize("name", sorted(TABLE))
def test_simplification_properties(oracle, name):
    _, _, _, vox, (v, n, t) = welded(oracle, name)
    # a cell below the smallest vertex spacing: every vertex alone in its cell, the input byte for byte
    fine = np.float32(np.abs(v).max() / 30000)
    assert len(np.unique(cluster_keys(v, fine))) == len(v)
    assert same(simplify(v, n, t, cell=fine), (v, n, t))
    assert same(simplify(v, n, t, cell=0.0), (v, n, t)) and same(simplify(v, n, t, cell=-1.0), (v, n, t))
    # counts do not increase as the cell doubles
    last = (len(v), len(t), len(v))
    perm = np.random.default_rng(17).permutation(len(t))
    for k in (1, 2, 4, 8):
        cell = np.float32(k * vox)
        (sv, sn, st), stats = simplify(v, n, t, cell=cell, stats=True)
        now = (len(sv), len(st), stats["clusters"])
        assert all(a <= b for a, b in zip(now, last)), (k, now, last)
        last = now
        # three distinct in-range indices per triangle, every vertex referenced
        if len(st):
            assert np.all(st[:, 0] == 3) and st[:, 1:].min() >= 0 and st[:, 1:].max() < len(sv)
            assert np.all((st[:, 1] != st[:, 2]) & (st[:, 2] != st[:, 3]) & (st[:, 1] != st[:, 3]))
        assert len(np.unique(st[:, 1:])) == len(sv)
        # every vertex in its cell's closed box, widened by 2^-20 m plus one float ulp
        lo = stats["cells"].astype(np.float64) * np.float64(cell)
        hi = (stats["cells"].astype(np.float64) + 1.0) * np.float64(cell)
        slack = 2.0 ** -20 + np.spacing(np.abs(sv)).astype(np.float64)
        assert np.all(sv.astype(np.float64) >= lo - slack) and np.all(sv.astype(np.float64) <= hi + slack), k
        assert np.all(np.isfinite(sn))
        # a permutation of the triangle order permutes the kept triangles and changes nothing else
        (pv, pn, pt), pstats = simplify(v, n, t[perm], cell=cell, stats=True)
        assert same((pv, pn), (sv, sn)) and np.array_equal(pstats["kept"], stats["kept"][perm])
        at = np.full(len(t), -1)
        at[stats["kept"]] = np.arange(len(st))
        assert np.array_equal(pt, st[at[perm][pstats["kept"]]])
    # one cell spanning the whole mesh: every triangle collapses, nothing is referenced
    (sv, sn, st), stats = simplify(v, n, t, cell=1024.0, origin=(-512.0, -512.0, -512.0), stats=True)
    assert sv.shape == (0, 3) and sn.shape == (0, 3) and st.shape == (0, 4) and stats["clusters"] == 1


def test_colours_round_to_nearest_and_singletons_keep_their_bits():
    v = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.3, 0.1, 0.2]], np.float32)
    n = np.array([[1, 0, 0], [np.nan, 1e30, 3], [0, 0, 1], [0, 1, 0], [2, -1e30, np.inf]], np.float32)
    c = np.array([[0, 1, 255], [1, 2, 255], [9, 9, 9], [7, 7, 7], [0, 0, 254]], np.uint8)
    t = np.array([[3, 0, 2, 3], [3, 1, 2, 3], [3, 0, 1, 2], [3, 4, 3, 2]], np.int32)
    sv, sn, st, sc = simplify(v, n, t, c, cell=1.0)
    assert st.tolist() == [[3, 0, 1, 2], [3, 0, 1, 2], [3, 0, 2, 1]]             # equal triples are both kept
    assert sv[1:].tobytes() == v[2:4].tobytes() and sn[1:].tobytes() == n[2:4].tobytes() and sc[1:].tolist() == [[9] * 3, [7] * 3]
    assert sc[0].tolist() == [0, 1, 255]                                         # 1/3 -> 0, 3/3 -> 1, 764/3 -> 255
    q = lambda x: np.rint(np.ldexp(np.float64(np.float32(x)), 20))
    assert sv[0, 0] == np.float32((q(0.1) + q(0.2) + q(0.3)) / 3 * 2.0 ** -20)
    assert sn[0].tolist() == [1.0, 0.0, 1.0]                                     # NaN, 1e30, -1e30 and inf count as 0


def test_table_keeps_models_apart():
    v = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [0.2, 0.2, 0.2]], np.float32)
    t = np.array([[3, 0, 1, 2], [3, 3, 1, 2]], np.int32)
    one = simplify(v, -v, t, cell=1.0)
    assert len(one[0]) == 3 and len(one[2]) == 2
    got = simplify_table(np.concatenate([v, v]), np.concatenate([-v, -v]), np.concatenate([t, t]), cells=[1.0, 1.0, 0.0],
                         tri_bases=[0, 2, 2, 4], vertex_bases=[0, 4, 4, 8])
    assert same(got[0], one) and got[1][0].shape == (0, 3) and same(got[2], (v, -v, t))


def test_refusals():
    v = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [-3.2, 0.2, 0.2]], np.float32)
    t = np.array([[3, 0, 1, 2], [3, 3, 1, 2]], np.int32)
    assert len(simplify(v, v, t, cell=0.1)[0]) == 4
    for bad in (np.nan, np.inf, -np.inf, 1024.0, -1024.0):
        w = v.copy()
        w[2, 1] = bad
        with pytest.raises(Refused) as e:
            simplify(w, v, t, cell=0.1)
        assert e.value.code == E_LIMIT
        assert same(simplify(w, v, t, cell=0.0), (w, v, t))                      # a pass-through looks at no position
    w = v.copy()
    w[2, 1] = np.float32(1023.9999)
    assert len(simplify(w, v, t, cell=0.1)[0]) == 4
    for cell, origin, ok in ((1e-5, 0.0, False), (3.2 / 32700, 0.0, True), (3.2 / 32800, 0.0, False),
                             (1.0, 32764.0, True), (1.0, 32765.0, False), (1.0, -32767.0, False), (1.0, -32766.0, True)):
        if ok:
            simplify(v, v, t, cell=cell, origin=(origin,) * 3)
        else:
            with pytest.raises(Refused) as e:
                simplify(v, v, t, cell=cell, origin=(origin,) * 3)
            assert e.value.code == E_LIMIT, (cell, origin)
    for bad in (-1, 4, 2 ** 31 - 1):
        u = np.concatenate([t, [[3, 0, bad, 1]], t[:1]]).astype(np.int32)
        with pytest.raises(Refused) as e:
            simplify(v, v, u, cell=0.1)
        assert e.value.code == E_ARG
        assert same(e.value.partial, simplify(v, v, np.concatenate([t, t[:1]]), cell=0.1))
