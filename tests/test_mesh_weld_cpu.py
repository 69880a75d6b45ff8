"""Welded meshes without a GPU: the new entries are declared, exported and typed, and the numpy restatement
(tests/weld_reference.py) agrees with the oracle's marching cubes about what the soup is."""
import numpy as np
import pytest

from tests import weld_volumes as WV
from tests.weld_reference import edge_keys, weld

ENTRIES = ["emf_hip_meshEdgeKeys", "emf_hip_meshEdgeKeysBatched", "emf_hip_meshWeldScratchBytes",
           "emf_hip_meshWeldCount", "emf_hip_meshWeldCountBatched", "emf_hip_meshWeldStatus", "emf_hip_meshWeldEmit",
           "emf_hip_meshWeldEmitBatched"]


def test_entries_are_declared_exported_and_typed():
    import ctypes as C

    from emfusion_amd import _lib, pipeline
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name], name
    assert lib.emf_hip_meshWeldScratchBytes.restype is C.c_size_t
    # scratch is sized by the soup: under 57 bytes per soup vertex plus 1 KiB, and nothing for too large a soup
    for nv in (0, 1, 31, 32, 33, 4128, 1 << 20, (1 << 20) + 1):
        b = lib.emf_hip_meshWeldScratchBytes(nv)
        assert 0 < b <= 57 * nv + 1024, (nv, b)
    assert lib.emf_hip_meshWeldScratchBytes((1 << 30) + 1) == 0
    assert "emf_fusion_set_mesh_weld" in pipeline.declared_symbols()
    assert hasattr(pipeline.load(), "emf_fusion_set_mesh_weld")


def _edge_use(tri):
    e = np.sort(np.concatenate([tri[:, [1, 2]], tri[:, [2, 3]], tri[:, [3, 1]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


# soup vertices, welded vertices, triangles (DESIGN.md 5.10 quotes the sphere's); the random-sign volume's are those of
# WV.random_sign()'s draw order (magnitudes first, then the signs).
@pytest.mark.parametrize("name,want", [("sphere", (4128, 1032, 2060)), ("masked_sphere", (1718, 745, 860)),
                                       ("zero_plane", (100, 36, 50)), ("random_sign", (9223, 3012, 4935))])
def test_restatement_agrees_with_the_oracle_soup(oracle, name, want):
    tsdf, wts, fg, vox = getattr(WV, name)()
    v, n, t = oracle.marching_cubes(tsdf, wts, vox, fg=fg) if fg is not None else oracle.marching_cubes(tsdf, wts, vox)
    keys = edge_keys(tsdf, wts, fg)
    assert keys.dtype == np.uint64 and len(keys) == len(v)
    wv, wn, wt = weld(v, n, t, keys)
    assert (len(v), len(wv), len(t)) == want
    assert wt.shape == t.shape and np.all(wt[:, 0] == 3) and wt[:, 1:].min() >= 0 and wt[:, 1:].max() == len(wv) - 1
    a, b, c = wt[:, 1], wt[:, 2], wt[:, 3]
    assert not np.any((a == b) | (b == c) | (a == c))              # welding by edge never collapses a triangle
    # welded vertex j is the first copy of the j-th key: first occurrences are ascending and their bits are the soup's
    _, first = np.unique(keys, return_index=True)
    first = np.sort(first)
    assert wv.tobytes() == v[first].tobytes() and wn.tobytes() == n[first].tobytes()
    # every soup corner's key is its welded corner's key
    assert np.array_equal(keys[t[:, 1:]], keys[first][wt[:, 1:]])
    if name == "sphere":   # closed surface: every edge used by exactly two triangles, Euler characteristic 2
        cnt = _edge_use(wt)
        assert np.all(cnt == 2) and len(cnt) == 3090 and len(wv) - len(cnt) + len(wt) == 2
        assert np.all(np.unique(keys, return_counts=True)[1] == 4)  # every vertex stored exactly four times
    if name == "masked_sphere":
        assert _edge_use(wt).min() == 1                             # open borders


def test_duplicates_differ_in_their_bits(oracle):
    """Why welding is by edge: a share of the duplicates is not bit-equal to the first copy (adjacent cubes interpolate
    the same grid edge in opposite directions)."""
    for name in ("sphere", "random_sign"):
        tsdf, wts, fg, vox = getattr(WV, name)()
        v, n, t = oracle.marching_cubes(tsdf, wts, vox)
        keys = edge_keys(tsdf, wts, fg)
        _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
        differs = np.any(v.view(np.uint32) != v[first[inv.reshape(-1)]].view(np.uint32), axis=1)
        dup = len(v) - len(first)
        assert 0.01 < differs.sum() / dup < 0.15, (name, differs.sum(), dup)
