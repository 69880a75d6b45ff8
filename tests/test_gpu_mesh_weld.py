"""Welded meshes on the device (include/emf_hip.h "Welded meshes"): emf_hip_meshEdgeKeys / meshWeldCount / meshWeldEmit
and their table forms against the numpy restatement (tests/weld_reference.py) applied to the oracle's soup.  The switch
through Fusion, the result files and the two apps: tests/test_gpu_weld_pipeline.py."""
import numpy as np
import pytest

from tests import weld_volumes as WV
from tests.parity_util import to_dev
from tests.weld_reference import edge_keys, weld

pytestmark = pytest.mark.gpu

VOLUMES = ["fused_32", "fused_30x22x37", "fused_64x48x40", "fused_masked", "zero_plane", "single_cube", "empty_0",
           "empty_1", "empty_2", "random_sign"]
_cache = {}


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def case(oracle, name):
    """(tsdf, weights, fg, voxel size, grads or None, the oracle's soup, the restatement's keys) -- computed once."""
    if name not in _cache:
        grads = None
        if name.startswith("fused_") and name != "fused_masked":
            res = {"fused_32": (32, 32, 32), "fused_30x22x37": (30, 22, 37), "fused_64x48x40": (64, 48, 40)}[name]
            t, w, fg, vox = WV.fused(oracle, res)
        elif name == "fused_masked":
            t, w, fg, vox = WV.fused_masked(oracle)
            grads = oracle.compute_tsdf_grads(t)
        elif name.startswith("empty_"):
            t, w, fg, vox = WV.empties()[int(name[-1])]
        else:
            t, w, fg, vox = getattr(WV, name)()
        kw = {k: v for k, v in (("fg", fg), ("grads", grads)) if v is not None}
        soup = oracle.marching_cubes(t, w, vox, **kw)
        _cache[name] = (t, w, fg, vox, grads, soup, edge_keys(t, w, fg))
    return _cache[name]


def dev_or_none(a):
    return None if a is None else to_dev(a)


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


@pytest.mark.parametrize("name", VOLUMES)
def test_edge_keys_equal_the_restatement(oracle, ops, name):
    t, w, fg, vox, grads, soup, keys = case(oracle, name)
    assert len(keys) == len(soup[0])
    if name.startswith("empty_"):
        assert len(keys) == 0
    elif name not in ("single_cube", "zero_plane"):
        assert len(keys) > 500
    got = ops.mesh_edge_keys(to_dev(t), to_dev(w), fg_mask=dev_or_none(fg))
    assert got.dtype == np.uint64 and got.shape == keys.shape
    assert np.array_equal(got, keys)


@pytest.mark.parametrize("name", VOLUMES)
def test_welded_mesh_equals_the_welded_oracle_soup(oracle, ops, name):
    t, w, fg, vox, grads, soup, keys = case(oracle, name)
    want = weld(*soup, keys)
    got = ops.extract_mesh(to_dev(t), to_dev(w), vox, fg_mask=dev_or_none(fg), grads=dev_or_none(grads), weld=True)
    same(got, want, name)
    if len(keys):
        assert len(got[0]) == len(np.unique(keys)) <= len(soup[0])
        assert name == "single_cube" or 3 * len(got[0]) < len(soup[0]) * 2   # (a lone cube has nothing to weld)
    else:
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 4)
    # the soup itself is what it was
    same(ops.extract_mesh(to_dev(t), to_dev(w), vox, fg_mask=dev_or_none(fg), grads=dev_or_none(grads)), soup, name)


def test_welded_colours(oracle, ops):
    t, w, fg, vox, grads, soup, keys = case(oracle, "fused_masked")
    rng = np.random.default_rng(8)
    col = rng.integers(0, 65281, t.shape + (4,), dtype=np.uint16)
    col[..., 3] = rng.integers(0, 3, t.shape) * 128  # a third of the voxels uncoloured
    args = (to_dev(t), to_dev(w), vox)
    v, n, tr, c = ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col))
    same((v, n, tr), soup)
    assert len(np.unique(c, axis=0)) > 20
    same(ops.extract_mesh(*args, fg_mask=to_dev(fg), color=to_dev(col), weld=True), weld(v, n, tr, keys, c))


def test_sphere_is_a_closed_surface_by_index(oracle, ops):
    """Without the restatement: the welded analytic sphere is closed by INDEX -- no rounding of positions."""
    t, w, fg, vox = WV.sphere()
    sv, sn, st = ops.extract_mesh(to_dev(t), to_dev(w), vox)
    wv, wn, wt = ops.extract_mesh(to_dev(t), to_dev(w), vox, weld=True)
    keys = ops.mesh_edge_keys(to_dev(t), to_dev(w))
    assert (len(sv), len(wv), len(wt)) == (4128, 1032, 2060) and wt.tobytes() != st.tobytes()
    tri = wt[:, 1:]
    assert not np.any((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]))
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    edges, cnt = np.unique(e, axis=0, return_counts=True)
    assert np.all(cnt == 2)                                     # every edge used by exactly two triangles
    assert len(wv) - len(edges) + len(wt) == 2                  # V - E + F
    # corner for corner the welded triangle refers to the same grid edge as the soup's ...
    _, first = np.unique(keys, return_index=True)
    wkeys = keys[np.sort(first)]
    assert np.array_equal(wkeys[wt[:, 1:]], keys[st[:, 1:]])
    # ... and its position is the soup's to within what the duplicates of this volume differ from their first copy
    # by in the ORACLE's soup (adjacent cubes interpolate the same edge in opposite directions)
    ov = oracle.marching_cubes(t, w, vox)[0]
    okeys = edge_keys(t, w)
    _, ofirst, oinv = np.unique(okeys, return_index=True, return_inverse=True)
    bound = np.abs(ov.astype(np.float64) - ov[ofirst[oinv.reshape(-1)]]).max()
    assert 0 < bound < 1e-6
    assert np.abs(wv[wt[:, 1:]].astype(np.float64) - sv[st[:, 1:]]).max() <= bound


def test_table_slices_equal_the_volumes_own_welded_meshes(oracle, ops):
    rng = np.random.default_rng(8)
    names = ["fused_64x48x40", "fused_32", "fused_32", "fused_masked", "empty_0"]
    vols, singles = [], []
    for k, name in enumerate(names):
        t, w, fg, vox, grads, soup, keys = case(oracle, name)
        v = dict(tsdf=to_dev(t), weights=to_dev(w), voxel_size=vox, fg_mask=dev_or_none(fg), grads=dev_or_none(grads))
        if k in (0, 3):
            col = rng.integers(0, 65281, t.shape + (4,), dtype=np.uint16)
            v["color"] = to_dev(col)
        vols.append(v)
    plain = [dict(v, color=None) for v in vols]
    got = ops.extract_meshes(plain, weld=True)
    for k, name in enumerate(names):
        t, w, fg, vox, grads, soup, keys = case(oracle, name)
        same(got[k], weld(*soup, keys), (k, name))     # model-local indices: the volume's own welded mesh
    same(got[1], got[2])                                # identical volumes in two slots: neither merged into the other
    assert len(got[1][0]) > 100 and got[4][0].shape == (0, 3) and got[4][2].shape == (0, 4)
    # with colours: each slice is the level-1 welded mesh with colours (black where the model has no colour volume)
    gotc = ops.extract_meshes(vols, weld=True)
    for k, v in enumerate(vols):
        same(gotc[k][:3], got[k], k)
        if v.get("color") is not None:
            one = ops.extract_mesh(v["tsdf"], v["weights"], v["voxel_size"], fg_mask=v["fg_mask"], grads=v["grads"],
                                   color=v["color"], weld=True)
            same(gotc[k], one, k)
        else:
            assert gotc[k][3].shape == (len(got[k][0]), 3) and not gotc[k][3].any()


def test_two_runs_give_the_same_bytes(oracle, ops):
    t, w, fg, vox, grads, soup, keys = case(oracle, "random_sign")
    a = ops.extract_mesh(to_dev(t), to_dev(w), vox, weld=True)
    b = ops.extract_mesh(to_dev(t), to_dev(w), vox, weld=True)
    same(a, b)
    assert len(a[0]) > 2000


def test_entries_check_their_arguments(ops):
    import ctypes as C

    from emfusion_amd import _lib
    L = _lib.load()
    dummy = to_dev(np.zeros(4096, np.uint64))
    p = C.c_void_p(dummy.ptr)
    assert L.emf_hip_meshWeldCount(p, 8, None, p, None) == -1            # EMF_E_NULL: scratch
    assert L.emf_hip_meshWeldCount(None, 8, p, p, None) == -1            # keys
    assert L.emf_hip_meshWeldCount(p, (1 << 30) + 1, p, p, None) == -5   # EMF_E_LIMIT
    assert L.emf_hip_meshWeldCountBatched(p, 8, None, 1, p, p, p, None) == -1
    assert L.emf_hip_meshWeldCountBatched(p, 8, p, 0, p, p, p, None) == -5
    assert L.emf_hip_meshWeldEmit(p, 8, 1, None, p, None, p, p, p, None, p, None) == -1
    assert L.emf_hip_meshWeldEmit(p, 8, 1, p, p, p, p, p, p, None, p, None) == -1    # colours in, none out
    assert L.emf_hip_meshWeldEmit(p, 0, 1, p, p, None, p, p, p, None, p, None) == -4  # triangles over no vertex
    assert L.emf_hip_meshWeldEmit(None, 0, 0, None, None, None, None, None, None, None, None, None) == 0
    assert L.emf_hip_meshEdgeKeys(p, p, None, (C.c_int32 * 3)(8, 8, 8), p, None, None) == -1
    # an empty soup: zero counts, no launch
    scratch = to_dev(np.zeros(max(L.emf_hip_meshWeldScratchBytes(0) // 8, 1), np.uint64))
    out = to_dev(np.full(4, 7, np.uint32))
    assert L.emf_hip_meshWeldCount(None, 0, C.c_void_p(scratch.ptr), C.c_void_p(out.ptr), None) == 0
    assert L.emf_hip_meshWeldStatus(C.c_void_p(scratch.ptr), 0, None) == 0
    assert out.numpy().tolist() == [0, 7, 7, 7]
