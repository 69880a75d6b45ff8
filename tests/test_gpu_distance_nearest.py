"""The nearest-site kernels (include/emf_hip.h "Distance field"; ops.distance_transform(nearest=True),
ops.distance_query) against tests/nearest_reference.py.  Everything is an integer function of the class bytes: every
comparison is tobytes() equality."""
import numpy as np
import pytest

from tests import distance_reference as dr
from tests import nearest_reference as nr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

VOXEL = 0.04
_expected = {}


def ident(s):
    return "x".join(str(v) for v in s)


def sites_of_case(shape, content):
    return nr.tie_field(shape, content) if content in nr.TIE_CONTENTS else dr.site_field(shape, content, seed=11)


def expected(shape, content):
    """(sites, d2, nearest) without a cap, computed once per case and shared; a cap only masks them."""
    key = (shape, content)
    if key not in _expected:
        sites = sites_of_case(shape, content)
        d2, near = nr.nearest_separable(sites)
        nr.check_against_d2(sites, d2, near)
        if sites.size <= dr.BRUTE_LIMIT:
            assert near.tobytes() == nr.nearest_brute(sites)[1].tobytes()
        for a in (sites, d2, near):
            a.setflags(write=False)
        _expected[key] = (sites, d2, near)
    return _expected[key]


def capped(d2, near, cap):
    d2 = dr.apply_cap(d2, cap)
    return d2, np.where(d2 == dr.FAR, nr.NONE, near).astype(np.int32)


def run_case(shape, content):
    from emfusion_amd import ops
    sites, d2, near = expected(shape, content)
    for site_mask in (2, 6, 1):
        classes = dr.classes_with_sites(sites, site_mask, seed=5)
        d_classes = to_dev(classes)
        for cap in (0, 1, 5):
            want2, want = capped(d2, near, cap)
            g2, gn = ops.distance_transform(d_classes, site_mask=site_mask, cap=cap, nearest=True)
            g2, gn = g2.numpy(), gn.numpy()
            assert gn.dtype == np.int32 and gn.shape == shape
            bad = gn != want
            assert gn.tobytes() == want.tobytes(), \
                (shape, content, site_mask, cap, int(bad.sum()), np.argwhere(bad)[:4].tolist(), gn[bad][:4].tolist(),
                 want[bad][:4].tolist())
            assert g2.tobytes() == want2.tobytes()
            assert ((gn == nr.NONE) == (g2 == dr.FAR)).all()
            plain = ops.distance_transform(d_classes, site_mask=site_mask, cap=cap).numpy()
            assert g2.tobytes() == plain.tobytes()
        assert d_classes.numpy().tobytes() == classes.tobytes()  # the input is only read


@pytest.mark.parametrize("content", dr.CONTENTS)
@pytest.mark.parametrize("shape", dr.SHAPES, ids=ident)
def test_nearest_is_exact(dev, shape, content):
    run_case(shape, content)


@pytest.mark.parametrize("case", [(c, s) for c in nr.TIE_CONTENTS for s in nr.TIE_SHAPES[c]],
                         ids=lambda c: c[0] + "-" + ident(c[1]))
def test_nearest_breaks_ties_toward_the_smallest_index(dev, case):
    content, shape = case
    run_case(shape, content)


def test_the_tie_at_the_octahedrons_centre(dev):
    """Six sites equally near: the smallest linear index, which a scan that stops at d * d >= best does not find."""
    from emfusion_amd import ops
    sites, d2, near = expected((9, 9, 9), "octa")
    g2, gn = ops.distance_transform(to_dev(dr.classes_with_sites(sites, 2, seed=5)), nearest=True)
    gn = gn.numpy()
    assert gn[4, 4, 4] == near[4, 4, 4] == (0 * 9 + 4) * 9 + 4 and g2.numpy()[4, 4, 4] == 16
    assert gn[4, 3, 3] == (4 * 9 + 0) * 9 + 4
    assert gn.tobytes() != nr.nearest_by_scan(sites, early_stop=True)[1].tobytes()


@pytest.mark.parametrize("shape", [(11, 11, 11), (3, 4, 11), (11, 3, 2), (2, 11, 70)], ids=ident)
def test_sites_at_exactly_the_cap_on_both_sides(dev, shape):
    """Sites at the ends of every axis of 11 and a cap of 5: the middle has both at exactly the cap, still within it."""
    from emfusion_amd import ops
    sites = np.zeros(shape, bool)
    for axis, n in enumerate(shape):
        if n == 11:
            at = [s // 2 for s in shape]
            for end in (0, 10):
                at[axis] = end
                sites[tuple(at)] = True
    want2, want = nr.nearest_separable(sites, cap=5)
    nr.check_against_d2(sites, want2, want, cap=5)
    assert want.tobytes() == nr.nearest_brute(sites, cap=5)[1].tobytes()
    mid = tuple(s // 2 for s in shape)
    assert want2[mid] == 25 and want[mid] == np.flatnonzero(sites.reshape(-1))[0]
    g2, gn = ops.distance_transform(to_dev(dr.classes_with_sites(sites, 2, seed=1)), cap=5, nearest=True)
    assert g2.numpy().tobytes() == want2.tobytes() and gn.numpy().tobytes() == want.tobytes()
    assert (want2 == dr.FAR).any()


@pytest.mark.parametrize("content", ["none", "far_corner", "p01", "all"])
@pytest.mark.parametrize("shape", [(9, 17, 65), (2, 600, 3), (600, 3, 2), (5, 1, 70)], ids=ident)
def test_metres_and_repeatability(dev, shape, content):
    from emfusion_amd import ops
    sites, d2, near = expected(shape, content)
    classes = dr.classes_with_sites(sites, 2, seed=5)
    d_classes = to_dev(classes)
    for cap in (0, 5):
        want2, want = capped(d2, near, cap)
        g2, gm, gn = ops.distance_transform(d_classes, site_mask=2, cap=cap, voxel_size=VOXEL, nearest=True)
        g2, gm, gn = g2.numpy(), gm.numpy(), gn.numpy()
        p2, pm = ops.distance_transform(d_classes, site_mask=2, cap=cap, voxel_size=VOXEL)
        assert g2.tobytes() == p2.numpy().tobytes() == want2.tobytes()
        assert gm.dtype == np.float32 and gm.tobytes() == pm.numpy().tobytes() == dr.metres_of(want2, VOXEL).tobytes()
        assert gn.tobytes() == want.tobytes()
        # a second run, into buffers that hold the first one's result (the d2 passes run in place, the indices ping-pong)
        out = (to_dev(g2), to_dev(gm), to_dev(gn))
        h2, hm, hn = ops.distance_transform(d_classes, site_mask=2, cap=cap, voxel_size=VOXEL, out=out, nearest=True)
        assert h2 is out[0] and hn is out[2]
        assert h2.numpy().tobytes() == g2.tobytes() and hm.numpy().tobytes() == gm.tobytes() and hn.numpy().tobytes() == gn.tobytes()
    assert d_classes.numpy().tobytes() == classes.tobytes()


def test_invalid_class_bytes_are_never_sites(dev):
    from emfusion_amd import ops
    classes = np.full((4, 5, 70), 3, np.uint8)
    classes[2, 3, 41] = 200
    classes[1, 1, 1] = 2
    classes[3, 4, 69] = 0
    g2, gn = ops.distance_transform(to_dev(classes), site_mask=7, nearest=True)
    want2, want = nr.nearest_separable(dr.sites_of(classes, 7))
    assert g2.numpy().tobytes() == want2.tobytes() and gn.numpy().tobytes() == want.tobytes()
    gn = gn.numpy()
    assert gn[1, 1, 1] == (1 * 5 + 1) * 70 + 1 and gn[2, 3, 41] != (2 * 5 + 3) * 70 + 41
    assert set(np.unique(gn)) == {(1 * 5 + 1) * 70 + 1, (3 * 5 + 4) * 70 + 69}


# ---- the gather ----------------------------------------------------------------------------------------------------

def query_points(shape, n, seed):
    """n voxels (x, y, z): inside, on every face, one step outside on every side, far outside."""
    nz, ny, nx = shape
    rng = np.random.default_rng([seed, n])
    p = np.stack([rng.integers(-2, nx + 2, n), rng.integers(-2, ny + 2, n), rng.integers(-2, nz + 2, n)], 1).astype(np.int32)
    fixed = np.array([[0, 0, 0], [nx - 1, ny - 1, nz - 1], [-1, 0, 0], [nx, 0, 0], [0, -1, 0], [0, ny, 0], [0, 0, -1],
                      [0, 0, nz], [2 ** 31 - 1, 0, 0], [0, -2 ** 31, 0], [nx - 1, 0, nz - 1]], np.int32)
    k = min(n, len(fixed))
    p[n - k:] = fixed[:k]
    return p


def host_lookup(p, a, outside):
    nz, ny, nx = a.shape
    x, y, z = (p[:, i].astype(np.int64) for i in range(3))
    inside = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
    out = np.full(len(p), outside, a.dtype)
    out[inside] = a[z[inside], y[inside], x[inside]]
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_query_equals_host_indexing(dev, n):
    from emfusion_amd import ops
    shape = (9, 17, 65)
    sites, _, _ = expected(shape, "p01")
    classes = dr.classes_with_sites(sites, 2, seed=5)
    d_classes = to_dev(classes)
    d2, near = ops.distance_transform(d_classes, cap=5, nearest=True)
    h2, hn = d2.numpy(), near.numpy()
    assert (h2 == dr.FAR).any() and (h2 != dr.FAR).any()
    p = query_points(shape, n, 31)
    want = dict(classes=host_lookup(p, classes, 255), d2=host_lookup(p, h2, dr.FAR), nearest=host_lookup(p, hn, nr.NONE))
    arrays = dict(classes=d_classes, d2=d2, nearest=near)
    for keys in (("classes", "d2", "nearest"), ("classes",), ("d2",), ("nearest",), ("d2", "nearest"), ("classes", "nearest")):
        got = ops.distance_query(p, **{k: arrays[k] for k in keys})
        assert set(got) == set(keys)
        for k in keys:
            assert got[k].dtype == want[k].dtype and got[k].shape == (n,) and got[k].tobytes() == want[k].tobytes(), (n, keys, k)
    if n >= 11:
        assert (want["classes"] == 255).sum() >= 8 and (want["classes"] != 255).sum() >= 3
    # the inputs are only read
    assert d_classes.numpy().tobytes() == classes.tobytes() and d2.numpy().tobytes() == h2.tobytes() and near.numpy().tobytes() == hn.tobytes()
