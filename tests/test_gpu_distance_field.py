"""The distance-field kernels (include/emf_hip.h "Distance field"; ops.occupancy_classes,
ops.stamp_objects, ops.distance_transform) against tests/distance_reference.py.  Every comparison is tobytes()
equality: the classes are single float comparisons, the stamping is restated in float32 operation by operation, and
the squared distance is an integer."""
import numpy as np
import pytest

from tests import distance_reference as dr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

VOXEL = 0.04
_expected = {}


def expected_d2(shape, content, site_mask):
    """(classes, sites-only d2 without a cap), computed once per case and shared."""
    key = (shape, content, site_mask)
    if key not in _expected:
        sites = dr.site_field(shape, content, seed=11)
        classes = dr.classes_with_sites(sites, site_mask, seed=5)
        d2 = dr.d2_scipy(sites)
        if sites.size <= dr.BRUTE_LIMIT:
            assert d2.tobytes() == dr.d2_brute(sites).tobytes()
        for a in (classes, d2):
            a.setflags(write=False)
        _expected[key] = (classes, d2)
    return _expected[key]


@pytest.mark.parametrize("content", dr.CONTENTS)
@pytest.mark.parametrize("shape", dr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_transform_is_exact(dev, shape, content):
    from emfusion_amd import ops
    for site_mask in (2, 6, 1):
        classes, d2 = expected_d2(shape, content, site_mask)
        d_classes = to_dev(classes)
        for cap in (0, 1, 5):
            got = ops.distance_transform(d_classes, site_mask=site_mask, cap=cap).numpy()
            want = dr.apply_cap(d2, cap)
            assert got.dtype == np.int32 and got.shape == shape
            assert got.tobytes() == want.tobytes(), \
                (shape, content, site_mask, cap, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert d_classes.numpy().tobytes() == classes.tobytes()  # the input is only read


@pytest.mark.parametrize("content", ["none", "far_corner", "p01", "all"])
@pytest.mark.parametrize("shape", [(9, 17, 65), (2, 600, 3), (600, 3, 2), (5, 1, 70)], ids=lambda s: "x".join(str(v) for v in s))
def test_metres_and_repeatability(dev, shape, content):
    from emfusion_amd import ops
    classes, d2 = expected_d2(shape, content, 2)
    d_classes = to_dev(classes)
    for cap in (0, 5):
        want = dr.apply_cap(d2, cap)
        g2, gm = ops.distance_transform(d_classes, site_mask=2, cap=cap, voxel_size=VOXEL)
        g2, gm = g2.numpy(), gm.numpy()
        assert g2.tobytes() == want.tobytes()
        assert gm.dtype == np.float32 and gm.tobytes() == dr.metres_of(want, VOXEL).tobytes()
        assert np.isposinf(gm[want == dr.FAR]).all() and np.isfinite(gm[want != dr.FAR]).all()
        # a second run, into buffers that hold the first one's result (the passes run in place)
        out = (to_dev(g2), to_dev(gm))
        h2, hm = ops.distance_transform(d_classes, site_mask=2, cap=cap, voxel_size=VOXEL, out=out)
        assert h2.numpy().tobytes() == g2.tobytes() and hm.numpy().tobytes() == gm.tobytes()
    assert d_classes.numpy().tobytes() == classes.tobytes()


def test_invalid_class_bytes_are_never_sites(dev):
    from emfusion_amd import ops
    classes = np.full((4, 5, 70), 3, np.uint8)
    classes[2, 3, 41] = 200
    classes[1, 1, 1] = 2
    got = ops.distance_transform(to_dev(classes), site_mask=7).numpy()
    assert got.tobytes() == dr.distance_transform(classes, 7).tobytes() and got[1, 1, 1] == 0 and got[2, 3, 41] != 0


def volume_values(shape, seed):
    """Random tsdf / weights with the values the class rule names: -0.0, NaN, weight 0, negative and NaN weights."""
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, shape).astype(np.float32)
    wts = rng.uniform(0.5, 64, shape).astype(np.float32)
    k = rng.integers(0, 12, shape)
    tsdf[k == 0] = -0.0
    tsdf[k == 1] = np.nan
    tsdf[k == 2] = 0.0
    wts[k == 3] = 0.0
    wts[k == 4] = -1.0
    wts[k == 5] = np.nan
    wts[k == 6] = -0.0
    return tsdf, wts


@pytest.mark.parametrize("nx", [5, 33, 66, 260])
def test_classes(dev, nx):
    from emfusion_amd import ops
    ny, nz = 7, 6
    tsdf, wts = volume_values((nz, ny, nx), 0xDF00 + nx)
    d_t, d_w = to_dev(tsdf), to_dev(wts)
    boxes = [None, ((1, 1, 1), (nx - 2, 5, 3)), ((3, 0, 5), (nx - 3, 7, 1)), ((0, 2, 0), (1, 3, 6)),
             ((nx - 4, 0, 0), (4, 7, 6)) if nx % 4 == 0 else ((1, 3, 1), (nx - 1, 1, 1))]
    for box in boxes:
        want = dr.classes_of(tsdf, wts, box)
        got = ops.occupancy_classes(d_t, d_w, box=box).numpy()
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (nx, box)
        assert set(np.unique(want)) == {0, 1, 2} or want.size < 30
    assert d_t.numpy().view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes()
    assert d_w.numpy().view(np.uint32).tobytes() == wts.view(np.uint32).tobytes()


# ---- stamping ------------------------------------------------------------------------------------------------------

BG_RES, BG_VOXEL = (48, 48, 48), 0.02


def sphere_object(voxel, n=24, seed=1):
    """A solid sphere of radius 8 voxels in an n^3 volume: tsdf negative inside, weights with holes, negative and NaN
    entries, a foreground mask a little wider than the sphere."""
    rng = np.random.default_rng(seed)
    c = (np.arange(n, dtype=np.float32) - np.float32(n - 1) / 2) * np.float32(voxel)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    tsdf = np.clip((r - np.float32(8 * voxel)) / np.float32(3 * voxel), -1, 1).astype(np.float32)
    wts = np.where(rng.random(r.shape) < 0.15, 0.0, rng.uniform(1, 5, r.shape)).astype(np.float32)
    k = rng.integers(0, 40, r.shape)
    wts[k == 0] = -2.0
    tsdf[k == 1] = np.nan
    tsdf[k == 2] = -0.0
    fg = (r < np.float32(10.5 * voxel)).astype(np.uint8)
    return tsdf, wts, fg


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


EYE = np.eye(3, dtype=np.float32)
POSES = {
    "identity": (0.02, EYE, (0.0, 0.0, 0.0)),
    "whole_voxels": (0.02, EYE, (3 * 0.02, -2 * 0.02, 1 * 0.02)),
    "oblique_rotation": (0.02, rotation((1, 2, 3), 0.7), (0.05, -0.03, 0.02)),
    "coarser_object": (0.03, rotation((3, -1, 2), 0.3), (0.01, 0.02, -0.04)),
    "finer_object": (0.013, rotation((0, 1, 1), 1.1), (-0.06, 0.0, 0.03)),
    "partly_outside": (0.02, rotation((1, 0, 1), 0.2), (0.4, 0.1, -0.35)),
}
BOXES = {"whole": None, "box": ((5, 3, 1), (30, 40, 44))}


def run_stamp(objects_host, box, seed=9):
    """(initial classes, device result, reference, union of the objects' sub-boxes as a bool volume of the box)."""
    from emfusion_amd import ops
    (x0, y0, z0), (sx, sy, sz) = box if box is not None else ((0, 0, 0), BG_RES)
    start = np.random.default_rng(seed).integers(0, 3, (sz, sy, sx)).astype(np.uint8)
    dev_objs = [(to_dev(t), to_dev(w), None if f is None else to_dev(f), vo, R, tt) for t, w, f, vo, R, tt in objects_host]
    table = ops.occupancy_objects(dev_objs, BG_RES, BG_VOXEL)
    got = ops.stamp_objects(to_dev(start), BG_RES, BG_VOXEL, (table, len(dev_objs)), box=box).numpy()
    want = dr.stamp(start, BG_RES, BG_VOXEL, box, objects_host)
    union = np.zeros(start.shape, bool)
    for k in range(len(dev_objs)):
        lo, size = list(table[k].lo), list(table[k].size)
        a = [max(lo[i] - o, 0) for i, o in enumerate((x0, y0, z0))]
        b = [max(lo[i] + max(size[i], 0) - o, 0) for i, o in enumerate((x0, y0, z0))]
        union[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = True
    return start, got, want, union


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("pose", list(POSES))
def test_stamp_one_object(dev, pose, box):
    vo, R, t = POSES[pose]
    tsdf, wts, fg = sphere_object(vo)
    start, got, want, union = run_stamp([(tsdf, wts, fg, vo, R, t)], BOXES[box])
    assert got.tobytes() == want.tobytes(), (pose, box, int((got != want).sum()))
    changed = want != start
    assert changed.sum() > (50 if pose == "partly_outside" else 300)  # the object does land in the box
    assert (want[changed] == dr.OCCUPIED).all() and not changed[~union].any()
    assert got[~union].tobytes() == start[~union].tobytes()  # nothing outside the object's sub-box is touched
    if pose in ("identity", "whole_voxels") and box == "whole":
        assert union.sum() == 28 ** 3  # the launch covers the object's sub-box, not the background


def test_stamp_foreground_mask(dev):
    vo, R, t = POSES["oblique_rotation"]
    tsdf, wts, fg = sphere_object(vo)
    start, got, want, _ = run_stamp([(tsdf, wts, None, vo, R, t)], None)  # NULL: no gate
    assert got.tobytes() == want.tobytes()
    gated = dr.stamp(start, BG_RES, BG_VOXEL, None, [(tsdf, wts, fg, vo, R, t)])
    assert (want != start).sum() >= (gated != start).sum() > 0
    start, got, want, _ = run_stamp([(tsdf, wts, np.zeros_like(fg), vo, R, t)], None)  # all zero: nothing is solid
    assert got.tobytes() == want.tobytes() == start.tobytes()


def test_stamp_33_objects_take_two_launches(dev):
    tsdf, wts, fg = sphere_object(0.02, n=12, seed=4)
    tsdf = (tsdf - np.float32(1.0)).astype(np.float32)  # 8-voxel radius in a 12^3 volume: solid throughout
    objects = []
    for k in range(33):
        centre = np.array([(k % 4) * 11 + 6 - 23.5, ((k // 4) % 3) * 15 + 8 - 23.5, (k // 12) * 15 + 8 - 23.5]) * BG_VOXEL
        R = rotation((1 + k, 2, 3), 0.1 * k)
        objects.append((tsdf, wts, fg if k % 2 else None, 0.02, R, (-(R.astype(np.float64) @ centre)).astype(np.float32)))
    start, got, want, union = run_stamp(objects, None)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())
    last = dr.stamp(start, BG_RES, BG_VOXEL, None, objects[32:])
    assert (last != start).sum() > 100  # the 33rd object, alone in the second launch, does stamp
    assert got[~union].tobytes() == start[~union].tobytes()


def test_classes_with_objects_and_the_composed_field(dev):
    from emfusion_amd import ops
    vo, R, t = POSES["oblique_rotation"]
    tsdf, wts, fg = sphere_object(vo)
    bg_t, bg_w = volume_values(BG_RES[::-1], 77)
    bg_t[np.isnan(bg_t)] = 0.5
    bg_t = np.abs(bg_t) + np.float32(0.1)  # a background without a surface: the object is the only obstacle
    box = BOXES["box"]
    objs = [(to_dev(tsdf), to_dev(wts), to_dev(fg), vo, R, t)]
    want_c = dr.stamp(dr.classes_of(bg_t, bg_w, box), BG_RES, BG_VOXEL, box, [(tsdf, wts, fg, vo, R, t)])
    d_t, d_w = to_dev(bg_t), to_dev(bg_w)
    got_c = ops.occupancy_classes(d_t, d_w, box=box, objects=objs, voxel_size=BG_VOXEL)
    assert got_c.numpy().tobytes() == want_c.tobytes() and (want_c == dr.OCCUPIED).sum() > 300
    classes, d2, metres = ops.distance_field(d_t, d_w, BG_VOXEL, box=box, objects=objs, site_mask=6, cap=7)
    want = dr.distance_transform(want_c, 6, 7)
    assert classes.numpy().tobytes() == want_c.tobytes() and d2.numpy().tobytes() == want.tobytes()
    assert metres.numpy().tobytes() == dr.metres_of(want, BG_VOXEL).tobytes()
