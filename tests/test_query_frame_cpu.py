"""The frame the scene queries share (emfusion_amd.pipeline._BoxFrame, _metres_to_voxels) on the
host alone: box voxels to world points with the bytes of the float64 formula the GPU pipeline tests restate, world
points back to their voxels, points that are no points, linear indices, and the float32 rounding of metres."""
import numpy as np

from emfusion_amd.pipeline import _BoxFrame, _metres_to_voxels


def rot(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


R = (rot(2, 30.0) @ rot(0, 20.0)).astype(np.float32)  # not axis-aligned
T = np.array([0.35, -1.2, 2.05], np.float32)
RES, VOX, LO = (64, 48, 40), np.float32(0.01), (3, 5, 7)


def world64(vox):
    """The formula of tests/test_gpu_plan_pipeline.py world_of, before its one rounding to float32."""
    p = (np.asarray(vox, np.float64) + np.asarray(LO, np.float64) - (np.asarray(RES, np.float64) - 1) / 2.0) * np.float64(VOX)
    return p @ R.astype(np.float64).T + T.astype(np.float64)


def frame():
    return _BoxFrame(R, T, RES, VOX, LO)


def voxels(n=300):
    return np.random.default_rng(0x5EED).integers(-20, 80, size=(n, 3)).astype(np.int32)


def test_world_has_the_bytes_of_the_formula():
    v = voxels()
    got = frame().world(v)
    assert got.dtype == np.float32 and got.shape == v.shape
    assert got.tobytes() == world64(v).astype(np.float32).tobytes()


def test_to_voxels_inverts_world():
    v = voxels()
    got = frame().to_voxels(world64(v))
    assert got.dtype == np.int32 and (got == v).all()
    assert (frame().to_voxels(world64(v[0])) == v[:1]).all()  # one point is a list of one


def test_to_voxels_of_points_that_are_no_points():
    p = world64(np.array([[4, 5, 6]] * 4))
    p[0, 0], p[1, 1], p[2, 2] = np.nan, np.inf, -np.inf
    got = frame().to_voxels(p)
    # the rotation carries what is not finite to every axis (0 * inf and 0 * nan are nan too): -1 wherever it arrives
    with np.errstate(invalid="ignore"):
        q = (p[:3] - T.astype(np.float64)) @ R.astype(np.float64)
    assert ((got[:3] == -1) == ~np.isfinite(q)).all() and (got[:3] == -1).any(axis=1).all() and (got[3] == (4, 5, 6)).all()
    axis = _BoxFrame(np.eye(3, dtype=np.float32), T, RES, VOX, LO)  # axis-aligned: the coordinate itself
    pts = T.astype(np.float64) + np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, -1e30, 0]])
    got, centre = axis.to_voxels(pts), axis.to_voxels(T)[0]
    assert got[0, 0] == got[1, 1] == got[2, 2] == -1
    assert got[3].tolist() == [2 ** 31 - 1, -2 ** 31, centre[2]]  # clipped, not wrapped


def test_unravel_inverts_the_linear_index():
    nx, ny, nz = size = (5, 4, 3)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    got = _BoxFrame.unravel(((z * ny + y) * nx + x).reshape(-1), size)
    assert got.shape == (60, 3) and (got == np.stack([x, y, z], axis=-1).reshape(-1, 3)).all()
    assert _BoxFrame.unravel(np.zeros(0, np.int32), size).shape == (0, 3)


def test_metres_are_rounded_up_in_float32():
    assert int(np.ceil(0.07 / 0.01)) == 8  # the float64 quotient lies above 7
    assert _metres_to_voxels(0.07, 0.01) == 7
    assert _metres_to_voxels(0.0, 0.01) == 0
    assert _metres_to_voxels(0.0701, 0.01) == 8
    assert _metres_to_voxels(1e30, 0.01) == 4096 and _metres_to_voxels(np.inf, 0.01) == 4096
