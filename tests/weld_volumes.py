"""The volumes of the welded-mesh tests (CPU and GPU): each returns (tsdf, weights, fg or None, voxel size)."""
import numpy as np

from tests.scenes import Pose, camera_path, intrinsics, render_depth, rel_OC

f32 = np.float32
W, H = 160, 120
K = intrinsics(W, H)
SPHERES = [((0.25, 0.05, 1.3), 0.22), ((-0.3, -0.1, 1.6), 0.18)]


def sphere(n=24, vox=0.05):
    """test_gpu_meshing's fully observed analytic sphere."""
    c = (np.arange(n, dtype=f32) - f32(n - 1) / 2) * f32(vox)
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    sdf = (np.sqrt(xx * xx + yy * yy + zz * zz) - f32(0.37)).astype(f32)
    return sdf, np.ones_like(sdf), None, vox


def masked_sphere():
    """The same sphere with 3 % unobserved voxels and 7 % masked out of the foreground."""
    sdf, _, _, vox = sphere()
    rng = np.random.default_rng(8)
    wts = (rng.uniform(size=sdf.shape) < 0.97).astype(f32)
    fg = (rng.uniform(size=sdf.shape) < 0.93).astype(np.uint8) * 255
    return sdf, wts, fg, vox


def zero_plane():
    """Exact zeros on voxels: vertexInterp's |val| < 1e-5 branches return the corner itself."""
    plane = np.zeros((6, 6, 6), f32)
    plane[:, :, :3] = -0.5
    plane[:, :, 3] = 0.0
    plane[:, :, 4:] = 0.5
    return plane, np.ones_like(plane), None, 0.02


def single_cube():
    tiny = np.array([[[-1, 1], [1, 1]], [[1, 1], [1, 1]]], f32)
    return tiny, np.ones_like(tiny), None, 1.0


def empties():
    z, ones = np.zeros((8, 8, 8), f32), np.ones((8, 8, 8), f32)
    return [(z, z, None, 0.01), (ones, ones, None, 0.01), (-ones, ones, None, 0.01)]


def random_sign():
    """Nx = 66, Ny = 7, Nz = 5, random signs, magnitudes uniform in [0.1, 1): rows shorter and longer than a wave, chunks
    that span rows and planes, the densest surface a chunk can hold (most vertices per chunk, most hash collisions)."""
    rng = np.random.default_rng(8)
    mag = rng.uniform(0.1, 1.0, size=(5, 7, 66))
    sign = rng.choice([-1.0, 1.0], size=(5, 7, 66))
    t = (mag * sign).astype(f32)
    return t, np.ones_like(t), None, 0.01


def fused(oracle, res, vox=None, frames=3, seed=50):
    """test_gpu_meshing's recipe: a few noisy depth frames of the sphere scene fused by the oracle."""
    nx, ny, nz = res
    vox = 0.64 / nx if vox is None else vox
    pose = Pose(t=SPHERES[0][0])
    tsdf, wts = np.zeros((nz, ny, nx), f32), np.zeros((nz, ny, nx), f32)
    for i in range(frames):
        cam = camera_path(i)
        depth, _ = render_depth(W, H, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=seed + i)
        oc = rel_OC(cam, pose)
        oracle.update_tsdf(depth, np.ones((H, W), f32), tsdf, wts, oc.R32, oc.t32, K, vox, 10 * vox, 64.0)
    return tsdf, wts, None, vox


def fused_masked(oracle):
    """(40, 36, 32) with the 93 % foreground mask."""
    tsdf, wts, _, vox = fused(oracle, (40, 36, 32), 0.016)
    fg = (np.random.default_rng(8).uniform(size=tsdf.shape) < 0.93).astype(np.uint8) * 255
    return tsdf, wts, fg, vox
