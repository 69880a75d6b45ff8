"""The volumes of the world-mesh tests (CPU and GPU), computed once per process and left unchanged."""
import numpy as np

from tests import weld_volumes as WV

f32 = np.float32
_cache = {}


def fused(oracle, res):
    """weld_volumes.fused at a resolution of whole tiles: (tsdf, weights, voxel size)."""
    key = ("fused",) + tuple(res)
    if key not in _cache:
        t, w, _, vox = WV.fused(oracle, res)
        _cache[key] = (t, w, vox)
    return _cache[key]


def random_sign():
    """64 x 16 x 16, random signs, magnitudes uniform in [0.1, 1), weights all 1: 85481 vertices, up to 2030 surface
    cubes in one tile, and a cube that straddles the corner where all 8 tiles meet."""
    rng = np.random.default_rng(8)
    mag = rng.uniform(0.1, 1.0, size=(16, 16, 64))
    sign = rng.choice([-1.0, 1.0], size=(16, 16, 64))
    t = (mag * sign).astype(f32)
    return t, np.ones_like(t), 0.01


def colours(shape, seed=8):
    """A colour volume with a third of its voxels uncoloured (test_gpu_mesh_weld's recipe)."""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 65281, tuple(shape) + (4,), dtype=np.uint16)
    col[..., 3] = rng.integers(0, 3, shape) * 128
    return col
