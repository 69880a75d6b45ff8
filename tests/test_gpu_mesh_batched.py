"""Marching cubes over a table of volumes (emf_hip_meshCountBatched / emf_hip_meshEmitBatched): every model's slice of
the concatenated outputs is byte for byte the level-1 mesh of that volume alone, for mixed tables, more models than
one batch and the configs[4] share at full size; one volume is checked against the oracle directly."""
import numpy as np
import pytest

from tests.parity_util import to_dev
from tests.scenes import Pose, camera_path, intrinsics, render_depth, rel_OC

pytestmark = pytest.mark.gpu

W, H = 160, 120
K = intrinsics(W, H)
SPHERES = [((0.25, 0.05, 1.3), 0.22), ((-0.3, -0.1, 1.6), 0.18)]


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def fused(ops, res, vox, center, frames=2, seed=70):
    """A volume fused on the device from the synthetic spheres (res = (nx, ny, nz), centred at `center`)."""
    nx, ny, nz = res
    t = to_dev(np.zeros((nz, ny, nx), np.float32))
    w = to_dev(np.zeros((nz, ny, nx), np.float32))
    ones = to_dev(np.ones((H, W), np.float32))
    for i in range(frames):
        cam = camera_path(i)
        depth, _ = render_depth(W, H, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=seed + i)
        oc = rel_OC(cam, Pose(t=center))
        ops.update_tsdf(to_dev(depth), ones, t, w, oc.R32, oc.t32, K, vox, 10 * vox, 64.0)
    return t, w


def vol(tsdf, weights, vox, fg=None, grads=None):
    return dict(tsdf=tsdf, weights=weights, voxel_size=vox, fg_mask=fg, grads=grads)


def same_mesh(got, want, what=""):
    for g, w, name in zip(got, want, ("vertices", "normals", "triangles")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def single(ops, v):
    return ops.extract_mesh(v["tsdf"], v["weights"], v["voxel_size"], fg_mask=v["fg_mask"], grads=v["grads"])


def check_table(ops, vols):
    got = ops.extract_meshes(vols)
    assert len(got) == len(vols)
    for k, v in enumerate(vols):
        same_mesh(got[k], single(ops, v), f"model {k}")
    return got


@pytest.fixture(scope="module")
def mixed(ops, oracle):
    rng = np.random.default_rng(5)
    vols = []
    bt, bw = fused(ops, (512, 512, 512), 0.01, (0.0, 0.0, 1.4))
    vols.append(vol(bt, bw, 0.01))
    for k in range(4):  # 4 x 128^3 objects with foreground masks, two with materialised gradients
        c = SPHERES[k % 2][0]
        t, w = fused(ops, (128, 128, 128), 0.005, c, seed=80 + k)
        fg = to_dev((rng.uniform(size=(128, 128, 128)) < 0.95).astype(np.uint8) * 255)
        g = None
        if k % 2:
            g = to_dev(np.zeros((128, 128, 128, 3), np.float32))
            ops.compute_tsdf_grads(t, g)
        vols.append(vol(t, w, 0.005, fg=fg, grads=g))
    # a non-cubic volume, checked against the oracle too
    ht, hw = np.zeros((37, 22, 30), np.float32), np.zeros((37, 22, 30), np.float32)
    for i in range(2):
        cam = camera_path(i)
        depth, _ = render_depth(W, H, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=90 + i)
        oc = rel_OC(cam, Pose(t=SPHERES[0][0]))
        oracle.update_tsdf(depth, np.ones((H, W), np.float32), ht, hw, oc.R32, oc.t32, K, 0.02, 0.2, 64.0)
    vols.append(vol(to_dev(ht), to_dev(hw), 0.02))
    empty = np.zeros((40, 40, 40), np.float32)  # never observed: 0 vertices
    vols.insert(2, vol(to_dev(empty), to_dev(empty), 0.01))
    inside = -np.ones((24, 24, 24), np.float32)  # all inside: no sign change
    vols.insert(4, vol(to_dev(inside), to_dev(np.ones_like(inside)), 0.01))
    cube = np.array([-1, 1, 1, 1, 1, 1, 1, 1], np.float32).reshape(2, 2, 2)  # one cube, one corner inside
    vols.append(vol(to_dev(cube), to_dev(np.ones_like(cube)), 1.0))
    return vols, (ht, hw)


def test_mixed_table_slices_equal_the_level1_meshes(ops, oracle, mixed):
    vols, (ht, hw) = mixed
    got = check_table(ops, vols)
    counts = [len(g[0]) for g in got]
    assert counts[0] > 10000 and counts[2] == 0 and counts[4] == 0 and counts[-1] == 3
    assert all(c > 100 for k, c in enumerate(counts[:-1]) if k not in (2, 4))
    # independent check: the non-cubic volume against the oracle's marching cubes
    same_mesh(got[-2], oracle.marching_cubes(ht, hw, 0.02), "oracle")
    for _, _, tri in got:  # triangle indices are local to the model
        if len(tri):
            assert tri[:, 1:].min() == 0


def test_permuted_table_order(ops, mixed):
    vols, _ = mixed
    perm = np.random.default_rng(11).permutation(len(vols))
    base = ops.extract_meshes(vols)
    got = ops.extract_meshes([vols[i] for i in perm])
    for k, i in enumerate(perm):
        same_mesh(got[k], base[i], f"slot {k}")


def test_more_models_than_one_batch(ops):
    rng = np.random.default_rng(3)
    vols = []
    for k in range(65):
        n = int(rng.integers(16, 41))
        res = (n, int(rng.integers(16, 41)), int(rng.integers(16, 41)))
        t, w = fused(ops, res, 0.64 / n, SPHERES[k % 2][0], frames=1, seed=100 + k)
        vols.append(vol(t, w, 0.64 / n))
    got = check_table(ops, vols)
    assert sum(len(g[0]) for g in got) > 10000


def test_config4_share_at_full_size(ops):
    """configs[4]'s share: a 1024^3 background (offsets past 32 bits in bytes) and 2 x 256^3 objects."""
    vols = []
    bt, bw = fused(ops, (1024, 1024, 1024), 0.005, (0.0, 0.0, 1.4), frames=1)
    vols.append(vol(bt, bw, 0.005))
    for k in range(2):
        t, w = fused(ops, (256, 256, 256), 0.003, SPHERES[k][0], frames=1, seed=120 + k)
        vols.append(vol(t, w, 0.003))
    got = check_table(ops, vols)
    assert len(got[0][0]) > 100000
    del vols, bt, bw
