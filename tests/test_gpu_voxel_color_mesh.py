"""Vertex colours of the meshes (emf_hip_meshColors / emf_hip_meshColorsBatched, Fusion.mesh_colors /
Fusion.meshes(colors=True)): colour volumes written directly through the EMF_VOL_COLOR pointer, so that what a vertex
must get is known without a second implementation of marching cubes."""
import ctypes as C

import numpy as np
import pytest

from tests import color_scene as cs
from tests.parity_util import to_dev
from tests.test_gpu_voxel_color import _run_pipeline

pytestmark = pytest.mark.gpu


def _color_view(fus, obj_id):
    """The model's colour volume as a writable device view."""
    from emfusion_amd import devmem, pipeline
    ptr, res = C.c_void_p(), (C.c_int32 * 3)()
    pipeline._check("emf_fusion_get_volume",
                    pipeline.load().emf_fusion_get_volume(fus._h, pipeline.VOL["color"], obj_id, C.byref(ptr), res))
    return devmem.DeviceView(ptr.value, (res[2], res[1], res[0], 4), np.uint16)


def _index_colours(shape):
    nz, ny, nx = shape[:3]
    c = np.empty((nz, ny, nx, 4), np.uint16)
    c[..., 0] = 256 * np.arange(nx)[None, None, :]
    c[..., 1] = 256 * np.arange(ny)[None, :, None]
    c[..., 2] = 256 * np.arange(nz)[:, None, None]
    c[..., 3] = 256
    return c


@pytest.fixture(scope="module")
def fused(dev):
    """The smoke scene after 3 frames with colour on (kept open for the module's tests)."""
    gen = _run_pipeline(3, True)
    for fus, oid, f, _, _ in gen:
        if f == 2:
            break  # the generator stays suspended: the handle stays open until gen.close()
    yield fus, oid
    gen.close()


def test_vertex_colours_follow_the_vertices(fused):
    """R, G, B = 256 * voxel index: every vertex colour is within 1 level of the vertex's own index coordinates
    v / voxelSize + (n - 1) / 2 -- rounding to u8 (<= 0.5) plus float error, not a measured number."""
    fus, oid = fused
    for who in (0, oid):
        view = _color_view(fus, who)
        assert max(view.shape[:3]) <= 128
        view.copy_from(_index_colours(view.shape))
        v, n, t = fus.mesh(who)
        c = fus.mesh_colors(who)
        assert len(v) > 500 and c.shape == (len(v), 3) and c.dtype == np.uint8
        vox = fus.params.bg_voxel_size if who == 0 else fus.object_info(who)["voxel_size"]
        res = np.array(view.shape[2::-1], np.float64)  # nx, ny, nz
        idx = v.astype(np.float64) / vox + (res - 1) / 2
        assert np.abs(c.astype(np.float64) - idx).max() <= 1.0, who
        assert len(np.unique(c, axis=0)) > 50  # they do vary
        # same count and order as mesh(): the batched call's slices, byte for byte
        both = fus.meshes([0, oid], colors=True)
        assert both[who][0].tobytes() == v.tobytes() and both[who][2].tobytes() == t.tobytes()
        assert both[who][3].tobytes() == c.tobytes()
        assert len(fus.meshes([0, oid])[who]) == 3


def test_constant_and_uncoloured_volumes(fused):
    fus, oid = fused
    view = _color_view(fus, oid)
    const = np.zeros(view.shape, np.uint16)
    const[...] = (200 * 256 + 77, 3 * 256 + 128, 255 * 256, 1)  # 200.3 -> 200, 3.5 -> 4 (half to even), 255
    view.copy_from(const)
    c = fus.mesh_colors(oid)
    assert len(c) > 100 and (c == np.array([200, 4, 255], np.uint8)).all()
    # every other x plane uncoloured: an edge with one coloured end takes that end's colour, one with none is black
    holes = const.copy()
    holes[:, :, 0::2, 3] = 0
    holes[:, :, 0::2, :3] = 999  # must not leak
    view.copy_from(holes)
    c = fus.mesh_colors(oid)
    kinds = {tuple(r) for r in np.unique(c, axis=0)}
    assert kinds == {(200, 4, 255), (0, 0, 0)}
    view.copy_from(np.zeros(view.shape, np.uint16))
    assert not fus.mesh_colors(oid).any()


def test_level1_and_batched_entries_agree(dev):
    """ops level: volumes fused on the device, random colour volumes; the batched call's slices equal the per-volume
    call, vertex for vertex, and the geometry equals the calls without colour."""
    from emfusion_amd import ops
    from tests.test_gpu_mesh_batched import fused as fuse_volume, vol
    rng = np.random.default_rng(8)
    vols = []
    for res, vox, cen in (((48, 40, 32), 0.0125, (0.25, 0.05, 1.3)), ((32, 32, 32), 0.015, (-0.3, -0.1, 1.6))):
        t, w = fuse_volume(ops, res, vox, cen)
        v = vol(t, w, vox)
        col = rng.integers(0, 65281, res[::-1] + (4,), dtype=np.uint16)
        col[..., 3] = rng.integers(0, 3, res[::-1]) * 128  # a third of the voxels uncoloured
        v["color"] = to_dev(col)
        vols.append(v)
    singles = [ops.extract_mesh(v["tsdf"], v["weights"], v["voxel_size"], color=v["color"]) for v in vols]
    plain = [ops.extract_mesh(v["tsdf"], v["weights"], v["voxel_size"]) for v in vols]
    batched = ops.extract_meshes(vols)
    for k in range(len(vols)):
        assert len(singles[k][0]) > 200
        for a, b in zip(singles[k][:3], plain[k]):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(batched[k], singles[k]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
        assert len(np.unique(singles[k][3], axis=0)) > 20
    # a table with a model that has no colour volume: that model's vertices are black, the other's unchanged
    vols[0]["color"] = None
    mixed = ops.extract_meshes(vols)
    assert not mixed[0][3].any() and mixed[1][3].tobytes() == singles[1][3].tobytes()


def test_mesh_colours_need_colour(dev):
    from emfusion_amd import pipeline
    for fus, oid, f, _, _ in _run_pipeline(1, False):
        with pytest.raises(pipeline.FusionError):
            fus.mesh_colors(0)
        with pytest.raises(pipeline.FusionError):
            fus.meshes([0], colors=True)
