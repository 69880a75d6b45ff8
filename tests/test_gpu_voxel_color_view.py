"""Coloured views: Fusion.render_view(shading="color") -- the unchanged view kernel, then emf_hip_sampleColor and
emf_hip_renderPhongColor over its vertex / segmentation outputs -- against the label-shaded view with the colours
substituted in the colour map, the fall-back for voxels nobody coloured, and label shading left byte for byte as it was."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import color_scene as cs
from tests.parity_util import to_dev
from tests.test_gpu_voxel_color import _run_pipeline
from tests.test_gpu_voxel_color_mesh import _color_view

pytestmark = pytest.mark.gpu
F = np.float32
VIEW = (200, 150)  # not the frame's size


def _viewer():
    from emfusion_amd import pipeline
    R, t = pipeline.look_at((0.5, -0.3, -0.2), (0.05, 0.0, 1.3))
    f = 160.0
    K = np.array([f, 0, VIEW[0] / 2 - 0.5, 0, f, VIEW[1] / 2 - 0.5, 0, 0, 1], F)
    return R, t, K


@pytest.fixture(scope="module")
def scenes(dev):
    """The smoke scene after 4 frames, once with colour and once without (both kept open)."""
    gens, out = [], []
    for color in (True, False):
        gen = _run_pipeline(4, color)
        for fus, oid, f, _, _ in gen:
            if f == 3:
                break
        gens.append(gen)
        out.append((fus, oid))
    yield out
    for gen in gens:
        gen.close()


def _device_volume(fus, which, mid, dtype):
    from emfusion_amd import devmem, pipeline
    ptr, r = C.c_void_p(), (C.c_int32 * 3)()
    pipeline._check("emf_fusion_get_volume",
                    pipeline.load().emf_fusion_get_volume(fus._h, pipeline.VOL[which], mid, C.byref(ptr), r))
    return devmem.DeviceView(ptr.value, (r[2], r[1], r[0]), dtype)


def _label_view_with_map(fus, oid, cmap):
    """emf_hip_renderView on a table over the instance's own volumes with `cmap` as the colour map."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    prm = fus.params
    R, t, K = _viewer()
    one, hit = DeviceArray.zeros((1, 1), F), DeviceArray.zeros((1, 1), np.uint8)
    entries, poses = [], []
    for mid in (0, oid):
        if mid == 0:
            vox, trunc = prm.bg_voxel_size, F(prm.bg_rel_truncdist) * F(prm.bg_voxel_size)
            Rv, tv = np.eye(3), np.array(prm.volume_pose_t, np.float64)
        else:
            info = fus.object_info(mid)
            vox, trunc = info["voxel_size"], info["truncdist"]
            Rv, tv = (np.asarray(x, np.float64) for x in fus.pose(mid))
        fg = None if mid == 0 else _device_volume(fus, "fgmask", mid, np.uint8)
        entries.append(ops.make_model(_device_volume(fus, "tsdf", mid, F), _device_volume(fus, "weights", mid, F), one, one,
                                      one, one, hit, float(vox), float(trunc), prm.max_tsdf_weight, 0.02, 0.8, 1.0,
                                      model_id=mid, fg_mask=fg))
        poses.append((Rv.T @ np.asarray(R, np.float64), Rv.T @ (np.asarray(t, np.float64) - tv)))
    rgb = DeviceArray.zeros((VIEW[1], VIEW[0], 3), np.uint8)
    ops.render_view(ops.upload_models(entries), ops.upload_poses(poses), [oid], VIEW[0], VIEW[1], K, rgb, color_map=cmap)
    return rgb.numpy()


def _constant(view, rgb, w=256):
    c = np.zeros(view.shape, np.uint16)
    c[...] = (rgb[0] * 256, rgb[1] * 256, rgb[2] * 256, w)
    view.copy_from(c)


# sha256 of render_view (label shading) of this scene and viewer, recorded from the colour-off path of the parent commit
LABEL_VIEW_DIGEST = "63e9b508e5de8d44cea32c25b86c2ac4b994be2414b013f4994a8c4579dd3eac"


def test_label_shading_is_what_it_was(scenes):
    (fus_on, _), (fus_off, _) = scenes
    R, t, K = _viewer()
    off = fus_off.render_view(R, t, K, VIEW)
    on = fus_on.render_view(R, t, K, VIEW)
    assert (off[0].any(axis=2)).sum() > 5000 and len(np.unique(off[2])) >= 2  # background and object in view
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()  # enabling colour does not touch label shading
    assert hashlib.sha256(off[0].tobytes()).hexdigest() == LABEL_VIEW_DIGEST


def test_colour_view_equals_label_view_with_the_colours_in_the_map(scenes):
    (fus, oid), _ = scenes
    R, t, K = _viewer()
    label, ray, seg = fus.render_view(R, t, K, VIEW)
    _, cmap = fus.render()
    # the harness itself: the level-3 launch on the instance's volumes is the instance's label view
    assert _label_view_with_map(fus, oid, cmap).tobytes() == label.tobytes()
    c_bg, c_obj = (31, 200, 97), (250, 3, 128)
    _constant(_color_view(fus, 0), c_bg)
    _constant(_color_view(fus, oid), c_obj, w=1)
    colour, ray2, seg2 = fus.render_view(R, t, K, VIEW, shading="color")
    assert ray2.tobytes() == ray.tobytes() and seg2.tobytes() == seg.tobytes()
    cm2 = cmap.copy()
    cm2[0], cm2[oid] = c_bg, c_obj
    want = _label_view_with_map(fus, oid, cm2)
    assert (seg == oid).sum() > 300 and (seg[label.any(axis=2)] == 0).sum() > 3000
    assert colour.tobytes() == want.tobytes()
    assert colour.tobytes() != label.tobytes()
    # voxels nobody coloured fall back to the label colour: the whole object, then a slab of the background
    _constant(_color_view(fus, oid), (9, 9, 9), w=0)
    cm3 = cmap.copy()
    cm3[0] = c_bg
    assert fus.render_view(R, t, K, VIEW, shading="color")[0].tobytes() == _label_view_with_map(fus, oid, cm3).tobytes()
    view = _color_view(fus, 0)
    c = np.zeros(view.shape, np.uint16)
    c[...] = (c_bg[0] * 256, c_bg[1] * 256, c_bg[2] * 256, 256)
    c[:, :, : view.shape[2] // 2, 3] = 0  # the left half of the background volume: uncoloured
    view.copy_from(c)
    half = fus.render_view(R, t, K, VIEW, shading="color")[0]
    full_label = _label_view_with_map(fus, oid, cmap)
    full_colour = _label_view_with_map(fus, oid, cm3)
    same_l, same_c = (half == full_label).all(axis=2), (half == full_colour).all(axis=2)
    assert (same_l | same_c).all()  # every pixel is one or the other ...
    differ = (full_label != full_colour).any(axis=2)
    assert (same_l & differ).sum() > 500 and (same_c & differ).sum() > 500  # ... and both occur


def test_shading_choice_is_checked(scenes):
    from emfusion_amd import pipeline
    (fus_on, _), (fus_off, _) = scenes
    R, t, K = _viewer()
    with pytest.raises(pipeline.FusionError, match="needs colour"):
        fus_off.render_view(R, t, K, VIEW, shading="color")
    with pytest.raises(pipeline.FusionError, match="needs colour"):
        fus_off.set_3d_view_shading("color")
    fus_on.set_3d_view_shading("color")
    fus_on.set_3d_view_shading("label")
    with pytest.raises(KeyError):
        fus_on.render_view(R, t, K, VIEW, shading="texture")


def test_sample_and_shade_entries_on_their_own(dev):
    """ops level: nearest voxel without interpolation, rounding of 8.8 to the nearest level, labels without a model."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    n, vox = 8, 0.1
    col = np.zeros((n, n, n, 4), np.uint16)
    col[..., 0] = 256 * np.arange(n)[None, None, :] + 100  # x + 0.39 -> x
    col[..., 1] = 256 * np.arange(n)[None, :, None] + 128  # y + 0.5  -> y + 1
    col[..., 2] = 256 * np.arange(n)[:, None, None]
    col[..., 3] = 1
    col[0, 0, 0, 3] = 0
    zeros = to_dev(np.zeros((n, n, n), F))
    one, hit = DeviceArray.zeros((1, 1), F), DeviceArray.zeros((1, 1), np.uint8)
    entry = ops.make_model(zeros, zeros, one, one, one, one, hit, vox, 0.3, 64.0, 0.02, 0.8, 1.0)
    table = ops.upload_models([entry])
    half = (n - 1) / 2
    idx = np.array([[3.4, 2.6, 5.49], [0.2, 0.1, -0.3], [7.49, 0, 0], [7.6, 0, 0], [2, 2, 2], [0, 0, 0]], np.float64)
    verts = np.zeros((1, 6, 3), F)
    verts[0] = ((idx - half) * vox).astype(F)
    verts[0, 5] = 0  # no hit
    seg = np.array([[0, 0, 0, 0, 7, 0]], np.uint8)
    cmap = np.zeros((256, 3), np.uint8)
    cmap[0], cmap[7] = (1, 2, 3), (70, 71, 72)
    out = DeviceArray.zeros((1, 6, 3), np.uint8)
    ops.sample_color(table, [to_dev(col)], [(np.eye(3), np.zeros(3))], [], to_dev(verts), to_dev(seg), cmap, out)
    got = out.numpy()[0]
    assert got.tolist() == [[3, 4, 5],      # nearest voxel (3, 3, 5): 3.39 -> 3, 3.5 -> 4, 5
                            [1, 2, 3],      # voxel (0, 0, 0) is uncoloured: label colour
                            [7, 1, 0],      # still inside
                            [1, 2, 3],      # rounds to x = 8: outside the volume
                            [70, 71, 72],   # a label no slot carries
                            [0, 0, 0]]      # no vertex
    # the shading from the colour image equals the label shading when the image holds the label colours
    rng = np.random.default_rng(2)
    v = rng.normal(size=(12, 16, 3)).astype(F) + np.array([0, 0, 2], F)
    v[0, :4] = 0
    nrm = rng.normal(size=(12, 16, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    s = rng.integers(0, 5, (12, 16), dtype=np.uint8)
    cm = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    a, b = DeviceArray.zeros((12, 16, 3), np.uint8), DeviceArray.zeros((12, 16, 3), np.uint8)
    ops.render_phong(to_dev(v), to_dev(nrm), to_dev(s), cm, a)
    ops.render_phong_color(to_dev(v), to_dev(nrm), to_dev(cm[s]), b)
    assert a.numpy().tobytes() == b.numpy().tobytes() and a.numpy().any()
