"""Per-voxel colour on the GPU: emf_hip_integrateColorBatched and the pipeline's colour pass against the numpy
restatement (tests/color_reference.py, itself pinned to the oracle) bit for bit, algebraic properties that need no
restatement, the resize copy, and "colour must not perturb geometry"."""
import hashlib

import numpy as np
import pytest

from tests import color_reference as ref
from tests import color_scene as cs
from tests.parity_util import to_dev
from tests.scenes import Pose, intrinsics, rel_OC, render_depth

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


class Vol:
    """Device side of one model of a level-3 table."""

    def __init__(self, ops, m, w, h, model_id):
        nx, ny, nz = m["res"]
        self.m = m
        self.tsdf = to_dev(np.zeros((nz, ny, nx), F))
        self.wts = to_dev(np.zeros((nz, ny, nx), F))
        self.color = to_dev(np.zeros((nz, ny, nx, 4), np.uint16))
        self.assoc = to_dev(np.zeros((h, w), F))
        self.img1 = to_dev(np.zeros((h, w), F))
        self.img3 = to_dev(np.zeros((h, w, 3), F))
        self.hit = to_dev(np.zeros((h, w), np.uint8))
        self.entry = ops.make_model(self.tsdf, self.wts, self.assoc, self.img1, self.img3, self.img3, self.hit,
                                    m["vox"], m["trunc"], cs.MAXW, 0.02, 0.8, 0.05, model_id=model_id)


def _assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere((got != want).any(-1))
    assert len(bad) == 0, (f"{what}: {len(bad)} voxels differ, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def test_kernel_matches_the_restatement_bit_for_bit(ops):
    """Level-3 entry on the smoke scene (background + object), 6 frames, seeded RGB noise: u16 equality of all four
    channels, with and without the 1 / lambda table."""
    models = [cs.BG, cs.OBJ]
    want = cs.run_reference(models)
    assert (want[0]["c"][..., 3] > 0).sum() >= 1000 and (want[1]["c"][..., 3] > 0).sum() >= 100
    # an object voxel fused with 0 < aw < 1: every weight of the maps is a multiple of 1 / 16 and the first frame's lands
    # unblended, so a colour weight that is no whole number can only come from a fractional association weight
    assert ((want[1]["c"][..., 3] % 256) != 0).any()
    K = intrinsics(cs.W, cs.H)
    for use_table in (False, True):
        vols = [Vol(ops, m, cs.W, cs.H, i) for i, m in enumerate(models)]
        table = ops.upload_models([v.entry for v in vols])
        il = None
        if use_table:
            il = to_dev(np.zeros((cs.H, cs.W), F))
            ops.compute_inv_lambda(K, il)
        stats = to_dev(np.zeros(1, np.uint64))
        frac_seen = False
        for f, (cam, depth, ids, rgb) in enumerate(cs.frames()):
            maps = cs.assoc_maps(ids, f)
            for v, a in zip(vols, maps):
                v.assoc.copy_from(a)
            frac_seen |= bool(((maps[1] > 0) & (maps[1] < 1)).any())
            poses = [(rel_OC(cam, m["pose"]).R32, rel_OC(cam, m["pose"]).t32) for m in models]
            ops.integrate_color_batched(table, [v.color for v in vols], poses, [m["res"] for m in models], None,
                                        to_dev(depth), to_dev(rgb), K, stats=stats, inv_lambda=il)
        assert frac_seen
        for name, v, s in zip(("background", "object"), vols, want):
            _assert_same(v.color.numpy(), s["c"], f"{name} (table={use_table})")
        assert int(stats.numpy()[0]) == want[0]["n"] + want[1]["n"]


def test_kernel_tile_and_row_tails_at_vga(ops):
    """640 x 480 against a 256^3 volume that the view cone cuts (culled tiles, tiles behind the camera), plus a
    volume whose sides are no multiples of the tile (tails in x, y and z)."""
    w, h = 640, 480
    K = intrinsics(w, h)
    cam = Pose(t=[0.02, -0.01, 0.3])  # inside the big volume: part of it lies behind the camera
    depth, ids = render_depth(w, h, K, cam, [cs.SPHERE], noise=0.002, dropout=0.01, seed=9)
    rgb = cs.rgb_noise(3, w, h)
    big = dict(res=(256, 256, 256), vox=0.01, trunc=0.03, pose=Pose(t=[0, 0, 1.28]))
    odd = dict(res=(38, 13, 27), vox=0.0125, trunc=0.05, pose=Pose(t=cs.SPHERE[0]))
    models = [big, odd]
    rng = np.random.default_rng(5)
    maps = [rng.choice(np.array([0, 0.5, 1], F), size=(h, w)).astype(F), np.where(ids == 1, F(0.75), F(0)).astype(F)]
    vols = [Vol(ops, m, w, h, i) for i, m in enumerate(models)]
    for v, a in zip(vols, maps):
        v.assoc.copy_from(a)
    table = ops.upload_models([v.entry for v in vols])
    poses = [(rel_OC(cam, m["pose"]).R32, rel_OC(cam, m["pose"]).t32) for m in models]
    d_depth, d_rgb = to_dev(depth), to_dev(rgb)
    stats = to_dev(np.zeros(1, np.uint64))
    for _ in range(2):  # the second pass blends into the first
        ops.integrate_color_batched(table, [v.color for v in vols], poses, [m["res"] for m in models], None, d_depth,
                                    d_rgb, K, stats=stats)
    counted = 0
    for name, m, v, a in zip(("256^3", "38x13x27"), models, vols, maps):
        nx, ny, nz = m["res"]
        t, wt = np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), F)
        c = np.zeros((nz, ny, nx, 4), np.uint16)
        oc = rel_OC(cam, m["pose"])
        n = 0
        for _ in range(2):
            n = ref.update(depth, a, t, wt, oc.R32, oc.t32, K, m["vox"], m["trunc"], cs.MAXW, rgb, c)
        assert n > 1000, name
        counted += 2 * n  # both passes colour the same voxels
        _assert_same(v.color.numpy(), c, name)
    assert int(stats.numpy()[0]) == counted  # the count's wave reduction in tiles with lanes beyond the volume


def _one_model(ops, assoc_value, rgb, visible=None, color0=None):
    K = intrinsics(cs.W, cs.H)
    cam, depth, ids, _ = cs.frames(1)[0]
    v = Vol(ops, cs.BG, cs.W, cs.H, 0)
    if color0 is not None:
        v.color.copy_from(color0)
    v.assoc.copy_from(np.full((cs.H, cs.W), assoc_value, F))
    table = ops.upload_models([v.entry])
    oc = rel_OC(cam, cs.BG["pose"])
    vis = None if visible is None else to_dev(np.array([visible], np.int32))
    ops.integrate_color_batched(table, [v.color], [(oc.R32, oc.t32)], [cs.BG["res"]], vis, to_dev(depth), to_dev(rgb), K)
    return v.color.numpy()


def test_constant_image_gives_exactly_that_colour(ops):
    rgb = np.empty((cs.H, cs.W, 3), np.uint8)
    rgb[...] = (201, 17, 255)
    c = _one_model(ops, 0.375, rgb)
    col = c[..., 3] > 0
    assert col.sum() >= 1000
    assert (c[col][:, :3] == np.array([201, 17, 255]) * 256).all()
    assert (c[col][:, 3] == 96).all()  # 0.375 * 256
    assert (c[~col] == 0).all()
    # a second, different constant image on top of it: still inside [min, max] of the two, weight doubled
    rgb2 = np.empty_like(rgb)
    rgb2[...] = (1, 17, 0)
    c2 = _one_model(ops, 0.375, rgb2, color0=c)
    assert (c2[col][:, 1] == 17 * 256).all() and (c2[col][:, 3] == 192).all()
    assert (c2[col][:, 0] == 101 * 256).all()  # (0.375 * 201 + 0.375 * 1) / 0.75, exact in float32


def test_zero_association_and_closed_gate_leave_the_volume_untouched(ops):
    rng = np.random.default_rng(3)
    start = rng.integers(0, 65536, cs.BG["res"][::-1] + (4,), dtype=np.uint16)
    rgb = cs.rgb_noise(0)
    assert np.array_equal(_one_model(ops, 0.0, rgb, color0=start), start)        # assoc == 0 everywhere
    assert np.array_equal(_one_model(ops, 1.0, rgb, visible=0, color0=start), start)  # invisible model
    assert not np.array_equal(_one_model(ops, 1.0, rgb, visible=1, color0=start), start)


def test_copy_color_values_shifts_and_zero_fills(ops):
    rng = np.random.default_rng(11)
    src = rng.integers(1, 65536, (10, 12, 14, 4), dtype=np.uint16)
    for dres, off in (((16, 16, 16), (-2, 1, 3)), ((8, 8, 8), (3, 2, 1)), ((14, 12, 10), (0, 0, 0))):
        dst = to_dev(np.full(dres[::-1] + (4,), 0xABCD, np.uint16))
        ops.copy_color_values(to_dev(src), dst, off)
        want = np.zeros(dres[::-1] + (4,), np.uint16)
        for z in range(dres[2]):
            for y in range(dres[1]):
                for x in range(dres[0]):
                    sx, sy, sz = x + off[0], y + off[1], z + off[2]
                    if 0 <= sx < 14 and 0 <= sy < 12 and 0 <= sz < 10:
                        want[z, y, x] = src[sz, sy, sx]
        assert np.array_equal(dst.numpy(), want), (dres, off)


# ---- through the pipeline ---------------------------------------------------------------------------

def _params():
    from emfusion_amd import pipeline
    return pipeline.make_params(cs.W, cs.H, 64, 0.04, 32, visibility_thresh=100, boundary=5)


def _pipeline_frames(n):
    """Static camera (process_rgbd takes no poses): the smoke scene with fresh noise, drop-outs and RGB per frame."""
    K = intrinsics(cs.W, cs.H)
    out = []
    for f in range(n):
        depth, ids = render_depth(cs.W, cs.H, K, Pose(), [cs.SPHERE], noise=0.002, dropout=0.01, seed=300 + f)
        out.append((depth, ids, cs.rgb_noise(50 + f)))
    return out


def _run_pipeline(n, color, rgb_on=True, skip_rgb=()):
    """Frame 0 through process_frame (device depth, the object's mask, set_color_image), the others through
    process_rgbd(depth, rgb).  Yields (fusion, object id, frame, depth, rgb) after every frame."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    fus = pipeline.Fusion(_params())
    try:
        if color:
            fus.enable_color()
        oid = fus.add_object(cs.SPHERE[0], cs.OBJ_SIZE)
        eye, zero = np.eye(3, dtype=F).reshape(-1), np.zeros(3, F)
        for f, (depth, ids, rgb) in enumerate(_pipeline_frames(n)):
            give = color and rgb_on and f not in skip_rgb
            if f == 0:
                d_depth, d_mask, d_rgb = to_dev(depth), to_dev((ids == 1).astype(np.uint8)), to_dev(rgb)
                if give:
                    fus.set_color_image(image_view(d_rgb))
                fus.process_frame(image_view(d_depth), eye, zero, {oid: (eye, np.array(cs.SPHERE[0], F))},
                                  {oid: image_view(d_mask)}, True)
            else:
                fus.process_rgbd(depth, rgb if give else None)
            fus.synchronize()
            yield fus, oid, f, depth, rgb if give else None
    finally:
        fus.close()


def test_pipeline_matches_the_restatement_bit_for_bit(dev):
    """Association weights, the depth the integration read (the z of the frame's points: pre-processed from frame 1
    on) and the visibility gate are the pipeline's own, read back per frame and fed to the restatement."""
    prm = _params()
    K = np.array(prm.K, F).reshape(3, 3)
    bg = dict(res=(64, 64, 64), vox=prm.bg_voxel_size, trunc=float(F(prm.bg_rel_truncdist) * F(prm.bg_voxel_size)),
              pose=Pose(t=list(prm.volume_pose_t)))
    state, frac, gated = None, 0, 0
    for fus, oid, f, _, rgb in _run_pipeline(cs.NFRAMES, True):
        info = fus.object_info(oid)
        Ro, to = fus.pose(oid)
        obj = dict(res=tuple(info["res"]), vox=info["voxel_size"], trunc=info["truncdist"], pose=Pose(Ro, to))
        if state is None:
            state = [np.zeros(m["res"][::-1] + (4,), np.uint16) for m in (bg, obj)]
        Rc, tc = fus.pose(0)
        cam = Pose(Rc, tc)
        depth = np.ascontiguousarray(fus.image("points")[..., 2])
        visible = [True, oid in fus.visible_objects()]
        gated += not visible[1]
        maps = [fus.image("bg_assoc"), fus.image("obj_assoc", oid)]
        for m, c, a, vis, who in zip((bg, obj), state, maps, visible, (0, oid)):
            if vis:
                nz, ny, nx = c.shape[:3]
                oc = rel_OC(cam, m["pose"])
                # float32 of the device's own pose product is not reproduced on the host: take R, t as the
                # restatement's inputs from the same double product the existing oracle pipeline uses
                ref.update(depth, a, np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), F), oc.R32, oc.t32, K,
                           m["vox"], m["trunc"], prm.max_tsdf_weight, rgb, c)
            _assert_same(fus.volume("color", who), c, f"frame {f}, model {who}")
        inband = state[1][..., 3] > 0
        frac += int(((maps[1] > 0) & (maps[1] < 1)).sum()) if visible[1] else 0
    assert (state[0][..., 3] > 0).sum() >= 1000 and (state[1][..., 3] > 0).sum() >= 100
    assert inband.any() and frac > 0
    # a fractional colour weight in the object proves a voxel was fused with 0 < aw < 1
    wq = state[1][..., 3]
    assert ((wq % 256) != 0).any()


def test_frame_without_a_colour_image_leaves_colour_untouched(dev):
    last = None
    for fus, oid, f, _, rgb in _run_pipeline(4, True, skip_rgb=(2,)):
        now = [fus.volume("color", 0), fus.volume("color", oid)]
        if f == 2:
            assert rgb is None
            assert all(np.array_equal(a, b) for a, b in zip(now, last))
        if f == 3:
            assert not np.array_equal(now[0], last[0])
        last = now
    assert (last[0][..., 3] > 0).sum() >= 1000


def test_reset_clears_colour_and_setter_is_refused_mid_run(dev):
    from emfusion_amd import pipeline
    gen = _run_pipeline(2, True)
    for fus, oid, f, _, _ in gen:
        if f == 1:
            assert (fus.volume("color", 0)[..., 3] > 0).any()
            with pytest.raises(pipeline.FusionError) as e:
                fus.enable_color(False)
            assert e.value.code == -4  # EMF_E_ARG
            fus.reset()
            assert not fus.volume("color", 0).any()
            fus.enable_color(False)
            with pytest.raises(pipeline.FusionError):
                fus.volume("color", 0)
            fus.enable_color(True)
            assert not fus.volume("color", 0).any()


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).hexdigest()


def test_colour_does_not_perturb_geometry(dev):
    """20 frames of the smoke scene: tsdf, weights, composite images and meshes have the same digests with the feature
    built and disabled as with enable_color() and RGB supplied."""
    def digests(color):
        out = {}
        for fus, oid, f, _, _ in _run_pipeline(20, color):
            if f % 5 == 4 or f == 19:
                for who in (0, oid):
                    out[f, who, "tsdf"] = _digest(fus.volume("tsdf", who))
                    out[f, who, "weights"] = _digest(fus.volume("weights", who))
                for im in ("raylengths", "vertices", "normals", "segmentation", "bg_assoc"):
                    out[f, im] = _digest(fus.image(im))
                out[f, "obj_assoc"] = _digest(fus.image("obj_assoc", oid))
                out[f, "vis"] = tuple(fus.visible_objects())
            if f == 19:
                for who in (0, oid):
                    for k, a in enumerate(fus.mesh(who)):
                        out["mesh", who, k] = _digest(a)
                if color:
                    assert (fus.volume("color", 0)[..., 3] > 0).sum() >= 1000
        return out
    off, on = digests(False), digests(True)
    assert off.keys() == on.keys()
    assert [k for k in off if off[k] != on[k]] == []


def test_resize_carries_colour(dev):
    """update_object with a mask that reaches beyond the volume: the overlapping region of the colour volume equals
    the old one shifted, the rest is zero."""
    from emfusion_amd.ops import image_view
    for fus, oid, f, depth, _ in _run_pipeline(2, True):
        if f != 1:
            continue
        before = fus.volume("color", oid)
        info0, (R0, t0) = fus.object_info(oid), fus.pose(oid)
        assert (before[..., 3] > 0).sum() >= 100
        # the sphere's silhouette plus a band of the wall to its right: the percentile box leaves the volume
        K = intrinsics(cs.W, cs.H)
        _, ids = render_depth(cs.W, cs.H, K, Pose(), [cs.SPHERE])
        mask = (ids == 1)
        ys, xs = np.nonzero(mask)
        mask[ys.min():ys.max(), xs.max():min(xs.max() + 40, cs.W)] = True
        off = fus.update_object(oid, image_view(to_dev(mask.astype(np.uint8))))
        assert np.abs(off).max() > 0, "the volume did not move: enlarge the mask"
        after = fus.volume("color", oid)
        info1 = fus.object_info(oid)
        n0, n1 = info0["res"][0], info1["res"][0]
        shift = np.rint(off / info0["voxel_size"]).astype(int) - (n1 - n0) // 2  # ObjTSDF::resize's pixOffset
        want = np.zeros_like(after)
        for z in range(n1):
            sz = z + shift[2]
            if not 0 <= sz < n0:
                continue
            for y in range(n1):
                sy = y + shift[1]
                if not 0 <= sy < n0:
                    continue
                x0, x1 = max(0, -shift[0]), min(n1, n0 - shift[0])
                if x1 > x0:
                    want[z, y, x0:x1] = before[sz, sy, x0 + shift[0]:x1 + shift[0]]
        assert want.any()
        assert np.array_equal(after, want)
