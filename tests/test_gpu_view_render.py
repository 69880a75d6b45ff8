"""The free-viewpoint view (emf_hip_renderView, EMFusion::renderView, the --3d-vis log).

Bar: bit-identical to the chain it fuses -- per-model raycast at the viewer's pose, composite with a zeroed diff
buffer, hide, Phong with the light at the viewer -- whether that chain runs in the oracle or as the existing GPU
launches, at any viewpoint, size and intrinsics, for any number of models in one launch; and invisible to the frame
path."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.oracle_pipeline import Affine32
from tests.parity_util import dev_full, to_dev, to_np
from tests.scenes import Pose, camera_path, intrinsics, rel_OC, render_depth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = 160, 120  # frames the scene is fused from
K = intrinsics(W, H)
SPHERES = [((0.25, 0.05, 1.3), 0.22), ((-0.3, -0.1, 1.6), 0.18), ((0.05, 0.3, 1.15), 0.12)]
IDS = [3, 7, 200]  # labels of the three objects (not the slot numbers)
MAXW = 64.0
SIGMA, ALPHA, PRIOR = 0.02, 0.8, 1.0
CMAP = np.random.default_rng(11).integers(0, 256, (256, 3)).astype(np.uint8)
SIZES = [(97, 61), (256, 192)]


def view_K(w, h):
    """fx != fy and an off-centre principal point"""
    return np.array([[0.9 * w, 0, 0.43 * w], [0, 1.05 * w, 0.56 * h], [0, 0, 1]], np.float32)


def viewers():
    from emfusion_amd.pipeline import look_at
    return {
        "inside_background": look_at((0.1, -0.15, 0.3), (0.0, 0.0, 1.5)),
        "outside_looking_in": look_at((1.6, -1.1, -1.2), (0.0, 0.1, 1.4)),
        "steep_from_above": look_at((0.1, -2.2, 1.0), (0.0, 0.2, 1.35)),
        "inside_object_box": look_at((0.25, 0.0, 1.0), SPHERES[0][0]),
    }


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0]}: {got[tuple(bad[0])]} vs " \
                          f"{want[tuple(bad[0])]}"


class Vol:
    """One volume integrated identically on the oracle and the device."""

    def __init__(self, ops, oracle, res, vox, pose, obj_id):
        self.ops, self.oracle = ops, oracle
        self.res, self.vox, self.pose, self.id = res, np.float32(vox), pose, obj_id
        self.tsdf = np.zeros((res[2], res[1], res[0]), np.float32)
        self.wts = np.zeros_like(self.tsdf)
        self.d_tsdf, self.d_wts = to_dev(self.tsdf), to_dev(self.wts)
        self.vmask = None
        if obj_id:
            self.fgbg = np.zeros(self.tsdf.shape + (2,), np.float32)

    @property
    def trunc(self):
        return np.float32(10) * self.vox

    def integrate(self, cam, depth, ids):
        oc = rel_OC(cam, self.pose)
        assoc = np.ones((H, W), np.float32)
        self.oracle.update_tsdf(depth, assoc, self.tsdf, self.wts, oc.R32, oc.t32, K, self.vox, self.trunc, MAXW)
        self.ops.update_tsdf(to_dev(depth), to_dev(assoc), self.d_tsdf, self.d_wts, oc.R32, oc.t32, K, self.vox,
                             self.trunc, MAXW)
        if self.id:
            sid = SPHERE_OF[self.id]
            self.oracle.update_fgbg_probs((ids == sid + 1).astype(np.uint8), np.zeros((H, W), np.uint8), self.tsdf,
                                          self.wts, self.fgbg, oc.R32, oc.t32, K, self.vox)
            self.probs, self.vmask = self.oracle.compute_fg_probs(self.fgbg)
            self.d_probs, self.d_vmask = to_dev(self.probs), to_dev(self.vmask)

    def entry(self, w, h):
        """A table entry with view-sized per-model images (what the GPU chain raycasts into)."""
        imgs = dict(assoc=dev_full((h, w), 1.0), ray=dev_full((h, w), 5.0), vert=dev_full((h, w, 3), 5.0),
                    nrm=dev_full((h, w, 3), 5.0), hit=dev_full((h, w), 5, np.uint8))
        e = self.ops.make_model(self.d_tsdf, self.d_wts, imgs["assoc"], imgs["ray"], imgs["vert"], imgs["nrm"],
                                imgs["hit"], float(self.vox), float(self.trunc), MAXW, SIGMA, ALPHA, PRIOR,
                                model_id=self.id, fg_probs=self.d_probs if self.id else None,
                                fg_mask=self.d_vmask if self.id else None,
                                rcp_voxel=self.ops.voxel_reciprocal(self.vox))
        return e, imgs


SPHERE_OF = {i: k for k, i in enumerate(IDS)}


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scene(ops, oracle, dev):
    vols = [Vol(ops, oracle, (64, 64, 64), 0.04, Pose(t=[0, 0, 1.28]), 0)]
    vols += [Vol(ops, oracle, (32, 32, 32), 0.025, Pose(t=SPHERES[k][0]), IDS[k]) for k in range(3)]
    for i in range(4):
        cam = camera_path(i)
        depth, ids = render_depth(W, H, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=300 + i)
        for v in vols:
            v.integrate(cam, depth, ids)
    dev.synchronize()
    return vols


def viewer_to_volume(viewer, vols, poses=None):
    """viewer -> volume per slot in float32 (emf::Affine3f arithmetic: vol.inv() * viewer)."""
    Rv, tv = viewer
    out = []
    for k, v in enumerate(vols):
        vp = poses[k] if poses is not None else Affine32(v.pose.R, v.pose.t)
        vo = vp.inv() * Affine32(Rv, tv)
        out.append((vo.R, vo.t))
    return out


def oracle_chain(oracle, vols, poses_vo, labels, w, h, Kv, hide=()):
    outs = [oracle.raycast_tsdf(v.tsdf, None, v.wts, v.vmask if v.id else None, w, h, R, t, Kv, v.vox, v.trunc,
                                count_steps=True)
            for v, (R, t) in zip(vols, poses_vo)]
    bg, obj = outs[0], outs[1:]
    diff = np.zeros((h, w), np.float32)
    ray, vert, nrm, seg, _, _ = oracle.composite_raycast(labels, [o[0] for o in obj], [o[1] for o in obj],
                                                         [o[2] for o in obj], [o[3] for o in obj], bg[0], bg[1],
                                                         bg[2], bg[3], diff, 0)
    for s in hide:  # emf_hip_hideLabel, restated
        m = seg == s
        seg[m] = 0
        vert[m] = bg[1][m]
        nrm[m] = bg[2][m]
    rgb = oracle.render_phong(vert, nrm, seg, CMAP, light=(0.0, 0.0, 0.0))
    stats = (sum(int(o[4].sum()) for o in outs), sum(int(o[3].sum()) for o in outs))
    return rgb, ray, seg, vert, nrm, stats


def render_view(ops, table, poses_vo, labels, w, h, Kv, hide=(), pad=0):
    rgb = dev_full((h, w, 3), 77, np.uint8, pad_cols=pad)
    ray = dev_full((h, w), 9.0, pad_cols=pad)
    seg = dev_full((h, w), 77, np.uint8, pad_cols=pad)
    vert = dev_full((h, w, 3), 9.0, pad_cols=pad)
    nrm = dev_full((h, w, 3), 9.0, pad_cols=pad)
    st = dev_full((4,), 0, np.uint64)
    ops.render_view(table, poses_vo, labels, w, h, Kv, rgb, ray, seg, vert, nrm, color_map=CMAP, hide=hide, stats=st)
    return [to_np(a) for a in (rgb, ray, seg, vert, nrm)], to_np(st)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("view", ["inside_background", "outside_looking_in", "steep_from_above", "inside_object_box"])
def test_view_equals_the_oracle_chain(ops, oracle, scene, view, size):
    w, h = size
    Kv = view_K(w, h)
    pv = viewer_to_volume(viewers()[view], scene)
    entries = [v.entry(w, h) for v in scene]
    table = ops.upload_models([e for e, _ in entries])
    got, st = render_view(ops, table, pv, IDS, w, h, Kv, pad=3 if w < 100 else 0)
    want = oracle_chain(oracle, scene, pv, IDS, w, h, Kv)
    for g, wnt, name in zip(got, want[:5], ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
        assert_bits(g, wnt, f"{view} {w}x{h} {name}")
    assert (got[2] != 0).sum() > 0 or view == "inside_object_box", "no object in view"
    assert (got[0].any(axis=2)).sum() > w * h // 20, "almost nothing in view"
    assert int(st[0]) == want[5][0] and int(st[1]) == want[5][1], (st, want[5])
    for _, imgs in entries:  # nothing of the table is written
        assert np.all(to_np(imgs["ray"]) == 5.0) and np.all(to_np(imgs["hit"]) == 5)


@pytest.mark.parametrize("view", ["inside_background", "outside_looking_in", "steep_from_above", "inside_object_box"])
def test_view_equals_the_gpu_chain(ops, scene, view):
    w, h = SIZES[1]
    Kv = view_K(w, h)
    pv = viewer_to_volume(viewers()[view], scene)
    entries = [v.entry(w, h) for v in scene]
    table = ops.upload_models([e for e, _ in entries])
    got, _ = render_view(ops, table, pv, IDS, w, h, Kv)
    want = gpu_chain(ops, table, entries, pv, [v.res for v in scene], IDS, w, h, Kv)
    for g, wnt, name in zip(got, want, ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
        assert_bits(g, wnt, f"{view} {name}")


def gpu_chain(ops, table, entries, pv, res, labels, w, h, Kv, hide=()):
    """emf_hip_raycastBatched -> emf_hip_compositeRaycast (zeroed diff) -> hideLabel -> renderPhong"""
    ops.raycast_batched(table, pv, res, w, h, Kv)
    im = [i for _, i in entries]
    ray, seg, no_obj = dev_full((h, w), 0.0), dev_full((h, w), 0, np.uint8), dev_full((h, w), 0, np.uint8)
    vert, nrm, diff = dev_full((h, w, 3), 0.0), dev_full((h, w, 3), 0.0), dev_full((h, w), 0.0)
    vis = dev_full((max(len(labels), 1),), 0, np.int32)
    ops.composite_raycast(labels, [i["ray"] for i in im[1:]], [i["vert"] for i in im[1:]], [i["nrm"] for i in im[1:]],
                          [i["hit"] for i in im[1:]], im[0]["ray"], im[0]["vert"], im[0]["nrm"], im[0]["hit"], ray,
                          vert, nrm, seg, diff, no_obj, 0, vis)
    for s in hide:
        ops.hide_label(seg, s, vert, nrm, im[0]["vert"], im[0]["nrm"])
    rgb = dev_full((h, w, 3), 0, np.uint8)
    ops.render_phong(vert, nrm, seg, CMAP, rgb)
    return [to_np(a) for a in (rgb, ray, seg, vert, nrm)]


def test_more_models_than_one_batch_in_one_launch(ops, oracle, scene):
    """1 + 40 objects (the three volumes reused at 40 poses, 40 labels): one launch, the oracle's composite."""
    w, h = SIZES[0]
    Kv = view_K(w, h)
    rng = np.random.default_rng(5)
    vols, poses = [scene[0]], [Affine32(scene[0].pose.R, scene[0].pose.t)]
    for k in range(40):
        v = scene[1 + k % 3]
        vols.append(v)
        c = np.array(SPHERES[k % 3][0]) + rng.uniform(-0.5, 0.5, 3) * np.array([1.0, 0.6, 0.8])
        poses.append(Affine32(np.eye(3), c.astype(np.float32)))
    labels = [20 + k for k in range(40)]
    viewer = viewers()["outside_looking_in"]
    pv = viewer_to_volume(viewer, vols, poses)
    table = ops.upload_models([v.entry(4, 4)[0] for v in vols])
    got, st = render_view(ops, table, pv, labels, w, h, Kv)
    want = oracle_chain(oracle, vols, pv, labels, w, h, Kv)
    for g, wnt, name in zip(got, want[:5], ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
        assert_bits(g, wnt, f"41 models {name}")
    assert len(set(np.unique(got[2])) - {0}) > 8, "the composite should see many of the objects"
    assert int(st[0]) == want[5][0]


def test_hidden_labels_show_the_background(ops, oracle, scene):
    w, h = SIZES[1]
    Kv = view_K(w, h)
    pv = viewer_to_volume(viewers()["outside_looking_in"], scene)
    table = ops.upload_models([v.entry(4, 4)[0] for v in scene])
    plain, _ = render_view(ops, table, pv, IDS, w, h, Kv)
    assert (plain[2] == IDS[0]).sum() > 50, "the hidden object must be in view"
    got, _ = render_view(ops, table, pv, IDS, w, h, Kv, hide=(IDS[0],))
    want = oracle_chain(oracle, scene, pv, IDS, w, h, Kv, hide=(IDS[0],))
    for g, wnt, name in zip(got, want[:5], ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
        assert_bits(g, wnt, f"hidden {name}")
    assert not (got[2] == IDS[0]).any()
    assert_bits(got[1], plain[1], "raylengths are not touched by the hide step")


# ---- the host classes ---------------------------------------------------------------------------------------------

FW, FH = 160, 120


def _fusion(nobj=2, **kw):
    from emfusion_amd import pipeline
    prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5, **kw)
    synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), nobj)
    fus = pipeline.Fusion(prm)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(nobj)]
    return prm, synth, fus, ids


def _frame(fus, synth, ids, f):
    from emfusion_amd.ops import image_view
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    masks = {i: to_dev((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if f == 0 else {}
    fus.process_frame(image_view(to_dev(depth)), R, t, poses, {i: image_view(m) for i, m in masks.items()}, f == 0)


def test_fusion_render_view_equals_the_oracle_chain_over_its_volumes(oracle, dev):
    from emfusion_amd import pipeline
    prm, synth, fus, ids = _fusion()
    for f in range(5):
        _frame(fus, synth, ids, f)
    fus.synchronize()

    class V:
        pass
    vols, poses = [], []
    bg = V()
    bg.id, bg.tsdf, bg.wts, bg.vmask = 0, fus.volume("tsdf", 0), fus.volume("weights", 0), None
    bg.vox = np.float32(prm.bg_voxel_size)
    bg.trunc = np.float32(prm.bg_rel_truncdist) * bg.vox
    vols.append(bg)
    poses.append(Affine32(np.eye(3), np.array(prm.volume_pose_t, np.float32)))
    for i in ids:
        o = V()
        info = fus.object_info(i)
        o.id, o.tsdf, o.wts, o.vmask = i, fus.volume("tsdf", i), fus.volume("weights", i), fus.volume("fgmask", i)
        o.vox, o.trunc = np.float32(info["voxel_size"]), np.float32(info["truncdist"])
        vols.append(o)
        R, t = fus.pose(i)
        poses.append(Affine32(R, t))
    _, cmap = fus.render()
    global CMAP
    keep = CMAP
    CMAP = cmap
    try:
        for name, (w, h) in (("outside_looking_in", (128, 96)), ("inside_background", (97, 61))):
            Rv, tv = viewers()[name]
            Kv = view_K(w, h)
            rgb, ray, seg = fus.render_view(Rv, tv, Kv, (w, h))
            pv = viewer_to_volume((Rv, tv), vols, poses)
            want = oracle_chain(oracle, vols, pv, ids, w, h, Kv)
            assert_bits(rgb, want[0], f"{name} rgb")
            assert_bits(ray, want[1], f"{name} raylengths")
            assert_bits(seg, want[2], f"{name} segmentation")
            assert rgb.any(axis=2).sum() > w * h // 20
        # defaults: the frame intrinsics and size
        rgb, ray, seg = fus.render_view(*pipeline.look_at((0, 0, -0.5), (0, 0, 1.3)))
        assert rgb.shape == (FH, FW, 3) and ray.shape == (FH, FW) and seg.shape == (FH, FW)
    finally:
        CMAP = keep
        fus.close()
        synth.close()


def test_render_view_before_the_first_frame_is_black(dev):
    prm, synth, fus, ids = _fusion(1)
    try:
        rgb, ray, seg = fus.render_view(np.eye(3), np.zeros(3), size=(33, 17))
        assert rgb.shape == (17, 33, 3) and not rgb.any() and not ray.any() and not seg.any()
    finally:
        fus.close()
        synth.close()


def _digest(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _state(fus, ids):
    from emfusion_amd.pipeline import IMG
    out = {"pose": [np.concatenate([x.reshape(-1) for x in fus.pose(i)]) for i in [0] + ids],
           "visible": sorted(fus.visible_objects())}
    for name in IMG:
        for i in ([0] if name not in ("obj_assoc", "obj_raylengths") else ids):
            out[f"img {name} {i}"] = _digest(fus.image(name, i))
    for i in [0] + ids:
        for v in ("tsdf", "weights"):
            out[f"vol {v} {i}"] = _digest(fus.volume(v, i))
    return out


def test_render_view_does_not_touch_the_frame_path(dev):
    from emfusion_amd import pipeline
    a = _fusion()
    b = _fusion()
    viewer = pipeline.look_at((0.5, -0.5, -0.5), (0, 0, 1.3))
    try:
        for f in range(6):
            _frame(a[2], a[1], a[3], f)
            _frame(b[2], b[1], b[3], f)
            rgb, _, _ = b[2].render_view(*viewer, size=(200, 150))
            assert rgb.any()
        a[2].synchronize()
        b[2].synchronize()
        sa, sb = _state(a[2], a[3]), _state(b[2], b[3])
        assert sa.keys() == sb.keys()
        for k in sa:
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k
    finally:
        for x in (a, b):
            x[2].close()
            x[1].close()


def test_3d_view_log_writes_one_png_per_rendered_frame(dev, tmp_path):
    import zlib
    from emfusion_amd import pipeline

    def decode_png(data):  # the project's own writer: 8-bit RGB, filter 0 per row
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, idat, w, h = 8, b"", 0, 0
        while pos < len(data):
            n = int.from_bytes(data[pos:pos + 4], "big")
            kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
            if kind == b"IHDR":
                w, h = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
                assert body[8] == 8 and body[9] == 2
            elif kind == b"IDAT":
                idat += body
            pos += 12 + n
        raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
        out = np.empty((h, 3 * w), np.uint8)
        prev = np.zeros(3 * w, np.int32)
        for y in range(h):
            f, line = raw[y, 0], raw[y, 1:].astype(np.int32)
            cur = np.zeros(3 * w, np.int32)
            for x in range(3 * w):
                a = cur[x - 3] if x >= 3 else 0
                b_, c = prev[x], prev[x - 3] if x >= 3 else 0
                pred = {0: 0, 1: a, 2: b_, 3: (a + b_) // 2}.get(int(f))
                if pred is None:  # Paeth
                    p = a + b_ - c
                    pa, pb, pc = abs(p - a), abs(p - b_), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b_ if pb <= pc else c)
                cur[x] = (line[x] + pred) & 255
            out[y] = cur
            prev = cur
        return out.reshape(h, w, 3)

    def run(with_view, out):
        prm, synth, fus, ids = _fusion()
        views = []
        try:
            fus.setup_output()
            if with_view:
                fus.set_3d_view(*pipeline.look_at((0.3, -0.4, -0.6), (0, 0, 1.3)), size=(64, 48))
            for f in range(4):
                _frame(fus, synth, ids, f)
                fus.render()
                if with_view:
                    views.append(fus.render_view(*pipeline.look_at((0.3, -0.4, -0.6), (0, 0, 1.3)), size=(64, 48))[0])
            fus.write_results(out, volumes=False)
        finally:
            fus.close()
            synth.close()
        return views

    views = run(True, tmp_path / "with")
    files = sorted((tmp_path / "with" / "mesh_vis_out").iterdir())
    assert [p.name for p in files] == [f"{f:04d}.png" for f in range(4)]
    for p, v in zip(files, views):
        assert np.array_equal(decode_png(p.read_bytes()), v), p.name
    assert any(v.any() for v in views)
    run(False, tmp_path / "without")
    assert not (tmp_path / "without" / "mesh_vis_out").exists()
    listing = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))  # noqa: E731
    assert listing(tmp_path / "without") == [x for x in listing(tmp_path / "with") if not x.startswith("mesh_vis_out")]


def test_sharded_render_view_is_refused_and_the_next_frame_runs(dev):
    from emfusion_amd import pipeline
    os.environ["EMF_FORCE_SHARDED"] = "1"
    try:
        comm = pipeline.Communicator(pipeline.Communicator.unique_id(), 0, 1)
        prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5)
        synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), 1)
        fus = pipeline.Fusion(prm, comm)
        ids = [fus.add_object(*[synth.sphere(0, 0)[i] for i in (0, 2)])]
        try:
            for f in range(2):
                _frame(fus, synth, ids, f)
            with pytest.raises(pipeline.FusionError) as e:
                fus.render_view(np.eye(3), np.array([0, 0, -1.0]))
            assert e.value.code == -4  # EMF_E_ARG
            _frame(fus, synth, ids, 2)
            fus.synchronize()
            assert fus.frame_index() == 3
        finally:
            fus.close()
            synth.close()
            comm.close()
    finally:
        os.environ.pop("EMF_FORCE_SHARDED", None)


def test_full_size_views_equal_the_gpu_chain(ops, dev):
    """configs[1]'s geometry (512^3 background + 4 x 128^3 objects) fused from 5 frames, seen at the reference
    window's default view (1024 x 768), and a background above 32-bit offsets (the 64-bit march) seen alone."""
    from emfusion_amd import pipeline
    fw, fh = 640, 480
    prm = pipeline.make_params(fw, fh, 512, 0.01, 128)
    Kf = np.array(prm.K, np.float32).reshape(3, 3)
    synth = pipeline.SyntheticStream(fw, fh, np.array(prm.K, np.float32), 4)

    class GV:
        def __init__(self, res, vox, t, obj_id):
            self.res, self.vox, self.pose, self.id = res, np.float32(vox), Pose(t=np.asarray(t, np.float64)), obj_id
            self.d_tsdf = dev_full((res[2], res[1], res[0]), 0.0)
            self.d_wts = dev_full((res[2], res[1], res[0]), 0.0)
            self.trunc = np.float32(10) * self.vox

        def integrate(self, cam, depth):
            oc = rel_OC(cam, self.pose)
            ops.update_tsdf(depth, dev_full((fh, fw), 1.0), self.d_tsdf, self.d_wts, oc.R32, oc.t32, Kf, self.vox,
                            self.trunc, MAXW)

        def entry(self, w, h):
            imgs = dict(assoc=dev_full((4, 4), 1.0), ray=dev_full((h, w), 0.0), vert=dev_full((h, w, 3), 0.0),
                        nrm=dev_full((h, w, 3), 0.0), hit=dev_full((h, w), 0, np.uint8))
            return ops.make_model(self.d_tsdf, self.d_wts, imgs["assoc"], imgs["ray"], imgs["vert"], imgs["nrm"],
                                  imgs["hit"], float(self.vox), float(self.trunc), MAXW, SIGMA, ALPHA, PRIOR,
                                  model_id=self.id, rcp_voxel=ops.voxel_reciprocal(self.vox)), imgs

    try:
        vols = [GV((512,) * 3, 0.01, (0, 0, 2.56), 0)]
        vols += [GV((128,) * 3, float(synth.sphere(k, 0)[2]) / 128, synth.sphere(k, 0)[0], k + 1) for k in range(4)]
        for f in range(5):
            depth, _ = synth.render(f)
            R, t = synth.camera_pose(f)
            cam = Pose(np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64))
            d = to_dev(depth)
            for v in vols:
                v.integrate(cam, d)
        Rv, tv, Kv, (w, h) = pipeline.default_3d_view(prm)
        pv = viewer_to_volume((Rv, tv), vols)
        entries = [v.entry(w, h) for v in vols]
        table = ops.upload_models([e for e, _ in entries])
        labels = [1, 2, 3, 4]
        got, st = render_view(ops, table, pv, labels, w, h, Kv)
        want = gpu_chain(ops, table, entries, pv, [v.res for v in vols], labels, w, h, Kv)
        for g, wnt, name in zip(got, want, ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
            assert_bits(g, wnt, f"configs[1] default view {name}")
        assert got[0].any(axis=2).sum() > w * h // 10 and (got[2] != 0).sum() > 1000
        del entries, table, vols
        # 1040 x 1024 x 1024 voxels > 2^30: the frame raycast takes MODE 0 (64-bit offsets), the view its 64-bit march
        big = GV((1040, 1024, 1024), 0.005, (0, 0, 2.56), 0)
        for f in range(2):
            depth, _ = synth.render(f)
            R, t = synth.camera_pose(f)
            big.integrate(Pose(np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64)), to_dev(depth))
        pv = viewer_to_volume(pipeline.look_at((0.4, -0.3, -0.2), (0, 0, 1.5)), [big])
        e = big.entry(w, h)
        table = ops.upload_models([e[0]])
        got, _ = render_view(ops, table, pv, [], w, h, Kv)
        want = gpu_chain(ops, table, [e], pv, [big.res], [], w, h, Kv)
        for g, wnt, name in zip(got, want, ["rgb", "raylengths", "segmentation", "vertices", "normals"]):
            assert_bits(g, wnt, f"64-bit background {name}")
        assert got[0].any(axis=2).sum() > w * h // 10
    finally:
        synth.close()


def test_synth_app_writes_one_3d_view_per_frame(dev, tmp_path):
    app = ROOT / "apps" / "emfusion_synth"
    r = subprocess.run([str(app), "--frames", "4", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width",
                        "160", "--height", "120", "--3d-vis", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    files = sorted(p.name for p in (tmp_path / "mesh_vis_out").iterdir())
    assert files == [f"{f:04d}.png" for f in range(4)]
    r = subprocess.run([str(app), "--frames", "2", "--objects", "1", "--bg-res", "128", "--obj-res", "32", "--width",
                        "160", "--height", "120", "--3d-vis", "--3d-vis-eye", "0.5", "-0.5", "-0.5", "--3d-vis-target",
                        "0", "0", "1.3", "--out", str(tmp_path / "placed")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert len(list((tmp_path / "placed" / "mesh_vis_out").iterdir())) == 2
