"""Cost of the voxel rays (Fusion.cast_rays / view_gain / plan(shortcut=W)) on the configs[1] scene
(512^3 + 4 x 128^3) after `frames` frames:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_castVoxelRays on the
    session's own classes for 256 candidate views x 32 x 24 rays of 3 m -- over the whole 512^3 and over a
    128 x 128 x 64 box around the camera, per-ray records and group records, and the group records alone -- and for
    1000 random segments between observed free voxels with and without a clearance of 20 voxels,
  - host wall time of Fusion.view_gain(), Fusion.cast_rays() and Fusion.plan(shortcut=64) against Fusion.plan(),
  - what the calls stand against: there is no earlier implementation, so the existing alternative, Fusion.distance_field()
    with its copies to the host plus the walk of tests/rays_reference.py over the same rays there (the 1000 segments in
    full; one view in `VIEW_STRIDE` of the 256, scaled).
Nothing is asserted.
python scripts/voxel_rays_timing.py [frames] [reps] [inner]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import rays_reference as rr  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4
VIEWS, GRID, RANGE, SEGMENTS, CLEARANCE, WINDOW, VIEW_STRIDE = 256, (32, 24), 3.0, 1000, 0.2, 64, 16


def scene():
    prm = pipeline.make_params(W, H, BG, VOX, OBJ)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        rm = f % prm.mask_frames == 0
        masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if rm else {}
        d = DeviceArray.from_numpy(depth)
        poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
        fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, rm)
        fus.synchronize()
    return synth, fus, ids


def timed(fn):
    """(median, min, max) ms per call over `reps` groups of `inner` calls."""
    fn()
    synchronize()
    out = []
    for _ in range(reps):
        a, b = Event(), Event()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_ms(b) / inner)
    return float(np.median(out)), min(out), max(out)


def wall(fn, n=None):
    fn()
    out = []
    for _ in range(n or reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), min(out), max(out)


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def candidate_views(fus, rng):
    """VIEWS poses around the camera: eyes within half a metre of it, each looking at a random point of the background."""
    _, cam = fus.pose(0)
    frame = fus._box_frame()
    views = []
    for _ in range(VIEWS):
        eye = cam.astype(np.float64) + rng.uniform(-0.5, 0.5, 3) * (1.0, 0.3, 1.0)
        target = frame.world([rng.uniform(0.15, 0.85, 3) * BG])[0].astype(np.float64)
        views.append(pipeline.look_at(eye, target))
    return views


synth, fus, ids = scene()
fus.synchronize()
rng = np.random.default_rng(0x5EED)
views = candidate_views(fus, rng)
prm = fus.params
K = np.array(prm.K, np.float64).reshape(3, 3)
K4 = (K[0, 0] * GRID[0] / W, K[1, 1] * GRID[1] / H, K[0, 2] * GRID[0] / W, K[1, 2] * GRID[1] / H)
bg_R, bg_t = fus.background_pose()
per = GRID[0] * GRID[1]
cv = int(np.ceil(np.float32(CLEARANCE) / np.float32(VOX)))
print(f"{frames} frames, {reps} groups of {inner} calls; {VIEWS} views x {GRID[0]} x {GRID[1]} rays of {RANGE} m, {SEGMENTS} segments, "
      f"clearance {CLEARANCE} m = {cv} voxels")
for name, box in (("whole 512^3", None), ("128 x 128 x 64 camera box", fus.camera_box((128, 128, 64)))):
    t_df = wall(lambda: fus.distance_field(box=box, metres=False), 3)
    df = fus.distance_field(box=box, cap=CLEARANCE, metres=False)
    lo, size = df["box"]
    classes, d2 = DeviceArray.from_numpy(df["classes"]), DeviceArray.from_numpy(df["d2"])
    print(f"{name}: box {lo} + {size}, {int(np.prod(size))} voxels; Fusion.distance_field() with its copies, wall {fmt(t_df)}")
    # the view rays
    t0 = time.perf_counter()
    ends = [pipeline.view_ray_targets(R, t, K4, GRID, RANGE, bg_R, bg_t, (BG, BG, BG), VOX, lo) for R, t in views]
    t_targets = 1e3 * (time.perf_counter() - t0)
    a = np.concatenate([np.repeat(o[None], per, axis=0) for o, _ in ends]).astype(np.int32)
    b = np.concatenate([t.reshape(-1, 3) for _, t in ends]).astype(np.int32)
    d_a, d_b = DeviceArray.from_numpy(a.reshape(-1)), DeviceArray.from_numpy(b.reshape(-1))
    res, grp = DeviceArray((len(a),), ops.RAY_RESULT_DTYPE), DeviceArray((VIEWS,), ops.RAY_GROUP_DTYPE)
    t_both = timed(lambda: ops.cast_voxel_rays(classes, d_a, d_b, pass_mask=5, count_mask=4, group=per, out=(res, grp)))
    t_groups = timed(lambda: ops.cast_voxel_rays(classes, d_a, d_b, pass_mask=5, count_mask=4, group=per, out=(None, grp)))
    host = res.numpy()
    steps = int(host["steps"].sum()) + int((host["status"] == rr.BLOCKED).sum())  # class bytes read
    inside = int((host["status"] < rr.OUTSIDE).sum())
    print(f"    view gain, {len(a)} rays ({inside} from inside the box), {steps} voxels visited ({steps / max(inside, 1):.0f} per ray): "
          f"records + groups {fmt(t_both)}, groups alone {fmt(t_groups)}; {steps / t_groups[0] / 1e6:.2f} G voxels/s; "
          f"targets on the host {t_targets:.1f} ms")
    w = wall(lambda: fus.view_gain(views, grid=GRID, range_m=RANGE, box=box))
    print(f"    Fusion.view_gain() with the classes, the targets, the upload and the groups copied, wall {fmt(w)}")
    sub = slice(0, None, VIEW_STRIDE)
    pick = np.concatenate([np.arange(v * per, (v + 1) * per) for v in range(VIEWS)[sub]])
    t0 = time.perf_counter()
    ref = rr.cast(df["classes"], a[pick], b[pick], None, 0, 5, 4)
    t_host = 1e3 * (time.perf_counter() - t0)
    assert ref.tobytes() == host[pick].tobytes()
    print(f"    the restatement's walk on the host over one view in {VIEW_STRIDE}: {t_host:.0f} ms, x {VIEW_STRIDE} = "
          f"{t_host * VIEW_STRIDE / 1e3:.1f} s for all, after the {t_df[0]:.0f} ms of distance_field()")
    # random segments
    free = np.argwhere(df["classes"] == rr.FREE)[:, ::-1]  # both ends in observed free space: most of the box is unknown
    sa = free[rng.integers(0, len(free), SEGMENTS)].astype(np.int32)
    sb = free[rng.integers(0, len(free), SEGMENTS)].astype(np.int32)
    d_sa, d_sb = DeviceArray.from_numpy(sa.reshape(-1)), DeviceArray.from_numpy(sb.reshape(-1))
    res = DeviceArray((SEGMENTS,), ops.RAY_RESULT_DTYPE)
    for label, kw in (("no clearance", {}), (f"clearance {cv} voxels", dict(d2=d2, min_d2=min(cv, 4095) ** 2))):
        t_seg = timed(lambda: ops.cast_voxel_rays(classes, d_sa, d_sb, pass_mask=1, out=(res, None), **kw))
        host = res.numpy()
        print(f"    {SEGMENTS} random segments, {label}: {fmt(t_seg)}; {int((host['status'] == rr.REACHED).sum())} reached, "
              f"{int(host['steps'].sum())} voxels passed, the longest ray {int(np.abs(sb - sa).sum(axis=1).max())} steps")
    frame = fus._box_frame(lo)
    pa, pb = frame.world(sa), frame.world(sb)
    for label, clearance in (("no clearance", 0.0), (f"clearance {cv} voxels", CLEARANCE)):
        w = wall(lambda: fus.cast_rays(pa, pb, box=box, clearance=clearance))
        print(f"    Fusion.cast_rays() of the segments, {label}, wall {fmt(w)}")
    t0 = time.perf_counter()
    rr.cast(df["classes"], sa, sb, None, 0, 1, 0)
    print(f"    the restatement's walk on the host over the segments: {1e3 * (time.perf_counter() - t0):.0f} ms")
    # the plan and its shortcuts
    for label, clearance in (("no clearance", 0.0), (f"clearance {cv} voxels", CLEARANCE)):
        w0 = wall(lambda: fus.plan(box=box, clearance=clearance))
        w1 = wall(lambda: fus.plan(box=box, clearance=clearance, shortcut=WINDOW))
        got = fus.plan(box=box, clearance=clearance, shortcut=WINDOW)
        reach = [g for g in got["goals"] if g["reachable"]]
        rays = sum(sum(min(i + WINDOW, len(g["path_vox"]) - 1) - i - 1 for i in range(len(g["path_vox"]) - 2)) for g in reach)
        print(f"    Fusion.plan(), {label}: wall {fmt(w0)}; with shortcut={WINDOW}: {fmt(w1)}; {len(reach)} reachable goals, "
              f"{sum(len(g['path_vox']) for g in reach)} path voxels -> {sum(len(g['waypoints']) for g in reach)} waypoints, "
              f"{rays} rays, {sum(g['length_m'] for g in reach):.2f} m -> {sum(g['waypoints_length_m'] for g in reach):.2f} m")
fus.close()
synth.close()
