"""Cost of the nearest-site index (emf_hip_distanceTransformNearest, Fusion.query_distance) on the
configs[1] scene (512^3 + 4 x 128^3) after `frames` frames, for the whole background and for a 128 x 128 x 64 box around
the camera:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of the transform on the
    session's own classes, sites = occupied, without the index (emf_hip_distanceTransform) and with it,
  - host wall time of Fusion.distance_field() with its copies to the host, of Fusion.distance_field(nearest=True), and
    of Fusion.query_distance() of `points` points on the field left on the device.
On a tree without the index only the plain transform and Fusion.distance_field() are measured: the same script gives
the figure of an earlier commit.
python scripts/distance_nearest_timing.py [frames] [reps] [inner] [points]"""
import inspect
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
points = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4
HAS_INDEX = "nearest" in inspect.signature(ops.distance_transform).parameters


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
    return synth, fus


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


def wall(fn):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), min(out), max(out)


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


synth, fus = scene()
fus.synchronize()
print(f"index available: {HAS_INDEX}; {frames} frames, {reps} groups of {inner}, {points} query points")
for name, box in (("whole 512^3", None), ("128 x 128 x 64 camera box", fus.camera_box((128, 128, 64)))):
    field = fus.distance_field(box=box, metres=False)
    lo, size = field["box"]
    shape = (size[2], size[1], size[0])
    voxels = int(np.prod(shape))
    classes = DeviceArray.from_numpy(field["classes"])
    d2 = DeviceArray(shape, np.int32)
    t_plain = timed(lambda: ops.distance_transform(classes, site_mask=2, out=(d2,)))
    w_field = wall(lambda: fus.distance_field(box=box))
    print(f"{name}: box {lo} + {size}, {voxels} voxels, {int((field['d2'] == 0).sum())} sites")
    print(f"    transform x + y + z without the index {fmt(t_plain)}; Fusion.distance_field() with its copies, wall {fmt(w_field)}")
    if not HAS_INDEX:
        continue
    import ctypes as C
    index, scratch = DeviceArray(shape, np.int32), DeviceArray(shape, np.int32)
    size3 = ops._i3(shape[::-1])

    def with_index():  # the entry itself: ops.distance_transform(nearest=True) would allocate the scratch array per call
        ops.check("emf_hip_distanceTransformNearest",
                  ops._L.emf_hip_distanceTransformNearest(ops._ptr(classes), size3, 2, 0, ops._ptr(d2), None, ops._ptr(index),
                                                          ops._ptr(scratch), C.c_float(0.0), None))

    t_index = timed(with_index)
    w_index = wall(lambda: fus.distance_field(box=box, nearest=True))
    rng = np.random.default_rng(5)
    R, t = field["pose"]
    world = (rng.uniform(0, 1, (points, 3)) * (np.array(size) - 1) * VOX) @ R.astype(np.float64).T + t.astype(np.float64)
    fus.distance_field(box=box, nearest=True)
    w_query = wall(lambda: fus.query_distance(world))
    q = fus.query_distance(world)
    print(f"    transform with the index {fmt(t_index)} (+{t_index[0] - t_plain[0]:.3f} ms, x{t_index[0] / t_plain[0]:.2f}); "
          f"Fusion.distance_field(nearest=True) with its copies, wall {fmt(w_index)}")
    print(f"    Fusion.query_distance({points} points), wall {fmt(w_query)}: {int(q['inside'].sum())} inside, "
          f"{int((q['nearest_voxel'][:, 0] >= 0).sum())} with an obstacle; x{w_field[0] / w_query[0]:.0f} below distance_field()")
    print(f"    byte model (a model, not a measurement): pass x + 4 B (index written), passes y and z + 8 B each (index "
          f"gathered and written) = + 20 B on the transform's 21 B per voxel, {20e-9 * voxels:.3f} GB more; two more i32 "
          f"arrays on the device, {8e-9 * voxels:.3f} GB")
fus.close()
synth.close()
