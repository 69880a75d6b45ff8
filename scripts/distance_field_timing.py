"""Cost of the distance field (Fusion.distance_field) on the configs[1] scene (512^3 + 4 x 128^3) after
`frames` frames, for the whole background and for a 128^3 box around the camera:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of the three entries on the
    session's own volumes: classify (emf_hip_occupancyClasses), stamp (emf_hip_occupancyStampObjects, all objects) and
    the transform (emf_hip_distanceTransform: pass x, pass y, pass z), with and without the metres output,
  - host wall time of Fusion.distance_field(), which adds the copies to the host,
  - how many voxels are sites, and the largest distance.
The split of the transform into its three passes is read from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/distance_field_timing.py): k_df_rows is pass x, k_df_lines<false>
pass y, k_df_lines<true> pass z; k_occ_classes and k_occ_stamp are the other two stages.
python scripts/distance_field_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, DeviceView, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4


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


def view(fus, which, obj_id, dtype=np.float32):
    """The session's own device array, not a copy."""
    ptr, res = C.c_void_p(), (C.c_int32 * 3)()
    pipeline._check("emf_fusion_get_volume",
                    pipeline.load().emf_fusion_get_volume(fus._h, pipeline.VOL[which], obj_id, C.byref(ptr), res))
    return DeviceView(ptr.value, (res[2], res[1], res[0]), dtype)


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


synth, fus, ids = scene()
fus.synchronize()
tsdf, wts = view(fus, "tsdf", 0), view(fus, "weights", 0)
first = fus.distance_field(metres=False)  # the poses the session stamps its objects with
objects = [(view(fus, "tsdf", i), view(fus, "weights", i), view(fus, "fgmask", i, np.uint8), fus.object_info(i)["voxel_size"], R, t)
           for i, R, t in first["objects"]]
res = (BG, BG, BG)
table = ops.occupancy_objects(objects, res, VOX)
for name, box in (("whole 512^3", None), ("128^3 camera box", fus.camera_box(128))):
    lo, size = ops._box(res, box)
    shape = (size[2], size[1], size[0])
    voxels = int(np.prod(shape))
    classes, d2, metres = DeviceArray(shape, np.uint8), DeviceArray(shape, np.int32), DeviceArray(shape, np.float32)
    t_classes = timed(lambda: ops.occupancy_classes(tsdf, wts, box=(lo, size), out=classes))
    t_stamp = timed(lambda: ops.stamp_objects(classes, res, VOX, (table, len(objects)), box=(lo, size)))
    lines = []
    for mask, label in ((2, "occupied"), (6, "occupied or unknown")):
        t_plain = timed(lambda: ops.distance_transform(classes, site_mask=mask, out=(d2,)))
        t_metres = timed(lambda: ops.distance_transform(classes, site_mask=mask, voxel_size=VOX, out=(d2, metres)))
        h = d2.numpy()
        sites, far = int((h == 0).sum()), int((h == ops.DF_FAR).sum())
        lines.append(f"    sites = {label}: {sites} sites ({100.0 * sites / voxels:.2f} %), largest d2 "
                     f"{int(h[h != ops.DF_FAR].max()) if far < voxels else -1}, {far} voxels without a site; transform x + y + z "
                     f"{fmt(t_plain)}, with metres {fmt(t_metres)}")
    w = wall(lambda: fus.distance_field(box=box))
    print(f"{name}: box {lo} + {size}, {voxels} voxels, {len(objects)} objects stamped")
    print(f"    classify {fmt(t_classes)}, stamp {fmt(t_stamp)}")
    print("\n".join(lines))
    print(f"    byte model (a model, not a measurement): classify 9 B, pass x 5 B, passes y and z 8 B each = 30 B per voxel, "
          f"{30e-9 * voxels:.3f} GB; Fusion.distance_field() with its copies to the host, wall {fmt(w)}")
fus.close()
synth.close()
