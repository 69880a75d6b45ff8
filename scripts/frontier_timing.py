"""Cost of the exploration frontiers (Fusion.frontiers) on the configs[1] scene (512^3 + 4 x 128^3) after
`frames` frames, for the whole background and for a 128 x 128 x 64 box around the camera:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of the stages on the session's
    own volumes: classify (emf_hip_occupancyClasses), stamp (emf_hip_occupancyStampObjects, all objects), the clearance
    transform (emf_hip_distanceTransform, sites = occupied, capped at the clearance), labels (emf_hip_frontierLabel:
    flags, hook, flatten, count) with and without the clearance gate, and the records (emf_hip_frontierClusters: roots,
    statistics, representative, filter),
  - host wall time of Fusion.frontiers(), which adds the two waits, the copy of the records and the sort,
  - how many voxels are frontier voxels, how many clusters there are and how many are kept.
The split of the two frontier entries into their kernels is read from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/frontier_timing.py): k_fr_flags, k_fr_hook, k_fr_flatten and
k_fr_count are the labels; k_fr_rootsums, k_fr_scan, k_fr_roots, k_fr_stats (statistics), k_fr_rep (representative),
k_fr_keepsums and k_fr_emit the records.
python scripts/frontier_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, DeviceView, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4
MIN_VOXELS, CLEARANCE = 8, 0.2  # metres: 20 voxels


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


def clusters_call(labels, min_voxels):
    """The records entry as one enqueue: scratch and records sized once, by the cluster count read once."""
    lib = _lib.load()
    size = (C.c_int32 * 3)(*labels.shape[::-1])
    n = int(labels.counters.numpy()[ops.FRONTIER_CLUSTERS])
    scratch = DeviceArray((max(int(lib.emf_hip_frontierScratchBytes(size, n)), 16),), np.uint8)
    records = DeviceArray((max(n, 1),), ops.FRONTIER_CLUSTER_DTYPE)

    def run():
        _lib.check("emf_hip_frontierClusters",
                   lib.emf_hip_frontierClusters(C.c_void_p(labels.ptr), size, min_voxels, n, C.c_void_p(scratch.ptr),
                                                C.c_void_p(records.ptr), n, C.c_void_p(labels.counters.ptr), None))
    return run, scratch.nbytes


synth, fus, ids = scene()
fus.synchronize()
tsdf, wts = view(fus, "tsdf", 0), view(fus, "weights", 0)
first = fus.distance_field(metres=False)  # the poses the session stamps its objects with
objects = [(view(fus, "tsdf", i), view(fus, "weights", i), view(fus, "fgmask", i, np.uint8), fus.object_info(i)["voxel_size"], R, t)
           for i, R, t in first["objects"]]
res = (BG, BG, BG)
table = ops.occupancy_objects(objects, res, VOX)
cv = int(np.ceil(np.float32(CLEARANCE) / np.float32(VOX)))
print(f"{frames} frames, {reps} groups of {inner} calls; min_voxels {MIN_VOXELS}, clearance {CLEARANCE} m = {cv} voxels")
for name, box in (("whole 512^3", None), ("128 x 128 x 64 camera box", fus.camera_box((128, 128, 64)))):
    lo, size = ops._box(res, box)
    shape = (size[2], size[1], size[0])
    voxels = int(np.prod(shape))
    classes, d2 = DeviceArray(shape, np.uint8), DeviceArray(shape, np.int32)
    t_classes = timed(lambda: ops.occupancy_classes(tsdf, wts, box=(lo, size), out=classes))
    t_stamp = timed(lambda: ops.stamp_objects(classes, res, VOX, (table, len(objects)), box=(lo, size)))
    t_clear = timed(lambda: ops.distance_transform(classes, site_mask=2, cap=cv, out=(d2,)))
    print(f"{name}: box {lo} + {size}, {voxels} voxels, {len(objects)} objects stamped")
    print(f"    classify {fmt(t_classes)}, stamp {fmt(t_stamp)}, clearance transform (cap {cv}) {fmt(t_clear)}")
    labels = DeviceArray(shape, np.int32)
    for label, gate in (("no clearance", None), (f"clearance {cv} voxels", d2)):
        t_label = timed(lambda: ops.frontier_labels(classes, d2=gate, min_d2=cv * cv if gate is not None else 0, out=labels))
        run, scratch_bytes = clusters_call(labels, MIN_VOXELS)
        t_records = timed(run)
        kept, every, front = (int(v) for v in labels.counters.numpy())
        print(f"    {label}: {front} frontier voxels ({100.0 * front / voxels:.3f} %), {every} clusters, {kept} of at least "
              f"{MIN_VOXELS} voxels; labels {fmt(t_label)}, records {fmt(t_records)} (scratch {scratch_bytes} B)")
    w0 = wall(lambda: fus.frontiers(box=box, min_voxels=MIN_VOXELS))
    w1 = wall(lambda: fus.frontiers(box=box, min_voxels=MIN_VOXELS, clearance=CLEARANCE))
    print(f"    byte model (a model, not a measurement): classify 9 B, flags 5 B (1 B read, the five neighbour rows from "
          f"cache, 4 B written), hook + flatten + count 12 B, root sums + roots + the two passes 16 B = 42 B per voxel "
          f"without the clearance, {42e-9 * voxels:.3f} GB; the unions, the binary searches and the atomics of the "
          f"frontier voxels are not in it")
    print(f"    Fusion.frontiers() with its two waits, the records copied and sorted, wall {fmt(w0)}; with the clearance {fmt(w1)}")
fus.close()
synth.close()
