"""Cost of merging an object into another object (Fusion.merge_objects) on the configs[1] scene (512^3 +
4 x 128^3) after `frames` frames.  The device entries are timed on a DUPLICATE: one 128^3 object of the scene as the
destination and a copy of it, under a pose of fractions of a voxel, as the source -- both with count volumes as the session
holds them, the colour entry with the weighted colour volumes of tests/transfer_color_reference.py.
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_mergeVolume and
    emf_hip_mergeVolumeColor, and of plain emf_hip_absorbVolume on the same volumes in the same run (the passes are in
    place: later calls of a group fuse into what the earlier ones left, the same voxels and the same work),
  - host wall time of Fusion.merge_objects() for the scene's objects in pairs (2 into 1, 4 into 3: they stand apart, so
    the call grows the destination; it contains the moments launch, the resize, the launch, volumesWritten() of the
    destination and the table rebuild, none of which the session exposes on its own),
  - the host route it replaces, as one sample: Fusion.volume() of both models plus the numpy restatement of
    tests/merge_reference.py.
Nothing is asserted but that the device's bytes equal the restatement's.
python scripts/merge_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import absorb_reference as ar  # noqa: E402
from tests import merge_reference as mr  # noqa: E402
from tests import transfer_color_reference as tc  # noqa: E402

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


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


lib = _lib.load()
synth, fus, ids = scene()
fus.synchronize()
print(f"{frames} frames, {reps} groups of {inner} calls; a duplicate of one {OBJ}^3 object into that object")
oid = ids[0]
info = fus.object_info(oid)
vox, trunc = np.float32(info["voxel_size"]), np.float32(info["truncdist"])
t0 = time.perf_counter()
host = {k: fus.volume(k, oid) for k in ("tsdf", "weights", "fgbg", "fgmask")}
t_copy = 2e3 * (time.perf_counter() - t0)  # the route downloads both models
pose = ar.pose_of(None, (0.37 * vox, -0.21 * vox, 0.5 * vox))
box = ((0, 0, 0), (OBJ, OBJ, OBJ))
dst = dict(ar.dst_vol(host["tsdf"], host["weights"], vox, trunc, fus.params.max_tsdf_weight), fgbg=host["fgbg"],
           color=tc.color_volume((OBJ, OBJ, OBJ), "weighted", 1))
src = dict(ar.src_vol(host["tsdf"], host["weights"], host["fgmask"], vox, trunc), fgbg=host["fgbg"],
           color=tc.color_volume((OBJ, OBJ, OBJ), "weighted", 2))
t0 = time.perf_counter()
want = mr.merge_color(dst, src, pose, box)
t_host = 1e3 * (time.perf_counter() - t0)
rec, cnt = want[2], want[4]
print(f"box {box[0]} + {box[1]}: {int(rec['visited'])} voxels, {int(rec['outside'])} outside, {int(rec['unknown'])} unknown, "
      f"{int(rec['masked'])} masked, {int(rec['saturated'])} saturated, {int(rec['fused'])} fused ({int(rec['fresh'])} fresh), "
      f"{int(cnt['foreground'])} foreground ({int(cnt['gained'])} gained), {int(want[6]['colored'])} coloured")
up = DeviceArray.from_numpy
d_src = dict(tsdf=up(src["tsdf"]), weights=up(src["weights"]), fg_mask=up(src["fg"]), fgbg=up(src["fgbg"]), color=up(src["color"]),
             voxel_size=vox, truncdist=trunc)
d_rec, d_cnt, d_col = DeviceArray((1,), ops.ABSORB_DTYPE), DeviceArray((1,), ops.MERGE_COUNTS_DTYPE), DeviceArray((1,), ops.COLOR_MOVED_DTYPE)
so = _lib.EmfAbsorbSource()
so.tsdf, so.weights, so.fgVolMask = d_src["tsdf"].ptr, d_src["weights"].ptr, d_src["fg_mask"].ptr
so.res, so.voxelSize, so.truncdist = (C.c_int32 * 3)(OBJ, OBJ, OBJ), float(vox), float(trunc)
i3 = lambda v: (C.c_int32 * 3)(*v)  # noqa: E731
Rc, tc_ = (C.c_float * 9)(*pose[0].reshape(-1).tolist()), (C.c_float * 3)(*pose[1].tolist())
head = (i3((OBJ, OBJ, OBJ)), float(vox), float(trunc), float(dst["max_weight"]), C.byref(so))
tail = (Rc, tc_, i3(box[0]), i3(box[1]), d_rec.ptr)


def fresh_dst(colored):
    d = dict(tsdf=up(dst["tsdf"]), weights=up(dst["weights"]), fgbg=up(dst["fgbg"]), voxel_size=vox, truncdist=trunc,
             max_weight=dst["max_weight"])
    if colored:
        d["color"] = up(dst["color"])
    return d


d = fresh_dst(False)
ops.absorb_volume(d, d_src, pose, box=box, out=d_rec)
assert d_rec.numpy()[0].tobytes() == rec.tobytes() and d["tsdf"].numpy().tobytes() == want[0].tobytes()
t = timed(lambda: lib.emf_hip_absorbVolume(d["tsdf"].ptr, d["weights"].ptr, *head, *tail, None))
print(f"    emf_hip_absorbVolume     {fmt(t)} with its init launch")
d = fresh_dst(False)
ops.merge_volume(d, d_src, pose, box=box, out=d_rec, counts_out=d_cnt)
assert d_rec.numpy()[0].tobytes() == rec.tobytes() and d_cnt.numpy()[0].tobytes() == cnt.tobytes()
assert d["tsdf"].numpy().tobytes() == want[0].tobytes() and d["fgbg"].numpy().tobytes() == want[3].tobytes()
t = timed(lambda: lib.emf_hip_mergeVolume(d["tsdf"].ptr, d["weights"].ptr, d["fgbg"].ptr, *head, d_src["fgbg"].ptr, *tail, d_cnt.ptr, None))
print(f"    emf_hip_mergeVolume      {fmt(t)} with its init launch")
d = fresh_dst(True)
ops.merge_volume(d, d_src, pose, box=box, out=d_rec, counts_out=d_cnt, color_out=d_col)
assert d_col.numpy()[0].tobytes() == want[6].tobytes() and d["color"].numpy().tobytes() == want[5].tobytes()
assert d["fgbg"].numpy().tobytes() == want[3].tobytes()
t = timed(lambda: lib.emf_hip_mergeVolumeColor(d["tsdf"].ptr, d["weights"].ptr, d["fgbg"].ptr, d["color"].ptr, *head, d_src["fgbg"].ptr,
                                               d_src["color"].ptr, *tail, d_cnt.ptr, d_col.ptr, None))
print(f"    emf_hip_mergeVolumeColor {fmt(t)} with its init launch")
walls = []
for a, b in ((ids[0], ids[1]), (ids[2], ids[3])):
    t0 = time.perf_counter()
    e = fus.merge_objects(a, b)
    walls.append(1e3 * (time.perf_counter() - t0))
    print(f"    merge_objects({a}, {b}): resolution {e['res_before']} -> {e['res_after']}, box {e['size']}, clipped {e['clipped']}, "
          f"{int(e['record']['fused'])} fused")
print(f"    Fusion.merge_objects(), wall, the two calls: {walls[0]:.3f} ms and {walls[1]:.3f} ms (the moments, the resize, the launch, "
      "the copy-back of the records, volumesWritten() of the destination, the table rebuild; none of them alone: not measured)")
print(f"    the host route, one sample: Fusion.volume() of both models, wall {t_copy:.1f} ms; then the numpy restatement {t_host:.1f} ms "
      "(and the upload of the result is not counted)")
fus.close()
synth.close()
