"""Cost of absorbing an object into the background (Fusion.absorb_object) on the configs[1] scene (512^3 +
4 x 128^3) after `frames` frames: one 128^3 object into the 512^3 background.
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_absorbVolume alone, on
    copies of the session's own volumes (the pass is in place: later calls of a group fuse into what the earlier ones
    left, the same voxels and the same work), with and without the object's unseen-tile map,
  - host wall time of Fusion.absorb_object(), once per object of the scene (the call removes the object); it contains the
    background.volumesWritten() that follows the launch (brick flags, gradients, the back copy), which the session does
    not expose on its own and which is therefore NOT measured separately,
  - the host route it replaces: Fusion.volume() of both models plus the numpy restatement of tests/absorb_reference.py.
A byte MODEL (not a measurement) of the launch: 8 B per voxel of the box for the destination, 64 B (+1 B with a mask) of
gathers per voxel whose sample lies inside the object, 8 B stored per fused voxel.  The kernel is a dependent-gather pass:
no roof is claimed.  Nothing is asserted but that the device's bytes equal the restatement's.
python scripts/absorb_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import absorb_reference as ar  # noqa: E402

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
print(f"{frames} frames, {reps} groups of {inner} calls; one object of {OBJ}^3 into the background {BG}^3")
oid = ids[0]
sides = dict(zip(*[fus.object_contacts(ids=[oid])[k] for k in ("ids", "sides")]))
t0 = time.perf_counter()
host_bg = (fus.volume("tsdf", 0), fus.volume("weights", 0))
host_obj = (fus.volume("tsdf", oid), fus.volume("weights", oid), fus.volume("fgmask", oid))
t_copy = 1e3 * (time.perf_counter() - t0)
pose = pipeline.absorb_pose(fus.background_pose(), fus.pose(oid))
box = ops.absorb_box((BG, BG, BG), VOX, (OBJ, OBJ, OBJ), sides[oid]["voxel_size"], pose)
dst = ar.dst_vol(*host_bg, VOX, sides[0]["truncdist"], fus.params.max_tsdf_weight)
src = ar.src_vol(*host_obj, sides[oid]["voxel_size"], sides[oid]["truncdist"])
t0 = time.perf_counter()
want = ar.absorb(dst, src, pose, box)
t_host = 1e3 * (time.perf_counter() - t0)
rec = want[2]
inside = int(rec["visited"] - rec["outside"])
model_bytes = 8 * int(rec["visited"]) + 65 * inside + 8 * int(rec["fused"])
print(f"box {box[0]} + {box[1]}: {int(rec['visited'])} voxels, {int(rec['outside'])} outside, {int(rec['unknown'])} unknown, "
      f"{int(rec['masked'])} masked, {int(rec['saturated'])} saturated, {int(rec['fused'])} fused ({int(rec['fresh'])} fresh, "
      f"{int(rec['solid'])} solid); byte MODEL {model_bytes / 1e6:.1f} MB")
d_src = dict(tsdf=DeviceArray.from_numpy(host_obj[0]), weights=DeviceArray.from_numpy(host_obj[1]),
             fg_mask=DeviceArray.from_numpy(host_obj[2]), voxel_size=src["voxel_size"], truncdist=src["truncdist"])
tiles = DeviceArray((ops.unseen_tile_bytes((OBJ, OBJ, OBJ)),), np.uint8)
ops.rebuild_unseen_tiles(d_src["tsdf"], d_src["weights"], tiles)
d_rec = DeviceArray((1,), ops.ABSORB_DTYPE)
for label, source in (("no unseen-tile map", d_src), ("with the unseen-tile map", dict(d_src, unseen_tiles=tiles))):
    d_dst = dict(tsdf=DeviceArray.from_numpy(host_bg[0]), weights=DeviceArray.from_numpy(host_bg[1]), voxel_size=VOX,
                 truncdist=dst["truncdist"], max_weight=dst["max_weight"])
    ops.absorb_volume(d_dst, source, pose, box=box, out=d_rec)
    assert d_rec.numpy()[0].tobytes() == rec.tobytes() and d_dst["tsdf"].numpy().tobytes() == want[0].tobytes()
    assert d_dst["weights"].numpy().tobytes() == want[1].tobytes()
    so = _lib.EmfAbsorbSource()
    so.tsdf, so.weights, so.fgVolMask = source["tsdf"].ptr, source["weights"].ptr, source["fg_mask"].ptr
    so.unseenTiles = source["unseen_tiles"].ptr if "unseen_tiles" in source else None
    so.res, so.voxelSize, so.truncdist = (C.c_int32 * 3)(OBJ, OBJ, OBJ), float(src["voxel_size"]), float(src["truncdist"])
    i3 = lambda v: (C.c_int32 * 3)(*v)  # noqa: E731
    Rc, tc = (C.c_float * 9)(*pose[0].reshape(-1).tolist()), (C.c_float * 3)(*pose[1].tolist())
    args = (d_dst["tsdf"].ptr, d_dst["weights"].ptr, i3((BG, BG, BG)), VOX, float(dst["truncdist"]), float(dst["max_weight"]),
            C.byref(so), Rc, tc, i3(box[0]), i3(box[1]), d_rec.ptr, None)
    t = timed(lambda: lib.emf_hip_absorbVolume(*args))
    print(f"    {label}: emf_hip_absorbVolume {fmt(t)} with its init launch, {model_bytes / t[0] / 1e6:.0f} GB/s of the model")
walls = []
for i in ids:
    t0 = time.perf_counter()
    fus.absorb_object(i)
    walls.append(1e3 * (time.perf_counter() - t0))
assert fus.absorbed()[0]["record"].tobytes() == rec.tobytes()
stat = lambda v: f"{float(np.median(v)):.3f} ms ({min(v):.3f} .. {max(v):.3f})"  # noqa: E731
print(f"    Fusion.absorb_object(), wall over the {len(ids)} objects: {stat(walls)} (the launch, the copy-back of the record, "
      "background.volumesWritten(), the table rebuild; volumesWritten alone: not measured)")
print(f"    the host route: Fusion.volume() of both models, wall {t_copy:.1f} ms; then the numpy restatement {t_host:.1f} ms "
      "(and the upload of the result is not counted)")
fus.close()
synth.close()
