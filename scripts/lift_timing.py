"""Cost of lifting an object out of the background (Fusion.lift_object) on the configs[1] scene (512^3 +
4 x 128^3) after `frames` frames: one 128^3 object against the 512^3 background.
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_seedVolume and of
    emf_hip_releaseVolume alone, on copies of the session's own volumes.  Both passes are in place: after the first call
    of a group the seed finds its seeded voxels KEPT and the release its released voxels EMPTY, so the later calls of a
    group read the same destination bytes but skip the transform for those voxels and store nothing -- the figures are
    those of a REPEATED call, a lower bound on the first one,
  - host wall time of Fusion.lift_object(), once per object of the scene; it contains the volumesWritten() of the
    object and of the background (brick flags, gradients, the back copy) and the table rebuild,
  - the host route it replaces: Fusion.volume() of both models plus the numpy restatement of tests/lift_reference.py,
    one sample.
A byte MODEL (not a measurement): the seed 4 B per voxel of the box, 64 B of gathers per voxel that is not kept and
whose sample lies inside the background, 8 B per seeded voxel; the release 8 B per voxel of the box, 1 B per band voxel
inside the object's cube, 8 B per released voxel.  No roof is claimed.  Nothing is asserted but that the device's bytes
equal the restatement's.
python scripts/lift_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import absorb_reference as ar  # noqa: E402
from tests import lift_reference as lr  # noqa: E402

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


def i3(v):
    return (C.c_int32 * 3)(*v)


def f_arr(v):
    v = np.asarray(v, np.float32).reshape(-1)
    return (C.c_float * len(v))(*v.tolist())


lib = _lib.load()
synth, fus, ids = scene()
fus.synchronize()
print(f"{frames} frames, {reps} groups of {inner} calls; one object of {OBJ}^3 against the background {BG}^3")
oid = ids[0]
sides = dict(zip(*[fus.object_contacts(ids=[oid])[k] for k in ("ids", "sides")]))
t0 = time.perf_counter()
host_bg = (fus.volume("tsdf", 0), fus.volume("weights", 0))
host_obj = (fus.volume("tsdf", oid), fus.volume("weights", oid), fus.volume("fgmask", oid))
t_copy = 1e3 * (time.perf_counter() - t0)
seed_pose = pipeline.absorb_pose(fus.pose(oid), fus.background_pose())     # background frame <- object frame
release_pose = pipeline.absorb_pose(fus.background_pose(), fus.pose(oid))  # object frame <- background frame
box = ops.absorb_box((BG, BG, BG), VOX, (OBJ, OBJ, OBJ), sides[oid]["voxel_size"], release_pose)
obj = ar.dst_vol(host_obj[0], host_obj[1], sides[oid]["voxel_size"], sides[oid]["truncdist"], fus.params.max_tsdf_weight)
bg_src = ar.src_vol(*host_bg, None, VOX, sides[0]["truncdist"])
bg_dst = ar.dst_vol(*host_bg, VOX, sides[0]["truncdist"], fus.params.max_tsdf_weight)
claim = lr.claim_of(host_obj[2], (OBJ, OBJ, OBJ), sides[oid]["voxel_size"])
t0 = time.perf_counter()
want_seed = lr.seed(obj, bg_src, seed_pose)
want_rel = lr.release(bg_dst, claim, release_pose, box)
t_host = 1e3 * (time.perf_counter() - t0)
s, r = want_seed[2], want_rel[2]
seed_bytes = 4 * int(s["visited"]) + 64 * int(s["visited"] - s["kept"] - s["outside"]) + 8 * int(s["seeded"])
rel_bytes = 8 * int(r["visited"]) + int(r["unclaimed"] + r["released"]) + 8 * int(r["released"])
print(f"seed, the whole object: {int(s['visited'])} voxels, {int(s['kept'])} kept, {int(s['outside'])} outside, {int(s['unknown'])} "
      f"unknown, {int(s['saturated'])} saturated, {int(s['seeded'])} seeded ({int(s['solid'])} solid); byte MODEL {seed_bytes / 1e6:.1f} MB")
print(f"release, box {box[0]} + {box[1]}: {int(r['visited'])} voxels, {int(r['empty'])} empty, {int(r['free_space'])} free, "
      f"{int(r['outside'])} outside, {int(r['unclaimed'])} unclaimed, {int(r['released'])} released ({int(r['solid'])} solid); byte "
      f"MODEL {rel_bytes / 1e6:.1f} MB")

d_bg = dict(tsdf=DeviceArray.from_numpy(host_bg[0]), weights=DeviceArray.from_numpy(host_bg[1]), voxel_size=VOX,
            truncdist=bg_src["truncdist"])
d_obj = dict(tsdf=DeviceArray.from_numpy(host_obj[0]), weights=DeviceArray.from_numpy(host_obj[1]), voxel_size=obj["voxel_size"],
             truncdist=obj["truncdist"], max_weight=obj["max_weight"])
d_mask = DeviceArray.from_numpy(host_obj[2])
seed_rec, rel_rec = DeviceArray((1,), ops.SEED_DTYPE), DeviceArray((1,), ops.RELEASE_DTYPE)
ops.seed_volume(d_obj, d_bg, seed_pose, box=((0, 0, 0), (OBJ, OBJ, OBJ)), out=seed_rec)
assert seed_rec.numpy()[0].tobytes() == s.tobytes() and d_obj["tsdf"].numpy().tobytes() == want_seed[0].tobytes()
assert d_obj["weights"].numpy().tobytes() == want_seed[1].tobytes()
ops.release_volume(d_bg, dict(fg_mask=d_mask, voxel_size=claim["voxel_size"]), release_pose, box=box, out=rel_rec)
assert rel_rec.numpy()[0].tobytes() == r.tobytes() and d_bg["tsdf"].numpy().tobytes() == want_rel[0].tobytes()
assert d_bg["weights"].numpy().tobytes() == want_rel[1].tobytes()
so = _lib.EmfAbsorbSource()
so.tsdf, so.weights = d_bg["tsdf"].ptr, d_bg["weights"].ptr
so.res, so.voxelSize, so.truncdist = i3((BG, BG, BG)), VOX, float(bg_src["truncdist"])
seed_args = (d_obj["tsdf"].ptr, d_obj["weights"].ptr, i3((OBJ, OBJ, OBJ)), float(obj["voxel_size"]), float(obj["truncdist"]),
             float(obj["max_weight"]), C.byref(so), f_arr(seed_pose[0]), f_arr(seed_pose[1]), i3((0, 0, 0)), i3((OBJ, OBJ, OBJ)),
             seed_rec.ptr, None)
t = timed(lambda: lib.emf_hip_seedVolume(*seed_args))
print(f"    emf_hip_seedVolume, repeated (its seeded voxels are KEPT): {fmt(t)} with its init launch")
rel_args = (d_bg["tsdf"].ptr, d_bg["weights"].ptr, i3((BG, BG, BG)), VOX, d_mask.ptr, i3((OBJ, OBJ, OBJ)), float(claim["voxel_size"]),
            f_arr(release_pose[0]), f_arr(release_pose[1]), i3(box[0]), i3(box[1]), rel_rec.ptr, None)
t = timed(lambda: lib.emf_hip_releaseVolume(*rel_args))
print(f"    emf_hip_releaseVolume, repeated (its released voxels are EMPTY): {fmt(t)} with its init launch")
walls = []
for i in ids:
    t0 = time.perf_counter()
    fus.lift_object(i)
    walls.append(1e3 * (time.perf_counter() - t0))
first = fus.lifted()[0]
assert first["seed"].tobytes() == s.tobytes() and first["release"].tobytes() == r.tobytes()
stat = lambda v: f"{float(np.median(v)):.3f} ms ({min(v):.3f} .. {max(v):.3f})"  # noqa: E731
print(f"    Fusion.lift_object(), wall over the {len(ids)} objects: {stat(walls)} (two launches, the records' copy-back, "
      "volumesWritten() of the object and of the background, the table rebuild)")
print(f"    the host route: Fusion.volume() of both models, wall {t_copy:.1f} ms; then the numpy restatement of both passes "
      f"{t_host:.1f} ms (one sample each; the upload of the result is not counted)")
fus.close()
synth.close()
