"""Cost of rolling the background (Fusion.set_background_follow / roll_background) on the configs[1]
scene (512^3 + 4 x 128^3, 640 x 480) after `frames` frames.  Device time from HIP events, median and range of `reps`
timed groups; wall time where a whole call is meant.
  (a) emf_hip_rollVolume, tile-granular, shift (64, 0, 0), from the session's front copy into a second pair of arrays
      with the maps moved along, plus what makes the copies equal: one device-to-device copy per array
  (b) the same end state from the entries that existed before: emf_hip_copyValues x 2, emf_hip_rebuildSignMaps,
      emf_hip_rebuildUnseenTiles, and the same copy per array
  (c) process_frame + synchronize of a frame that ends with a roll (keep_retired off) against an ordinary frame
  (d) roll_background with keep_retired on against off: retiring one 64-voxel slab (cut, mesh, download)
(a) and (b) alternate in one process; both end states are compared byte for byte once, before the timing.
python scripts/background_roll_timing.py [frames] [reps]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import devmem, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, DeviceView, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H, NOBJ, N = 640, 480, 4, 512
SHIFT = (64, 0, 0)
EYE = np.eye(3, dtype=np.float32).reshape(-1)

prm = pipeline.make_params(W, H, N, 0.01, 128)
synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
fus = pipeline.Fusion(prm, None)
ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
keep = []


def step(f):
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    poses = {i: (EYE, synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if f == 0 else {}
    d = DeviceArray.from_numpy(depth)
    keep[:] = [d, masks]
    fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
    fus.synchronize()


for f in range(frames):
    step(f)


def front(which):
    ptr, res = C.c_void_p(), (C.c_int32 * 3)()
    rc = pipeline.load().emf_fusion_get_volume(fus._h, pipeline.VOL[which], 0, C.byref(ptr), res)
    assert rc == 0 and tuple(res) == (N, N, N)
    return DeviceView(ptr.value, (N, N, N), np.float32)


hip = devmem._hip
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


def d2d(dst, src):
    rc = hip.hipMemcpyAsync(C.c_void_p(dst.ptr), C.c_void_p(src.ptr), src.nbytes, 3, None)  # hipMemcpyDeviceToDevice
    assert rc == 0, rc


src_t, src_w = front("tsdf"), front("weights")
res = (N, N, N)
src_sign = DeviceArray.zeros((ops.sign_map_bytes(res),), np.uint8)
src_unseen = DeviceArray.zeros((ops.unseen_tile_bytes(res),), np.uint8)
ops.rebuild_sign_maps(src_t, src_sign)
ops.rebuild_unseen_tiles(src_t, src_w, src_unseen)
dst = (DeviceArray((N, N, N), np.float32), DeviceArray((N, N, N), np.float32))
other = (DeviceArray((N, N, N), np.float32), DeviceArray((N, N, N), np.float32))
new_sign, new_unseen = DeviceArray.zeros(src_sign.shape, np.uint8), DeviceArray.zeros(src_unseen.shape, np.uint8)
state = {}


def new_way():
    _, _, _, s, u = ops.roll_volume(src_t, src_w, SHIFT, sign_maps=src_sign, unseen_tiles=src_unseen, out=dst)
    d2d(other[0], dst[0])
    d2d(other[1], dst[1])
    state["maps"] = (s, u)


def old_way():
    ops.copy_values(src_t, dst[0], SHIFT)
    ops.copy_values(src_w, dst[1], SHIFT)
    ops.rebuild_sign_maps(dst[0], new_sign)
    ops.rebuild_unseen_tiles(dst[0], dst[1], new_unseen)
    d2d(other[0], dst[0])
    d2d(other[1], dst[1])


def digest():
    import hashlib
    synchronize()
    h = hashlib.sha256()
    for a in dst + other:
        h.update(a.numpy().tobytes())
    return h.hexdigest()


old_way()
want, want_maps = digest(), (new_sign.numpy().tobytes(), new_unseen.numpy().tobytes())
new_way()
assert digest() == want, "the two ways give different volumes"
assert (state["maps"][0].numpy().tobytes(), state["maps"][1].numpy().tobytes()) == want_maps, "the moved maps differ from rebuilt ones"
unseen_share = float(src_unseen.numpy().mean())
print(f"after {frames} frames: {100 * unseen_share:.1f} % of the background's tiles are unseen; both ways give the same bytes")


def timed_pair(fa, fb, inner=3):
    """Interleaved: [(median, min, max) ms per call] of fa and fb over `reps` groups of `inner` calls each."""
    out = ([], [])
    for fn in (fa, fb):
        fn()
    synchronize()
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = Event(), Event()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_ms(b) / inner)
    return [(float(np.median(v)), min(v), max(v)) for v in out]


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


ta, tb = timed_pair(new_way, old_way)
gb = 4 * N ** 3 / 1e9
print(f"(a) emf_hip_rollVolume + a copy per array:                          {fmt(ta)}")
print(f"(b) copyValues x 2 + rebuildSignMaps + rebuildUnseenTiles + copies: {fmt(tb)}")
print(f"    (b) / (a) = {tb[0] / ta[0]:.2f}; one array is {gb:.2f} GB")
roll_only = timed_pair(lambda: ops.roll_volume(src_t, src_w, SHIFT, sign_maps=src_sign, unseen_tiles=src_unseen, out=dst),
                       lambda: (ops.copy_values(src_t, dst[0], SHIFT), ops.copy_values(src_w, dst[1], SHIFT)))
print(f"    the roll launch alone: {fmt(roll_only[0])}; copyValues x 2 alone: {fmt(roll_only[1])}")
del dst, other

# ---- (c), (d): whole calls on the session, rolling forth and back so that the scene stays in the cube
wall = {"frame": [], "frame+roll": [], "roll": [], "roll+retire": []}
f = frames
for rep in range(2 * reps + 2):
    sign = 1 if rep % 2 == 0 else -1
    synchronize()
    t0 = time.perf_counter()
    step(f)
    t1 = time.perf_counter()
    fus.roll_background((sign * 64, 0, 0), keep_retired=False)
    fus.synchronize()
    t2 = time.perf_counter()
    if rep >= 2:
        wall["frame"].append(1e3 * (t1 - t0))
        wall["frame+roll"].append(1e3 * (t2 - t0))
        wall["roll"].append(1e3 * (t2 - t1))
    f += 1
for rep in range(2 * min(reps, 3)):
    sign = 1 if rep % 2 == 0 else -1
    synchronize()
    t0 = time.perf_counter()
    fus.roll_background((sign * 64, 0, 0), keep_retired=True)
    fus.synchronize()
    wall["roll+retire"].append(1e3 * (time.perf_counter() - t0))
for k, v in wall.items():
    print(f"({'c' if 'frame' in k else 'd'}) {k:12s} wall: {np.median(v):.2f} ms ({min(v):.2f} .. {max(v):.2f})")
slabs = fus.retired_slabs()
print(f"    retired slabs: {len(slabs)}, triangles {[len(s['triangles']) for s in slabs]}")
fus.close()
synth.close()
