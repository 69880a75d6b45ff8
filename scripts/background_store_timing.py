"""Cost of the background store (Fusion.set_background_store) on the configs[1] scene (512^3 +
4 x 128^3, 640 x 480) after `frames` frames.  NO FIGURE HAS BEEN TAKEN FROM THIS YET (it has run once, with 10 frames
and 3 repeats, to see that it works): README.md and DESIGN.md carry a byte model, not a measurement, until someone
runs it properly.  Device time from HIP events, median and range of `reps` timed groups; wall time where a whole call
is meant.
  (a) emf_hip_spillTiles of the low-x slab one 64-voxel step thick: 2 x 64 x 64 tiles in four boxes of 2048, each with
      an arena for its worst case (32 MiB without colour); count only, and with the gather.  Every call reads its
      totals back, so the host waits once per box
  (b) emf_hip_fillTiles of those tiles into a second pair of arrays, lists and arenas already on the device
  (c) process_frame + roll_background + synchronize of a frame that rolls out, and of the next one that rolls back,
      with the store on against the same two frames with it off (keep_retired off in both)
Before the timing the filled slab is compared with the source slab byte for byte.
python scripts/background_store_timing.py [frames] [reps]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H, NOBJ, N = 640, 480, 4, 512
STEP = 64
EYE = np.eye(3, dtype=np.float32).reshape(-1)
prm = pipeline.make_params(W, H, N, 0.01, 128)


def session(store):
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    if store:
        fus.set_background_store(True)
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
    return fus, synth, step


def fmt(v):
    return f"{np.median(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def timed(fn, inner=3):
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
    return out


# ---- (a), (b): the two entries on the session's volumes
fus, synth, _ = session(False)
tsdf, wts = DeviceArray.from_numpy(fus.volume("tsdf", 0)), DeviceArray.from_numpy(fus.volume("weights", 0))
fus.close()
synth.close()
nt = (N // 32, N // 8, N // 8)
boxes = [((0, 0, z0), (STEP // 32, nt[1], nt[2] // 4)) for z0 in range(0, nt[2], nt[2] // 4)]
spilled = [ops.spill_tiles(tsdf, wts, lo, size) for lo, size in boxes]
units = sum(s["units"] for s in spilled)
tiles = sum(len(s["classes"]) for s in spilled)
kinds = np.concatenate([s["classes"][:, :2].reshape(-1) for s in spilled])
print(f"after {frames} frames the slab holds {tiles} tiles: {np.bincount(kinds, minlength=3).tolist()} arrays of class 0 / 1 / 2, "
      f"{units} literal units ({units * 8192 / 2 ** 20:.1f} MiB of {tiles * 16384 / 2 ** 20:.1f} MiB)")
dst = DeviceArray.zeros((N, N, N), np.float32), DeviceArray.zeros((N, N, N), np.float32)
lists = []
for (lo, size), s in zip(boxes, spilled):
    coords = np.array([(lo[0] + x, lo[1] + y, lo[2] + z) for z in range(size[2]) for y in range(size[1]) for x in range(size[0])],
                      np.int32)
    lists.append((coords, s))
    ops.fill_tiles(dst[0], dst[1], coords, s["classes"], s["words"], s["lits"], arena=s["arena"])
assert dst[0].numpy()[:, :, :STEP].tobytes() == tsdf.numpy()[:, :, :STEP].tobytes(), "fill(spill(slab)) differs from the slab"
assert dst[1].numpy()[:, :, :STEP].tobytes() == wts.numpy()[:, :, :STEP].tobytes(), "fill(spill(slab)) differs from the slab"
print(f"(a) spill, count only:  {fmt(timed(lambda: [ops.spill_tiles(tsdf, wts, lo, size, count_only=True) for lo, size in boxes], 1))}")
print(f"(a) spill with gather:  {fmt(timed(lambda: [ops.spill_tiles(tsdf, wts, lo, size) for lo, size in boxes], 1))}")
print(f"(b) fill (with the upload of its lists): "
      f"{fmt(timed(lambda: [ops.fill_tiles(dst[0], dst[1], c, s['classes'], s['words'], s['lits'], arena=s['arena']) for c, s in lists], 1))}")
del dst, tsdf, wts, spilled, lists

# ---- (c): whole calls on a session, store off and on, rolling out and back so that the scene stays in the cube
for store in (False, True):
    fus, synth, step = session(store)
    wall = {"frame + roll out": [], "frame + roll back": []}
    f = frames
    for rep in range(2 * reps + 2):
        out = rep % 2 == 0
        synchronize()
        t0 = time.perf_counter()
        step(f)
        fus.roll_background((STEP if out else -STEP, 0, 0), keep_retired=False)
        fus.synchronize()
        if rep >= 2:
            wall["frame + roll out" if out else "frame + roll back"].append(1e3 * (time.perf_counter() - t0))
        f += 1
    for k, v in wall.items():
        print(f"(c) store {'on ' if store else 'off'} {k:18s} wall: {fmt(v)}")
    if store:
        print(f"    store: {fus.background_store_info()}")
    fus.close()
    synth.close()
