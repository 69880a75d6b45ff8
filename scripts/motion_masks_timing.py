"""Cost of the motion masks (Fusion.set_motion_masks) at 640 x 480 on the configs[1] scene
(512^3 + 4 x 128^3) with one sphere displaced by 0.5 m, so that it stands clear of what the background holds of it:
  - the proposals of that frame (count, areas) and their equality with the restatement (tests/motion_reference.py),
  - device time (HIP events, median and range of `reps` timed groups of 20 calls) of emf_hip_motionMasks on the
    frame's points and background ray lengths, for erode = 0 .. 3: stages 1 and 3-5 are the erode = 0 line, one
    erosion pass (stage 2) the difference between two lines,
  - host wall time of process_frame + synchronize on a mask frame with the mode off and on, alternating.
The split of the entry into its stages' kernels (k_mm_candidates; k_mm_erode; k_mm_hook, k_mm_flatten; k_mm_count,
k_mm_flags, k_mm_scan, k_mm_compact, k_mm_select; k_mm_emit) is read from a kernel trace of this script, taken in a
run of its own (rocprofv3 --kernel-trace --stats -- python scripts/motion_masks_timing.py).
python scripts/motion_masks_timing.py [frames] [reps]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import motion_reference as mr  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H, NOBJ = 640, 480, 4
EYE = np.eye(3, dtype=np.float32).reshape(-1)
MOTION = dict(band=0.1, continuity=0.05, erode=1, min_pixels=200, max_masks=8)  # band: the background's 10 voxels

prm = pipeline.make_params(W, H, 512, 0.01, 128)
synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
fus = pipeline.Fusion(prm, None)
ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]


def frame_inputs(f, displaced=False):
    """Depth and poses of stream frame f; displaced: sphere 0 is painted 0.5 m nearer over its own pixels (it keeps its
    silhouette and comes forward), the object poses stay the stream's."""
    depth, sid = synth.render(f)
    if displaced:
        depth = np.where(sid == 1, np.maximum(depth - np.float32(0.5), np.float32(0.3)), depth).astype(np.float32)
    R, t = synth.camera_pose(f)
    poses = {i: (EYE, synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    return depth, sid, R, t, poses


def step(f, displaced=False, run_masks=False):
    depth, sid, R, t, poses = frame_inputs(f, displaced)
    d = DeviceArray.from_numpy(depth)
    fus.process_frame(ops.image_view(d), R, t, poses, {}, run_masks)
    fus.synchronize()
    return sid


for f in range(frames):  # the scene as the background knows it, objects fed by their ground-truth masks on frame 0
    depth, sid, R, t, poses = frame_inputs(f)
    masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if f == 0 else {}
    d = DeviceArray.from_numpy(depth)
    fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
    fus.synchronize()


def timed(fn, inner=20):
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
    return f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


# ---- the displaced frame: proposals, and the entry alone on its images
fus.set_motion_masks(True, **MOTION)
sid = step(frames, displaced=True, run_masks=True)
labels, proposals = fus.last_motion_masks()
points, bg = fus.image("points"), fus.image("bg_raylengths")
ref = mr.motion_masks(points, bg, **MOTION)
assert labels.tobytes() == ref["labels"].tobytes() and proposals == mr.proposals(ref), "proposals differ from the restatement"
truth = int((sid == 1).sum())
print(f"displaced frame: {len(proposals)} proposal(s), areas {[p['area'] for p in proposals]}, the sphere covers {truth} "
      f"pixels, {int(((labels >= 0) & (sid == 1)).sum())} of the proposed pixels lie on it; equal to the restatement")
dp, db = DeviceArray.from_numpy(points), DeviceArray.from_numpy(bg)
buffers = ops.MotionBuffers(W, H)
p = ops.motion_params(**MOTION)
import ctypes as C  # noqa: E402
lib = ops._L
for erode in (0, 1, 2, 3):
    p.erode = erode

    def entry():
        rc = lib.emf_hip_motionMasks(dp.ptr, db.ptr, W, H, C.byref(p), buffers.scratch.ptr, buffers.labels.ptr,
                                     buffers.masks.ptr, buffers.info.ptr, buffers.count.ptr, None)
        assert rc == 0, rc

    print(f"emf_hip_motionMasks, erode = {erode} ({9 + erode} launches): {fmt(timed(entry))}; "
          f"{int(buffers.count.numpy()[0])} proposal(s)")

# ---- a mask frame end to end, mode off and on, alternating (the same displaced frame again and again: the timing is
# of the frame, not of a scene that evolves)
wall = {False: [], True: []}
for rep in range(2 * reps + 2):
    on = rep % 2 == 1
    fus.set_motion_masks(on, **MOTION)
    depth, _, R, t, poses = frame_inputs(frames, displaced=True)
    d = DeviceArray.from_numpy(depth)
    synchronize()
    t0 = time.perf_counter()
    fus.process_frame(ops.image_view(d), R, t, poses, {}, True)
    fus.synchronize()
    if rep >= 2:
        wall[on].append(1e3 * (time.perf_counter() - t0))
for on in (False, True):
    v = wall[on]
    print(f"process_frame + synchronize on a mask frame, motion masks {'on ' if on else 'off'}: "
          f"{np.median(v):.3f} ms ({min(v):.3f} .. {max(v):.3f}); objects {fus.object_ids()}")
fus.close()
synth.close()
