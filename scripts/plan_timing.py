"""Cost of path planning (Fusion.plan) on the configs[1] scene (512^3 + 4 x 128^3) after `frames`
frames, for the whole background and for a 128 x 128 x 64 box around the camera, from the voxel under the camera to
the representatives of the scene's frontier clusters:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_planCost on the
    session's own classes -- the whole entry, which waits once per batch of rounds, and the same entry cut off after
    one round (k_pl_init, one k_pl_relax, k_pl_finish: what a call costs before the relaxation proper) -- with the
    rounds it enqueued and the voxels it reached, and of emf_hip_planPaths,
  - host wall time of Fusion.plan() with and without a clearance of 0.2 m, frontiers() included,
  - how many of the scene's frontier clusters are reachable.
The active tiles per round are not exported by the entry; a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/plan_timing.py) splits the entry into k_pl_init, k_pl_relax,
k_pl_finish and k_pl_paths.  What the call stands against is not another planner but the 167 ms that
Fusion.distance_field() needs merely to bring the classes of the 512^3 background to the host,
before any host search has begun.
python scripts/plan_timing.py [frames] [reps] [inner]"""
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
cv = int(np.ceil(np.float32(CLEARANCE) / np.float32(VOX)))
print(f"{frames} frames, {reps} groups of {inner} calls; min_voxels {MIN_VOXELS}, clearance {CLEARANCE} m = {cv} voxels")
for name, box in (("whole 512^3", None), ("128 x 128 x 64 camera box", fus.camera_box((128, 128, 64)))):
    for label, clearance in (("no clearance", 0.0), (f"clearance {cv} voxels", CLEARANCE)):
        got = fus.plan(box=box, min_voxels=MIN_VOXELS, clearance=clearance)
        lo, size = got["box"]
        df = fus.distance_field(box=box, cap=clearance, metres=False)
        classes = DeviceArray.from_numpy(df["classes"])
        d2 = DeviceArray.from_numpy(df["d2"]) if clearance > 0 else None
        seeds, radius = got["start_voxels"], got["start_radius_voxels"]
        goals = np.array([g["voxel"] for g in got["goals"]], np.int32).reshape(-1, 3)
        cost = DeviceArray(classes.shape, np.uint32)
        kw = dict(d2=d2, min_d2=min(cv, 4095) ** 2 if clearance > 0 else 0, seed_radius=radius, out=cost)
        t_first = timed(lambda: ops.plan_cost(classes, seeds, max_rounds=1, **kw))
        t_cost = timed(lambda: ops.plan_cost(classes, seeds, **kw))
        counters = cost.counters.numpy()
        print(f"{name}, {label}: box {lo} + {size}, {int(np.prod(size))} voxels, start {seeds[0].tolist()} radius {radius}")
        print(f"    cost field {fmt(t_cost)}: {int(counters[ops.PLAN_ROUNDS])} rounds enqueued, converged "
              f"{int(counters[ops.PLAN_CONVERGED])}, {int(counters[ops.PLAN_FINITE])} voxels reached; cut off after one round "
              f"(init + one round + count) {fmt(t_first)}")
        if len(goals):
            longest = max(max(len(g["path_vox"]) for g in got["goals"]), 1)
            paths = DeviceArray((len(goals), longest), np.int32)
            lengths, goal_cost = DeviceArray((len(goals),), np.int32), DeviceArray((len(goals),), np.uint32)
            t_paths = timed(lambda: ops.plan_paths(cost, goals, capacity=longest, paths=paths, lengths=lengths, goal_cost=goal_cost))
            print(f"    paths of {len(goals)} goals, the longest {longest} voxels: {fmt(t_paths)} (with the upload of the goals)")
        reach = [g for g in got["goals"] if g["reachable"]]
        print(f"    {len(reach)} of {len(got['goals'])} frontier clusters reachable"
              + (f"; the cheapest at {reach[0]['length_m']:.2f} m, the dearest at {reach[-1]['length_m']:.2f} m" if reach else ""))
        w = wall(lambda: fus.plan(box=box, min_voxels=MIN_VOXELS, clearance=clearance))
        print(f"    Fusion.plan() with frontiers(), the rounds' waits and the paths copied, wall {fmt(w)}")
fus.close()
synth.close()
