"""Cost of the plane finder (Fusion.planes) on the configs[1] scene (512^3 + 4 x 128^3) after `frames`
frames, over the whole background with and without the unseen-tile map and over a 128 x 128 x 64 camera box:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_planeSurface,
    emf_hip_planeDirections, emf_hip_planeOffsets and emf_hip_planeAssign on a copy of the volumes the session reports,
    with the directions and planes the session's own run chose,
  - host wall time of Fusion.planes(),
  - what the call stands against: there is no earlier implementation, so the existing alternative, the two
    Fusion.volume() copies plus the numpy restatement of tests/planes_reference.py on the host.
Nothing is asserted but that the records equal the restatement's.
python scripts/planes_timing.py [frames] [reps] [inner]"""
import ctypes as C
import math
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd import _lib  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import planes_reference as pr  # noqa: E402

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


def wall(fn, n=None):
    fn()
    out = []
    for _ in range(n or reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), min(out), max(out)


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


lib = _lib.load()
synth, fus, ids = scene()
fus.synchronize()
print(f"{frames} frames, {reps} groups of {inner} calls; background {BG}^3, voxel {VOX} m")
p = lambda a: None if a is None else C.c_void_p(a.ptr)  # noqa: E731
i3 = lambda v: (C.c_int32 * 3)(*[int(c) for c in v])  # noqa: E731
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
t0 = time.perf_counter()
tsdf, weights = fus.volume("tsdf", 0), fus.volume("weights", 0)
t_copy = 1e3 * (time.perf_counter() - t0)
d_tsdf, d_weights = DeviceArray.from_numpy(tsdf), DeviceArray.from_numpy(weights)
d_map = DeviceArray((ops.unseen_tile_bytes((BG, BG, BG)),), np.uint8)
ops.rebuild_unseen_tiles(d_tsdf, d_weights, d_map)
unseen = d_map.numpy()
print(f"the two Fusion.volume() copies: {t_copy:.0f} ms; unseen tiles: {int((unseen != 0).sum())} of {unseen.size} "
      f"({100.0 * (unseen != 0).mean():.1f} %)")
c = math.cos(math.radians(20.0))
cos2 = float(np.float32(c * c))
for box_name, box_args in (("whole background", {}), ("128 x 128 x 64 camera box", dict(box="camera", size=(128, 128, 64)))):
    got = fus.planes(labels=True, **box_args)
    lo, size = got["box"]
    voxels = size[0] * size[1] * size[2]
    capacity = min(voxels, max(1 << 16, voxels // 8))
    d_rec, d_cnt = DeviceArray((capacity,), ops.PLANE_VOXEL_DTYPE), DeviceArray((4,), np.uint32)
    d_scr = DeviceArray((max(ops.plane_surface_scratch_bytes(size), 4),), np.uint8)
    print(f"{box_name}: box {got['box']}, {voxels} voxels; counters {got['counters']}, min_votes {got['min_votes']}, "
          f"{len(got['planes'])} planes: " + "; ".join(f"{q['kind']} {q['count']}" for q in got["planes"]))
    for name, m in (("with the unseen-tile map", d_map), ("without it", None)):
        t = timed(lambda: lib.emf_hip_planeSurface(p(d_tsdf), p(d_weights), i3((BG, BG, BG)), i3(lo), i3(size), p(m), p(d_rec),
                                                   capacity, p(d_cnt), p(d_scr), None))
        print(f"    emf_hip_planeSurface {name}: {fmt(t)} (four launches), {8.0 * voxels / t[0] / 1e6:.0f} GB/s of the box's tsdf and weights")
    n = int(d_cnt.numpy()[2])
    assert d_rec.numpy()[:n].tobytes() == got["records"].tobytes()
    planes = np.array([list(q["normal_voxel"]) + [q["d_voxel"]] for q in got["planes"]] or [[0, 0, 1, 0]], np.float32)
    dirs = np.ascontiguousarray(planes[:, :3])
    frames_ = [pr.offset_frame([float(v) for v in d], size, 1.0) for d in dirs]
    shift = np.array([f[3] for f in frames_], np.float32)
    S = min(max(f[1] for f in frames_), pr.MAX_SLOTS)
    D, P = min(len(dirs), pr.MAX_DIRS), len(planes)
    d_bins, d_hist = DeviceArray((6 * 15 * 15,), np.uint32), DeviceArray((D * S,), np.uint32)
    d_lab, d_mom = DeviceArray((capacity,), np.int16), DeviceArray((P,), ops.PLANE_MOMENTS_DTYPE)
    t_dir = timed(lambda: lib.emf_hip_planeDirections(p(d_rec), p(d_cnt), capacity, 15, p(d_bins), None))
    t_off = timed(lambda: lib.emf_hip_planeOffsets(p(d_rec), p(d_cnt), capacity, i3(size), fp(dirs), fp(shift), D, cos2, 1.0, S,
                                                   p(d_hist), None))
    t_asg = timed(lambda: lib.emf_hip_planeAssign(p(d_rec), p(d_cnt), capacity, i3(size), fp(planes), P, cos2, 2.0, p(d_lab),
                                                  p(d_mom), None))
    print(f"    {n} records: emf_hip_planeDirections (K 15) {fmt(t_dir)}; emf_hip_planeOffsets ({D} directions, {S} slots) {fmt(t_off)}; "
          f"emf_hip_planeAssign ({P} planes) {fmt(t_asg)}")
    print(f"    Fusion.planes(), wall {fmt(wall(lambda: fus.planes(**box_args)))}; with labels=True {fmt(wall(lambda: fus.planes(labels=True, **box_args), 3))}")
    t0 = time.perf_counter()
    want = pr.find_planes(tsdf, weights, (lo, size), min_votes=None)
    t_host = time.perf_counter() - t0
    assert want[1].tobytes() == got["records"].tobytes() and len(want[0]) == len(got["planes"])
    print(f"    the alternative: the copies above, then the numpy restatement on the host {t_host:.1f} s")
fus.close()
synth.close()
