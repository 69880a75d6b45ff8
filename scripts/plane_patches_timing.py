"""Cost of the plane patches (Fusion.planes(patches=True)) on the configs[1] scene (512^3 + 4 x 128^3)
after `frames` frames, over the whole background:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_planePatchLabel at a
    reach of 1 and of 2 and of emf_hip_planePatches, on the records and labels the session's own planes() left,
  - host wall time of Fusion.planes(patches=True) against Fusion.planes(),
  - what the call stands against: there is no earlier implementation, so the existing alternative,
    Fusion.planes(labels=True) with its dense scatter, then scipy.ndimage.label per plane on the host.
Nothing is asserted but that the patch ids equal the restatement's.
python scripts/plane_patches_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd import _lib  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import patches_reference as qr  # noqa: E402

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
got = fus.planes(labels=True, patches=True)
lo, size = got["box"]
rec = got["records"]
n = len(rec)
labels = got["labels"].reshape(-1)[rec["index"]]
print(f"box {got['box']}; counters {got['counters']}, min_votes {got['min_votes']}, patch counters {got['patch_counters']}; "
      + "; ".join(f"{q['kind']} {q['count']}: " + ", ".join(f"{r['count']} (fill {r['fill']:.2f})" for r in q["patches"])
                  for q in got["planes"]))
capacity = max(n, 1)
d_rec, d_lab = DeviceArray.from_numpy(rec if n else np.zeros(1, rec.dtype)), DeviceArray.from_numpy(labels if n else np.zeros(1, np.int16))
d_cnt = DeviceArray.from_numpy(np.array([0, n, n, 0], np.uint32))
d_patch, d_pc = DeviceArray((capacity,), np.int32), DeviceArray((3,), np.uint32)
P = max([q["label"] for q in got["planes"]] + [0]) + 1
axes = np.zeros((P, 6), np.float32)
for q in got["planes"]:
    axes[q["label"]] = np.random.default_rng(q["label"]).normal(size=6)  # any axes cost the same
for reach in (2, 1):  # reach 1 last: its patches are the ones emf_hip_planePatches is timed on
    t = timed(lambda: lib.emf_hip_planePatchLabel(p(d_rec), p(d_lab), p(d_cnt), capacity, i3(size), reach, p(d_patch), p(d_pc), None))
    assert d_patch.numpy()[:n].tobytes() == qr.patch_ids(rec, labels, size, reach).tobytes()
    print(f"    {n} records: emf_hip_planePatchLabel, reach {reach} (four launches): {fmt(t)}; counters {d_pc.numpy().tolist()}")
n_patches = int(d_pc.numpy()[ops.PATCH_PATCHES])
d_scr = DeviceArray((max(ops.plane_patch_scratch_bytes(capacity, n_patches), 16),), np.uint8)
d_out = DeviceArray((max(n_patches, 1),), ops.PLANE_PATCH_DTYPE)
t = timed(lambda: lib.emf_hip_planePatches(p(d_rec), p(d_lab), p(d_patch), p(d_cnt), capacity, i3(size),
                                           axes.ctypes.data_as(C.POINTER(C.c_float)), P, 25, n_patches, p(d_scr), p(d_out), n_patches,
                                           p(d_pc), None))
print(f"    emf_hip_planePatches ({n_patches} patches, min_count 25, seven launches): {fmt(t)}; scratch {d_scr.shape[0]} bytes")
print(f"    Fusion.planes(), wall {fmt(wall(lambda: fus.planes()))}; with patches=True {fmt(wall(lambda: fus.planes(patches=True)))}")
from scipy import ndimage  # noqa: E402

t_labels = wall(lambda: fus.planes(labels=True), 3)
t0 = time.perf_counter()
for q in got["planes"]:
    ndimage.label(got["labels"] == q["label"], structure=np.ones((3, 3, 3), bool))
t_host = time.perf_counter() - t0
print(f"    the alternative: Fusion.planes(labels=True) {fmt(t_labels)}, then scipy.ndimage.label per plane on the host {t_host:.2f} s")
fus.close()
synth.close()
