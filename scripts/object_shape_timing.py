"""Cost of the object shapes (Fusion.object_shapes) on the configs[1] scene (512^3 + 4 x 128^3) after
`frames` frames:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_shapeMoments and
    emf_hip_shapeExtents on the session's own volumes, for the 4 objects of 128^3 in one launch and for the background,
    with and without the unseen-tile maps of the session,
  - host wall time of Fusion.object_shapes() for the objects and with the background,
  - what the call stands against: there is no earlier implementation, so the existing alternative, Fusion.volume() of
    tsdf, weights and fgmask per object plus the numpy restatement of tests/shape_reference.py on the host,
  - a byte MODEL (not a measurement): 8 B read per voxel (9 B with a mask) plus the neighbour gathers of the band.
Nothing is asserted but that the records equal the restatement's.
python scripts/object_shape_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd import _lib  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import shape_reference as sr  # noqa: E402

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


def device_volumes(fus, oid):
    """Device arrays of a model's volumes as the session holds them now, copied (the launches below only read)."""
    v = dict(tsdf=DeviceArray.from_numpy(fus.volume("tsdf", oid)), weights=DeviceArray.from_numpy(fus.volume("weights", oid)))
    if oid:
        v["fg_mask"] = DeviceArray.from_numpy(fus.volume("fgmask", oid))
    return v


def with_maps(volumes):
    out = []
    for v in volumes:
        nz, ny, nx = v["tsdf"].shape
        tiles = DeviceArray((ops.unseen_tile_bytes((nx, ny, nz)),), np.uint8)
        ops.rebuild_unseen_tiles(v["tsdf"], v["weights"], tiles)
        out.append(dict(v, unseen_tiles=tiles))
    return out


lib = _lib.load()
synth, fus, ids = scene()
fus.synchronize()
print(f"{frames} frames, {reps} groups of {inner} calls; {NOBJ} objects of {OBJ}^3, background {BG}^3")
for name, models in ((f"{NOBJ} objects of {OBJ}^3", ids), (f"background {BG}^3", [0])):
    plain = [device_volumes(fus, i) for i in models]
    host = [(v["tsdf"].numpy(), v["weights"].numpy(), v["fg_mask"].numpy() if "fg_mask" in v else None) for v in plain]
    t0 = time.perf_counter()
    want = np.array([sr.moments(*h) for h in host], sr.MOMENTS)
    axes = np.array([sr.frame(m)["f32"] for m in want], sr.AXES)
    want_ext = np.array([sr.extents(*h, a) for h, a in zip(host, axes)], sr.EXTENTS)
    t_host = 1e3 * (time.perf_counter() - t0)
    voxels = sum(int(np.prod(h[0].shape)) for h in host)
    solid, gathers = int(want["solid"].sum()), 6 * int(want["solid"].sum())
    model_bytes = sum(int(np.prod(h[0].shape)) * (9 if h[2] is not None else 8) for h in host) + 8 * gathers
    print(f"{name}: {voxels} voxels, {int(want['observed'].sum())} observed, {solid} solid; byte MODEL {model_bytes / 1e6:.1f} MB "
          f"({voxels} x 8 or 9 B + {gathers} neighbour gathers of up to 8 B)")
    d_axes = DeviceArray.from_numpy(axes)
    for label, volumes in (("no unseen-tile maps", plain), ("with unseen-tile maps", with_maps(plain))):
        mom, ext = DeviceArray((len(models),), ops.SHAPE_MOMENTS_DTYPE), DeviceArray((len(models),), ops.SHAPE_EXTENTS_DTYPE)
        table, res = ops.shape_table(volumes)  # uploaded once: the timed calls enqueue and return
        p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
        t_mom = timed(lambda: lib.emf_hip_shapeMoments(p(table), res, 0, len(models), p(mom), None))
        t_ext = timed(lambda: lib.emf_hip_shapeExtents(p(table), res, 0, len(models), p(d_axes), p(ext), None))
        assert mom.numpy().tobytes() == want.tobytes() and ext.numpy().tobytes() == want_ext.tobytes()
        skipped = sum(int((v["unseen_tiles"].numpy() != 0).sum()) for v in volumes if "unseen_tiles" in v)
        print(f"    {label} ({skipped} tiles skipped): emf_hip_shapeMoments {fmt(t_mom)}, {model_bytes / t_mom[0] / 1e6:.0f} GB/s of the "
              f"model; emf_hip_shapeExtents {fmt(t_ext)} (each with its init launch, the extents with their finish launch)")
    w = wall(lambda: fus.object_shapes(ids=[i for i in models if i], background=0 in models))
    print(f"    Fusion.object_shapes(), wall {fmt(w)}")
    copies = wall(lambda: [(fus.volume("tsdf", i), fus.volume("weights", i), fus.volume("fgmask", i) if i else None) for i in models], 3)
    print(f"    the alternative: Fusion.volume() of tsdf, weights and fgmask per model, wall {fmt(copies)}; then the numpy "
          f"restatement on the host {t_host:.0f} ms")
got = fus.object_shapes(background=True)
for r in got:
    print(f"    id {r['id']}: solid {r['solid']} observed {r['observed']} faces free {r['faces_free']} unknown {r['faces_unknown']} "
          f"completeness {r['completeness']:.3f} half extents [m] {None if r['box_half'] is None else np.round(r['box_half'], 3).tolist()}")
fus.close()
synth.close()
