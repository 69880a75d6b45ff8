"""Cost of carrying colour through absorb, seed and release on the configs[1] scene (512^3 + 4 x 128^3)
after `frames` COLOURED frames: one 128^3 object against the 512^3 background.
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of each colour entry beside its
    plain sibling in the same run, on copies of the session's own volumes, each with its init launch.  The passes are in
    place: after the first call of a group the seed finds its seeded voxels KEPT and the release its released voxels
    EMPTY, so their figures are those of a REPEATED call, a lower bound on the first one; a repeated absorption keeps
    fusing the same voxels and pays the colour work every time,
  - host wall time of Fusion.absorb_object() and Fusion.lift_object() with colour on and off (two sessions over the same
    frames), once per object of the scene.
A byte MODEL (not a measurement), on top of the siblings' models (scripts/absorb_timing.py, scripts/lift_timing.py): + 8 B
gathered per FUSED / SEEDED voxel from the source, + 8 B read and at most 8 B written in the destination (the seed and an
uncoloured FRESH absorption write without reading), + 8 B read per RELEASED voxel and 8 B written where the entry held
something.  No roof is claimed.  Nothing is asserted but that the colour entries' tsdf, weights and records equal the
plain entries'.
python scripts/transfer_color_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4


def scene(color):
    prm = pipeline.make_params(W, H, BG, VOX, OBJ)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    if color:
        fus.enable_color()
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        rm = f % prm.mask_frames == 0
        masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if rm else {}
        d = DeviceArray.from_numpy(depth)
        rgb = DeviceArray.from_numpy(np.random.default_rng(f).integers(0, 256, (H, W, 3), dtype=np.uint8))
        if color:
            fus.set_color_image(ops.image_view(rgb))
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


def stat(v):
    return f"{float(np.median(v)):.3f} ms ({min(v):.3f} .. {max(v):.3f})"


lib = _lib.load()
synth, fus, ids = scene(True)
fus.synchronize()
print(f"{frames} coloured frames, {reps} groups of {inner} calls; one object of {OBJ}^3 against the background {BG}^3")
oid = ids[0]
sides = dict(zip(*[fus.object_contacts(ids=[oid])[k] for k in ("ids", "sides")]))
ovox, otrunc, btrunc = float(sides[oid]["voxel_size"]), float(sides[oid]["truncdist"]), float(sides[0]["truncdist"])
maxw = float(fus.params.max_tsdf_weight)
host = {(k, i): fus.volume(k, i) for i in (0, oid) for k in ("tsdf", "weights", "color")}
host_mask = fus.volume("fgmask", oid)
to_bg = pipeline.absorb_pose(fus.pose(oid), fus.background_pose())    # background frame <- object frame (the seed)
to_obj = pipeline.absorb_pose(fus.background_pose(), fus.pose(oid))   # object frame <- background frame (absorb, release)
box = ops.absorb_box((BG, BG, BG), VOX, (OBJ, OBJ, OBJ), ovox, to_obj)
print(f"coloured entries: background {int((host['color', 0][..., 3] > 0).sum())}, object {int((host['color', oid][..., 3] > 0).sum())}")


def device(i):
    return {k: DeviceArray.from_numpy(host[k, i]) for k in ("tsdf", "weights", "color")}


def source(d, res, vox, trunc, mask=None):
    so = _lib.EmfAbsorbSource()
    so.tsdf, so.weights, so.fgVolMask = d["tsdf"].ptr, d["weights"].ptr, None if mask is None else mask.ptr
    so.res, so.voxelSize, so.truncdist = i3(res), vox, trunc
    return so


d_mask = DeviceArray.from_numpy(host_mask)
crec = DeviceArray((1,), ops.COLOR_MOVED_DTYPE)
bg3, obj3, zero3 = (BG, BG, BG), (OBJ, OBJ, OBJ), (0, 0, 0)
results = {}
for name, dtype in (("absorb", ops.ABSORB_DTYPE), ("seed", ops.SEED_DTYPE), ("release", ops.RELEASE_DTYPE)):
    rec = DeviceArray((1,), dtype)
    first = {}
    for colour in (False, True):
        bg, obj = device(0), device(oid)  # fresh copies: both variants start from the session's bytes
        if name == "absorb":
            so = source(obj, obj3, ovox, otrunc, d_mask)
            head = (bg["tsdf"].ptr, bg["weights"].ptr) + ((bg["color"].ptr,) if colour else ()) + (i3(bg3), VOX, btrunc, maxw, C.byref(so))
            tail = (f_arr(to_obj[0]), f_arr(to_obj[1]), i3(box[0]), i3(box[1]), rec.ptr)
            args = head + ((obj["color"].ptr,) if colour else ()) + tail + ((crec.ptr,) if colour else ()) + (None,)
            dst = bg
        elif name == "seed":
            so = source(bg, bg3, VOX, btrunc)
            head = (obj["tsdf"].ptr, obj["weights"].ptr) + ((obj["color"].ptr,) if colour else ()) + (i3(obj3), ovox, otrunc, maxw, C.byref(so))
            tail = (f_arr(to_bg[0]), f_arr(to_bg[1]), i3(zero3), i3(obj3), rec.ptr)
            args = head + ((bg["color"].ptr,) if colour else ()) + tail + ((crec.ptr,) if colour else ()) + (None,)
            dst = obj
        else:
            head = (bg["tsdf"].ptr, bg["weights"].ptr) + ((bg["color"].ptr,) if colour else ())
            args = head + (i3(bg3), VOX, d_mask.ptr, i3(obj3), ovox, f_arr(to_obj[0]), f_arr(to_obj[1]), i3(box[0]), i3(box[1]), rec.ptr) + \
                ((crec.ptr,) if colour else ()) + (None,)
            dst = bg
        entry = getattr(lib, "emf_hip_%sVolume%s" % (name, "Color" if colour else ""))
        assert entry(*args) == 0
        synchronize()
        first[colour] = (rec.numpy()[0].copy(), dst["tsdf"].numpy(), dst["weights"].numpy())
        if colour:
            moved = crec.numpy()[0].copy()
        results[name, colour] = timed(lambda: entry(*args))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[False], first[True])), name  # the same geometry, as bytes
    print(f"{name}: first call {first[True][0]}, colour {moved}")
    print(f"    emf_hip_{name}Volume       repeated: {fmt(results[name, False])} with its init launch")
    print(f"    emf_hip_{name}VolumeColor  repeated: {fmt(results[name, True])} with its init launch")

walls = {}
for colour, (s, f, i) in ((True, (synth, fus, ids)), (False, scene(False))):
    lift, absorb = [], []
    for k in i:
        t0 = time.perf_counter()
        f.lift_object(k)
        lift.append(1e3 * (time.perf_counter() - t0))
    for k in i:
        t0 = time.perf_counter()
        f.absorb_object(k)
        absorb.append(1e3 * (time.perf_counter() - t0))
    walls[colour] = (lift, absorb)
    if colour:
        print("    lifted_colors():", [(int(a["colored"]), int(b["colored"])) for a, b in f.lifted_colors()], "absorbed_colors():",
              [int(c["colored"]) for c in f.absorbed_colors()])
    f.close()
    s.close()
for colour in (False, True):
    word = "on " if colour else "off"
    print(f"    colour {word}: Fusion.lift_object() wall over the {NOBJ} objects {stat(walls[colour][0])}; Fusion.absorb_object() "
          f"{stat(walls[colour][1])}")
