"""Cost of the object contacts (Fusion.object_contacts) on the configs[1] scene (512^3 + 4 x 128^3) after
`frames` frames: the 4 objects against each other and the background, 16 ordered pairs.
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_contactProbe on the
    session's own volumes, with and without the unseen-tile maps of the probes,
  - host wall time of Fusion.object_contacts(),
  - what the call stands against: there is no earlier implementation, so the existing alternative, Fusion.volume() of
    tsdf, weights and fgmask per model plus the numpy restatement of tests/contacts_reference.py on the host,
  - how many surface voxels and samples the call made and a byte MODEL (not a measurement) of them: 8 B (9 B with a mask)
    per probe voxel for the surface test plus the neighbour gathers of the solid voxels, then 16 gathers of 4 B per sample
    inside a field.  The kernel is a dependent-gather pass (the address of a sample depends on the transform of the voxel):
    no roof is claimed.
Nothing is asserted but that the records equal the restatement's.  The 64-object scene is not measured here.
python scripts/object_contacts_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd import _lib  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import contacts_reference as cr  # noqa: E402
from tests.shape_reference import solid_mask  # noqa: E402

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


def copies(fus, models):
    return [(fus.volume("tsdf", i), fus.volume("weights", i), fus.volume("fgmask", i) if i else None) for i in models]


lib = _lib.load()
synth, fus, ids = scene()
fus.synchronize()
models = [0] + ids
print(f"{frames} frames, {reps} groups of {inner} calls; {NOBJ} objects of {OBJ}^3 against each other and the background {BG}^3")
found = fus.object_contacts(ids=ids)
sides = dict(zip(found["ids"], found["sides"]))
t_copy = wall(lambda: copies(fus, models), 3)
host = dict(zip(models, copies(fus, models)))
t0 = time.perf_counter()
vols = {i: cr.vol(*host[i], sides[i]["voxel_size"]) for i in models}
want = np.array([cr.probe(vols[p["a"]], vols[p["b"]], p["pair"]) for p in found["pairs"]], cr.CONTACT)
t_host = 1e3 * (time.perf_counter() - t0)
assert np.array([p["record"] for p in found["pairs"]], cr.CONTACT).tobytes() == want.tobytes()
probe_voxels = sum(int(np.prod(host[i][0].shape)) for i in ids)
solid = sum(int(solid_mask(*host[i]).sum()) for i in ids)
surface = sum(int(cr.surface_mask(*host[i]).sum()) for i in ids)
inside_field = int((want["surface"] - want["outside"]).sum())
model_bytes = 9 * probe_voxels + 8 * 6 * solid + 64 * inside_field
print(f"{len(want)} ordered pairs; {probe_voxels} probe voxels, {solid} solid, {surface} surface voxels; {int(want['surface'].sum())} "
      f"(surface voxel, field) pairs, {inside_field} inside a field (16 gathers each), {int(want['sampled'].sum())} sampled, "
      f"{int(want['touching'].sum())} touching; byte MODEL {model_bytes / 1e6:.1f} MB ({probe_voxels} x 9 B + {6 * solid} neighbour "
      f"gathers of up to 8 B + {16 * inside_field} gathers of 4 B)")
plain = []
for i in models:
    v = dict(tsdf=DeviceArray.from_numpy(host[i][0]), weights=DeviceArray.from_numpy(host[i][1]), voxel_size=sides[i]["voxel_size"])
    if i:
        v["fg_mask"] = DeviceArray.from_numpy(host[i][2])
    plain.append(v)
mapped = []
for v in plain:
    nz, ny, nx = v["tsdf"].shape
    tiles = DeviceArray((ops.unseen_tile_bytes((nx, ny, nz)),), np.uint8)
    ops.rebuild_unseen_tiles(v["tsdf"], v["weights"], tiles)
    mapped.append(dict(v, unseen_tiles=tiles))
slot = {i: k for k, i in enumerate(models)}
pairs = np.array([p["pair"] for p in found["pairs"]], ops.CONTACT_PAIR_DTYPE)
assert all(slot[p["a"]] == p["pair"]["a"] and slot[p["b"]] == p["pair"]["b"] for p in found["pairs"])
d_pairs = DeviceArray.from_numpy(pairs)
for label, volumes in (("no unseen-tile maps", plain), ("with unseen-tile maps", mapped)):
    table, res = ops.contact_table(volumes)  # uploaded once: the timed calls enqueue and return
    rec = DeviceArray((len(pairs),), ops.CONTACT_DTYPE)
    p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
    t = timed(lambda: lib.emf_hip_contactProbe(p(table), res, len(volumes), p(d_pairs), C.c_void_p(pairs.ctypes.data), len(pairs),
                                               p(rec), None))
    assert rec.numpy().tobytes() == want.tobytes()
    skipped = sum(int((v["unseen_tiles"].numpy() != 0).sum()) for v in volumes[1:] if "unseen_tiles" in v)
    print(f"    {label} ({skipped} probe tiles skipped): emf_hip_contactProbe {fmt(t)} with its init and finish launches, "
          f"{model_bytes / t[0] / 1e6:.0f} GB/s of the model")
w = wall(lambda: fus.object_contacts(ids=ids))
print(f"    Fusion.object_contacts(), wall {fmt(w)}")
print(f"    the alternative: Fusion.volume() of tsdf, weights and fgmask per model, wall {fmt(t_copy)}; then the numpy restatement "
      f"on the host {t_host:.0f} ms")
for s in found["summaries"]:
    print(f"    {s['a']} - {s['b']}: {s['state']}, distance {s['distance_m']:.4f} m{' (saturated)' if s['saturated'] else ''}")
fus.close()
synth.close()
