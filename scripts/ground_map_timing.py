"""Cost of the ground map (Fusion.ground_map / ground_plan) on the configs[1] scene (512^3 + 4 x 128^3)
after `frames` frames, over the whole background and over a 128 x 128 x 64 camera box, for two frames -- an up along a box
axis and a tilted one:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_groundColumns,
    emf_hip_groundCells and emf_hip_groundClasses on the classes the session's distance field reports,
  - the number of 64-bit atomics the columns pass needs at the least (one per destination word and plane that receives a
    bit) and at the most (one per known voxel), counted on the host from the restatement's slots; what the kernel issues
    lies between them and depends on how the lanes of a wave share their words,
  - host wall time of Fusion.ground_map() and Fusion.ground_plan(),
  - what the calls stand against: there is no earlier implementation, so the existing alternative, Fusion.distance_field()
    with its copies plus the numpy restatement of tests/ground_reference.py on the host (planes only: its cell loop is
    Python and is not timed),
  - a byte MODEL (not a measurement): the columns pass reads 1 B per voxel plus one 8-byte atomic per run of known lanes;
    the cells pass reads 16 B x words per cell.
Nothing is asserted but that the planes equal the restatement's.
python scripts/ground_map_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd import _lib  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402
from tests import ground_reference as rf  # noqa: E402

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
p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
# the wall the camera looks at as the floor (up along -z of the first pose), and the same tilted off the axes
UPS = (("up along a box axis", (0.0, 0.0, -1.0)), ("tilted up", (0.12, -0.2, -1.0)))
BAND = (-4.0, 0.5)
for box_name, box_args in (("whole background", {}), ("128 x 128 x 64 camera box", dict(box="camera", size=(128, 128, 64)))):
    t_df = wall(lambda: fus.distance_field(metres=False, **box_args), 3)
    df = fus.distance_field(metres=False, **box_args)
    classes = df["classes"]
    d_classes = DeviceArray.from_numpy(classes)
    known = int((classes <= 1).sum())
    print(f"{box_name}: box {df['box']}, {classes.size} voxels, {known} known ({100.0 * known / classes.size:.1f} %); "
          f"Fusion.distance_field() with its copies, wall {fmt(t_df)}")
    for up_name, up in UPS:
        kw = dict(up=up, band=BAND, robot_height=0.3, max_step=0.05)
        gm = fus.ground_map(**box_args, **kw)
        G, gw, gh, B = gm["frame"]
        words = rf.words_of(B)
        frame = ops.ground_frame(G, (gw, gh), B)
        t0 = time.perf_counter()
        occ, fre = rf.planes(classes, G, gw, gh, B)
        t_host = 1e3 * (time.perf_counter() - t0)
        iu, iv, ih, keep = rf.slots(classes.shape[::-1], G, gw, gh, B)
        hit = keep & (classes <= 1)
        dest = ((iv * gw + iu) * words + (ih >> 6)) * 2 + (classes == 1)
        fewest, most = int(np.unique(dest[hit]).size), int(hit.sum())
        d_occ, d_fre = DeviceArray((gh, gw, words), np.uint64), DeviceArray((gh, gw, words), np.uint64)
        d_cells, d_2d = DeviceArray((gh, gw), ops.GROUND_CELL_DTYPE), DeviceArray((1, gh, gw), np.uint8)
        size, map_ = (C.c_int32 * 3)(*classes.shape[::-1]), (C.c_int32 * 2)(gw, gh)
        t_col = timed(lambda: lib.emf_hip_groundColumns(p(d_classes), size, frame, p(d_occ), p(d_fre), None))
        t_cel = timed(lambda: lib.emf_hip_groundCells(p(d_occ), p(d_fre), map_, B, gm["robot_bins"], p(d_cells), None))
        t_cls = timed(lambda: lib.emf_hip_groundClasses(p(d_cells), map_, gm["max_step_bins"], p(d_2d), None))
        assert d_occ.numpy().tobytes() == occ.tobytes() and d_fre.numpy().tobytes() == fre.tobytes()
        assert d_cells.numpy().tobytes() == gm["cells"].tobytes() and d_2d.numpy()[0].tobytes() == gm["classes"].tobytes()
        print(f"    {up_name}: map {gw} x {gh} x {B} bins; emf_hip_groundColumns {fmt(t_col)} (with its zeroing launch), "
              f"{classes.size / t_col[0] / 1e6:.0f} GB/s of the classes; 64-bit atomics needed: at least {fewest} (one per word "
              f"and plane that receives a bit), at most {most} (one per known voxel inside the map); emf_hip_groundCells "
              f"{fmt(t_cel)} ({16 * words * gw * gh / 1e6:.2f} MB read); emf_hip_groundClasses {fmt(t_cls)}")
        free = int((gm["classes"] == 0).sum())
        print(f"        {free} free, {int((gm['classes'] == 1).sum())} occupied, {int((gm['classes'] == 2).sum())} unknown cells; "
              f"{int((gm['levels'] > 1).sum())} cells with more than one level")
        w_map = wall(lambda: fus.ground_map(**box_args, **kw))
        w_plan = wall(lambda: fus.ground_plan(**box_args, **kw))
        plan = fus.ground_plan(**box_args, **kw)
        print(f"        Fusion.ground_map(), wall {fmt(w_map)}; Fusion.ground_plan(), wall {fmt(w_plan)} "
              f"({len(plan['goals'])} goals, {sum(g['reachable'] for g in plan['goals'])} reachable, {plan['n_finite']} cells reached)")
        print(f"        the alternative: distance_field() above, then the numpy restatement of the planes on the host {t_host:.0f} ms")
fus.close()
synth.close()
