"""Cost and gain of the component filter (Fusion.set_mesh_filter) on the configs[1] scene (512^3 + 4 x 128^3) and the
65-model scene (512^3 + 64 x 128^3):
  - components, kept components, triangles and kept triangles of the scene, and the bytes the welded and the filtered
    form copy device to host,
  - device time (HIP events, median and range of `reps` timed groups) of the three entries on the welded arrays:
    label (init + hook + flatten + count), filter count (select + flags + scans + ranks + bases), emit,
  - host wall time of Fusion.meshes(), welded (the path of set_mesh_weld alone, unchanged) against welded + filtered.
The split of an entry into its launches (hook, flatten, count ...) is read from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/mesh_components_timing.py): the kernels are k_cc_*.
python scripts/mesh_components_timing.py [frames] [reps] [min_triangles]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 6
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
min_triangles = int(sys.argv[3]) if len(sys.argv) > 3 else 8
W, H = 640, 480


def scene(nobj):
    prm = pipeline.make_params(W, H, 512, 0.01, 128)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), nobj, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(nobj)]
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


def timed(fn, inner=5):
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


for name, nobj in (("configs[1] 512^3 + 4 x 128^3", 4), ("65 models 512^3 + 64 x 128^3", 64)):
    synth, fus, ids = scene(nobj)
    vols = [dict(tsdf=DeviceArray.from_numpy(fus.volume("tsdf", 0)),
                 weights=DeviceArray.from_numpy(fus.volume("weights", 0)), voxel_size=0.01)]
    vox = float(np.float32(synth.sphere(0, 0)[2]) / np.float32(128))
    for i in ids:
        vols.append(dict(tsdf=DeviceArray.from_numpy(fus.volume("tsdf", i)),
                         weights=DeviceArray.from_numpy(fus.volume("weights", i)),
                         fg_mask=DeviceArray.from_numpy(fus.volume("fgmask", i)), voxel_size=vox))
    n, L, P = len(vols), ops._L, ops._ptr
    # the welded arrays on the device, as extractWelded leaves them
    table, res = ops.mesh_table(vols)
    scratch = DeviceArray.zeros((int(L.emf_hip_meshScratchBytesBatched(res, n)) // 4 + 2,), np.uint32)
    counts, bases = DeviceArray.zeros((n, 2), np.uint32), DeviceArray.zeros((n + 1, 2), np.uint64)
    ops.check("meshCountBatched", L.emf_hip_meshCountBatched(P(table), res, n, P(scratch), P(counts), P(bases), None))
    nv, nt = (int(x) for x in bases.numpy()[n])
    verts, norms = DeviceArray.zeros((max(nv, 1), 3)), DeviceArray.zeros((max(nv, 1), 3))
    tris, keys = DeviceArray.zeros((max(nt, 1), 4), np.int32), DeviceArray.zeros((max(nv, 1),), np.uint64)
    ops.check("meshEmitBatched", L.emf_hip_meshEmitBatched(P(table), res, n, P(scratch), P(verts), P(norms), P(tris), None))
    ops.check("meshEdgeKeysBatched", L.emf_hip_meshEdgeKeysBatched(P(table), res, n, P(scratch), P(keys), None))
    wv, wn, wt, _, wcnt, _, wbases = ops._weld(keys, nv, nt, verts, norms, tris, None, soup_bases=bases, n=n)
    nw = int(wcnt.sum())
    cc = DeviceArray.zeros((int(L.emf_hip_meshComponentsScratchBytes(nw, nt)) // 4,), np.uint32)
    mins = np.full((n,), min_triangles, np.uint32)
    largest = np.array([0] + [1] * (n - 1), np.uint8)
    kcounts, kbases = DeviceArray.zeros((n, 2), np.uint32), DeviceArray.zeros((n + 1, 2), np.uint64)
    comps, kcomps = DeviceArray.zeros((n,), np.uint32), DeviceArray.zeros((n,), np.uint32)
    hp = lambda a: a.ctypes.data  # noqa: E731

    def label():
        ops.check("meshComponentsLabelBatched",
                  L.emf_hip_meshComponentsLabelBatched(P(wt), nw, nt, P(bases), P(wbases), n, P(cc), None, None, None))

    def filter_count():
        ops.check("meshComponentsFilterCountBatched",
                  L.emf_hip_meshComponentsFilterCountBatched(P(wt), nw, nt, P(bases), P(wbases), n, P(cc), hp(mins),
                                                             hp(largest), P(kcounts), P(kbases), P(comps), P(kcomps),
                                                             None))

    label()
    filter_count()
    ops.check("meshComponentsStatus", L.emf_hip_meshComponentsStatus(P(cc), nw, nt, None))
    knv, knt = (int(x) for x in kbases.numpy()[n])
    kv, kn = DeviceArray.zeros((max(knv, 1), 3)), DeviceArray.zeros((max(knv, 1), 3))
    kt = DeviceArray.zeros((max(knt, 1), 4), np.int32)

    def emit():
        ops.check("meshComponentsEmitBatched",
                  L.emf_hip_meshComponentsEmitBatched(P(cc), nw, nt, P(bases), P(wbases), n, P(wv), P(wn), None, P(wt),
                                                      P(kv), P(kn), None, P(kt), None))

    tl, tf, te = timed(label), timed(filter_count), timed(emit)
    d2h_weld, d2h_kept = nw * 24 + nt * 16, knv * 24 + knt * 16
    print(f"{name}: {n} models, {nw} welded vertices, {nt} triangles; min_triangles {min_triangles}, largest component "
          f"only for the objects")
    print(f"  components {int(comps.numpy().sum())} -> {int(kcomps.numpy().sum())} kept; triangles {nt} -> {knt}; "
          f"vertices {nw} -> {knv}; D2H {d2h_weld / 1e6:.3f} MB -> {d2h_kept / 1e6:.3f} MB; "
          f"scratch {cc.nbytes / 1e6:.2f} MB")
    print(f"  label (init + hook + flatten + count) {fmt(tl)}, filter count (select + flags + scans + ranks) {fmt(tf)}, "
          f"emit {fmt(te)}")
    all_ids = [0] + ids
    fus.set_mesh_weld(True)
    fus.set_mesh_filter()
    ww = wall(lambda: fus.meshes(all_ids))
    fus.set_mesh_filter(min_triangles, largest_objects=True)
    wf = wall(lambda: fus.meshes(all_ids))
    last = fus.last_mesh_filter()
    print(f"  Fusion.meshes() end to end: welded {fmt(ww)}, welded + filtered {fmt(wf)}; last_mesh_filter(): "
          f"{sum(s['components'] for s in last.values())} components, "
          f"{sum(s['kept_components'] for s in last.values())} kept, "
          f"{sum(s['triangles'] - s['kept_triangles'] for s in last.values())} triangles removed")
    fus.close()
    synth.close()
