"""Cost and gain of simplified meshes (Fusion.set_mesh_simplify) on the configs[1] scene (512^3 + 4 x 128^3) and the
65-model scene (512^3 + 64 x 128^3), at cells of 2 and 4 background voxels:
  - vertices and triangles in and out, the clusters met, and the bytes the welded and the simplified form copy device to
    host and write as PLY,
  - device time (HIP events, median and range of `reps` timed groups) of the two entries on the welded arrays:
    count (two clears + insert + accumulate + mark + flags + scans + ranks + bases), emit,
  - host wall time of Fusion.meshes(), welded (the path of set_mesh_weld alone, unchanged) against welded + simplified.
The split of the count entry into its launches is read from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/mesh_simplify_timing.py): the kernels are k_sp_*.
python scripts/mesh_simplify_timing.py [frames] [reps]"""
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 6
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H = 640, 480
VOX = 0.01


def scene(nobj):
    prm = pipeline.make_params(W, H, 512, VOX, 128)
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


def ply_bytes(meshes):
    total = 0
    with tempfile.TemporaryDirectory() as d:
        for i, m in meshes.items():
            p = Path(d) / f"{i}.ply"
            pipeline.write_mesh(str(p), *m[:3])
            total += p.stat().st_size
    return total


for name, nobj in (("configs[1] 512^3 + 4 x 128^3", 4), ("65 models 512^3 + 64 x 128^3", 64)):
    synth, fus, ids = scene(nobj)
    all_ids = [0] + ids
    fus.set_mesh_weld(True)
    welded = fus.meshes(all_ids)
    n = len(all_ids)
    vb = np.concatenate([[0], np.cumsum([len(welded[i][0]) for i in all_ids])]).astype(np.uint64)
    tb = np.concatenate([[0], np.cumsum([len(welded[i][2]) for i in all_ids])]).astype(np.uint64)
    nv, nt = int(vb[n]), int(tb[n])
    # the welded arrays on the device, as extractWelded leaves them
    v = DeviceArray.from_numpy(np.concatenate([welded[i][0] for i in all_ids]))
    nr = DeviceArray.from_numpy(np.concatenate([welded[i][1] for i in all_ids]))
    t = DeviceArray.from_numpy(np.concatenate([welded[i][2] for i in all_ids]))
    _, sb, wb = ops._table_bases(tb, vb)
    L, P = ops._L, ops._ptr
    scratch = DeviceArray.zeros((int(L.emf_hip_meshSimplifyScratchBytes(nv, nt)) // 4,), np.uint32)
    kcounts, kbases = DeviceArray.zeros((n, 2), np.uint32), DeviceArray.zeros((n + 1, 2), np.uint64)
    clusters = DeviceArray.zeros((n,), np.uint32)
    hp = lambda a: a.ctypes.data  # noqa: E731
    ww = wall(lambda: fus.meshes(all_ids))
    d2h_weld, ply_weld = nv * 24 + nt * 16, ply_bytes(welded)
    print(f"{name}: {n} models, {nv} welded vertices, {nt} triangles; D2H {d2h_weld / 1e6:.3f} MB, PLY "
          f"{ply_weld / 1e6:.3f} MB; Fusion.meshes() welded {fmt(ww)}; scratch {scratch.nbytes / 1e6:.2f} MB")
    for voxels in (2, 4):
        cells = np.full((n,), voxels * VOX, np.float32)

        def count():
            ops.check("meshSimplifyCount",
                      L.emf_hip_meshSimplifyCount(P(v), P(nr), None, P(t), nv, nt, P(sb), P(wb), n, hp(cells), None,
                                                  P(scratch), P(kcounts), P(kbases), P(clusters), None))

        count()
        ops.check("meshSimplifyStatus", L.emf_hip_meshSimplifyStatus(P(scratch), nv, nt, None))
        knv, knt = (int(x) for x in kbases.numpy()[n])
        kv, kn = DeviceArray.zeros((max(knv, 1), 3)), DeviceArray.zeros((max(knv, 1), 3))
        kt = DeviceArray.zeros((max(knt, 1), 4), np.int32)

        def emit():
            ops.check("meshSimplifyEmit",
                      L.emf_hip_meshSimplifyEmit(P(scratch), nv, nt, P(sb), P(wb), n, P(v), P(nr), None, P(t), P(kv), P(kn),
                                                 None, P(kt), None))

        tc, te = timed(count), timed(emit)
        fus.set_mesh_simplify(float(cells[0]))
        ws = wall(lambda: fus.meshes(all_ids))
        simple = fus.meshes(all_ids)
        last = fus.last_mesh_simplify()
        fus.set_mesh_simplify(0.0)
        assert sum(s["vertices_out"] for s in last.values()) == knv and sum(s["triangles_out"] for s in last.values()) == knt
        print(f"  cell {voxels} voxels: vertices {nv} -> {knv}, triangles {nt} -> {knt}, clusters "
              f"{int(clusters.numpy().sum())}; D2H {d2h_weld / 1e6:.3f} -> {(knv * 24 + knt * 16) / 1e6:.3f} MB, PLY "
              f"{ply_weld / 1e6:.3f} -> {ply_bytes(simple) / 1e6:.3f} MB")
        print(f"    count (clears + insert + accumulate + mark + flags + scans + ranks) {fmt(tc)}, emit {fmt(te)}; "
              f"Fusion.meshes() welded + simplified {fmt(ws)} against welded {fmt(ww)}")
    fus.close()
    synth.close()
