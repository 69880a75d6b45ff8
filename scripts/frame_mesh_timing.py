"""Cost of the per-frame mesh export (setup_output(exp_frame_meshes=True)) on the configs[1] scene (512^3 + 4 x 128^3)
and the 64-object configs[3] scene (512^3 + 64 x 128^3):
  - device time per launch of the table-wide count + scan and emit (HIP events) over the live table,
  - host wall time of a loop of Fusion.mesh(id) against one Fusion.meshes() over the same models,
  - host wall time per frame with the export on and off, and the bytes the export keeps per frame.
python scripts/frame_mesh_timing.py [frames]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 10
W, H = 640, 480


def scene(nobj, export):
    prm = pipeline.make_params(W, H, 512, 0.01, 128)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), nobj, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(nobj)]
    fus.setup_output(export, False)
    inputs = []
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        rm = f % prm.mask_frames == 0
        masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if rm else {}
        inputs.append((DeviceArray.from_numpy(depth), R, t, masks, rm,
                       {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}))
    walls = []
    for d, R, t, masks, rm, poses in inputs:
        t0 = time.perf_counter()
        fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, rm)
        fus.synchronize()
        walls.append(time.perf_counter() - t0)
    return synth, fus, ids, walls


def timed(fn, reps=10):
    fn()
    synchronize()
    a, b = Event(), Event()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) / reps


for name, nobj in (("configs[1] 512^3 + 4 x 128^3", 4), ("configs[3] 512^3 + 64 x 128^3", 64)):
    wall = {}
    for export in (False, True):
        synth, fus, ids, walls = scene(nobj, export)
        wall[export] = 1e3 * float(np.median(walls[2:]))
        if export:
            # device time of the table-wide launches over copies of the live volumes
            vols = [dict(tsdf=DeviceArray.from_numpy(fus.volume("tsdf", 0)),
                         weights=DeviceArray.from_numpy(fus.volume("weights", 0)), voxel_size=0.01)]
            vox = float(np.float32(synth.sphere(0, 0)[2]) / np.float32(128))
            for i in ids:
                vols.append(dict(tsdf=DeviceArray.from_numpy(fus.volume("tsdf", i)),
                                 weights=DeviceArray.from_numpy(fus.volume("weights", i)),
                                 fg_mask=DeviceArray.from_numpy(fus.volume("fgmask", i)), voxel_size=vox))
            meshes = ops.extract_meshes(vols)
            n = len(vols)
            L = ops._L
            table, res = ops.mesh_table(vols)
            scratch = DeviceArray.zeros((int(L.emf_hip_meshScratchBytesBatched(res, n)) // 4 + 2,), np.uint32)
            counts = DeviceArray.zeros((n, 2), np.uint32)
            nv = sum(len(m[0]) for m in meshes)
            nt = sum(len(m[2]) for m in meshes)
            verts = DeviceArray.zeros((max(nv, 1), 3))
            norms = DeviceArray.zeros((max(nv, 1), 3))
            tris = DeviceArray.zeros((max(nt, 1), 4), np.int32)

            def count():
                ops.check("meshCountBatched", L.emf_hip_meshCountBatched(ops._ptr(table), res, n, ops._ptr(scratch),
                                                                         ops._ptr(counts), None, None))

            def emit():
                ops.check("meshEmitBatched", L.emf_hip_meshEmitBatched(ops._ptr(table), res, n, ops._ptr(scratch),
                                                                       ops._ptr(verts), ops._ptr(norms), ops._ptr(tris),
                                                                       None))
            tc, te = timed(count), timed(emit)
            kept = nv * 24 + nt * 16
            print(f"{name}: {n} models, {nv} vertices, {nt} triangles; count+scan {tc:.3f} ms, emit {te:.3f} ms; "
                  f"{kept / 1e6:.1f} MB kept per frame")
            all_ids = [0] + ids
            t0 = time.perf_counter()
            for i in all_ids:
                fus.mesh(i)
            loop = time.perf_counter() - t0
            t0 = time.perf_counter()
            fus.meshes(all_ids)
            one = time.perf_counter() - t0
            print(f"  loop of getMesh over {n} models {1e3 * loop:.1f} ms, one extractMeshes {1e3 * one:.1f} ms")
        fus.close()
        synth.close()
    print(f"  host wall per frame (median of frames 2..): export off {wall[False]:.2f} ms, on {wall[True]:.2f} ms")
