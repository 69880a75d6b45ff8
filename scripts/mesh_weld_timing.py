"""Cost and gain of welded meshes (Fusion.set_mesh_weld) on the configs[1] scene (512^3 + 4 x 128^3) and the 65-model
scene (512^3 + 64 x 128^3):
  - soup and welded vertex counts and the bytes each form copies device to host,
  - device time (HIP events, median and range of `reps` timed groups) of count + scan + emit -- the soup's path,
    unchanged -- against the added keys / table + rank / compact launches,
  - host wall time of Fusion.meshes(), soup against welded,
  - bytes of one frame's PLY files, soup against welded.
python scripts/mesh_weld_timing.py [frames] [reps]"""
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
    soup = ops.extract_meshes(vols)
    welded = ops.extract_meshes(vols, weld=True)
    n, L, P = len(vols), ops._L, ops._ptr
    nv, nt = sum(len(m[0]) for m in soup), sum(len(m[2]) for m in soup)
    nw = sum(len(m[0]) for m in welded)
    table, res = ops.mesh_table(vols)
    scratch = DeviceArray.zeros((int(L.emf_hip_meshScratchBytesBatched(res, n)) // 4 + 2,), np.uint32)
    counts, bases = DeviceArray.zeros((n, 2), np.uint32), DeviceArray.zeros((n + 1, 2), np.uint64)
    verts, norms = DeviceArray.zeros((max(nv, 1), 3)), DeviceArray.zeros((max(nv, 1), 3))
    tris, keys = DeviceArray.zeros((max(nt, 1), 4), np.int32), DeviceArray.zeros((max(nv, 1),), np.uint64)
    wscratch = DeviceArray.zeros((int(L.emf_hip_meshWeldScratchBytes(nv)) // 4 + 4,), np.uint32)
    wcounts, wbases = DeviceArray.zeros((n,), np.uint32), DeviceArray.zeros((n + 1,), np.uint64)
    wv, wn = DeviceArray.zeros((max(nw, 1), 3)), DeviceArray.zeros((max(nw, 1), 3))
    wt = DeviceArray.zeros((max(nt, 1), 4), np.int32)

    def count():
        ops.check("meshCountBatched", L.emf_hip_meshCountBatched(P(table), res, n, P(scratch), P(counts), P(bases), None))

    def emit():
        ops.check("meshEmitBatched", L.emf_hip_meshEmitBatched(P(table), res, n, P(scratch), P(verts), P(norms), P(tris),
                                                               None))

    def edge_keys():
        ops.check("meshEdgeKeysBatched", L.emf_hip_meshEdgeKeysBatched(P(table), res, n, P(scratch), P(keys), None))

    def weld_count():
        ops.check("meshWeldCountBatched", L.emf_hip_meshWeldCountBatched(P(keys), nv, P(bases), n, P(wscratch),
                                                                         P(wcounts), P(wbases), None))

    def weld_emit():  # (out of place here, so that repeated calls read the same soup triangles)
        ops.check("meshWeldEmitBatched", L.emf_hip_meshWeldEmitBatched(P(wscratch), nv, nt, P(bases), P(wbases), n,
                                                                       P(verts), P(norms), None, P(tris), P(wv), P(wn),
                                                                       None, P(wt), None))
    tc, te, tk, twc, twe = timed(count), timed(emit), timed(edge_keys), timed(weld_count), timed(weld_emit)
    d2h_soup, d2h_weld = nv * 24 + nt * 16, nw * 24 + nt * 16
    print(f"{name}: {n} models, {nt} triangles, {nv} soup vertices -> {nw} welded ({nv / max(nw, 1):.2f}x); "
          f"D2H {d2h_soup / 1e6:.2f} MB -> {d2h_weld / 1e6:.2f} MB; weld scratch {wscratch.nbytes / 1e6:.2f} MB")
    print(f"  soup path:  count+scan {fmt(tc)}, emit {fmt(te)}")
    print(f"  added:      keys {fmt(tk)}, table+rank {fmt(twc)}, compact+remap {fmt(twe)}")
    all_ids = [0] + ids
    fus.set_mesh_weld(False)
    ws = wall(lambda: fus.meshes(all_ids))
    fus.set_mesh_weld(True)
    ww = wall(lambda: fus.meshes(all_ids))
    print(f"  Fusion.meshes() end to end: soup {fmt(ws)}, welded {fmt(ww)}")
    sizes = {}
    for on in (False, True):
        fus.set_mesh_weld(on)
        with tempfile.TemporaryDirectory() as tmp:
            fus.write_results(tmp, volumes=False)
            sizes[on] = sum(p.stat().st_size for p in Path(tmp).glob("mesh_*.ply"))
    print(f"  one frame's PLY files: soup {sizes[False] / 1e6:.2f} MB, welded {sizes[True] / 1e6:.2f} MB")
    fus.close()
    synth.close()
