"""Cost of the world mesh (Fusion.world_mesh, emf_hip_meshTiles*) on the configs[1] scene (512^3 +
4 x 128^3, 640 x 480) after `frames` frames.  No figure is a pass criterion.  Device time from HIP events, median and
range of `reps` groups of `inner` launches; the two meshers alternate group by group in one process.
  (a) never rolled: emf_hip_meshTilesCount (+ scan) and emf_hip_meshTilesEmit over the background's observed tiles, every
      one in place (class 3), against emf_hip_meshCount and emf_hip_meshEmit of the same dense background
  (b) after one 64-voxel roll along x with the store on: Fusion.world_mesh() as a whole (wall time: drain, the
      unseen-tile map, TileStore::gather() of the stored tiles through the pinned slab, table, count, emit, download)
      against Fusion.mesh(0) of the rolled background alone
python scripts/world_mesh_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, NOBJ, N = 640, 480, 4, 512
EYE = np.eye(3, dtype=np.float32).reshape(-1)
prm = pipeline.make_params(W, H, N, 0.01, 128)
L = _lib.load()


def session(store):
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    if store:
        fus.set_background_store(True)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
    keep = []
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        poses = {i: (EYE, synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
        masks = {i: DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if f == 0 else {}
        d = DeviceArray.from_numpy(depth)
        keep[:] = [d, masks]
        fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
        fus.synchronize()
    return fus, synth


def fmt(v):
    return f"{np.median(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def group(fn):
    a, b = Event(), Event()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) / inner


# ---- (a) the two meshers on the never-rolled background
fus, synth = session(True)
t_host, w_host = fus.volume("tsdf", 0), fus.volume("weights", 0)
tsdf, wts = DeviceArray.from_numpy(t_host), DeviceArray.from_numpy(w_host)
nt = (N // 32, N // 8, N // 8)
seen = ((w_host != 0) | ~(np.abs(t_host) <= np.float32(3.0e38))).reshape(nt[2], 8, nt[1], 8, nt[0], 32).any(axis=(1, 3, 5))
tz, ty, tx = np.nonzero(seen)                                          # (z, y, x) order
n = len(tz)
at = ((tz * 8 * N + ty * 8) * N + tx * 32).astype(np.uint64)
table = ops.mesh_tile_table(np.stack([tx, ty, tz], 1), np.tile(np.array([3, 3, 0], np.uint8), (n, 1)),
                            np.zeros((n, 4), np.uint32), np.stack([at, at, np.zeros_like(at)], 1))
d_table = DeviceArray.from_numpy(np.frombuffer(table, np.uint8).copy())
src = _lib.EmfMeshTilesSource(tsdf=tsdf.ptr, weights=wts.ptr, volume_elements=N ** 3, row_stride=N, plane_stride=N * N)
res = (C.c_int32 * 3)(N, N, N)
half = (C.c_float * 3)(*[(N - 1) / 2.0] * 3)
p = lambda a: C.c_void_p(a.ptr)
scr_t = DeviceArray.zeros((L.emf_hip_meshTilesScratchBytes(n) // 4,), np.uint32)
scr_d = DeviceArray.zeros((max(L.emf_hip_meshScratchBytes(res) // 4, 2),), np.uint32)
cnt_t, cnt_d = DeviceArray.zeros((2,), np.uint32), DeviceArray.zeros((2,), np.uint32)


def tiles_count():
    ops.check("meshTilesCount", L.emf_hip_meshTilesCount(p(d_table), C.cast(table, C.c_void_p), n, C.byref(src), p(scr_t),
                                                         p(cnt_t), None))


def dense_count():
    ops.check("meshCount", L.emf_hip_meshCount(p(tsdf), p(wts), None, res, p(scr_d), p(cnt_d), None))


tiles_count()
dense_count()
got_t, got_d = cnt_t.numpy(), cnt_d.numpy()
print(f"background {N}^3 after {frames} frames: {n} of {nt[0] * nt[1] * nt[2]} tiles listed; "
      f"tiles {tuple(int(v) for v in got_t)}, dense {tuple(int(v) for v in got_d)} (vertices, triangles)")
assert tuple(got_t) == tuple(got_d), "the two meshers disagree on a never-rolled background"
nv, ntri = (int(v) for v in got_t)
out_t = [DeviceArray.zeros((max(nv, 1), 3), np.float32), DeviceArray.zeros((max(nv, 1), 3), np.float32),
         DeviceArray.zeros((max(ntri, 1), 4), np.int32)]
out_d = [DeviceArray.zeros(a.shape, a.dtype) for a in out_t]


def tiles_emit():
    ops.check("meshTilesEmit", L.emf_hip_meshTilesEmit(p(d_table), n, C.byref(src), half, 0.01,
                                                       p(scr_t), p(out_t[0]), p(out_t[1]), p(out_t[2]), None))


def dense_emit():
    ops.check("meshEmit", L.emf_hip_meshEmit(p(tsdf), None, p(wts), None, res, 0.01, p(scr_d), p(out_d[0]), p(out_d[1]),
                                             p(out_d[2]), None))


for fn in (tiles_emit, dense_emit):
    fn()
synchronize()
times = {k: [] for k in ("tiles count + scan", "dense count + scan", "tiles emit", "dense emit")}
for _ in range(reps):                                                  # interleaved, group by group
    times["tiles count + scan"].append(group(tiles_count))
    times["dense count + scan"].append(group(dense_count))
    times["tiles emit"].append(group(tiles_emit))
    times["dense emit"].append(group(dense_emit))
for k, v in times.items():
    print(f"(a) {k:20s} {fmt(v)}")

# ---- (b) after one 64-voxel roll with the store on: the whole call
fus.roll_background((64, 0, 0), keep_retired=False)
fus.synchronize()
info = fus.background_store_info()
wall = {"world_mesh()": [], "mesh(0)": []}
for k in range(reps + 1):
    for name, fn in (("world_mesh()", fus.world_mesh), ("mesh(0)", lambda: fus.mesh(0))):
        t0 = time.perf_counter()
        m = fn()
        if k:
            wall[name].append((time.perf_counter() - t0) * 1e3)
print(f"(b) after the roll: store holds {info['tiles_held']} tiles, {info['bytes_held'] >> 20} MiB; {fus.world_mesh_info()}")
for k, v in wall.items():
    print(f"(b) {k:20s} {fmt(v)} wall")
fus.close()
synth.close()
