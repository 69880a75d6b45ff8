"""Cost of the world extent of the scene queries (Fusion.set_query_extent("world")) on the configs[1]
scene (512^3 + 4 x 128^3) after `frames` frames, store on:
  - device time (HIP events, median and range of `reps` timed groups of `inner` calls) of emf_hip_occupancyTiles against
    emf_hip_occupancyClasses on the never-rolled 512^3 background: the observed tiles only, and all tiles, each listed in
    place (class 3) over the session's own volumes;
  - the same over world_extent() after one roll by 64 voxels along x: the volume's observed tiles in place plus the slab
    that left, restated here from the volumes before the roll as the store keeps it (all-zero tiles dropped, one
    repeated word, literals in an arena);
  - host wall time of Fusion.distance_field / frontiers / plan with box="world" against their background forms, which
    adds the tile listing (an unseen-tile pass, the store's literals to the device) and the copies to the host.
The comparison is recorded, not asserted.
python scripts/world_queries_timing.py [frames] [reps] [inner]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, DeviceView, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H, BG, VOX, OBJ, NOBJ = 640, 480, 512, 0.01, 128, 4
TILE = (32, 8, 8)
ROLL = 64


def scene():
    prm = pipeline.make_params(W, H, BG, VOX, OBJ)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_background_store(True)
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


def view(fus, which, obj_id, dtype=np.float32):
    """The session's own device array, not a copy."""
    ptr, res = C.c_void_p(), (C.c_int32 * 3)()
    pipeline._check("emf_fusion_get_volume",
                    pipeline.load().emf_fusion_get_volume(fus._h, pipeline.VOL[which], obj_id, C.byref(ptr), res))
    return DeviceView(ptr.value, (res[2], res[1], res[0]), dtype)


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


def by_tile(a):
    """(nz, ny, nx) -> (tz, ty, tx, 2048) u32: every tile's words in tile order."""
    nz, ny, nx = a.shape
    w = np.ascontiguousarray(a).view(np.uint32).reshape(nz // 8, 8, ny // 8, 8, nx // 32, 32)
    return np.ascontiguousarray(w.transpose(0, 2, 4, 1, 3, 5)).reshape(nz // 8, ny // 8, nx // 32, 2048)


def in_place(seen, first):
    """Table rows of the volume's tiles where `seen` (tz, ty, tx) holds, class 3, at lattice tile `first` + (x, y, z)."""
    z, y, x = np.nonzero(seen)
    at = ((z * 8 * BG + y * 8) * BG + x * 32).astype(np.uint64)
    n = len(z)
    coords = np.stack([x + first[0], y + first[1], z + first[2]], 1)
    return coords, np.tile(np.array([3, 3, 0], np.uint8), (n, 1)), np.zeros((n, 4), np.uint32), np.stack([at, at, 0 * at], 1)


def stored_slab(t, w, first):
    """Table rows and arena of a slab that left, as the store keeps it: per array all zero / one word / a literal."""
    tw, ww = by_tile(t), by_tile(w)
    coords, classes, words, at, arena = [], [], [], [], []
    for z in range(tw.shape[0]):
        for y in range(tw.shape[1]):
            for x in range(tw.shape[2]):
                k, wd, a = [0, 0, 0], [0, 0, 0, 0], [0, 0, 0]
                for i, arr in enumerate((tw[z, y, x], ww[z, y, x])):
                    if (arr == arr[0]).all():
                        k[i], wd[i] = (1 if arr[0] else 0), int(arr[0])
                    else:
                        k[i], a[i] = 2, len(arena)
                        arena.append(arr)
                if k[0] == 0 and k[1] == 0:
                    continue
                coords.append((x + first[0], y + first[1], z + first[2]))
                classes.append(k)
                words.append(wd)
                at.append(a)
    n = len(coords)
    return (np.array(coords, np.int64).reshape(n, 3), np.array(classes, np.uint8).reshape(n, 3),
            np.array(words, np.uint32).reshape(n, 4), np.array(at, np.uint64).reshape(n, 3),
            np.stack(arena).view(np.uint8).reshape(-1, 8192) if arena else None)


class Table:
    """A tile table on the device, sorted in (z, y, x), over the session's volumes and an optional arena."""

    def __init__(self, parts, tsdf, wts, arena=None):
        coords, classes, words, at = (np.concatenate([p[i] for p in parts]) for i in range(4))
        order = np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2]))
        self.n = len(order)
        self.host = ops.mesh_tile_table(coords[order], classes[order], words[order], at[order], np.full((self.n, 7), -1, np.int32))
        self.dev = DeviceArray.from_numpy(np.frombuffer(self.host, np.uint8).copy())
        self.src = _lib.EmfMeshTilesSource()
        self.src.tsdf, self.src.weights = tsdf.ptr, wts.ptr
        self.src.volume_elements, self.src.row_stride, self.src.plane_stride = BG ** 3, BG, BG * BG
        self.arena = None
        if arena is not None:
            self.arena = DeviceArray.from_numpy(arena)
            self.src.arena, self.src.arena_units = self.arena.ptr, len(arena)

    def classify(self, lo, size, out):
        ops.check("emf_hip_occupancyTiles",
                  _lib.load().emf_hip_occupancyTiles(self.dev.ptr, C.cast(self.host, C.c_void_p), self.n, C.byref(self.src),
                                                     ops._i3(lo), ops._i3(size), out.ptr, None))


synth, fus, ids = scene()
fus.synchronize()
tsdf, wts = view(fus, "tsdf", 0), view(fus, "weights", 0)
t0, w0 = tsdf.numpy(), wts.numpy()
seen = (by_tile(w0) != 0).any(axis=3)
res = (BG, BG, BG)
dense = DeviceArray((BG, BG, BG), np.uint8)
sparse = DeviceArray((BG, BG, BG), np.uint8)
t_dense = timed(lambda: ops.occupancy_classes(tsdf, wts, out=dense))
print(f"never rolled, whole 512^3 ({BG ** 3} voxels, {seen.size} tiles, {int(seen.sum())} observed):")
print(f"    emf_hip_occupancyClasses {fmt(t_dense)}")
for label, which in (("observed tiles only", seen), ("all tiles listed", np.ones_like(seen))):
    table = Table([in_place(which, (0, 0, 0))], tsdf, wts)
    t_tiles = timed(lambda: table.classify((0, 0, 0), res, sparse))
    same = sparse.numpy().tobytes() == dense.numpy().tobytes()
    print(f"    emf_hip_occupancyTiles, {label} ({table.n}): {fmt(t_tiles)}; bytes equal the dense pass: {same}")

w_bg = {name: wall(fn) for name, fn in (("distance_field", lambda: fus.distance_field()), ("frontiers", lambda: fus.frontiers()),
                                        ("plan", lambda: fus.plan()))}
fus.roll_background((ROLL, 0, 0))
fus.synchronize()
fus.set_query_extent("world")
lo, size = fus.world_extent()
origin = fus.background_origin()
tsdf, wts = view(fus, "tsdf", 0), view(fus, "weights", 0)
seen = (by_tile(wts.numpy()) != 0).any(axis=3)
slab = stored_slab(t0[:, :, :ROLL], w0[:, :, :ROLL], (0, 0, 0))
table = Table([in_place(seen, tuple(o // t for o, t in zip(origin, TILE))), slab[:4]], tsdf, wts, slab[4])
shape = (size[2], size[1], size[0])
world = DeviceArray(shape, np.uint8)
lattice = tuple(a + o for a, o in zip(lo, origin))
t_world = timed(lambda: table.classify(lattice, size, world))
t_dense = timed(lambda: ops.occupancy_classes(tsdf, wts, out=dense))
info = fus.background_store_info()
print(f"after a roll by {ROLL} voxels along x: world extent {lo} + {size}, {int(np.prod(shape))} voxels; the store holds "
      f"{info['tiles_held']} tiles, the table {table.n} ({len(slab[0])} restated from the slab)")
print(f"    emf_hip_occupancyTiles over the world extent {fmt(t_world)}; emf_hip_occupancyClasses over the 512^3 volume {fmt(t_dense)}")
first = fus.distance_field(box="world", metres=False, exclude=ids)
same = first["classes"].tobytes() == world.numpy().tobytes()
print(f"    the session's classes over the world extent equal the restated table's: {same} (no object stamped)")
fus.set_query_extent("world")
w_world = {name: wall(fn) for name, fn in (("distance_field", lambda: fus.distance_field(box="world")),
                                           ("frontiers", lambda: fus.frontiers(box="world")),
                                           ("plan", lambda: fus.plan(box="world")))}
fus.set_query_extent("background")
w_after = {name: wall(fn) for name, fn in (("distance_field", lambda: fus.distance_field()), ("frontiers", lambda: fus.frontiers()),
                                           ("plan", lambda: fus.plan()))}
for name in ("distance_field", "frontiers", "plan"):
    print(f"    Fusion.{name}: box=\"world\" wall {fmt(w_world[name])}; the background after the roll {fmt(w_after[name])}, "
          f"before it {fmt(w_bg[name])}")
fus.close()
synth.close()
