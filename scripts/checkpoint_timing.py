"""Cost of a session checkpoint (Fusion.save_checkpoint / load_checkpoint) on the configs[1] scene (512^3 + 4 x 128^3)
after `frames` frames (default 100), beside the only way the same buffers could be fetched before: Fusion.volume() of
each, written with write_volume.
  - save: the stage times the call reports (classify + rank and gather on the device, copies and file writes on the
    host), chunks and bytes per class, file size against raw size;
  - the classify pass alone (emf_hip_packClassify over the background's tsdf, HIP events, median and range of `reps`
    groups) as bytes per second, beside this box's streaming-copy rate (emf_hip_streamCopy, the probe of bench.py);
  - load: wall time of load_checkpoint into a fresh instance, and that the restored volumes are the saved bytes;
  - the raw dump: wall time and bytes.
python scripts/checkpoint_timing.py [frames] [reps]"""
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import _lib, ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, H, NOBJ = 640, 480, 4

prm = pipeline.make_params(W, H, 512, 0.01, 128)
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


def timed(fn, inner=3):
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


out = {"frames": frames, "reps": reps, "device": ops.device_info()[0]}
with tempfile.TemporaryDirectory() as tmp:
    tmp = Path(tmp)
    saves = []
    for _ in range(reps):
        saves.append(fus.save_checkpoint(tmp / "session.ckpt"))
    st = sorted(saves, key=lambda s: s["ms"]["total"])[len(saves) // 2]
    out["save"] = st
    raw, size = st["raw_bytes"], st["file_bytes"]
    print(f"save: {raw / 2**20:.1f} MiB of volumes in {st['records']} records -> file of {size / 2**20:.1f} MiB "
          f"({100.0 * size / raw:.1f} %)")
    print(f"  chunks: zero {st['chunks']['zero']}, uniform {st['chunks']['uniform']}, literal {st['chunks']['literal']}")
    print("  median call: " + ", ".join(f"{k} {v:.2f} ms" for k, v in st["ms"].items())
          + f"  (total over {reps} calls: {min(s['ms']['total'] for s in saves):.1f} .. {max(s['ms']['total'] for s in saves):.1f} ms)")

    # the classify pass alone, and the box's own streaming copy
    L = _lib.load()
    n = 512 ** 3
    src = DeviceArray.from_numpy(fus.volume("tsdf", 0))
    nch = (src.nbytes + 1023) // 1024
    cls, words = DeviceArray((nch,), np.uint8), DeviceArray((nch,), np.uint32)
    t_cls = timed(lambda: _lib.check("emf_hip_packClassify", L.emf_hip_packClassify(src.ptr, src.nbytes, cls.ptr, words.ptr, None)))
    dst = DeviceArray((n,), np.float32)
    t_cpy = timed(lambda: ops.stream_copy(dst, src))
    out["classify_ms"], out["copy_ms"] = t_cls, t_cpy
    out["classify_GBps"] = src.nbytes / t_cls[0] / 1e6
    out["copy_read_GBps"] = src.nbytes / t_cpy[0] / 1e6
    print(f"classify, 512 MiB background tsdf: {fmt(t_cls)} = {out['classify_GBps']:.0f} GB/s read")
    print(f"stream copy of the same buffer:     {fmt(t_cpy)} = {out['copy_read_GBps']:.0f} GB/s read (+ as much written)")
    del src, dst, cls, words

    # the raw dump: every buffer fetched with Fusion.volume() and written with write_volume
    def dump():
        total = 0
        for i in [0] + ids:
            for which in ("tsdf", "weights") + (("fgbg",) if i else ()):
                v = fus.volume(which, i)
                total += v.nbytes
                flat = v.reshape(v.shape[0], v.shape[1], -1)  # (counts: two floats per voxel, written as a wider row)
                pipeline.write_volume(tmp / f"{which}_{i}.bin", flat, 0.01)
        return total
    walls = []
    for _ in range(max(reps // 2, 2)):
        t0 = time.perf_counter()
        dumped = dump()
        walls.append(1e3 * (time.perf_counter() - t0))
    out["raw_dump_ms"], out["raw_dump_bytes"] = float(np.median(walls)), dumped
    print(f"raw dump (volume() + write_volume): {np.median(walls):.0f} ms ({min(walls):.0f} .. {max(walls):.0f}) for "
          f"{dumped / 2**20:.1f} MiB; save_checkpoint: {st['ms']['total']:.0f} ms for a file of {size / 2**20:.1f} MiB")

    # load into a fresh instance
    before = {(i, w): fus.volume(w, i) for i in [0] + ids for w in ("tsdf", "weights")}
    twin = pipeline.Fusion(prm, None)
    loads = []
    for _ in range(max(reps // 2, 2)):
        t0 = time.perf_counter()
        twin.load_checkpoint(tmp / "session.ckpt")
        loads.append(1e3 * (time.perf_counter() - t0))
    assert twin.frame_index() == frames and twin.object_ids() == ids
    for (i, w), v in before.items():
        assert np.array_equal(twin.volume(w, i).view(np.uint32), v.view(np.uint32)), (i, w)
    out["load_ms"] = (float(np.median(loads)), min(loads), max(loads))
    print(f"load into a fresh instance: {np.median(loads):.0f} ms ({min(loads):.0f} .. {max(loads):.0f}); volumes equal the saved ones")
    twin.close()
print("JSON " + json.dumps(out))
fus.close()
synth.close()
