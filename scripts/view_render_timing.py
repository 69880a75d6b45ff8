"""The free-viewpoint view (emf_hip_renderView) at the reference window's 1024 x 768 on the bench scenes, after the usual
warm-up frames: device ms per view (HIP events around the launch, table and poses built from the fused volumes), march
samples per ray (the kernel's stats), and the extra wall ms per frame that --3d-vis costs (render() with the 3D view
set against render() without it).  One JSON line.

    python scripts/view_render_timing.py [--frames 12] [--reps 20] [--skip cfg3,cfg4]

Scenes: cfg1 = configs[1] (512^3 + 4 x 128^3, 640 x 480); cfg3 = configs[3]'s 64 objects on one GPU (512^3 + 64 x
128^3); cfg4 = one GPU's share of configs[4] (1024^3 + 2 x 256^3, 1280 x 960)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

SCENES = {"cfg1": (640, 480, 512, 0.01, 128, 4), "cfg3": (640, 480, 512, 0.01, 128, 64),
          "cfg4": (1280, 960, 1024, 0.005, 256, 2)}


def fused(w, h, bg_res, bg_vox, obj_res, nobj, frames):
    prm = pipeline.make_params(w, h, bg_res, bg_vox, obj_res)
    synth = pipeline.SyntheticStream(w, h, np.array(prm.K, np.float32), nobj, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(nobj)]

    def frame(f):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(i - 1, f)[0]) for i in ids}
        rm = f % prm.mask_frames == 0
        masks = {i: DeviceArray.from_numpy((sid == i).astype(np.uint8)) for i in ids} if rm else {}
        d = DeviceArray.from_numpy(depth)
        fus.process_frame(ops.image_view(d), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, rm)
        fus.synchronize()
    for f in range(frames):
        frame(f)
    return prm, synth, fus, ids, frame


def view_kernel_ms(prm, fus, ids, reps):
    """The launch alone on a table built from the fused volumes (downloaded and re-uploaded: the same values)."""
    R3, t3, K3, (w, h) = pipeline.default_3d_view(prm)
    keep, entries, poses = [], [], []
    one = DeviceArray.zeros((1, 1), np.float32)
    hit = DeviceArray.zeros((1, 1), np.uint8)
    viewer = (np.asarray(R3, np.float64), np.asarray(t3, np.float64))
    for mid in [0] + ids:
        tsdf = DeviceArray.from_numpy(fus.volume("tsdf", mid))
        wts = DeviceArray.from_numpy(fus.volume("weights", mid))
        fg = None if mid == 0 else DeviceArray.from_numpy(fus.volume("fgmask", mid))
        if mid == 0:
            vox, trunc = prm.bg_voxel_size, np.float32(prm.bg_rel_truncdist) * np.float32(prm.bg_voxel_size)
            Rv, tv = np.eye(3), np.array(prm.volume_pose_t, np.float64)
        else:
            info = fus.object_info(mid)
            vox, trunc = info["voxel_size"], info["truncdist"]
            Rv, tv = (np.asarray(x, np.float64) for x in fus.pose(mid))
        keep += [tsdf, wts, fg]
        entries.append(ops.make_model(tsdf, wts, one, one, one, one, hit, float(vox), float(trunc), 64.0, 0.02, 0.8,
                                      1.0, model_id=mid, fg_mask=fg, rcp_voxel=ops.voxel_reciprocal(vox)))
        poses.append((Rv.T @ viewer[0], Rv.T @ (viewer[1] - tv)))  # volume.inv() * viewer
    table = ops.upload_models(entries)
    pv = ops.upload_poses(poses)
    rgb = DeviceArray.zeros((h, w, 3), np.uint8)
    st = DeviceArray.zeros((4,), np.uint64)
    ops.render_view(table, pv, ids, w, h, K3, rgb, stats=st)  # warm
    synchronize()
    st = DeviceArray.zeros((4,), np.uint64)
    a, b = Event(), Event()
    a.record()
    for _ in range(reps):
        ops.render_view(table, pv, ids, w, h, K3, rgb)
    b.record()
    b.synchronize()
    ms = a.elapsed_ms(b) / reps
    ops.render_view(table, pv, ids, w, h, K3, rgb, stats=st)
    s = st.numpy()
    lit = int((rgb.numpy().any(axis=2)).sum())
    return dict(view_ms=round(ms, 4), samples_per_ray=round(float(s[0]) / (w * h), 1),
                samples_per_ray_per_model=round(float(s[0]) / (w * h * (1 + len(ids))), 2), hits=int(s[1]),
                lit_pixels=lit, models=1 + len(ids))


def extra_per_frame_ms(prm, fus, frame, first, frames):
    """render() per frame with the default 3D view set, against render() per frame without it."""
    out = {}
    for with_view in (False, True):
        if with_view:
            fus.set_3d_view()
        t0 = time.perf_counter()
        for f in range(first, first + frames):
            frame(f)
            fus.render()
        out[with_view] = (time.perf_counter() - t0) * 1e3 / frames
        first += frames
        fus.clear_3d_view()
    return round(out[True] - out[False], 3), round(out[False], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12, help="warm-up frames before anything is timed")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--extra-frames", type=int, default=10)
    ap.add_argument("--skip", default="", help="comma-separated scene names to skip")
    args = ap.parse_args()
    result = {"metric": "view_render_1024x768", "size": [1024, 768]}
    for name, spec in SCENES.items():
        if name in args.skip.split(","):
            continue
        prm, synth, fus, ids, frame = fused(*spec, args.frames)
        r = view_kernel_ms(prm, fus, ids, args.reps)
        r["extra_ms_per_frame_3d_vis"], r["frame_ms_with_render"] = extra_per_frame_ms(prm, fus, frame, args.frames,
                                                                                        args.extra_frames)
        result[name] = r
        fus.close()
        synth.close()
        synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
