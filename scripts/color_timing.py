"""What per-voxel colour costs a frame: the configs[1] scene (background 512^3 + 4 x 128^3, 640 x 480, full schedule, poses
and masks supplied as in bench.py) with a seeded RGB stream, timed with colour OFF and ON alternating in one process:
two instances fed the same frames, blocks of frames bracketed by device events, after warm-up, more than a second of
device work per arm.  Reports ms per frame of both arms, the run-to-run spread of the OFF arm over its blocks (the
resolution of the comparison), the colour launch alone (device events around emf_hip_integrateColorBatched on the ON
instance's own table state), the voxels it coloured and the bytes that implies.  One JSON line.

    python scripts/color_timing.py [--warmup 30] [--block 170] [--rounds 10] [--reps 50]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: F401,E402  (one HIP runtime, see bench.py)

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, DeviceView, Event, synchronize  # noqa: E402

W, H, BG_RES, BG_VOX, OBJ_RES, NOBJ = 640, 480, 512, 0.01, 128, 4
NSCENE = 60  # pre-rendered frames, walked back and forth (poses are supplied, so the turn-round is an ordinary frame)


def scene_order(count):
    fwd = list(range(NSCENE)) + list(range(NSCENE - 2, 0, -1))
    return [fwd[i % len(fwd)] for i in range(count)]


class Arm:
    def __init__(self, prm, synth, color):
        self.fus = pipeline.Fusion(prm, None)
        if color:
            self.fus.enable_color()
        self.color = color
        self.ids = [self.fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
        self.count = 0  # frames processed: frame index of the schedule (mask frames every prm.mask_frames)

    def frame(self, prm, scene, s):
        depth, masks, rgb, R, t, centers = scene[s]
        poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), centers[i - 1]) for i in self.ids}
        rm = self.count % prm.mask_frames == 0
        if self.color:
            self.fus.set_color_image(ops.image_view(rgb))
        self.fus.process_frame(ops.image_view(depth), R, t, poses,
                               {i: ops.image_view(masks[i - 1]) for i in self.ids} if rm else {}, rm)
        self.count += 1


def kernel_alone(prm, arm, scene, reps):
    """emf_hip_integrateColorBatched by itself on the ON instance's volumes, association maps and poses."""
    fus, lib = arm.fus, pipeline.load()
    depth, _, rgb, R, t, centers = scene[scene_order(arm.count)[-1]]
    cam_R, cam_t = (np.asarray(x, np.float64) for x in fus.pose(0))
    entries, colors, poses, res = [], [], [], []
    one = DeviceArray.zeros((1, 1), np.float32)
    hit = DeviceArray.zeros((1, 1), np.uint8)

    def vol(which, mid, dtype, last=()):
        ptr, r = C.c_void_p(), (C.c_int32 * 3)()
        pipeline._check("emf_fusion_get_volume", lib.emf_fusion_get_volume(fus._h, pipeline.VOL[which], mid, C.byref(ptr), r))
        return DeviceView(ptr.value, (r[2], r[1], r[0]) + last, dtype)
    for mid in [0] + arm.ids:
        v = fus.image_view("bg_assoc" if mid == 0 else "obj_assoc", mid)
        assoc = DeviceView(v.data, (v.height, v.width), np.float32)
        if mid == 0:
            vox, trunc = prm.bg_voxel_size, np.float32(prm.bg_rel_truncdist) * np.float32(prm.bg_voxel_size)
            Rv, tv = np.eye(3), np.array(prm.volume_pose_t, np.float64)
        else:
            info = fus.object_info(mid)
            vox, trunc = info["voxel_size"], info["truncdist"]
            Rv, tv = (np.asarray(x, np.float64) for x in fus.pose(mid))
        tsdf = vol("tsdf", mid, np.float32)
        entries.append(ops.make_model(tsdf, vol("weights", mid, np.float32), assoc, one, one, one, hit, float(vox),
                                      float(trunc), prm.max_tsdf_weight, 0.02, 0.8, 1.0, model_id=mid))
        colors.append(DeviceArray.zeros(tsdf.shape + (4,), np.uint16))  # a scratch copy: the instance's own stays as it is
        poses.append((cam_R.T @ Rv, cam_R.T @ (tv - cam_t)))  # camera.inv() * volume
        res.append(tsdf.shape[::-1])
    table = ops.upload_models(entries)
    il = DeviceArray.zeros((H, W), np.float32)
    K = np.array(prm.K, np.float32)
    ops.compute_inv_lambda(K, il)
    stats = DeviceArray.zeros((1,), np.uint64)
    visible = DeviceArray.from_numpy(np.ones(len(entries), np.int32))
    ptrs = DeviceArray.from_numpy(np.array([c.ptr for c in colors], np.uint64))
    resc = (C.c_int32 * (3 * len(res)))(*[int(x) for r in res for x in r])

    def launch(st):
        ops.check("emf_hip_integrateColorBatched",
                  ops._L.emf_hip_integrateColorBatched(ops._ptr(table), ops._ptr(ptrs), ops._poses(poses), resc, len(res),
                                                       ops._ptr(visible), C.byref(ops.image_view(depth)),
                                                       C.byref(ops.image_view(il)), C.byref(ops.image_view(rgb)),
                                                       ops._f(K, 9), ops._ptr(st), None))
    launch(stats)  # warm; counts one launch's coloured voxels
    synchronize()
    coloured = int(stats.numpy()[0])
    a, b = Event(), Event()
    a.record()
    for _ in range(reps):
        launch(None)
    b.record()
    b.synchronize()
    ms = a.elapsed_ms(b) / reps
    voxels = sum(int(np.prod(r)) for r in res)
    # per coloured voxel: 8 B colour read + 8 B written; gathers: depth 4, 1 / lambda 4, association 4, rgb 3
    return dict(kernel_ms=round(ms, 4), coloured_voxels=coloured, table_voxels=voxels,
                coloured_fraction=round(coloured / voxels, 5), colour_bytes=16 * coloured, gather_bytes=15 * coloured,
                implied_GBs=round((31 * coloured) / (ms * 1e-3) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--block", type=int, default=170, help="frames per timed block")
    ap.add_argument("--rounds", type=int, default=10, help="timed blocks per arm, the arms alternating")
    ap.add_argument("--reps", type=int, default=50, help="launches of the colour kernel alone")
    args = ap.parse_args()
    prm = pipeline.make_params(W, H, BG_RES, BG_VOX, OBJ_RES)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), NOBJ, seed=0xE3F5)
    rng = np.random.default_rng(0xC0105)
    scene = []
    for f in range(NSCENE):  # everything resident in HBM before anything is timed
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        scene.append((DeviceArray.from_numpy(depth),
                      [DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k in range(NOBJ)],
                      DeviceArray.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)), R, t,
                      [synth.sphere(k, f)[0] for k in range(NOBJ)]))
    arms = {"off": Arm(prm, synth, False), "on": Arm(prm, synth, True)}
    order = scene_order(args.warmup + args.block * args.rounds)
    for arm in arms.values():
        for s in order[:args.warmup]:
            arm.frame(prm, scene, s)
        arm.fus.synchronize()
    per_block = {"off": [], "on": []}
    for r in range(args.rounds):
        block = order[args.warmup + r * args.block: args.warmup + (r + 1) * args.block]
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            arm = arms[name]
            a, b = Event(), Event()
            synchronize()
            a.record()
            for s in block:
                arm.frame(prm, scene, s)
            arm.fus.synchronize()
            b.record()
            b.synchronize()
            per_block[name].append(a.elapsed_ms(b) / len(block))
    out = {"metric": "color_timing", "scene": "configs[1]: 512^3 + 4 x 128^3, 640 x 480", "frames_per_arm": args.block * args.rounds}
    for name, v in per_block.items():
        out[name] = dict(ms_per_frame=round(statistics.median(v), 4), mean=round(statistics.fmean(v), 4),
                         min=round(min(v), 4), max=round(max(v), 4), seconds=round(sum(v) * args.block / 1e3, 3))
    off = per_block["off"]
    out["off_spread_rel"] = round((max(off) - min(off)) / statistics.median(off), 4)
    out["on_minus_off_ms"] = round(out["on"]["ms_per_frame"] - out["off"]["ms_per_frame"], 4)
    out["off_fps"] = round(1e3 / out["off"]["ms_per_frame"], 1)
    out["coloured_voxels_per_frame_in_run"] = round(arms["on"].fus.colored_voxels() / arms["on"].count, 1)
    out["kernel"] = kernel_alone(prm, arms["on"], scene, args.reps)
    print(json.dumps(out))
    for arm in arms.values():
        arm.fus.close()
    synth.close()


if __name__ == "__main__":
    main()
