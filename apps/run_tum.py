#!/usr/bin/env python3
"""The reference's main loop (apps/EM-Fusion.cpp:139-156) for a TUM RGB-D sequence with preprocessed
Mask R-CNN results (BASELINE.json configs[2]: `config/tum.cfg`, `--preproc-masks`), on the
MI355X-native classes:

    python apps/run_tum.py /data/rgbd_dataset_freiburg3_walking_xyz/ --masks /data/masks/ --out results/

Every frame: depth PNG (/5000) -> bilateral pre-filter -> E-step / LM-ICP tracking of camera and
objects / E-step -> raycast -> (every maskRCNNFrames-th frame: match the instance masks to the
models, spawn volumes for unmatched ones) -> weighted integration -> mask integration -> clean-up.
Writes poses-cam.txt / poses-<id>.txt (TUM format) and the volume dumps.  Needs an MI355X and a
staged dataset; neither the sequence nor the masks ship with this repository.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sequence", help="TUM sequence directory (associations.txt, depth/*.png)")
    ap.add_argument("--cofusion", nargs=2, metavar=("COLORDIR", "DEPTHDIR"),
                    help="the sequence is a Co-Fusion style dataset (reference ImageReader): "
                         "<sequence>/COLORDIR/ColorNNNN.png, <sequence>/DEPTHDIR/DepthNNNN.exr")
    ap.add_argument("--intrinsics", nargs=4, type=float, metavar=("FX", "FY", "CX", "CY"),
                    help="camera intrinsics (default: 525 px focal length scaled to the image width)")
    ap.add_argument("--ignore-person", action="store_true",
                    help="Params.ignore_person of config/tum.cfg: person objects stay out of renderings and meshes")
    ap.add_argument("--masks", help="directory with Mask%%04d.plk files of the reference's preprocessing")
    ap.add_argument("--motion-masks", dest="motion_masks", action="store_true",
                    help="no mask files: every mask frame proposes its own instance masks from the depth that lies in "
                         "front of the background model (Fusion.set_motion_masks); excludes --masks")
    ap.add_argument("--motion-band", dest="motion_band", type=float, default=None, metavar="M",
                    help="metres in front of the background a pixel must lie (default: the background's truncation distance)")
    ap.add_argument("--motion-min-pixels", dest="motion_min_pixels", type=int, default=200, metavar="N")
    ap.add_argument("--motion-max-masks", dest="motion_max_masks", type=int, default=8, metavar="N")
    ap.add_argument("--follow-camera", dest="follow_camera", action="store_true",
                    help="roll the background by whole voxels after the camera (Fusion.set_background_follow); what leaves "
                         "the cube is meshed and written as OUT/bg_retired/")
    ap.add_argument("--follow-step", dest="follow_step", default="64,64,64", metavar="X,Y,Z",
                    help="voxels a roll moves by per axis: positive multiples of 32,8,8")
    ap.add_argument("--follow-lookahead", dest="follow_lookahead", type=float, default=0.0, metavar="M",
                    help="follow the point M metres in front of the camera")
    ap.add_argument("--follow-store", dest="follow_store", action="store_true",
                    help="remember what rolls out of the background and put it back when the camera returns "
                         "(Fusion.set_background_store; needs --follow-camera)")
    ap.add_argument("--world-queries", dest="world_queries", action="store_true",
                    help="the scene queries and their result files cover the background and the stored tiles "
                         "(Fusion.set_query_extent(\"world\"); needs --follow-camera --follow-store)")
    ap.add_argument("--follow-store-mib", dest="follow_store_mib", type=int, default=1024, metavar="N",
                    help="the store's budget in MiB (default 1024: a cap, not a measurement); past it the oldest spills are dropped")
    ap.add_argument("--out", default=None, help="results directory (default emfusion_out)")
    ap.add_argument("--3d-vis", dest="vis3d", action="store_true",
                    help="the reference's 3D view: every frame also seen from a viewer 1 m behind the origin at "
                         "1024 x 768, written to OUT/mesh_vis_out/%%04d.png (needs --out)")
    ap.add_argument("--3d-vis-eye", dest="vis3d_eye", nargs=3, type=float, metavar=("X", "Y", "Z"),
                    help="place the 3D viewer at this world point instead (with --3d-vis-target)")
    ap.add_argument("--3d-vis-target", dest="vis3d_target", nargs=3, type=float, metavar=("X", "Y", "Z"),
                    default=(0.0, 0.0, 0.0), help="the world point the 3D viewer looks at (default the origin)")
    ap.add_argument("--export-frame-meshes", dest="frame_meshes", action="store_true",
                    help="the reference's per-frame mesh export: the background and every shown object meshed at the "
                         "end of every frame, written to OUT/frame_meshes/bg/%%04d.ply and OUT/frame_meshes/<id>/ "
                         "(needs --out)")
    ap.add_argument("--world-mesh", dest="world_mesh", action="store_true",
                    help="also write OUT/world.ply: one mesh of the current background and of the tiles the background "
                         "store holds, without duplicates or seams (needs --out)")
    ap.add_argument("--distance-field", dest="distance_field", action="store_true",
                    help="also write OUT/distance.bin (f32 metres to the nearest obstacle of the background, objects "
                         "stamped in at their poses) and OUT/occupancy.bin (u8: 0 free, 1 occupied, 2 unknown) (needs --out)")
    ap.add_argument("--distance-cap", dest="distance_cap", type=float, default=0.0, metavar="M",
                    help="with --distance-field: voxels farther than M metres from an obstacle get +inf (0: no cap)")
    ap.add_argument("--distance-unknown-obstacle", dest="distance_unknown", action="store_true",
                    help="with --distance-field: unobserved voxels count as obstacles too")
    ap.add_argument("--distance-nearest", dest="distance_nearest", action="store_true",
                    help="with --distance-field: also write OUT/nearest.bin (i32: the linear index of the nearest obstacle "
                         "voxel of the background, -1 where there is none)")
    ap.add_argument("--frontiers", dest="frontiers", action="store_true",
                    help="also write OUT/frontiers.txt: one line per cluster of frontier voxels (free next to unknown) of "
                         "the background, largest first")
    ap.add_argument("--frontier-min-voxels", dest="frontier_min_voxels", type=int, default=8, metavar="N",
                    help="with --frontiers: drop clusters of fewer than N voxels (default 8)")
    ap.add_argument("--frontier-clearance", dest="frontier_clearance", type=float, default=0.0, metavar="M",
                    help="with --frontiers: only frontier voxels at least M metres from the nearest occupied voxel")
    ap.add_argument("--plan", dest="plan", action="store_true",
                    help="also write OUT/plan.txt: the plan from the voxel under the last camera position to every kept "
                         "frontier cluster of the background (reachable, cost, length, path)")
    ap.add_argument("--plan-clearance", dest="plan_clearance", type=float, default=0.0, metavar="M",
                    help="with --plan: keep paths and goals at least M metres from the nearest occupied voxel")
    ap.add_argument("--plan-through-unknown", dest="plan_through_unknown", action="store_true",
                    help="with --plan: unobserved voxels are traversable too")
    ap.add_argument("--plan-shortcut", dest="plan_shortcut", type=int, default=0, metavar="W",
                    help="with --plan: plan.txt also carries one waypoints line per reachable goal, the path shortened by "
                         "lines of sight over at most W path voxels")
    ap.add_argument("--object-shapes", dest="object_shapes", action="store_true",
                    help="also write OUT/shapes.txt: one line per live object in id order, the integer moments of its "
                         "observed solid band (not its body), then its box in the world frame")
    ap.add_argument("--object-contacts", dest="object_contacts", action="store_true",
                    help="also write OUT/contacts.txt: one line per ordered pair (probe object, field object or background) "
                         "with a sampled surface voxel: the ids, the eight counts, min_s (1: at least one truncation distance "
                         "apart, not a distance) and the world contact point and normal")
    ap.add_argument("--absorb-objects", dest="absorb_objects", action="store_true",
                    help="absorb an object that the clean-up deletes because it left view into the background volume first "
                         "(the band of its signed-distance volume, not the free space around it) and also write "
                         "OUT/absorbed.txt: one line per absorbed object")
    ap.add_argument("--lift-objects", dest="lift_objects", action="store_true",
                    help="seed an object created from a mask with the band the background already holds inside its cube, "
                         "let the background release what the object then holds as foreground, and also write "
                         "OUT/lifted.txt: one line per lifted object")
    ap.add_argument("--merge-objects", dest="merge_objects", action="store_true",
                    help="merge duplicate objects at the end of every mask frame (one physical thing with two volumes: the "
                         "contact probe over all object pairs, the older object stays) and also write OUT/merged.txt: one "
                         "line per merge")
    ap.add_argument("--merge-overlap", dest="merge_overlap", type=float, default=None, metavar="F",
                    help="with --merge-objects: the share of one object's surface that has to lie on the other's (default "
                         "0.5, a policy value)")
    ap.add_argument("--merge-max-res", dest="merge_max_res", type=int, default=None, metavar="N",
                    help="with --merge-objects: the largest resolution per axis a merge grows an object to (default 256)")
    ap.add_argument("--contact-touch", dest="contact_touch", type=float, default=None, metavar="M",
                    help="with --object-contacts: the touching threshold in metres (default: one voxel of the probe)")
    ap.add_argument("--ground-map", dest="ground_map", action="store_true",
                    help="also write OUT/ground.bin and OUT/ground.txt: the 2-D traversability map of the whole background "
                         "with a floor height per cell (classes, then records of floor, top, clear, levels)")
    ap.add_argument("--ground-up", dest="ground_up", default=None, metavar="X,Y,Z",
                    help="with --ground-map: the world direction that is up (default: minus the background's y axis), or "
                         "'floor': the normal of the floor the plane search finds (the run ends with a message without one)")
    ap.add_argument("--planes", dest="planes", action="store_true",
                    help="also write OUT/planes.txt: one line per dominant plane of the whole background ordered by count: kind "
                         "count, the world normal, d, a point, the thickness in metres and the bounds in voxels")
    ap.add_argument("--planes-angle", dest="planes_angle", type=float, default=20.0, metavar="DEG",
                    help="with --planes: the alignment gate in degrees")
    ap.add_argument("--planes-min-votes", dest="planes_min_votes", type=int, default=None, metavar="N",
                    help="with --planes: the votes a direction and an offset need (default: max(50, records / 200))")
    ap.add_argument("--plane-patches", dest="plane_patches", action="store_true",
                    help="with --planes: planes.txt also lists every plane's connected patches (id, count, world point, the four "
                         "corners of its rectangle, fill) and, with --object-shapes, which patch each object rests on")
    ap.add_argument("--plane-patch-reach", dest="plane_patch_reach", type=int, default=None, metavar="R",
                    help="with --plane-patches: members within R voxels of each other (1 or 2) are one patch (default 1)")
    ap.add_argument("--plane-patch-min", dest="plane_patch_min", type=int, default=None, metavar="N",
                    help="with --plane-patches: the members a patch needs (default: max(25, min votes / 4))")
    ap.add_argument("--ground-cell", dest="ground_cell", type=float, default=None, metavar="M",
                    help="with --ground-map: the side of a ground cell in metres (default: two voxels)")
    ap.add_argument("--ground-bin", dest="ground_bin", type=float, default=None, metavar="M",
                    help="with --ground-map: the height of a bin in metres (default: two voxels)")
    ap.add_argument("--ground-band", dest="ground_band", default="-1.5,0.5", metavar="LO,HI",
                    help="with --ground-map: the heights looked at, metres relative to the camera along up")
    ap.add_argument("--ground-robot-height", dest="ground_robot_height", type=float, default=0.3, metavar="M",
                    help="with --ground-map: the free height a floor needs above it")
    ap.add_argument("--ground-max-step", dest="ground_max_step", type=float, default=0.05, metavar="M",
                    help="with --ground-map: a larger difference between neighbouring floors is an obstacle")
    ap.add_argument("--weld-meshes", dest="weld_meshes", action="store_true",
                    help="weld every mesh written (mesh_*.ply of the live models, frame_meshes/) by grid edge on the "
                         "device: one vertex per edge instead of one per cube that touches it")
    ap.add_argument("--mesh-min-triangles", dest="mesh_min_triangles", type=int, default=0, metavar="N",
                    help="remove connected components of fewer than N triangles from every mesh written, on the "
                         "device (implies --weld-meshes)")
    ap.add_argument("--mesh-largest-object", dest="mesh_largest_object", action="store_true",
                    help="keep only the largest connected component of every object mesh written (the background "
                         "keeps its pieces; implies --weld-meshes)")
    ap.add_argument("--mesh-simplify", dest="mesh_simplify", type=float, default=0.0, metavar="CELL",
                    help="simplify every mesh written (world.ply and the slabs retired from then on included) on the "
                         "device, behind the weld and the filter: the vertices of a model that share a cubic cell of CELL "
                         "metres become one vertex, collapsed triangles are dropped (implies --weld-meshes)")
    ap.add_argument("--color", action="store_true",
                    help="fuse the sequence's colour images into per-voxel colour: mesh_*.ply (and frame meshes, volume "
                         "dumps) carry colours")
    ap.add_argument("--checkpoint", metavar="PATH", help="save the session to PATH after every N-th frame (--checkpoint-every)")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="N")
    ap.add_argument("--resume", metavar="PATH",
                    help="build the instance from the parameters of the checkpoint PATH, load it and continue the "
                         "sequence at its frame index (the sizing options of this command line are not applied)")
    ap.add_argument("--frames", type=int, default=0, help="0 = all")
    ap.add_argument("--bg-res", type=int, default=512)
    ap.add_argument("--bg-voxel", type=float, default=0.01)
    ap.add_argument("--obj-res", type=int, default=128)
    ap.add_argument("--volumes", action="store_true", help="also dump the TSDF volumes")
    ap.add_argument("--visibility-thresh", type=int, default=0, help="0 = 1600 scaled by the image area")
    ap.add_argument("--mask-frames", type=int, default=30, help="Mask R-CNN every n-th frame (maskRCNNFrames)")
    args = ap.parse_args()
    if args.motion_masks and args.masks:  # (before the device is opened)
        ap.error("--motion-masks and --masks exclude each other")
    if (args.merge_overlap is not None or args.merge_max_res is not None) and not args.merge_objects:
        ap.error("--merge-overlap F and --merge-max-res N are parameters of --merge-objects")
    if args.distance_nearest and not args.distance_field:
        ap.error("--distance-nearest writes nearest.bin beside distance.bin and needs --distance-field")
    if args.plan_shortcut and not args.plan:
        ap.error("--plan-shortcut W adds the waypoints lines to plan.txt and needs --plan")
    if args.plan_shortcut < 0:
        ap.error("--plan-shortcut takes a positive window W")
    if args.contact_touch is not None and (not args.object_contacts or not args.contact_touch >= 0):
        ap.error("--contact-touch M (>= 0, metres) needs --object-contacts")
    if args.plane_patches and not args.planes:
        ap.error("--plane-patches adds the patch lines to planes.txt and needs --planes")
    if (args.plane_patch_reach is not None or args.plane_patch_min is not None) and not args.plane_patches:
        ap.error("--plane-patch-reach and --plane-patch-min need --plane-patches")
    if args.plane_patch_reach is not None and args.plane_patch_reach not in (1, 2):
        ap.error("--plane-patch-reach takes 1 or 2")
    try:
        follow_step = tuple(int(v) for v in args.follow_step.split(","))
        assert len(follow_step) == 3
    except (ValueError, AssertionError):
        ap.error("--follow-step takes three integers X,Y,Z")
    if args.follow_store and not args.follow_camera:
        ap.error("--follow-store needs --follow-camera")
    if args.world_queries and not (args.follow_camera and args.follow_store):
        ap.error("--world-queries needs --follow-camera --follow-store")
    if args.follow_store_mib != 1024 and not args.follow_store:
        ap.error("--follow-store-mib needs --follow-store")
    if args.follow_store_mib < 1:
        ap.error("--follow-store-mib takes a positive number of MiB")
    if args.vis3d and args.out is None:
        ap.error("--3d-vis writes OUT/mesh_vis_out/ and needs --out")
    if args.frame_meshes and args.out is None:
        ap.error("--export-frame-meshes writes OUT/frame_meshes/ and needs --out")
    if args.vis3d_eye and not args.vis3d:
        ap.error("--3d-vis-eye needs --3d-vis")
    if bool(args.checkpoint) != (args.checkpoint_every > 0):
        ap.error("--checkpoint PATH and --checkpoint-every N (> 0) go together")

    import torch  # noqa: F401  (one HIP runtime, see bench.py)
    from emfusion_amd import pipeline, readers
    from emfusion_amd.devmem import DeviceArray
    from emfusion_amd.ops import image_view

    if args.cofusion:
        reader = readers.ImageReader(args.sequence, *args.cofusion)
        index0 = reader.first
    else:
        reader = readers.TUMReader(args.sequence)
        index0 = 0
    n = len(reader) if args.frames <= 0 else min(args.frames, len(reader))
    first = reader.depth(index0)
    h, w = first.shape
    scale = w / 640.0
    prm = pipeline.make_params(w, h, args.bg_res, args.bg_voxel, args.obj_res,
                               visibility_thresh=args.visibility_thresh or int(round(1600 * scale * scale)),
                               boundary=int(round(20 * scale)), mask_frames=args.mask_frames)
    if args.intrinsics:
        fx, fy, cx, cy = args.intrinsics
        prm.K[:] = [fx, 0, cx, 0, fy, cy, 0, 0, 1]
    if args.resume:  # every parameter from the file; colour on / off comes back with the session
        fus = pipeline.Fusion.from_checkpoint(args.resume)
        prm = fus.params
        if (prm.width, prm.height) != (w, h):
            raise SystemExit(f"--resume: the checkpoint was saved at {prm.width} x {prm.height}, the images are {w} x {h}")
        args.color = bool(pipeline.checkpoint_info(args.resume)["color"])
    else:
        fus = pipeline.Fusion(prm, None)
        if args.color:
            fus.enable_color()
    fus.set_mesh_weld(args.weld_meshes)
    fus.set_mesh_filter(args.mesh_min_triangles, args.mesh_largest_object)
    fus.set_mesh_simplify(args.mesh_simplify)
    if args.motion_masks:  # (not stored in a checkpoint: set again on --resume)
        fus.set_motion_masks(True, band=args.motion_band, min_pixels=args.motion_min_pixels, max_masks=args.motion_max_masks)
    if args.follow_camera:
        fus.set_background_follow(True, step=follow_step, look_ahead=args.follow_lookahead)
    if args.follow_store:
        fus.set_background_store(True, max_bytes=args.follow_store_mib << 20)
    if args.world_queries:
        fus.set_query_extent("world")
    fus.set_ignore_person(args.ignore_person)
    if args.absorb_objects:
        fus.set_absorb_objects(True)
    if args.lift_objects:
        fus.set_lift_objects(True)
    if args.merge_objects:
        fus.set_merge_objects(True, min_overlap=0.5 if args.merge_overlap is None else args.merge_overlap,
                              max_res=256 if args.merge_max_res is None else args.merge_max_res)
    fus.set_preprocess(True)
    fus.set_cleanup(True)
    fus.setup_output(args.frame_meshes, args.volumes, args.world_mesh, exp_distance_field=args.distance_field,
                     distance_cap=max(args.distance_cap, 0.0), distance_unknown_is_obstacle=args.distance_unknown,
                     exp_frontiers=args.frontiers, frontier_min_voxels=max(args.frontier_min_voxels, 1),
                     frontier_clearance=max(args.frontier_clearance, 0.0), exp_plan=args.plan,
                     plan_clearance=max(args.plan_clearance, 0.0), plan_through_unknown=args.plan_through_unknown,
                     exp_distance_nearest=args.distance_nearest, exp_plan_shortcut=args.plan_shortcut,
                     exp_object_shapes=args.object_shapes, exp_object_contacts=args.object_contacts,
                     contact_touch=args.contact_touch, exp_absorbed=args.absorb_objects, exp_lifted=args.lift_objects, exp_merged=args.merge_objects, exp_ground_map=args.ground_map,
                     ground_up=None if args.ground_up is None else "floor" if args.ground_up == "floor"
                     else [float(v) for v in args.ground_up.split(",")],
                     exp_planes=args.planes, planes_angle=args.planes_angle, planes_min_votes=args.planes_min_votes,
                     exp_plane_patches=args.plane_patches, plane_patch_reach=args.plane_patch_reach or 1,
                     plane_patch_min=args.plane_patch_min,
                     ground_cell=args.ground_cell, ground_bin=args.ground_bin,
                     ground_band=[float(v) for v in args.ground_band.split(",")],
                     ground_robot_height=args.ground_robot_height, ground_max_step=args.ground_max_step)  # EMFusion::setupOutput of the reference app (apps/EM-Fusion.cpp:112)
    if args.vis3d:  # the reference's window (apps/EM-Fusion.cpp:118-131), or a viewer placed with look_at
        R3, t3, K3, size3 = pipeline.default_3d_view(prm)
        if args.vis3d_eye:
            R3, t3 = pipeline.look_at(args.vis3d_eye, args.vis3d_target)
        fus.set_3d_view(R3, t3, K3, size3)
    eye, zero = np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)
    t0 = time.time()
    for f in range(fus.frame_index(), n):
        depth = np.ascontiguousarray(reader.depth(index0 + f), np.float32)
        depth[~np.isfinite(depth)] = 0
        d = DeviceArray.from_numpy(depth)
        keep = [d]
        if args.masks and f % prm.mask_frames == 0:
            plk = Path(args.masks) / f"Mask{f:04d}.plk"  # numbered by frameCount (EMFusion.cpp:384-386)
            if plk.exists():
                _, masks, scores = readers.load_preprocessed_masks(plk)
                dev_masks = [DeviceArray.from_numpy(m) for m in masks]
                keep += dev_masks
                fus.queue_instance_masks([image_view(m) for m in dev_masks])
                fus.queue_instance_scores(scores)
        if args.color:
            rgb = reader.color_image(index0 + f) if args.cofusion else reader.color(f)
            if rgb.shape[:2] != depth.shape:
                raise SystemExit(f"frame {f}: the colour image is {rgb.shape[1]} x {rgb.shape[0]}, the depth image {w} x {h}")
            c = DeviceArray.from_numpy(rgb)
            keep.append(c)
            fus.set_color_image(image_view(c))
        if f >= 1:
            fus.set_tracking(camera=True, objects=True)  # frame 0 defines the world frame
        fus.process_frame(image_view(d), eye, zero, {}, {}, args.motion_masks and f % prm.mask_frames == 0)
        fus.synchronize()
        if args.vis3d:
            fus.render()  # apps/EM-Fusion.cpp:156: the rendering and, logged, the 3D view
        if f % 50 == 0:
            r = fus.track_result(0) if f else None
            print(f"frame {f}/{n}: objects {sorted(fus.visible_objects())}"
                  + (f", camera LM steps {r['iterations']} ({r['accepted']} accepted)" if r else ""),
                  flush=True)
        if args.checkpoint and (f + 1) % args.checkpoint_every == 0:
            st = fus.save_checkpoint(args.checkpoint)
            print(f"checkpoint after frame {f}: {st['raw_bytes'] / 2**20:.1f} MiB of volumes in a file of "
                  f"{st['file_bytes'] / 2**20:.1f} MiB, {st['ms']['total']:.1f} ms", flush=True)
    out = Path(args.out or "emfusion_out")
    out.mkdir(parents=True, exist_ok=True)
    fus.write_results(out, volumes=args.volumes)
    print(f"{n} frames in {time.time() - t0:.1f} s (incl. PNG decoding on the host); results in {out}/")
    fus.close()


if __name__ == "__main__":
    main()
