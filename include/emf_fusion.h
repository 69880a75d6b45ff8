/*
 * emf_fusion.h -- C handle API over the C++ host classes (emf::EMFusion / emf::TSDF / emf::ObjTSDF,
 * emfusion_amd/csrc/core) for callers that cannot include C++ headers: the Python harness
 * (tests/, bench.py) and FFI users.  C++ callers -- such as a port of the reference's
 * apps/EM-Fusion.cpp main loop -- use the classes directly (see apps/emfusion_synth.cpp).
 *
 * The handle wraps one emf::EMFusion: one background volume + N object volumes, driven frame by
 * frame with externally supplied poses and masks (tracking and Mask R-CNN are outside this
 * build's scope).  Every function returns 0 on success, a negative EMF_E_* code or a positive
 * hipError_t / ncclResult_t; emf_fusion_last_error_string() describes the last failure on the
 * calling thread.  Nothing throws across this boundary.
 */
#ifndef EMF_FUSION_H
#define EMF_FUSION_H

#include "emf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emf_fusion emf_fusion_t;
typedef struct emf_comm emf_comm_t;
typedef struct emf_synth emf_synth_t;

/* Mirror of the fields of emf::Params / emf::TSDFParams the volumetric path reads
 * (reference include/EMFusion/core/data.h; defaults = reference defaults). */
typedef struct emf_fusion_params {
    int32_t width, height;
    float K[9];
    int32_t bg_res[3];
    float bg_voxel_size;
    float bg_rel_truncdist;
    float volume_pose_t[3]; /* background volume centre relative to the first camera */
    int32_t obj_res[3];
    float obj_rel_truncdist;
    float max_tsdf_weight, assoc_sigma, alpha, uni_prior;
    int32_t visibility_thresh, boundary, mask_frames;
    int32_t materialize_gradients; /* 0: normals from on-the-fly differences; 1: gradient volume */
    int32_t max_tracking_iter;     /* LM iterations per tracking stage (data.h:106: 100) */
} emf_fusion_params_t;

/* per-stage GPU milliseconds of the last frame (HIP events on the main stream) */
typedef struct emf_frame_timings {
    float points, estep, raycast, composite, integrate, masks, total;
} emf_frame_timings_t;

enum emf_fusion_image {
    EMF_IMG_POINTS = 0,          /* f32x3 */
    EMF_IMG_BG_ASSOC = 1,        /* f32   normalised background association weights */
    EMF_IMG_OBJ_ASSOC = 2,       /* f32   per object (obj_id) */
    EMF_IMG_ASSOC_NORM = 3,      /* f32 */
    EMF_IMG_RAYLENGTHS = 4,      /* f32   composite */
    EMF_IMG_VERTICES = 5,        /* f32x3 composite */
    EMF_IMG_NORMALS = 6,         /* f32x3 composite */
    EMF_IMG_SEGMENTATION = 7,    /* u8    composite model segmentation */
    EMF_IMG_BG_RAYLENGTHS = 8,   /* f32 */
    EMF_IMG_OBJ_RAYLENGTHS = 9   /* f32   per object (obj_id) */
};

enum emf_fusion_volume {
    EMF_VOL_TSDF = 0,     /* f32 */
    EMF_VOL_WEIGHTS = 1,  /* f32 */
    EMF_VOL_FGPROBS = 2,  /* f32, objects only */
    EMF_VOL_FGMASK = 3,   /* u8,  objects only */
    EMF_VOL_BRICKS = 4,   /* u8,  brick uniformity flags, ceil(N/4) per axis (res = brick grid) */
    EMF_VOL_COLOR = 5,    /* u16 x 4 (R, G, B, Wc in 8.8 fixed point), only after emf_fusion_set_color(on) */
    EMF_VOL_FGBG = 6      /* f32 x 2 (foreground, background) counts, objects only: what fgprobs / fgmask derive from */
};

const char* emf_fusion_last_error_string(void);

void emf_fusion_default_params(emf_fusion_params_t* p);
/* comm may be NULL (single GPU).  The handle shares ownership of comm. */
int emf_fusion_create(const emf_fusion_params_t* p, emf_comm_t* comm, emf_fusion_t** out);
/* The instance apps/emfusion_synth --configfile builds: EVERY key of one of the reference's configuration files (config/default.cfg, tum.cfg ...;
 * apps/EM-Fusion.cpp:268-371) and, optionally, a Co-Fusion calibration.txt -- including the ones emf_fusion_params_t has no
 * field for (ignore_person, FILTER_CLASSES, STATIC_OBJECTS, huberThresh, tau, eps1, eps2, nu_init, bilateral_*, volPad,
 * existenceThresh, volIOUThresh, matchIOUThresh, distanceThresh, assocThresh).  path NULL or "": the defaults of data.h.
 * params_out (may be NULL) receives the subset the struct does carry. */
int emf_fusion_create_from_config(const char* path, const char* calibration, int materialize_gradients, emf_comm_t* comm,
                                  emf_fusion_params_t* params_out, emf_fusion_t** out);
void emf_fusion_destroy(emf_fusion_t* h);
int emf_fusion_reset(emf_fusion_t* h);
/* Device buffers released by destroyed / resized volumes wait in a process-wide pool instead of going through
 * hipFree (which synchronises the device; EMF_POOL_MIB caps the pool, default 16 GiB).  This really frees them
 * -- it waits for the device -- and reports how many bytes were held (bytes_freed may be NULL). */
int emf_fusion_trim_pool(uint64_t* bytes_freed);
/* The run-time switches (environment variables) of the host classes -- the table of emfusion_amd/csrc/core/Switches.hpp
 * -- as parsed from the CURRENT environment, as JSON: {"debug_switches": bool, "switches": [{"name", "field", "kind"
 * ("product" | "demoted"), "type", "rule", "default", "read" (does this build read the variable?), "value" (what an
 * instance constructed now would use), "path", "doc"}, ...]}.  Needs no device and no handle.  A value the table refuses
 * (EMF_MARCH_ROWS other than 1, 2, 4) gives EMF_E_ARG and the constructor's message; a demoted variable that is set
 * gives the product build's one line on stderr, once per process.  EMF_E_ARG if `capacity` is too small (16 KiB is enough). */
int emf_fusion_describe_switches(char* json, size_t capacity);
/* emf::EMFusion::processFrame(const RGBD&) -- the reference's entry (EMFusion.h:66): a HOST depth image in metres
 * (width x height floats), uploaded, bilateral-filtered and run through the schedule with the frame inputs set by the
 * emf_fusion_set_* / queue_* calls; with emf_fusion_use_preproc_masks the instance masks of every mask frame come
 * from <path>/Mask%04d.plk (EMFusion::usePreprocMasks, EMFusion.h:98).  emf_fusion_get_last_masks: EMFusion::
 * getLastMasks (EMFusion.h:83) -- W x H x 3 bytes (may be NULL), *instances of the last mask frame. */
int emf_fusion_process_rgbd(emf_fusion_t* h, const float* depth_host, int32_t width, int32_t height);
/* Per-voxel colour (include/emf_hip.h "Per-voxel colour"; off by default, and with it off nothing of a frame changes).
 *   set_color          on != 0: every model gets a colour volume (EMF_VOL_COLOR), zeroed at creation and at reset,
 *                      carried through ObjTSDF::resize, freed with its model; a frame that was handed a colour image
 *                      fuses it behind its TSDF integration, weighted by the association maps of that integration.
 *                      Before the first frame and after emf_fusion_reset only (EMF_E_ARG otherwise); refused as
 *                      unsupported on the sharded path and on the per-volume path.
 *   set_color_image    the u8 x 3 DEVICE image (frame size) that goes with the NEXT frame (emf_fusion_process_frame,
 *                      emf_fusion_process_rgbd, emf_fusion_stage_integrate) and with that one only; it must stay
 *                      valid until that frame has run.  A frame without one leaves the colour volumes untouched.
 *   process_rgbd_color emf_fusion_process_rgbd with a HOST rgb image (width x height x 3 bytes): uploaded, handed to
 *                      set_color_image, then the frame.
 *   colored_voxels     voxels the colour pass has updated since the last call (waits for the device) */
int emf_fusion_set_color(emf_fusion_t* h, int on);
/* Welded meshes (include/emf_hip.h "Welded meshes"; off by default, may be switched at any time).  on != 0:
 * emf_fusion_extract_mesh / copy_mesh / copy_mesh_colors, emf_fusion_extract_meshes / copy_meshes / copy_meshes_colors,
 * emf_fusion_write_results' mesh_bg.ply and mesh_<id>.ply of the live models and the per-frame frame_meshes/ of
 * emf_fusion_setup_output deliver one vertex per grid edge (the first soup copy's position, normal and colour, bit for
 * bit) and the soup's triangles re-indexed; the counts are the welded counts.  Welded on the device before the copies
 * to the host.  An output form only: poses, the object life cycle and every image are the same bytes either way, and
 * the last mesh kept of an object deleted during the run stays the soup the life cycle took.  On the sharded path:
 * wherever emf_fusion_extract_mesh works, for this rank's models. */
int emf_fusion_set_mesh_weld(emf_fusion_t* h, int on);
/* The component filter (include/emf_hip.h "Mesh components"; off by default -- min_triangles <= 1 and
 * largest_objects == 0 --, may be switched at any time).  Exactly where emf_fusion_set_mesh_weld acts, every mesh
 * loses its connected components of fewer than min_triangles triangles and, with largest_objects != 0, every OBJECT
 * mesh all components but its largest (by triangles, a tie to the smaller label; the background keeps its pieces).
 * Labelled, filtered and compacted on the device behind the weld; only the filtered arrays travel to the host.  An
 * active filter implies the welded form whatever set_mesh_weld says; a mesh may come out empty.  An output form only,
 * as the weld: nothing else changes, and the last mesh kept of an object deleted during the run stays the soup.  Not
 * stored in a checkpoint.
 *   mesh_components       labels and component sizes of model id's welded, UNFILTERED mesh: kept in the handle,
 *                         copy_mesh_components hands them out (num_vertices int32 labels -- the smallest welded index
 *                         of the vertex's component --, num_vertices uint32 sizes in triangles; NULL: not wanted)
 *   last_mesh_filter      per model of the last emf_fusion_extract_mesh / extract_meshes (write_results and the
 *                         per-frame export run the latter) under an active filter: ids ascending and 4 uint32 per id
 *                         (components, kept components, triangles, kept triangles); count = how many there are,
 *                         at most `capacity` are written */
int emf_fusion_set_mesh_filter(emf_fusion_t* h, uint32_t min_triangles, int largest_objects);
int emf_fusion_mesh_components(emf_fusion_t* h, int id, uint32_t* num_vertices);
int emf_fusion_copy_mesh_components(emf_fusion_t* h, int32_t* labels, uint32_t* sizes);
int emf_fusion_last_mesh_filter(emf_fusion_t* h, int32_t* ids, uint32_t* stats, int capacity, int32_t* count);
/* Simplified meshes (include/emf_hip.h "Simplified meshes"; off by default -- cell_metres <= 0 --, may be switched at
 * any time).  Exactly where emf_fusion_set_mesh_weld and the filter act, and in emf_fusion_world_mesh and the slabs
 * retired after the call, the vertices of a model's welded and filtered mesh that share a cubic cell of cell_metres
 * (counted from 0 in the mesh's own frame) become one vertex: the member itself if it is alone, else the mean of
 * positions, normals and colours in integers; triangles are re-indexed, the collapsed ones dropped, and so are the
 * vertices nothing references.  Done on the device behind the filter, so fragment sizes are counted in original
 * triangles; only the simplified arrays travel to the host.  A cell > 0 implies the welded form whatever set_mesh_weld
 * says; a mesh may come out empty.  A cell so small that a vertex lies 2^15 cells or more from 0 is refused by the call
 * that meshes (EMF_E_LIMIT).  An output form only, as the weld: nothing else changes, and the last mesh kept of an
 * object deleted during the run stays the soup.  Not stored in a checkpoint.
 *   last_mesh_simplify    per model of the last emf_fusion_extract_mesh / extract_meshes (write_results and the
 *                         per-frame export run the latter) with a cell set: ids ascending and 5 uint32 per id (vertices
 *                         in, triangles in, vertices out, triangles out, clusters); count = how many there are, at most
 *                         `capacity` are written */
int emf_fusion_set_mesh_simplify(emf_fusion_t* h, float cell_metres);
int emf_fusion_last_mesh_simplify(emf_fusion_t* h, int32_t* ids, uint32_t* stats, int capacity, int32_t* count);
int emf_fusion_set_color_image(emf_fusion_t* h, const emf_image_t* rgb_dev);
int emf_fusion_process_rgbd_color(emf_fusion_t* h, const float* depth_host, const uint8_t* rgb_host, int32_t width,
                                  int32_t height);
int emf_fusion_colored_voxels(emf_fusion_t* h, uint64_t* count);
int emf_fusion_use_preproc_masks(emf_fusion_t* h, const char* path);
int emf_fusion_get_last_masks(emf_fusion_t* h, uint8_t* rgb, size_t capacity, int32_t* instances);
/* Motion masks (include/emf_hip.h "Motion masks"; off by default, may be switched at any time, and with it off no
 * launch and no output byte of a frame changes).  on != 0: a frame that ran a raycast (every frame but the first), is
 * a mask frame (run_masks of emf_fusion_process_frame; every mask_frames-th frame of emf_fusion_process_rgbd) and was
 * handed NO masks of any kind -- queued instance or new-object masks, a Mask%04d.plk of use_preproc_masks, the masks
 * argument of process_frame: those take precedence -- proposes its own instance masks from the frame's points and the
 * background's ray lengths, on the frame's stream between raycast and integration, and hands them to the object life
 * cycle exactly as queued instance masks are (no class scores).  One wait per such frame, for the count.
 *   params             NULL: the defaults.  band < 0 (the default here): the background's truncation distance.
 *                      EMF_E_ARG for a value outside the ranges of emf_motion_params_t.
 *   last_motion_masks  of the last processed frame: *count proposals (0 if the frame proposed nothing or did not run
 *                      the proposal at all), at most `capacity` records to info_out (may be NULL), and to labels_out
 *                      (may be NULL) the W x H int32 rank image, -1 where no proposal is.  Waits for the device.
 * emf_fusion_get_last_masks draws the proposals of the last frame that made any attempt, in instance colours by rank.
 * Nothing is kept from frame to frame and nothing goes into a checkpoint: a resumed session switches it on again.
 * Refused (EMF_E_ARG, "... not supported on the sharded path", the session stays usable) on the sharded path. */
int emf_fusion_set_motion_masks(emf_fusion_t* h, int on, const emf_motion_params_t* params);
int emf_fusion_last_motion_masks(emf_fusion_t* h, int32_t* labels_out, emf_motion_info_t* info_out, int capacity,
                                 int32_t* count);
/* Follow the camera (new behaviour, off by default, may be switched at any time, and with it off no
 * launch and no output byte of a frame changes).  The background is rolled by whole voxels along its own axes
 * (include/emf_hip.h "Rolling a volume") so that the followed point q = bgPose^-1 (camT + camR (0, 0, look_ahead))
 * stays within one step of its centre; what slides out is meshed first (keep_retired) and kept on the host.  The
 * background at any time and every retired slab sit on one integer voxel lattice, index (0, 0, 0) = voxel (0, 0, 0) of
 * the background at its initial pose.  Object poses are in the world frame and are untouched.
 *   set_background_follow  params NULL: the defaults, step (64, 64, 64), look_ahead 0, keep_retired 1.  EMF_E_ARG for
 *                      a step component that is not a positive multiple of the tile (32, 8, 8), and ("... not
 *                      supported on the sharded path", the session stays usable) on the sharded path.  The policy
 *                      runs at the end of every frame: after the integration, before the per-frame meshes.
 *                      A checkpoint carries the switch and its parameters only once the background has rolled
 *                      (version 2; a never-rolled session writes version 1 byte for byte): a session saved before its
 *                      first roll resumes with follow off and the caller sets it again, as with the motion masks.
 *   roll_background    rolls now by `shift` voxels (any integers; multiples of the tile take the fast path).
 *                      keep_retired < 0: retire first if the session's keep_retired is set (it is by default, also
 *                      with follow off); 0: only re-centre, nothing is meshed or kept; > 0: retire first.
 *   background_origin  the cumulative shift; R, t (either may be NULL): the background's current pose, volume centre
 *                      -> world.  After a roll by k: t' = t + R (float(k_i) * voxel_size), as an object's resize.
 *   retired_slabs      *count slabs so far; up to `capacity` records of 7 int32 to info (may be NULL): frame, origin
 *                      x y z (lattice index of the slab's voxel (0, 0, 0)), resolution x y z.  frame: the one at whose
 *                      end the roll happened; for roll_background the last one processed.
 *   retired_slab_mesh  makes slab `index`'s mesh the one emf_fusion_copy_mesh / emf_fusion_copy_mesh_colors copy.  Its
 *                      vertices are in the slab's own frame (its centre at 0), exactly what meshing a volume of that
 *                      size holding those voxels gives; emf_fusion_write_results writes them as bg_retired/%04d.ply
 *                      translated into the frame of the background's INITIAL pose, with bg_retired/origins.txt
 *                      (one line per slab: the 7 numbers above), and creates bg_retired/ only if there is a slab.
 *   follow_shift       the policy alone, no device and no handle: shift_i = trunc(q_i / (float(step_i) * voxel_size))
 *                      * step_i in single precision.  EMF_E_ARG for a refused step, voxel size or q. */
typedef struct emf_follow_params {
    int32_t step[3];
    float look_ahead;
    int32_t keep_retired;
} emf_follow_params_t;
int emf_fusion_set_background_follow(emf_fusion_t* h, int on, const emf_follow_params_t* params);
int emf_fusion_roll_background(emf_fusion_t* h, const int32_t shift[3], int keep_retired);
int emf_fusion_background_origin(emf_fusion_t* h, int32_t origin[3], float R[9], float t[3]);
int emf_fusion_retired_slabs(emf_fusion_t* h, int32_t* info, int capacity, int32_t* count);
int emf_fusion_retired_slab_mesh(emf_fusion_t* h, int index, uint32_t* num_vertices, uint32_t* num_triangles);
/* The world mesh: ONE mesh of the current background's observed tiles and of every tile the
 * background store holds, meshed as one lattice -- no duplicates, no seams, the current volume winning where both
 * claim a tile.  It becomes the mesh that emf_fusion_copy_mesh / emf_fusion_copy_mesh_colors copy, as
 * retired_slab_mesh's does.  weld < 0: the session's switch (emf_fusion_set_mesh_weld); an active component filter
 * implies the weld.  Nothing of the session changes.  EMF_E_ARG on a sharded session and when the background's
 * resolution or origin is not a multiple of the tile (32, 8, 8). */
int emf_fusion_world_mesh(emf_fusion_t* h, int weld, uint32_t* num_vertices, uint32_t* num_triangles);
/* Of the last world mesh: tiles taken from the volume, tiles taken from the store, stored tiles skipped because the
 * volume holds their coordinate, surface cubes owned by stored tiles. */
int emf_fusion_world_mesh_info(emf_fusion_t* h, uint64_t out[4]);
/* setup_output's exp_world_mesh, as an entry of its own so that emf_fusion_setup_output keeps its signature:
 * emf_fusion_write_results also writes world.ply, the PLY of the world mesh at that moment, byte for byte
 * emf_io_write_mesh of it, and nothing else new.  Off (the default): no output byte changes. */
int emf_fusion_set_world_mesh_output(emf_fusion_t* h, int on);
/* The extent of the scene queries (new behaviour, sticky, off by default, never in a checkpoint; with it
 * off no launch, no output byte and no refusal changes).  world != 0: the box of emf_fusion_distance_field[_nearest],
 * emf_fusion_frontiers, emf_fusion_plan, emf_fusion_cast_rays, emf_fusion_view_gain and emf_fusion_ground_map may leave
 * the background.  It stays in voxels of the CURRENT background volume -- box_lo may be negative, box_lo + box_size may
 * exceed the resolution -- and the classes come from the tiles the world mesh reads (the observed tiles of the volume
 * and every tile the background store holds; emf_hip_occupancyTiles); what lies in no tile is unknown.  The limits
 * of a box stay.  Such a query is refused (EMF_E_ARG) on the sharded path and when the background's resolution or
 * origin is not a multiple of the tile (32, 8, 8), with the session untouched.  emf_fusion_planes reads tsdf values and
 * keeps refusing a box that leaves the background.  emf_fusion_write_results then takes emf_fusion_world_extent
 * wherever distance.bin, nearest.bin, frontiers.txt, plan.txt and ground.bin / ground.txt take the whole background
 * (the two text files say so in a second comment line), and refuses an extent above the limits naming the axis.
 * These are entries of their own so that every existing entry keeps its signature. */
int emf_fusion_set_query_extent(emf_fusion_t* h, int world);
/* The bounding box, in voxels of the current background volume, of the background and every tile the background
 * store holds: lo = (0, 0, 0) and size = the resolution when nothing is stored.  Host state only: nothing is launched. */
int emf_fusion_world_extent(emf_fusion_t* h, int32_t lo[3], int32_t size[3]);
int emf_fusion_follow_shift(const float q[3], const int32_t step[3], float voxel_size, int32_t shift[3]);
/* The distance field of the scene (include/emf_hip.h "Distance field"; new behaviour, nothing of the
 * session changes and nothing goes into a checkpoint).  Over the box [box_lo, box_lo + box_size) of the background, in
 * voxels (x, y, z), inside the volume -- both NULL: the whole background -- the occupancy classes of the background
 * (0 free, 1 occupied, 2 unknown), every live object whose id is not in exclude_ids stamped as occupied at its current
 * pose, and d2, the exact squared distance in voxels to the nearest voxel whose class bit is set in site_mask (1 free,
 * 2 occupied, 4 unknown), EMF_DF_FAR where there is none or, with cap_voxels > 0, beyond the cap; with metres != 0
 * also sqrtf(d2) * voxel size as f32, +inf for EMF_DF_FAR.  Enqueued on the main stream after the frame; the results
 * stay on the device until the next call.  lo_out / size_out (may be NULL): the box; R / t (may be NULL): the pose of
 * voxel (0, 0, 0) of the box -> world, i.e. the background's current pose composed with the box origin, so it stays
 * right after rolls.  EMF_E_ARG on a sharded session ("not supported on the sharded path"). */
int emf_fusion_distance_field(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], uint32_t site_mask,
                              int32_t cap_voxels, const int32_t* exclude_ids, int32_t num_exclude, int metres,
                              int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]);
/* Copies the last distance field to the host (waits for the main stream): one u8, one i32 and one f32 per voxel of
 * the box in (z, y, x) order; any of the three may be NULL. */
int emf_fusion_copy_distance_field(emf_fusion_t* h, uint8_t* classes, int32_t* d2, float* metres);
/* The objects the last distance field stamped, in creation order: ids[k], and R[9 k ..] / t[3 k ..], object volume <-
 * background volume exactly as passed to the kernel.  count is always the full number; at most capacity are written. */
int emf_fusion_distance_field_objects(emf_fusion_t* h, int32_t* ids, float* R, float* t, int capacity, int32_t* count);
/* setup_output's exp_distance_field, as an entry of its own so that emf_fusion_setup_output keeps its signature:
 * emf_fusion_write_results also writes distance.bin (f32 metres to the nearest occupied voxel -- or occupied or unknown
 * with unknown_is_obstacle -- of the whole background, +inf beyond cap_metres, which is rounded up to whole voxels; 0:
 * no cap) and occupancy.bin (u8 classes), both in the container of the tsdfs/ dumps.  Off: no output byte changes. */
int emf_fusion_set_distance_output(emf_fusion_t* h, int on, float cap_metres, int unknown_is_obstacle);
/* The distance field with the nearest site (include/emf_hip.h emf_hip_distanceTransformNearest): the
 * arguments and results of emf_fusion_distance_field, and also, per voxel of the box, the linear index
 * (z * size_y + y) * size_x + x -- box coordinates -- of the nearest voxel whose class bit is set in site_mask, the
 * smallest index among equally near ones, -1 exactly where d2 is EMF_DF_FAR.  Two more i32 per voxel on the device,
 * allocated at first use.  EMF_E_ARG on a sharded session ("not supported on the sharded path"). */
int emf_fusion_distance_field_nearest(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], uint32_t site_mask,
                                      int32_t cap_voxels, const int32_t* exclude_ids, int32_t num_exclude, int metres,
                                      int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]);
/* Copies the index of the last distance field to the host (waits for the main stream): one i32 per voxel of the box in
 * (z, y, x) order.  EMF_E_ARG when the last field was computed by emf_fusion_distance_field, i.e. without the index. */
int emf_fusion_copy_distance_nearest(emf_fusion_t* h, int32_t* nearest);
/* Point queries on the last distance field, answered from its device arrays: for n voxels (x, y, z) in BOX coordinates
 * (host memory) the class byte, d2 and the nearest-site index, n of each; any of the three outputs may be NULL.  A
 * voxel outside the box yields 255, EMF_DF_FAR and -1.  Only the n voxels and the n records cross the bus (waits for the
 * main stream).  lo_out / size_out (may be NULL): the box of the last field, in voxels of the background.  EMF_E_ARG
 * when no field has been computed, for a non-NULL nearest when the last field has no index, and on a sharded session
 * ("not supported on the sharded path"). */
int emf_fusion_query_distance(emf_fusion_t* h, const int32_t* voxels, int32_t n, uint8_t* classes, int32_t* d2, int32_t* nearest,
                              int32_t lo_out[3], int32_t size_out[3]);
/* setup_output's exp_distance_nearest, as an entry of its own: with emf_fusion_set_distance_output on,
 * emf_fusion_write_results also writes nearest.bin, i32 in the container of distance.bin (the element size in its header
 * is 4): the linear index (z * res_y + y) * res_x + x of the nearest obstacle voxel of the whole background, -1 where
 * distance.bin holds +inf.  Off, or without the distance output: no output byte changes. */
int emf_fusion_set_distance_nearest_output(emf_fusion_t* h, int on);
/* Exploration frontiers of the scene (include/emf_hip.h "Frontiers"; new behaviour, nothing of the
 * session changes -- the last distance field included -- and nothing goes into a checkpoint).  Over the box of the
 * background as for emf_fusion_distance_field, on the same occupancy classes (every live object whose id is not in
 * exclude_ids stamped as occupied): the free voxels with an unknown face neighbour inside the box -- with
 * clearance_voxels > 0 only those at least that many voxels from the nearest occupied voxel of the box -- their
 * 26-connected clusters, and one record per cluster of at least min_voxels (>= 1) voxels.  Enqueued on the main stream
 * after the frame; waits for the number of clusters and for the records, which are kept sorted by count descending,
 * ties by label ascending, until the next call.  lo_out / size_out / R / t (may be NULL): the box and the pose of its
 * voxel (0, 0, 0) -> world, as emf_fusion_distance_field returns them.  counters (may be NULL): kept clusters, all
 * clusters, frontier voxels (EMF_FRONTIER_*).  EMF_E_ARG on a sharded session ("not supported on the sharded path"). */
int emf_fusion_frontiers(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], int32_t min_voxels,
                         int32_t clearance_voxels, const int32_t* exclude_ids, int32_t num_exclude, int32_t lo_out[3],
                         int32_t size_out[3], float R[9], float t[3], uint32_t counters[3]);
/* The last frontiers: the first min(kept, capacity) records in the sorted order; per record (x, y, z) of the
 * representative and of the centroid in the world frame, in double -- the voxel (rep, or sum / count) plus
 * box_lo - (res - 1) / 2, times the voxel size, through the background's pose; and the label volume, one i32 per voxel
 * of the box in (z, y, x) order (waits for the main stream).  Any of the four may be NULL. */
int emf_fusion_copy_frontiers(emf_fusion_t* h, emf_frontier_cluster_t* records, int32_t capacity, double* rep_world,
                              double* centroid_world, int32_t* labels);
/* setup_output's exp_frontiers, as an entry of its own so that emf_fusion_setup_output keeps its signature:
 * emf_fusion_write_results also writes frontiers.txt of the whole background -- after one comment line, one line per
 * cluster of at least min_voxels voxels, largest first:  count (%d), x y z of the representative voxel and x y z of the
 * centroid in the world frame (metres, the double value rounded once to float, %.9g each), and the inclusive bounding
 * box lo_x lo_y lo_z hi_x hi_y hi_z in voxels of the background (%d).  clearance_metres is rounded up to whole voxels.
 * Off: no output byte changes. */
int emf_fusion_set_frontier_output(emf_fusion_t* h, int on, int32_t min_voxels, float clearance_metres);
/* Path planning over the scene (include/emf_hip.h "Planning"; new behaviour, nothing of the session
 * changes -- the last distance field and the last frontiers included -- and nothing goes into a checkpoint).  Over the box
 * of the background as for emf_fusion_frontiers, on the same occupancy classes (every live object whose id is not in
 * exclude_ids stamped as occupied): the cost-to-go field from the start voxels -- num_start x (x, y, z) in BOX
 * coordinates; num_start == 0: the background voxel under the camera, or the nearest one where the camera is outside -- through the free voxels (and the unknown ones,
 * with through_unknown) at least clearance_voxels from the nearest occupied voxel of the box, plus whatever is not
 * occupied within seed_radius_voxels of a start; 26-connected moves of weight 3 / 4 / 5; max_cost 0: no cap.  Then the
 * paths from the goal voxels (num_goals x (x, y, z), box coordinates; a goal is never moved to another voxel) back to a
 * start, at most path_capacity voxels of each, or all of each with path_capacity < 0.  Enqueued on the main stream after
 * the frame; waits for the rounds of the relaxation and for the results, which are kept until the next call.
 * lo_out / size_out / R / t (may be NULL): as emf_fusion_frontiers.  counters (may be NULL): EMF_PLAN_* -- converged,
 * rounds, voxels with a finite cost, start voxels used.  longest_path (may be NULL): the voxels of the longest kept path.
 * EMF_E_ARG on a sharded session ("not supported on the sharded path"); EMF_E_LIMIT for a box above 2^29 voxels. */
int emf_fusion_plan(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* start_voxels,
                    int32_t num_start, int32_t seed_radius_voxels, int through_unknown, int32_t clearance_voxels,
                    uint32_t max_cost, const int32_t* goal_voxels, int32_t num_goals, int32_t path_capacity,
                    const int32_t* exclude_ids, int32_t num_exclude, int32_t lo_out[3], int32_t size_out[3], float R[9],
                    float t[3], uint32_t counters[4], int32_t* longest_path);
/* The last plan, per goal in the order given: goal_cost (EMF_PLAN_UNREACHED / EMF_PLAN_BLOCKED: no path), lengths (the
 * voxels of the whole path, 0: none), steps (3 per goal: the face, edge and corner moves of the kept path), paths
 * (capacity i32 per goal: linear indices (z * ny + y) * nx + x of the box, the goal first; untouched beyond the kept
 * length), path_world (3 doubles per path entry, the voxel in the world frame as emf_fusion_copy_frontiers computes
 * it), and cost: the field, one u32 per voxel of the box in (z, y, x) order (waits for the main stream).  Any may be NULL. */
int emf_fusion_copy_plan(emf_fusion_t* h, uint32_t* goal_cost, int32_t* lengths, int32_t* steps, int32_t* paths,
                         int32_t capacity, double* path_world, uint32_t* cost);
/* The device pointer of the last plan's cost field (NULL before the first plan); valid until the next plan. */
int emf_fusion_plan_cost_ptr(emf_fusion_t* h, const uint32_t** cost_dev);
/* setup_output's exp_plan, as an entry of its own so that emf_fusion_setup_output keeps its signature:
 * emf_fusion_write_results also writes plan.txt of the whole background, planned from the voxel under the last camera
 * position (start radius max(clearance, one voxel)) to the representative of every frontier cluster that
 * emf_fusion_set_frontier_output's min_voxels keeps at this clearance.  After one comment line, per cluster in the order
 * of frontiers.txt:  count (%d) reachable (0 / 1) cost (%u) length_m (%.9g: (faces + sqrt 2 edges + sqrt 3 corners) *
 * voxel, in double) x y z of the representative in the world frame (%.9g, the double rounded once to float) n_path (%d),
 * followed by n_path lines x y z: the path's voxels in the world frame, from the goal to the start (%.9g each).
 * clearance_metres is rounded up to whole voxels.  Off: no output byte changes. */
int emf_fusion_set_plan_output(emf_fusion_t* h, int on, float clearance_metres, int through_unknown);
/* Voxel rays over the scene (include/emf_hip.h "Voxel rays"; new behaviour, nothing of the session
 * changes -- the last distance field, frontiers and plan included -- and nothing goes into a checkpoint).  Over the box of
 * the background as for emf_fusion_frontiers, on the same occupancy classes (every live object whose id is not in
 * exclude_ids stamped as occupied): n rays from[k] -> to[k], 3 * n i32 each in BOX coordinates, used as they are.  A ray
 * is the integer walk of the header -- it is NOT symmetric in its two ends -- and ends at the first voxel that is
 * outside the box, whose class bit is not in pass_mask or, with clearance_voxels > 0, that is nearer than that to an
 * occupied voxel of the box; count_mask: the classes counted on the way.  results (n records, or NULL) and groups
 * (ceil(n / group) records with group > 0, else NULL): at least one of the two.  Uploads the rays, launches once, copies
 * the records back and waits once.  lo_out / size_out / R / t (may be NULL): as emf_fusion_frontiers.  EMF_E_ARG on a
 * sharded session ("not supported on the sharded path"). */
int emf_fusion_cast_rays(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* from,
                         const int32_t* to, int32_t n, uint32_t pass_mask, uint32_t count_mask, int32_t clearance_voxels,
                         const int32_t* exclude_ids, int32_t num_exclude, int32_t group, emf_ray_result_t* results,
                         emf_ray_group_t* groups, int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]);
/* The integer ray targets of one candidate view; needs no handle and no device.  (R, t): viewer -> world, OpenCV camera
 * (as emf_fusion_render_view), row-major, in double; K = (fx, fy, cx, cy) of a gw x gh grid image; range in metres; the
 * background's pose (bg_R, bg_t), resolution and voxel size, and the box origin.  origin: the box voxel under the
 * camera, rint(bg_R^T (t - bg_t) / voxel + (res - 1) / 2) - box_lo; targets: 3 * gw * gh i32, cell (i, j) at j * gw + i.
 * Everything in float64, every line a single operation in this order:
 *     x = (i - cx) / fx;  y = (j - cy) / fy
 *     m = sqrt(x * x + y * y + 1.0)                  summed left to right
 *     c = (x / m, y / m, 1.0 / m)
 *     M = bg_R^T * R                                 each element a three-term sum left to right, once per view
 *     dir = M c                                      rows summed left to right
 *     target = origin + rint(dir * (range / voxel))  ties to even
 * range / voxel above EMF_RAY_MAX_DELTA is EMF_E_ARG. */
int emf_fusion_view_ray_targets(const double R[9], const double t[3], const double K[4], int32_t gw, int32_t gh, double range,
                                const float bg_R[9], const float bg_t[3], const int32_t res[3], float voxel_size,
                                const int32_t box_lo[3], int32_t origin[3], int32_t* targets);
/* The unknown space each of num_views candidate views would see (views_R: 9 doubles per view, views_t: 3): the targets
 * of all views by emf_fusion_view_ray_targets, then ONE emf_fusion_cast_rays from each view's origin voxel with pass_mask
 * = FREE | UNKNOWN and count_mask = UNKNOWN -- a ray sees through unknown space and stops at the first occupied voxel --
 * and group = gw * gh.  groups: num_views records, one per view (a camera outside the box: invalid == gw * gh, zero
 * counts).  Optional copy-outs, each may be NULL: origins (3 i32 per view), targets (3 * gw * gh i32 per view), results
 * (gw * gh records per view; only then are the per-ray records written and copied).  A count over rays is a score, not a
 * volume.  EMF_E_ARG on a sharded session. */
int emf_fusion_view_gain(emf_fusion_t* h, const double* views_R, const double* views_t, int32_t num_views, int32_t gw, int32_t gh,
                         const double K[4], double range, const int32_t box_lo[3], const int32_t box_size[3],
                         const int32_t* exclude_ids, int32_t num_exclude, emf_ray_group_t* groups, int32_t* origins,
                         int32_t* targets, emf_ray_result_t* results, int32_t lo_out[3], int32_t size_out[3], float R[9],
                         float t[3]);
/* Shortcuts of the last plan's paths: for every goal with a kept path p_0 .. p_k (goal first) the rays p_i -> p_j, 2 <=
 * j - i <= window clipped at k, over the plan's own classes, traverse mask and clearance gate (no bubble) in one launch;
 * then greedily from i the largest such j whose ray is REACHED, else i + 1 (a step of the planner's own path is accepted
 * untested).  counts (may be NULL): per goal the number of waypoints, 0 for a goal without a path; longest (may be
 * NULL): their maximum.  EMF_E_ARG without a plan, with window < 1 and on a sharded session. */
int emf_fusion_plan_shortcut(emf_fusion_t* h, int32_t window, int32_t* counts, int32_t* longest);
/* The waypoints of the last emf_fusion_plan_shortcut: capacity i32 per goal, the ascending indices into the goal's path
 * from 0 to k, untouched beyond the goal's count. */
int emf_fusion_copy_plan_shortcut(emf_fusion_t* h, int32_t* waypoints, int32_t capacity);
/* setup_output's exp_plan_shortcut, as an entry of its own: with window > 0 plan.txt (emf_fusion_set_plan_output) gains,
 * after the path lines of every reachable goal, one line "waypoints n i_0 .. i_(n-1)": emf_fusion_plan_shortcut(window)
 * of that goal's path.  0: plan.txt as before, byte for byte. */
int emf_fusion_set_plan_shortcut_output(emf_fusion_t* h, int32_t window);
/* Object shapes (include/emf_hip.h "Object shapes"; new behaviour, opt-in): where in its volume each
 * asked model is, how large it is, how it is oriented and how much of its surface has been seen.  WHAT IS MEASURED IS THE
 * OBSERVED SOLID BAND, NOT THE BODY -- a TSDF observes a band around the surface, the interior of an object has weight
 * 0 -- so nothing here is a volume in cubic metres.
 *   object_shapes   ids: n live objects (emf_fusion_object_ids lists them), in the order of the result;
 *                   include_background != 0 puts the background (id 0) in front.  The outputs hold n (+ 1) records each,
 *                   NULL = not wanted: ids_out, res_out (3 per model), voxel_size_out, poses_out (12 per model: R row-major,
 *                   then t; volume -> world as the call found it), the integer moments, the frame from them, the extents along the frame, and the box (voxels, metres in the model's frame, world frame
 *                   through the model's pose as emf_fusion_get_pose gives it).  One moments launch for all models and
 *                   one wait, the frames on the host, one extents launch and one more wait.  An id that does not exist
 *                   is EMF_E_ARG; an object without a solid voxel has frames[k].valid == 0 and zeros for frame and box.
 *                   Changes nothing of the session.  EMF_E_ARG on the sharded path.
 *   shape_frame     needs no device and no handle: the frame of one moments record, float64 in the fixed operation order
 *                   of include/emf_hip.h (moments->solid == 0: valid = 0 and nothing else is written).
 *   shape_box       needs no device and no handle: the box of a model from its moments, a frame with valid != 0, the
 *                   extents along it, the model's resolution, voxel size and pose (R, t: volume -> world).
 *   set_shape_output  setup_output's exp_object_shapes, as an entry of its own so that the existing entries keep their
 *                   signatures: emf_fusion_write_results also writes shapes.txt, after a comment line one line per live
 *                   object in id order: id valid solid observed faces_free faces_unknown lo(3) hi(3), the integers, then
 *                   the world-frame box in %.9g: centre (3), half extents in metres (3), axes (9).  Off: the set of
 *                   result files and every byte of them as before. */
int emf_fusion_object_shapes(emf_fusion_t* h, const int32_t* ids, int32_t n, int32_t include_background, int32_t* ids_out,
                             int32_t* res_out, float* voxel_size_out, float* poses_out, emf_shape_moments_t* moments,
                             emf_shape_frame_t* frames, emf_shape_extents_t* extents, emf_shape_box_t* boxes);
int emf_fusion_shape_frame(const emf_shape_moments_t* moments, emf_shape_frame_t* frame);
int emf_fusion_shape_box(const emf_shape_moments_t* moments, const emf_shape_frame_t* frame, const emf_shape_extents_t* extents,
                         const int32_t res[3], float voxel_size, const float R[9], const float t[3], emf_shape_box_t* box);
int emf_fusion_set_shape_output(emf_fusion_t* h, int on);
/* Object contacts (include/emf_hip.h "Object contacts"; new behaviour, opt-in): whether the asked objects
 * touch each other or the background, how far apart their surfaces are and whether they interpenetrate, read from the
 * signed-distance volumes.  IT MEASURES WHAT THE VOLUMES SAY: min_s == 1 (summary.saturated) means "at least one
 * truncation distance apart" and is no distance; a penetration deeper than the fused band reads UNKNOWN; a clearance
 * reads up to one probe voxel large.
 *   object_contacts ids: n live objects, each once: the probes.  The fields are those objects and, with
 *                   include_background != 0, the background (id 0, in front); the background as a probe is not built.
 *                   touch_m: the TOUCHING threshold in metres; < 0: one voxel of the probe (a policy, not a
 *                   measurement).  With m = n + (include_background != 0) models the call makes n * (m - 1) ordered
 *                   pairs, grouped by probe, and one summary per unordered pair: n * (n - 1) / 2 + n with the background,
 *                   else n * (n - 1) / 2.  Outputs, NULL = not wanted: ids_out and sides_out (m: res, voxel size,
 *                   truncation distance, pose world <- model as the call found it), pair_ids_out (2 per pair: the ids of
 *                   probe and field), pairs_out (what each pair carried; a, b: slots of the call's table), records_out,
 *                   summary_ids_out (4 per summary: the ids a, b, the index of the record a -> b, and of b -> a or -1),
 *                   summaries_out, and the two counts.  One launch and one wait.  An id that does not exist or is named
 *                   twice is EMF_E_ARG.  Changes nothing of the session.  EMF_E_ARG on the sharded path.
 *   contact_pose / contact_touch / contact_summary   need no device and no handle: the host stage, float64 in the fixed
 *                   operation order of include/emf_hip.h.  ba NULL: the field was no probe.
 *   set_contacts_output  setup_output's exp_object_contacts, as an entry of its own: emf_fusion_write_results also writes
 *                   contacts.txt, after a comment line one line per ordered pair with sampled > 0 (the live objects in
 *                   id order against each other and the background): a b surface outside unknown masked sampled inside
 *                   touching normals, the integers, then in %.9g min_s and the world contact point (3) and normal (3) of
 *                   that record alone, zeros without.  Off: the set of result files and every byte of them as before. */
int emf_fusion_object_contacts(emf_fusion_t* h, const int32_t* ids, int32_t n, int32_t include_background, double touch_m,
                               int32_t* ids_out, emf_contact_side_t* sides_out, int32_t* pair_ids_out, emf_contact_pair_t* pairs_out,
                               emf_contact_t* records_out, int32_t* summary_ids_out, emf_contact_summary_t* summaries_out,
                               int32_t* n_pairs_out, int32_t* n_summaries_out);
int emf_fusion_contact_pose(const float Ra[9], const float ta[3], const float Rb[9], const float tb[3], float R[9], float t[3]);
int emf_fusion_contact_touch(double touch_m, float truncdist_b, float* touch);
int emf_fusion_contact_summary(const emf_contact_t* ab, const emf_contact_t* ba, const emf_contact_side_t* a,
                               const emf_contact_side_t* b, emf_contact_summary_t* summary);
int emf_fusion_set_contacts_output(emf_fusion_t* h, int on, double touch_m);
/* Absorbing objects into the background (include/emf_hip.h "Absorbing a volume"; new behaviour, opt-in).
 * An object that leaves view is deleted, as in the reference, and every scene query forgets it.  With the switch on its
 * signed-distance band is first resampled through the relative pose into the background volume and fused there by the
 * background's own running average, so that the distance field, plans, the ground map, the world mesh, the tile store and
 * a checkpoint keep it.  IT CARRIES THE BAND ONLY, not the free space around it; in a coloured session
 * (emf_fusion_enable_color) the colour entry of every fused voxel goes with it, blended into the background's by the
 * colour weights (emf_hip_absorbVolumeColor), in a colourless one the plain entry is called as before;
 * an absorbed object that later moves leaves a ghost until free space carves it;
 * what lies outside the background's cube is clipped and lost.
 *   absorb_pose     needs no device and no handle: (R, t) taking the DESTINATION's volume frame into the SOURCE's from the
 *                   poses (world <- volume) of the destination d and the source s; float64 in the fixed order of
 *                   contact_pose with a = d, b = s, rounded to f32 once.
 *   set_absorb_objects  sticky, off by default.  On: an object the frame's clean-up deletes BECAUSE IT IS NOT VISIBLE is
 *                   absorbed before it is erased -- not one deleted as spurious (low existence on a mask frame, association
 *                   mass below assocThresh), not a person under ignore_person.  The pose is the object's current pose
 *                   against the background's current pose (correct after rolls); one launch per object on the main stream,
 *                   in list order; the background's derived state is renewed once after the last.  The kept mesh and the
 *                   exp_vols copies of the deleted object stay as they are.  Off: no launch, no output byte and no
 *                   checkpoint byte changes.  Neither the switch nor the log is written to a checkpoint.
 *   absorb_object   absorbs the LIVE object `id` now and removes it from the session as a deletion would (leaving it
 *                   live would let two models explain one surface).  An explicit call absorbs what it names, a person
 *                   under ignore_person too.  event NULL: not wanted.  EMF_E_ARG: an unknown id, the background (0), an
 *                   object this rank does not own.
 *   absorbed        the session's log, oldest first: the first min(capacity, *count) events; *count is the number logged.
 *                   emf_fusion_reset and a loaded checkpoint start it empty.
 *   set_absorbed_output  setup_output's exp_absorbed: emf_fusion_write_results also writes absorbed.txt, after a comment
 *                   line one line per event: id frame clipped, box_lo (3), box_size (3), the eight counts, lo (3), hi (3),
 *                   then R (9) and t (3) in %.9g.  Off: the set of result files and every byte of them as before.  In a
 *                   coloured session each line ends with the event's colored and uncolored counts and the comment line
 *                   names them; a colourless session writes the bytes it always wrote.
 *   absorbed_colors the colour records of the log, parallel to `absorbed` (emf_absorb_event_t keeps its layout): the first
 *                   min(capacity, *count) of them, colored + uncolored == record.fused; zeros for the events of a
 *                   colourless session.  Like the log they are session state and in no checkpoint.
 * set_absorb_objects (on) and absorb_object are EMF_E_ARG on the sharded path. */
typedef struct emf_absorb_event {
    int32_t id;             /* the absorbed object */
    int32_t frame;          /* the frame index at which it happened */
    int32_t clipped;        /* the object's cube, in background voxels rounded outwards, leaves the background's: that part
                               is lost.  Conservative by less than a voxel; 0 for a pose without a finite inverse */
    int32_t reserved;       /* 0 */
    float R[9], t[3];       /* the pose used: the object's volume frame <- the background's volume frame */
    int32_t lo[3], size[3]; /* the box of background voxels the launch covered */
    emf_absorb_t record;    /* include/emf_hip.h "Absorbing a volume" */
} emf_absorb_event_t;       /* 176 bytes */
int emf_fusion_absorb_pose(const float Rd[9], const float td[3], const float Rs[9], const float ts[3], float R[9], float t[3]);
int emf_fusion_set_absorb_objects(emf_fusion_t* h, int on);
int emf_fusion_absorb_object(emf_fusion_t* h, int32_t id, emf_absorb_event_t* event);
int emf_fusion_absorbed(emf_fusion_t* h, emf_absorb_event_t* events, int32_t capacity, int32_t* count);
int emf_fusion_absorbed_colors(emf_fusion_t* h, emf_color_moved_t* records, int32_t capacity, int32_t* count);
int emf_fusion_set_absorbed_output(emf_fusion_t* h, int on);
/* Lifting objects out of the background (include/emf_hip.h "Lifting a volume"; new behaviour, opt-in):
 * the other half of absorbing.  A new object is SEEDED with the band the background already holds inside its cube, only
 * where it has no observation of its own, and the background RELEASES the band voxels the object then holds as
 * foreground, so that one surface has one explanation and no ghost stays behind when the object moves.  In a coloured
 * session the seeded voxels take the background's colour entries (the nearest voxel's, its weight capped) and the released
 * voxels' entries are cleared (emf_hip_seedVolumeColor, emf_hip_releaseVolumeColor); in a colourless one
 * the plain entries are called as before.  A voxel behind the object along a mask ray inside the cube is released too; an object discovered by motion
 * masks sits in free space: the seed finds nothing there and the ghost at the OLD place is not addressed.
 *   set_lift_objects   sticky, off by default.  On: every object a frame creates from a mask is seeded after the frame's
 *                   integration and before its masks are integrated (so the frame's own mask classifies the seeded
 *                   voxels), and released after them; several creations of a frame run in list order.  Neither the
 *                   switch nor the log is written to a checkpoint; with it off no launch, no output byte and no
 *                   checkpoint byte changes.
 *   lift_object     seed, then release, for the LIVE object `id` now; the object stays live.  Its seeded voxels carry no
 *                   foreground count until the next mask frame: until then they are neither raycast nor released.
 *                   `event` may be NULL.  EMF_E_ARG: an unknown id, id 0, an object of another rank.
 *   lifted          the session's log, oldest first: the first min(capacity, *count) events; *count is the number logged.
 *                   reset() and a loaded checkpoint start it empty.
 *   set_lifted_output  setup_output's exp_lifted: emf_fusion_write_results also writes lifted.txt, after a comment line
 *                   one line per event: id frame clipped, box_lo (3), box_size (3), the seed's eight counts, lo (3), hi
 *                   (3), the release's seven counts, lo (3), hi (3), then the seed's R (9) and t (3) and the release's R
 *                   (9) and t (3) in %.9g.  Off: the set of result files and every byte of them as before.  In a coloured
 *                   session each line ends with the colored and uncolored counts of the seed, then of the release, and
 *                   the comment line names them; a colourless session writes the bytes it always wrote.
 *   lifted_colors   the colour records of the log, parallel to `lifted` (emf_lift_event_t keeps its layout), TWO per event:
 *                   records[2 k] the seed's (colored + uncolored == seed.seeded), records[2 k + 1] the release's
 *                   (== release.released); `capacity` and *count are in events.  Zeros for a colourless session.
 * set_lift_objects (on) and lift_object are EMF_E_ARG on the sharded path. */
typedef struct emf_lift_event {
    int32_t id;             /* the lifted object */
    int32_t frame;          /* the frame index at which it happened */
    int32_t clipped;        /* as emf_absorb_event_t.clipped */
    int32_t reserved;       /* 0 */
    float seed_R[9], seed_t[3];       /* the seed's pose: the background's volume frame <- the object's volume frame */
    float release_R[9], release_t[3]; /* the release's pose: the object's volume frame <- the background's */
    int32_t lo[3], size[3]; /* the box of background voxels the release covered */
    emf_seed_t seed;        /* include/emf_hip.h "Lifting a volume" */
    emf_release_t release;
} emf_lift_event_t;         /* 304 bytes */
int emf_fusion_set_lift_objects(emf_fusion_t* h, int on);
int emf_fusion_lift_object(emf_fusion_t* h, int32_t id, emf_lift_event_t* event);
int emf_fusion_lifted(emf_fusion_t* h, emf_lift_event_t* events, int32_t capacity, int32_t* count);
int emf_fusion_lifted_colors(emf_fusion_t* h, emf_color_moved_t* records, int32_t capacity, int32_t* count);
int emf_fusion_set_lifted_output(emf_fusion_t* h, int on);
/* Merging an object into another object (include/emf_hip.h "Merging a volume"; new behaviour, opt-in): the
 * repair for one physical thing that ended up with two volumes -- an instance segmenter that cut it into two masks, a
 * re-detection from its other side, a drifted track.  With the switch off and no call nothing of a session changes.
 *   set_merge_objects  sticky, off by default; the parameters are kept either way.  On: at the end of every mask frame,
 *                   after the clean-up, with at least two live objects, one emf_hip_contactProbe launch over all ordered
 *                   object pairs (no background); overlap(a -> b) = touching / surface of the record, a float64 quotient;
 *                   a pair qualifies when max(overlap(a -> b), overlap(b -> a)) >= min_overlap and both surfaces hold at
 *                   least min_surface voxels; qualifying pairs are merged in descending overlap, ties to the smaller pair
 *                   of ids, the older object (smaller id) the destination, an object at most once per frame.  min_overlap
 *                   0.5, min_surface 64, touch_m < 0 = half a truncation distance (through contact_touch) and max_res 256
 *                   ARE POLICY, NOT MEASUREMENTS.  IT FINDS DUPLICATES: two halves that merely abut reach no sensible
 *                   overlap; they are merged by merge_objects or by a caller's own rule on object_contacts.  EMF_E_ARG: a
 *                   NaN, min_surface < 0, max_res < 2; on the sharded path (on).
 *   merge_union     needs no device and no handle: the box (metres, the destination's volume frame) that holds the bands
 *                   of both objects, from their inclusive voxel bounds (emf_shape_moments_t lo, hi; hi[0] < 0: none), their
 *                   resolutions and voxel sizes and (R, t) = the destination's volume frame <- the source's.  Float64 in
 *                   the fixed operation order core/EMFusion.hpp states for mergeUnion, rounded to f32 once.  *any == 0, lo
 *                   and hi untouched, where neither object has a solid voxel.
 *   merge_objects   between frames: GROWS the destination's cube until it holds the source's band (the existing resize of
 *                   the union above; set_merge_objects' max_res caps the grown resolution per axis -- 256, a policy value,
 *                   the largest object volume of BASELINE.json's configs; beyond it the destination is not grown and
 *                   `clipped` says so), MERGES the source's band into it through absorb_pose(destination, source) as they are -- the
 *                   volumes are not registered first, a drifted duplicate merges blurred -- the (fg, bg) counts of every
 *                   fused voxel following the band (emf_hip_mergeVolume; emf_hip_mergeVolumeColor in a coloured session),
 *                   and sums the BOOKKEEPING: existence counts and class scores.  The destination keeps its id and its
 *                   tracking state; the source is deleted and NEITHER ITS MESH NOR ITS exp_vols COPY IS KEPT: its
 *                   geometry lives on in the destination.  `event` may be NULL.  EMF_E_ARG: id 0, an unknown id, dst ==
 *                   src, an object of another rank, the sharded path.
 *   merged          the session's log, oldest first: the first min(capacity, *count) events; *count is the number logged.
 *                   Not in a checkpoint; reset() and a loaded checkpoint start it empty.
 *   set_merged_output  setup_output's exp_merged: emf_fusion_write_results also writes merged.txt, after a comment line one
 *                   line per event: dst src frame clipped automatic res_before res_after, box_lo (3), box_size (3), the
 *                   eight counts, lo (3), hi (3), foreground gained colored uncolored, then the two overlaps, the
 *                   destination's R (9) t (3), the source's and the pose used in %.9g.  Off: every result byte as before. */
typedef struct emf_merge_event {
    int32_t dst, src;       /* the object that stays and the one that went into it */
    int32_t frame;          /* the frame index at which it happened */
    int32_t clipped;        /* the source's cube leaves the destination's (as emf_absorb_event_t.clipped) */
    int32_t automatic;      /* 1: merged by set_merge_objects at the end of a mask frame */
    int32_t res_before, res_after;  /* the destination's resolution per axis before and after the growth */
    int32_t reserved;       /* 0 */
    float dst_R[9], dst_t[3];       /* the destination's pose (volume -> world) after the growth */
    float src_R[9], src_t[3];       /* the source's pose */
    float R[9], t[3];       /* the pose used: the source's volume frame <- the destination's */
    int32_t lo[3], size[3]; /* the box of destination voxels the launch covered */
    double overlap[2];      /* what decided an automatic merge: dst -> src, src -> dst; 0 for an explicit call */
    emf_absorb_t record;    /* include/emf_hip.h "Merging a volume" */
    emf_merge_counts_t counts;
    emf_color_moved_t color;        /* zeros in a colourless session */
} emf_merge_event_t;        /* 336 bytes */
int emf_fusion_merge_union(const int32_t dst_lo[3], const int32_t dst_hi[3], const int32_t dst_res[3], float dst_voxel_size,
                           const int32_t src_lo[3], const int32_t src_hi[3], const int32_t src_res[3], float src_voxel_size,
                           const float R[9], const float t[3], float lo[3], float hi[3], int32_t* any);
int emf_fusion_set_merge_objects(emf_fusion_t* h, int on, double min_overlap, int64_t min_surface, double touch_m, int32_t max_res);
int emf_fusion_merge_objects(emf_fusion_t* h, int32_t dst, int32_t src, emf_merge_event_t* event);
int emf_fusion_set_merged_output(emf_fusion_t* h, int on);
/* What a merge sums: the existence counts of the live object `id` (frames it was matched / was not) and its accumulated
 * class scores, the first min(capacity, *count) of them; *count is their number.  EMF_E_ARG: no such object. */
int emf_fusion_object_bookkeeping(emf_fusion_t* h, int32_t id, int32_t* exists, int32_t* not_exists, double* scores, int32_t capacity,
                                  int32_t* count);
int emf_fusion_merged(emf_fusion_t* h, emf_merge_event_t* events, int32_t capacity, int32_t* count);
/* Planes (include/emf_hip.h "Planes"; new behaviour, opt-in): the dominant planes of a box of the
 * background (box_lo / box_size NULL: all of it) -- floor, walls, table tops.  A plane is the plane of the SHELL's voxel
 * centres: up to one voxel behind the surface, and nothing corrects that.
 *   planes          params NULL: K 15, refine 1, max_planes 64, peak_gap 2, angle 20 degrees, separation = angle, bins of
 *                   1 voxel, a band of 2 voxels, min_votes max(50, records / 200) -- policy, not measurements.  Outputs,
 *                   NULL = not wanted: the box and its pose (box voxel -> world), the four counters of the surface pass,
 *                   the threshold applied, and up to `capacity` planes ordered by count (ties to the lower label), in BOX
 *                   VOXEL coordinates; *count is the number found.  Waits 3 + refine times.  At most max(2^16, voxels / 8)
 *                   records are kept: counters[1] > counters[2] says that the surface held more.
 *   copy_plane_labels  the records of the last call and their labels (i16, the `label` of a plane, -1: none), the first
 *                   min(capacity, counters[2]) of them; labels are all -1 where no plane was found.
 *   plane_directions / plane_offsets / plane_fit   need no device and no handle: the host steps between the stages,
 *                   float64 in the fixed operation order of include/emf_hip.h.  directions: dirs = 3 doubles, bins_out
 *                   and votes_out one entry per direction, capacity EMF_PLANE_MAX_DIRS; returns the count in *count.
 *                   offsets: the frame (lo, S, inv_bin, shift) of one direction and, with a row of S votes, its peaks
 *                   (slot, votes), at most `capacity`.  fit: one plane from its moments and its seed.
 * Refused (EMF_E_ARG) on the sharded path; changes nothing of the session and nothing goes into a checkpoint. */
int emf_fusion_planes(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const emf_plane_params_t* params,
                      int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3], uint32_t counters[4], uint32_t* min_votes,
                      emf_plane_t* planes, int32_t capacity, int32_t* count);
int emf_fusion_copy_plane_labels(emf_fusion_t* h, emf_plane_voxel_t* records, int16_t* labels, int64_t capacity);
/*   set_planes_output  setup_output's exp_planes and ground_up="floor", as an entry of its own so that the existing entries
 *                   keep their signatures.  on: emf_fusion_write_results also writes planes.txt of the whole background
 *                   (angle_deg in (0, 90], min_votes <= 0: the policy above; the other parameters at their defaults; kinds
 *                   relative to minus the background's y axis): a comment line, then one line per plane ordered by count:
 *                   kind count, then in %.9g the world normal (3), d, the point (3), the thickness in metres, then the
 *                   bounds lo (3) hi (3) in voxels.  ground_up_floor: the ground output (emf_fusion_set_ground_output)
 *                   takes the normal of the floor the plane search finds as up; write_results fails where there is none.
 *                   Both off: the set of result files and every byte of them as before. */
int emf_fusion_set_planes_output(emf_fusion_t* h, int on, double angle_deg, int64_t min_votes, int ground_up_floor);
int emf_fusion_plane_directions(const uint32_t* bins, int32_t K, uint32_t min_votes, double separation_deg, double* dirs,
                                int32_t* bins_out, uint32_t* votes_out, int32_t* count);
int emf_fusion_plane_offsets(const double n[3], const int32_t box_size[3], double bin_vox, double* lo, int64_t* slots,
                             double* inv_bin, double* shift, const uint32_t* row, uint32_t min_votes, int32_t peak_gap,
                             int32_t* peak_slots, uint32_t* peak_votes, int32_t capacity, int32_t* count);
int emf_fusion_plane_fit(const emf_plane_moments_t* moments, const double seed_n[3], double seed_d, emf_plane_t* plane);
/* Plane patches (include/emf_hip.h "Planes", stage 4; new behaviour, opt-in): the planes of the last
 * emf_fusion_planes split into connected surfaces, so that two tables of one height are two patches of one plane.
 *   plane_patches   works on what the last emf_fusion_planes left on the device; EMF_E_ARG where there is none.  reach in
 *                   1 .. EMF_PLANE_MAX_REACH (above: EMF_E_LIMIT), min_count >= 1.  counters[3]: kept patches, all
 *                   patches, records with a label.  patches: the kept ones in ascending id order, the first
 *                   min(capacity, kept) of them; *count = kept.  patch.plane is the `label` of its plane.  Waits twice.
 *   copy_plane_patch_ids  one i32 per record of the last emf_fusion_planes (the order of copy_plane_labels): the id of the
 *                   record's patch under the last plane_patches, -1 for none; the first min(capacity, counters[2]).
 *   plane_patch_rect / plane_support   need no device and no handle: float64 in the fixed operation order of
 *                   include/emf_hip.h.  rect: the fit, the rectangle and the fill of one patch from its plane, box voxel
 *                   coordinates.  support: one oriented box (centre, three unit row axes, half sizes) against one patch
 *                   (plane n, d; rectangle centre, two row axes, half sizes), all in world metres:
 *                   *s = (n . c - d) - sum_k |n . A_k| * h_k, the height of the box's lowest point above the plane, every
 *                   dot product left to right; *over = 1 iff |(c - centre) . axis_j| <= half_j + margin for j = 0, 1.
 *   set_plane_patches_output  with emf_fusion_set_planes_output on, planes.txt gains after each plane's line one line per
 *                   patch of that plane, by count descending, ties to the lower id: "patch" id count, then in %.9g the
 *                   world point of its own fit (3), the four corners (12) and fill; and, with the shapes output on as
 *                   well, after all planes one line "support <object id> <plane> <patch id> <s>" per object that rests on
 *                   a patch (gap 0.05 m, margin 0): plane is the index of the plane's line.  min_count <= 0:
 *                   max(25, min_votes / 4) of the planes.  Off: every byte of every result file as before.
 * Refused (EMF_E_ARG) on the sharded path; changes nothing of the session and nothing goes into a checkpoint. */
int emf_fusion_plane_patches(emf_fusion_t* h, int32_t reach, int64_t min_count, uint32_t counters[3], emf_plane_patch_t* patches,
                             int32_t capacity, int32_t* count);
int emf_fusion_copy_plane_patch_ids(emf_fusion_t* h, int32_t* ids, int64_t capacity);
int emf_fusion_plane_patch_rect(const emf_plane_t* plane, const emf_plane_patch_t* patch, emf_plane_patch_rect_t* rect);
int emf_fusion_plane_support(const double n[3], double d, const double center[3], const double axes[6], const double half[2],
                             const double box_center[3], const double box_axes[9], const double box_half[3], double margin,
                             double* s, int32_t* over);
int emf_fusion_set_plane_patches_output(emf_fusion_t* h, int on, int32_t reach, int64_t min_count);
/* Ground map (include/emf_hip.h "Ground map"; new behaviour, opt-in): where a robot that drives on a
 * floor can stand -- a 2-D traversability map with a floor height per cell, projected on the device from the occupancy
 * classes of a box of the background (box_lo / box_size NULL: all of it) with every live object not in exclude_ids
 * stamped.
 *   ground_map      up: the world direction that is up; cell, bin: the side of a ground cell and the height of a bin in
 *                   metres; reference: a world point; (band_lo, band_hi): the height band in metres relative to the
 *                   reference along up; robot_bins >= 1: the FREE bins a floor needs above it; max_step_bins >= 0: a
 *                   larger difference between the floors of neighbouring cells is an obstacle.  Outputs, NULL = not
 *                   wanted: the box, the frame (G, W, H, B), ground_pose (12 doubles: R row-major with the ground axes
 *                   u, v, h as columns, then t; ground metres -> world), and cells / classes for `capacity` cells each
 *                   (fewer than W * H with a non-NULL output: EMF_E_ARG; emf_fusion_ground_frame gives W and H before
 *                   the call, emf_fusion_copy_ground_map copies after it).  The arrays stay on the device as the input
 *                   of 2-D distance, frontier and plan entries with size (W, H, 1).  One wait.  Changes nothing of the
 *                   session; EMF_E_ARG on the sharded path.
 *   copy_ground_map the cells (W * H emf_ground_cell_t) and the classes (W * H bytes, v-major) of the last ground_map.
 *   ground_classes_ptr  the device pointers of those classes and cells (NULL = not wanted), valid until the next
 *                   ground_map: what Fusion.ground_plan hands to the 2-D entries of include/emf_hip.h.
 *   ground_frame    needs no device and no handle: the frame and the ground pose of a box (box_lo, box_size) of a
 *                   background of resolution bg_res, voxel size and pose (R, t: volume -> world), float64 in the fixed
 *                   operation order of include/emf_hip.h.  A zero or non-finite up, a cell or bin that is not positive,
 *                   an empty band: EMF_E_ARG; W or H above EMF_DF_MAX_AXIS or more than EMF_GROUND_MAX_BINS bins:
 *                   EMF_E_LIMIT.
 *   set_ground_output  setup_output's exp_ground_map, as an entry of its own: emf_fusion_write_results also writes
 *                   ground.bin -- the W * H class bytes, then the W * H cell records -- and ground.txt -- a comment
 *                   line, then "map W H", "bins B robot R step S", "cell c bin b", three lines "G ..." of four values
 *                   and four lines "pose ..." of three (the rows of R, then t), floats in %.9g -- of the whole
 *                   background with the given parameters; the reference is the camera position.  on == 0: the set of
 *                   result files and every byte of them as before. */
int emf_fusion_ground_map(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* exclude_ids,
                          int32_t num_exclude, const double up[3], double cell, double bin, const double reference[3],
                          double band_lo, double band_hi, int32_t robot_bins, int32_t max_step_bins, int32_t lo_out[3],
                          int32_t size_out[3], emf_ground_frame_t* frame, double ground_pose[12], emf_ground_cell_t* cells,
                          uint8_t* classes, int64_t capacity);
int emf_fusion_copy_ground_map(emf_fusion_t* h, emf_ground_cell_t* cells, uint8_t* classes);
int emf_fusion_ground_classes_ptr(emf_fusion_t* h, void** classes_dev, void** cells_dev);
int emf_fusion_ground_frame(const int32_t box_lo[3], const int32_t box_size[3], const int32_t bg_res[3], float voxel_size,
                            const float R[9], const float t[3], const double up[3], double cell, double bin,
                            const double reference[3], double band_lo, double band_hi, emf_ground_frame_t* frame,
                            double ground_pose[12]);
int emf_fusion_set_ground_output(emf_fusion_t* h, int on, const double up[3], double cell, double bin, double band_lo,
                                 double band_hi, double robot_height, double max_step);
/* Remember what rolls out (new behaviour, off by default; with it off no launch, no output byte and no
 * checkpoint byte changes).  With the store on, the whole integration tiles (32 x 8 x 8) that a roll moves out of the
 * background go to host memory as the bytes they are, after the slabs are retired; the tiles that a later roll moves
 * back in are taken out of the store and written into the rolled volume (tsdf, weights, colour, sign and unseen-tile
 * entries) before its two copies are made equal, so a camera that returns finds what it left.
 *   set_background_store   max_bytes: the budget (0: the default, 1 GiB -- a cap, not a measurement).  A tile costs 40
 *                      bytes plus its literal arrays; a spill that pushes the store past the budget drops whole
 *                      spills, the oldest first.  Turning the store off drops what it holds.  Refused on the sharded
 *                      path, as follow is.  With the store on, a roll whose shift, background resolution or
 *                      background origin is not a multiple of the tile is refused (EMF_E_ARG, nothing changed); every
 *                      roll of the policy passes.  retired_slabs stays the chronological log it is: a region that
 *                      leaves twice is logged (and written to bg_retired/) twice.
 *   background_store_info  out[5]: tiles held, bytes held, tiles spilled, tiles restored, tiles evicted. */
int emf_fusion_set_background_store(emf_fusion_t* h, int on, uint64_t max_bytes);
int emf_fusion_background_store_info(emf_fusion_t* h, uint64_t out[5]);

/* Create an object volume (edge vol_size metres, obj_res voxels) centred at `center` in world
 * coordinates; every rank issues the same calls.  *id_out = object id (1-based). */
int emf_fusion_add_object(emf_fusion_t* h, const float center[3], float vol_size, int32_t* id_out);

/* Run one frame of the schedule (emf::EMFusion::processFrame) on a depth map resident in device
 * memory.  obj_R / obj_t: nposes x 9 / nposes x 3 floats for the object ids in pose_ids.
 * masks: device u8 0/1 images for the ids in mask_ids; used when run_masks != 0. */
int emf_fusion_process_frame(emf_fusion_t* h, const emf_image_t* depth_dev, const float cam_R[9],
                             const float cam_t[3], int nposes, const int32_t* pose_ids,
                             const float* obj_R, const float* obj_t, int nmasks,
                             const int32_t* mask_ids, const emf_image_t* masks, int run_masks);

/* Tracking (SURVEY f-1).  set_tracking: from the next frame on, process_frame ignores the supplied
 * camera pose / object poses and tracks them instead (EMFusion::performTracking); frame 0 always
 * takes the supplied poses.  get_pose: id 0 = camera -> world, else object volume -> world.
 * track_result: iterations / accepted / converged / error of the last run of model id. */
int emf_fusion_set_tracking(emf_fusion_t* h, int track_camera, int track_objects);
/* Object creation / matching from a device instance mask (u8 W x H, non-zero = inside) of the
 * current frame (EMFusion::initNewObjVolume / matchSegmentation, SURVEY f-3).  *id = new / matched
 * object id, or -1.  *iou is in/out for match (start it at 0). */
int emf_fusion_create_object_from_mask(emf_fusion_t* h, const emf_image_t* mask, int32_t* id);
/* In-frame creation, as the reference does it (initOrMatchObjs before integrateDepth): the masks
 * queued here are run through initNewObjVolume by the NEXT process_frame, after its raycast and
 * before its integration; last_created returns the ids (-1 = rejected), in queue order. */
int emf_fusion_queue_new_object_masks(emf_fusion_t* h, int n, const emf_image_t* masks);
/* The instance masks of a Mask R-CNN frame for the NEXT process_frame: it runs the reference's
 * initOrMatchObjs on them after its raycast (match, resolve double matches, carve and spawn the
 * unmatched -- the masks are MODIFIED in place), integrates the matched masks and, if clean-up is
 * on, deletes spurious objects.  last_mask_assignment: the object id each mask ended up with. */
int emf_fusion_queue_instance_masks(emf_fusion_t* h, int n, const emf_image_t* masks);
/* The class scores that go with the queued instance masks (n x num_classes doubles, mask-major;
 * MaskRCNN::getScores): a matched object accumulates them.  object_class: index of its largest
 * accumulated score (0 before any).  set_ignore_person: Params.ignore_person (config/tum.cfg) --
 * "person" objects (COCO class 1) stay out of renderings and mesh files. */
int emf_fusion_queue_instance_scores(emf_fusion_t* h, int n, int num_classes, const double* scores);
int emf_fusion_object_class(emf_fusion_t* h, int id, int32_t* class_id);
int emf_fusion_set_ignore_person(emf_fusion_t* h, int on);
/* geometry of an object volume as it is now (objects are created and resized inside frames): resolution, voxel size,
 * truncation distance [m], existence probability (ObjTSDF::getExProb); any output pointer may be NULL */
int emf_fusion_object_info(emf_fusion_t* h, int id, int32_t res[3], float* voxel_size, float* truncdist, float* existence);
int emf_fusion_last_mask_assignment(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count);
int emf_fusion_last_created(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count);
int emf_fusion_match_mask(emf_fusion_t* h, const emf_image_t* mask, int32_t* id, float* iou);
/* EMFusion::updateObj + ObjTSDF::resize (EMFusion.cpp:827-863, ObjTSDF.cpp:80-165) for one object and
 * one mask of the current frame's points: the volume grows / recentres if the 10th..90th percentile
 * box of (surface vertices + masked points) leaves it.  offset: the centre shift in the old volume
 * frame (all 0: nothing changed).  process_frame does this for every matched instance mask. */
int emf_fusion_update_object(emf_fusion_t* h, int id, const emf_image_t* mask, float offset[3]);
/* From the next frame on, run the reference's cleanUpObjs at the end of every frame (delete objects
 * that are not visible, whose association mass does not fit their mask, or -- on mask frames --
 * whose existence probability is low); last_deleted lists the ids the last frame removed. */
int emf_fusion_set_cleanup(emf_fusion_t* h, int on);
int emf_fusion_last_deleted(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count);
/* Results in the reference's formats (SURVEY f-4, mesh-free part): enable the per-frame pose log
 * before processing, then write <dir>/poses-cam.txt, poses-<id>.txt (TUM: "frame tx ty tz qx qy qz
 * qw") and, if volumes != 0, <dir>/tsdfs/{bg_tsdf,tsdf_<id>,weights_<id>,fgProbs_<id>}.bin
 * (int32 res[3], uint64 element size, float voxel size, voxels).  emf_io_* are host-only helpers. */
/* TSDF::getMesh / ObjTSDF::getMesh of model `id` (0 = background): extract runs marching cubes and
 * keeps the result in the handle, copy hands it out (vertices, normals: 3 floats per vertex;
 * triangles: 4 int32 per triangle = 3, i0, i1, i2).  emf_io_write_mesh writes the reference's PLY. */
int emf_fusion_extract_mesh(emf_fusion_t* h, int id, uint32_t* num_vertices, uint32_t* num_triangles);
int emf_fusion_copy_mesh(emf_fusion_t* h, float* vertices, float* normals, int32_t* triangles);
/* EMFusion::extractMeshes: the meshes of n models at once (ids[k]: 0 = background or a live object of this rank;
 * emf_fusion_object_ids lists them), one pass over the model table; the same bytes as emf_fusion_extract_mesh per id.
 * counts: 2 n uint32 (vertices, triangles of model k).  copy hands them out concatenated in list order (NULL: not
 * wanted), each model's triangle indices local to its own vertices. */
int emf_fusion_extract_meshes(emf_fusion_t* h, const int32_t* ids, int n, uint32_t* counts);
int emf_fusion_copy_meshes(emf_fusion_t* h, float* vertices, float* normals, int32_t* triangles);
/* The vertex colours (3 bytes per vertex, RGB; emf_hip_meshColors) of the mesh / meshes the last emf_fusion_extract_mesh
 * / emf_fusion_extract_meshes kept, in copy_mesh's / copy_meshes' vertex order.  EMF_E_ARG unless colour was on
 * (emf_fusion_set_color) when the mesh was extracted. */
int emf_fusion_copy_mesh_colors(emf_fusion_t* h, uint8_t* colors);
int emf_fusion_copy_meshes_colors(emf_fusion_t* h, uint8_t* colors);
int emf_io_write_mesh(const char* filename, uint32_t num_vertices, const float* vertices,
                      const float* normals, uint32_t num_triangles, const int32_t* triangles);
/* The same PLY with `property uchar red / green / blue` behind the normals (colors: 3 bytes per vertex) -- what
 * write_results writes for mesh_*.ply and frame_meshes with colour on (emf_fusion_set_color); with colour off its files
 * are emf_io_write_mesh's, byte for byte. */
int emf_io_write_mesh_colors(const char* filename, uint32_t num_vertices, const float* vertices, const float* normals,
                             const uint8_t* colors, uint32_t num_triangles, const int32_t* triangles);
/* EMFusion::render (EMFusion.cpp:131-160): Phong-shaded RGB view of the models, width*height*3 bytes
 * into host memory; color_map (may be NULL) receives the 256 x RGB label colours. */
int emf_fusion_render(emf_fusion_t* h, uint8_t* rgb, uint8_t* color_map);
/* EMFusion::renderView: the map seen from a free viewpoint (the reference's --3d-vis view, ray-cast): viewer -> world
 * (R row-major, t; OpenCV camera: +z forward, +y down), intrinsics K, width x height.  Host outputs, NULL = not
 * wanted (rgb is required): rgb width*height*3 bytes, raylengths f32, seg u8.  Ordered after the last frame; changes
 * nothing of the frame path.  EMF_E_ARG on the sharded path. */
int emf_fusion_render_view(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                           int32_t height, uint8_t* rgb, float* raylengths, uint8_t* seg);
/* EMFusion::set3dView: from now on render() also renders this view and, with setup_output's log on, keeps it for
 * write_results' mesh_vis_out/%04d.png.  emf_fusion_clear_3d_view turns it off. */
int emf_fusion_set_3d_view(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                           int32_t height);
int emf_fusion_clear_3d_view(emf_fusion_t* h);
/* Shading of the views: EMF_SHADE_LABEL (default; the bytes of emf_fusion_render_view) paints every model in its label
 * colour, EMF_SHADE_COLOR gives each hit pixel the colour of the voxel nearest to its vertex in the model the
 * segmentation names (no interpolation; voxels nobody coloured fall back to the label colour) and feeds it to the same
 * Phong terms -- a pixel pass (emf_hip_sampleColor, emf_hip_renderPhongColor) behind the unchanged view kernel.
 * EMF_SHADE_COLOR needs emf_fusion_set_color(on): EMF_E_ARG otherwise.  set_3d_view_shading: the shading of the
 * view of emf_fusion_set_3d_view. */
enum emf_fusion_shading { EMF_SHADE_LABEL = 0, EMF_SHADE_COLOR = 1 };
int emf_fusion_render_view_shaded(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                                  int32_t height, int shading, uint8_t* rgb, float* raylengths, uint8_t* seg);
int emf_fusion_set_3d_view_shading(emf_fusion_t* h, int shading);
/* Multi-GPU: broadcast the depth image of every frame from rank `root` (whose process_frame argument
 * is the source; on the other ranks it is the destination and must have the same size and pitch)
 * before anything else runs.  root < 0 (default): every rank is handed the frame itself. */
int emf_fusion_set_depth_broadcast(emf_fusion_t* h, int root);
int emf_fusion_enable_pose_log(emf_fusion_t* h, int on);
/* EMFusion::setupOutput (EMFusion.cpp:243-247): log on; exp_vols != 0 also keeps the volumes of
 * objects deleted during the run for write_results.  exp_frame_meshes != 0 meshes the background and every live
 * object not hidden by ignore_person at the end of every frame (one pass over the table) and keeps the meshes for
 * write_results' frame_meshes/bg/%04d.ply and frame_meshes/<id>/%04d.ply; EMF_E_ARG on the sharded path. */
int emf_fusion_setup_output(emf_fusion_t* h, int exp_frame_meshes, int exp_vols);
/* EMFusion::writeResults (EMFusion.cpp:248-292): pose files, mesh_bg.ply and mesh_<id>.ply always;
 * tsdfs/ *.bin only if volumes != 0 or setup_output asked for them. */
int emf_fusion_write_results(emf_fusion_t* h, const char* dir, int volumes);
int emf_io_write_volume(const char* filename, const float* voxels, const int32_t res[3], float voxel_size);
int emf_io_write_pose_file(const char* filename, int n, const int32_t* frames, const float* R,
                           const float* t);
/* Undo the PNG scan-line filters (PNG specification 9.2; what cv::imread does inside
 * TUMRGBDReader.cpp for the depth images): rows = height x (1 + stride) bytes, each line preceded by
 * its filter type 0..4; out = height x stride reconstructed bytes; bpp = bytes per pixel (1 or 2: the depth images,
 * 3 or 4: 8-bit RGB / RGBA colour images). */
int emf_io_png_unfilter(const uint8_t* rows, int height, int stride, int bpp, uint8_t* out);
/* The C++ dataset readers behind apps/emfusion_synth --sequence (core/Readers.hpp; reference
 * src/utils/TUMRGBDReader.cpp, src/core/MaskRCNN.cpp:250-282), exposed for tests and FFI users.
 *   read_depth_png     an 8/16-bit grayscale PNG as float = raw * scale (TUM: 1 / 5000); out may be NULL to ask
 *                      for the size only; capacity in floats
 *   tum_associations   entry `index` of <file>: depth file name and time stamp; *count = number of entries
 *   load_preproc_masks a Mask%04d.plk of the reference's preprocessing: *n instances of *width x *height; masks
 *                      (n * height * width bytes, 0/1), boxes (n * 4) and scores (n * *nscores) are filled when
 *                      not NULL and large enough (mask_capacity in bytes, score_capacity in doubles) */
int emf_io_read_depth_png(const char* path, float scale, float* out, size_t capacity, int32_t* width, int32_t* height);
/*   read_color_png     an 8-bit RGB or RGBA (alpha dropped) PNG as width x height x 3 bytes (emf::readPngColor: the
 *                      colour images of the TUM / Co-Fusion sequences); palette, 16-bit, grayscale, interlaced and
 *                      oversized files are rejected with a message; out may be NULL to ask for the size only; capacity
 *                      in bytes */
int emf_io_read_color_png(const char* path, uint8_t* out, size_t capacity, int32_t* width, int32_t* height);
/*   read_exr           one channel (NULL / "": the only one, else the first of Z, Y, R) of a single-part scan-line
 *                      OpenEXR file as float (emf::readExr; reference src/utils/ImageReader.cpp:105-110 reads its
 *                      depth files with cv::imread); out may be NULL to ask for the size only
 *   image_reader       emf::ImageReader on <base><colordir> / <base><depthdir> (ColorNNNN.png / DepthNNNN.exr):
 *                      number of frames and first index; the reference's error messages for unusable directories */
/*   load_config        emf::loadConfigFile (core/Config.hpp): the reference's config files (config/default.cfg ...;
 *                      apps/EM-Fusion.cpp:268-371) applied to the reference defaults, then -- if calibration is not
 *                      NULL and the file exists -- <dir>/calibration.txt (EM-Fusion.cpp:399-410); the fields the
 *                      volumetric path reads come back in *p (may be NULL), every configurable field as
 *                      "Section.key = value" lines in dump (may be NULL; truncated to dump_capacity - 1 characters) */
int emf_io_load_config(const char* path, const char* calibration, emf_fusion_params_t* p, char* dump, size_t dump_capacity);
int emf_io_read_exr(const char* path, const char* channel, float* out, size_t capacity, int32_t* width, int32_t* height);
int emf_io_image_reader(const char* base, const char* colordir, const char* depthdir, int32_t* num_frames, int32_t* first);
int emf_io_tum_associations(const char* file, int index, char* depth_name, int name_capacity, double* stamp, int32_t* count);
/* capacities in elements (bytes of masks, doubles of boxes and scores); an output whose capacity is too small is not written */
int emf_io_load_preproc_masks(const char* path, int32_t* n, int32_t* width, int32_t* height, uint8_t* masks,
                              size_t mask_capacity, double* boxes, size_t box_capacity, double* scores, size_t score_capacity,
                              int32_t* nscores);
/* from the next frame on, filter the incoming depth (EMFusion::preprocessDepth, SURVEY f-2) */
int emf_fusion_set_preprocess(emf_fusion_t* h, int on);
int emf_fusion_get_pose(emf_fusion_t* h, int id, float R[9], float t[3]);
int emf_fusion_track_result(emf_fusion_t* h, int id, int32_t* iterations, int32_t* accepted,
                            int32_t* converged, float* error);

/* Individual stages (emf::EMFusion::{computeAssociationWeights, raycast, integrateDepth}) acting
 * on the state left by the last process_frame; for stage-level tests and profiling. */
int emf_fusion_stage_estep(emf_fusion_t* h);
int emf_fusion_stage_raycast(emf_fusion_t* h);
int emf_fusion_stage_integrate(emf_fusion_t* h);

int emf_fusion_synchronize(emf_fusion_t* h);
int emf_fusion_enable_timings(emf_fusion_t* h, int on);
int emf_fusion_last_timings(emf_fusion_t* h, emf_frame_timings_t* out);
/* counters: [0] march samples, [1] hits, [2] samples that read the volume, [3] samples
 * fast-forwarded inside uniform bricks -- accumulated by raycast while enabled */
int emf_fusion_enable_raycast_stats(emf_fusion_t* h, int on);
int emf_fusion_raycast_stats(emf_fusion_t* h, uint64_t counters[4]);

/* Per-launch HIP-event timers: every kernel launch of the schedule is bracketed by an event pair
 * on the stream it is launched on.  enable(max_launches) allocates the pool (0 = off); collect()
 * must be called with the device idle (after emf_fusion_synchronize). */
enum emf_kernel_kind {
    EMF_K_POINTS = 0, EMF_K_ASSOC, EMF_K_NORMALIZE, EMF_K_RAYCAST, EMF_K_COMPOSITE,
    EMF_K_INTEGRATE, EMF_K_GRADS, EMF_K_FGBG, EMF_K_TRACK, EMF_K_INTEGRATE_BG, EMF_K_NUM_KINDS
};
typedef struct emf_kernel_summary {
    uint64_t launches;
    double total_ms;
    double units; /* voxels (volume sweeps) or pixels (image kernels), summed over launches */
} emf_kernel_summary_t;
int emf_fusion_kernel_timers_enable(emf_fusion_t* h, uint64_t max_launches);
int emf_fusion_kernel_timers_clear(emf_fusion_t* h);
/* restrict the event pairs to the kinds whose bit (1 << emf_kernel_kind) is set; default all */
int emf_fusion_kernel_timers_select(emf_fusion_t* h, uint32_t kind_mask);
/* Bracket only every `every`-th launch of a kind (1 = all): the event records themselves cost the frame. */
int emf_fusion_kernel_timers_stride(emf_fusion_t* h, uint32_t every);
int emf_fusion_kernel_timers_collect(emf_fusion_t* h, emf_kernel_summary_t out[EMF_K_NUM_KINDS],
                                     uint64_t* dropped);

/* Device views of per-frame images / volumes (valid until the next frame / destroy).
 * obj_id is ignored unless the selector is per object; 0 selects the background volume. */
int emf_fusion_get_image(emf_fusion_t* h, int which, int obj_id, emf_image_t* view);
int emf_fusion_get_volume(emf_fusion_t* h, int which, int obj_id, void** dev_ptr, int32_t res[3]);
/* ids of the objects classified visible by the last raycast; returns count in *n (<= cap) */
int emf_fusion_visible_objects(emf_fusion_t* h, int32_t* ids, int cap, int* n);
/* ids of all live objects of the job in creation order (deleted ones are gone); count in *n (<= cap) */
int emf_fusion_object_ids(emf_fusion_t* h, int32_t* ids, int cap, int* n);
int emf_fusion_frame_index(emf_fusion_t* h);
/* 1 if the background's integration runs out of place beside the raycast (double-buffered background) */
int emf_fusion_background_overlap(emf_fusion_t* h);
/* Which path the frames run on: 0 = per-volume (one stream per volume, host visibility gate: EMF_PER_VOLUME=1, materialised
 * gradients), k >= 1 = batched with k launches per stage (1 up to EMF_MAX_BATCH models, then one per chunk of the table) */
int emf_fusion_batched_chunks(emf_fusion_t* h);
/* Host time emf_fusion_process_rgbd has spent so far handing depth maps to the device -- staging memcpy + enqueue with the
 * double-buffered pinned upload (default), the blocking pageable copy with EMF_ASYNC_UPLOAD=0 -- and the frames it covers */
int emf_fusion_upload_host_time(emf_fusion_t* h, double* seconds, uint64_t* frames);
/* 1 if this rank holds object id's volume */
int emf_fusion_owns_object(emf_fusion_t* h, int obj_id);

/* ---- checkpoint and resume (emfusion_amd/csrc/core/Checkpoint.cpp holds the file format) ----
 * save_checkpoint  waits for this instance's work, then writes its primary state -- parameters, frame count, camera
 *                  pose, object table with existence and class bookkeeping, pose logs, the meshes kept of deleted
 *                  objects and every volume (tsdf, weights, fg/bg counts, colour), packed losslessly on the device
 *                  (include/emf_hip.h "Packed buffers") -- to <path>.tmp and renames it to path.  Changes nothing in
 *                  the session.  stats may be NULL.  Format version 1; 2 once the background has rolled; 3 with the
 *                  background store on (the store travels with the file; checkpoint_info: "stored_tiles",
 *                  "stored_bytes").
 * load_checkpoint  acts as emf_fusion_reset followed by the restore; allowed at any time.  EMF_E_ARG, with the
 *                  session left as it was, if the file was saved with another frame size, intrinsics, background
 *                  resolution, voxel size or TSDF parameters, or if its magic, version, header checksum, section
 *                  lengths or end marker are wrong (a truncated file).  The derived state (fgprobs / fgmask, sign
 *                  maps, tile lists, brick flags, the back copy) is rebuilt; the switches of the emf_fusion_set_*
 *                  calls and emf_fusion_enable_pose_log / setup_output are the caller's to set again, as at start.
 *                  A restored session continues with the bytes of one that was never interrupted.
 * Both return EMF_E_ARG on the sharded path.
 * checkpoint_info  needs no device and no handle: the parameters, frame index, object ids and resolutions, colour
 *                  flag and per-record chunk counts of a file as JSON ({"version", "file_bytes", "frame_index",
 *                  "next_id", "color", "params": {...}, "objects": [{"id", "res", ...}], "kept_meshes", "logged_frames",
 *                  "records": [{"id", "which", "offset", "bytes", "packed_bytes", "chunks": [zero, uniform, literal]}]});
 *                  the same checks as load_checkpoint's, EMF_E_ARG if they fail or `capacity` is too small.
 * create_from_checkpoint  the instance emf_fusion_create would build from the file's parameters (every field of
 *                  emf::Params, also those emf_fusion_params_t does not carry), with the file loaded; params_out
 *                  (may be NULL) receives the subset the struct carries. */
typedef struct emf_checkpoint_stats {
    uint64_t raw_bytes, file_bytes; /* bytes of the packed device buffers; size of the file */
    uint64_t chunks[3];             /* 1 KiB chunks per class: zero, uniform, literal */
    double ms_classify, ms_gather;  /* device time: classify + rank, gather */
    double ms_copy, ms_file, ms_total; /* host time: device-to-host copies, file writes, the whole call */
    uint32_t records, reserved;
} emf_checkpoint_stats_t;
int emf_fusion_save_checkpoint(emf_fusion_t* h, const char* path, emf_checkpoint_stats_t* stats);
int emf_fusion_load_checkpoint(emf_fusion_t* h, const char* path);
int emf_fusion_checkpoint_info(const char* path, char* json, size_t capacity);
int emf_fusion_create_from_checkpoint(const char* path, emf_comm_t* comm, emf_fusion_params_t* params_out,
                                      emf_fusion_t** out);

/* ---- RCCL communicator for the object-sharded multi-GPU path (one process per GPU) ---- */
#define EMF_COMM_UNIQUE_ID_BYTES 128
int emf_comm_unique_id(void* out128);
int emf_comm_create(const void* unique_id128, int rank, int world, emf_comm_t** out);
void emf_comm_destroy(emf_comm_t* c);
/* Rehearsal backend: `world` communicators of one process sharing one GPU, one per host thread (RCCL
 * refuses two ranks on a device).  N emf_fusion handles driven from N threads then run the code path
 * of an N-GPU job; collectives are staged through host memory.  out: array of `world` handles. */
int emf_comm_create_local_group(int world, emf_comm_t** out);
/* Direct peer-write exchanges (include/emf_hip.h "direct peer-write exchanges"): no library collective,
 * three small launches per exchange.  slot_bytes bounds one message (W * H * 8 for the hit keys).
 *   ..._peer_local_group: `world` (<= 8) ranks of one process sharing a GPU, for N handles on N threads;
 *   ..._peer            : one process per rank; the receive buffers are mapped into every peer through
 *                         hipIpc*, the 128 handle bytes per rank travel through `all_gather` (0 = success;
 *                         all[r * bytes ...] := rank r's block), e.g. torch.distributed over gloo.
 * Untested on xGMI (no multi-GPU box in the build environment); exercised on one GPU.
 * Image sizes: the transport moves whole 16-byte units, so emf_fusion_create* refuses such a communicator with
 * EMF_E_SHAPE unless width * height % 4 == 0 (% 16 with slots below emf_hip_peerRaycastSlotBytes, which exchange
 * unfused) -- on every rank alike, before any exchange.  The other transports take any size. */
typedef int (*emf_allgather_fn)(void* user, const void* mine, size_t bytes, void* all);
int emf_comm_create_peer_local_group(int world, size_t slot_bytes, emf_comm_t** out);
int emf_comm_create_peer(int rank, int world, size_t slot_bytes, emf_allgather_fn all_gather, void* user,
                         emf_comm_t** out);
/* The four exchanges of a communicator, callable on their own (tests of a transport without a frame around
 * it).  dev pointers on the current device, `stream` a hipStream_t or NULL. */
int emf_comm_all_reduce_sum_f32(emf_comm_t* c, float* dev, size_t count, void* stream);
int emf_comm_all_reduce_min_u64(emf_comm_t* c, uint64_t* dev, size_t count, void* stream);
int emf_comm_broadcast(emf_comm_t* c, void* dev, size_t bytes, int root, void* stream);
int emf_comm_gather_row_bands(emf_comm_t* c, void* dev, size_t bytes_per_row, int band_rows, int total_rows,
                              void* stream);
/* Latency model around another communicator (which must outlive the new handle's users but may be
 * destroyed after it): every exchange -- a grouped one counts once -- first keeps its stream busy for
 * `microseconds`.  With a 1-rank RCCL communicator and EMF_FORCE_SHARDED=1 it measures, on one GPU, how
 * much per-collective latency the frame's schedule hides.  emf_comm_exchanges: exchanges issued so far
 * through a delayed communicator (0 for the others). */
int emf_comm_create_delayed(emf_comm_t* inner, int microseconds, emf_comm_t** out);
int emf_comm_exchanges(emf_comm_t* c, uint64_t* out);
/* What the transport reports about this rank (asked of RCCL: ncclCommCount / ncclCommUserRank / ncclCommCuDevice /
 * ncclGetVersion, + the device's PCI bus id), as a JSON object in `json` (cap >= 512): {"transport", "ranks", "rank",
 * "device", "pci_bus_id", "version"}.  bench.py --gpus N gathers one per rank into its line. */
int emf_comm_describe(emf_comm_t* c, char* json, size_t cap);
/* Rehearsal backend, one process per rank: collectives are staged through host memory and handed to
 * the caller's functions (0 = success), e.g. torch.distributed over gloo -- lets the N-rank job run on
 * a box with fewer than N GPUs (bench.py --comm gloo). */
typedef struct emf_comm_callbacks {
    int32_t rank, world;
    int (*all_reduce_sum_f32)(void* user, float* host, size_t count);
    int (*all_reduce_min_u64)(void* user, uint64_t* host, size_t count);
    int (*broadcast)(void* user, void* host, size_t bytes, int root);
    void* user;
} emf_comm_callbacks_t;
int emf_comm_create_host_staged(const emf_comm_callbacks_t* cb, emf_comm_t** out);

/* ---- synthetic RGB-D stream (host side, replaces the dataset readers) ---- */
int emf_synth_create(int width, int height, const float K[9], int num_spheres, uint64_t seed,
                     float noise_sigma, float dropout, emf_synth_t** out);
void emf_synth_destroy(emf_synth_t* s);
/* depth: HOST float[w*h]; ids: HOST u8[w*h] or NULL */
int emf_synth_render(emf_synth_t* s, int frame, float* depth, uint8_t* ids);
int emf_synth_camera_pose(emf_synth_t* s, int frame, float R[9], float t[3]);
int emf_synth_sphere(emf_synth_t* s, int k, int frame, float center[3], float* radius,
                     float* volume_size);

#ifdef __cplusplus
}
#endif
#endif /* EMF_FUSION_H */
