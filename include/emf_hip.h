/*
 * emf_hip.h -- C ABI of the MI355X-native (gfx950) EM-Fusion volumetric hot path.
 *
 * This is the drop-in boundary.  Each entry point replaces either one of
 * the reference's kernel-wrapper free functions (namespace emf::cuda::{TSDF,ObjTSDF,EMFusion},
 * declared in include/EMFusion/core/cuda/{TSDF,ObjTSDF,EMFusion}.cuh) or one chain of
 * OpenCV-CUDA element-wise launches inside emf::TSDF / emf::ObjTSDF / emf::EMFusion methods; the
 * reference interface each one replaces is cited as file:line (relative to the reference root).
 * INTEGRATION.md shows the C++ stub a maintainer adds on the reference side to bind GpuMat
 * arguments to these calls.
 *
 * Contract for every function
 *   - all pointers are DEVICE pointers unless the parameter is named *_host or documented so;
 *     R / t / K / res are small HOST arrays copied into the launch arguments
 *   - never allocates, frees or synchronises: work is enqueued on `stream` (0 = null stream) and
 *     the call returns; launch errors surface as the return value of this or a later call
 *   - returns EMF_OK (0), a negative EMF_E_* for rejected arguments (nothing enqueued), or a
 *     positive hipError_t; never throws; re-entrant, no global state except a thread-local
 *     message buffer read by emf_hip_last_error_string()
 *   - volumes: continuous (Nz*Ny) rows x Nx cols float arrays, element (z*Ny + y, x), i.e. what
 *     cv::cuda::createContinuous(Ny*Nz, Nx, CV_32FCn) allocates (TSDF.cpp:35-42); res = {Nx,Ny,Nz}
 *   - images: emf_image_t = pointer + row pitch in bytes + width/height, the PtrStepSz of a GpuMat
 *   - R row-major 3x3, t 3-vector, K row-major 3x3 intrinsics, exactly the memory of
 *     cv::Matx33f / cv::Vec3f (TSDF.cu:417-422)
 *   - arithmetic is IEEE binary32 in the reference's operation order with a*b+c contraction
 *     disabled; see DESIGN.md "Numerics"
 */
#ifndef EMF_HIP_H
#define EMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMF_HIP_ABI_VERSION 8

/* hipStream_t without dragging HIP headers into C callers */
typedef struct ihipStream_t* emf_stream_t;

enum {
    EMF_OK = 0,
    EMF_E_NULL = -1,      /* a required pointer is NULL */
    EMF_E_SHAPE = -2,     /* non-positive or inconsistent width/height/resolution */
    EMF_E_PITCH = -3,     /* pitch smaller than a row or not a multiple of the element alignment */
    EMF_E_ARG = -4,       /* scalar argument out of domain (voxelSize <= 0, channels not in 1..3 ...) */
    EMF_E_LIMIT = -5,     /* count exceeds a documented limit (EMF_MAX_*) */
    EMF_E_NODEVICE = -6,  /* no HIP device / library built without device code for this GPU */
    EMF_E_NOTREADY = -7,  /* the answer is not known yet (emf_hip_voxelReciprocalCached: size never checked) */
    EMF_E_PEER_TIMEOUT = -8 /* a peer's flag did not arrive within the bound of a direct peer-write exchange (reported by
                             the host classes; the kernels raise the group's error word and skip the exchange's consumer) */
};

/* GpuMat-like image view: `data` device pointer, `pitch` bytes per row (>= width * elemsize) */
typedef struct emf_image {
    void* data;
    size_t pitch;
    int32_t width;
    int32_t height;
} emf_image_t;

#define EMF_MAX_MODELS 256 /* background + objects handled by one call (seg ids are u8) */
#define EMF_MAX_BATCH 32   /* models per batched (model-table) launch */
#define EMF_MAX_PEERS 8    /* ranks of a direct peer-write exchange group (one MI355X node) */

/* Brick uniformity flags: one byte per 4x4x4 brick of a TSDF volume, B = ceil(Nx/4) * ceil(Ny/4) *
 * ceil(Nz/4) bricks, x fastest.  0 = mixed; 1 / 2 / 4 = every voxel of the brick is exactly
 * 0 / +1 / -1.  A flag BUFFER holds 2 * B bytes: the raw flags, then the dilated flags
 * (class | D << 3, D in 1..3 = every brick within Chebyshev distance D shares the class; 0 else).  emf_hip_updateTSDF maintains both;
 * emf_hip_raycastTSDF uses the dilated half to evaluate lookups in uniform regions without
 * gathering and to fast-forward through them (bit-identical results).  A buffer starts as all 1
 * for a zeroed volume (emf_hip_resetBrickFlags) and must be passed to EVERY integration of that
 * volume. */
#define EMF_BRICK 4
#define EMF_BRICK_MIXED 0
#define EMF_BRICK_ALL_ZERO 1
#define EMF_BRICK_ALL_ONE 2
#define EMF_BRICK_ALL_NEG_ONE 4

int emf_hip_abi_version(void);
/* message for the most recent non-zero return on this thread ("" if none) */
const char* emf_hip_last_error_string(void);
/* 0 if a HIP device is usable, EMF_E_NODEVICE otherwise; fills name/arch (may be NULL) */
int emf_hip_device_info(char* name, size_t name_len, char* arch, size_t arch_len, int* num_cus);

/* ------------------------------------------------------------------------------------------------
 * Level 1: one call per reference kernel wrapper (reference memory layout in, same layout out)
 * ---------------------------------------------------------------------------------------------- */

/* Replaces emf::cuda::EMFusion::computePoints (EMFusion.cuh:39-40, EMFusion.cu:29-61).
 * depth: f32 W x H; points: f32x3 W x H, every pixel is written (the reference's setTo(0) is
 * therefore redundant).  Deviation: no cudaDeviceSynchronize -- stream ordered. */
int emf_hip_computePoints(const emf_image_t* depth, const emf_image_t* points, const float K[9],
                          emf_stream_t stream);

/* Replaces emf::cuda::TSDF::updateTSDF (TSDF.cuh:115-122, TSDF.cu:327-427).
 * depth, assocWeights: f32 W x H (same size); tsdf, weights: N^3 f32 read-modify-write.
 * brickFlags: NULL, or the volume's brick uniformity flags, kept consistent by this call.
 * invLambda : NULL, or the table written by emf_hip_computeInvLambda for the same K and image size;
 *             identical results, about a quarter fewer instructions per fused voxel. */
int emf_hip_updateTSDF(const emf_image_t* depth, const emf_image_t* assocWeights, float* tsdf,
                       float* weights, uint8_t* brickFlags, const float R_OC[9],
                       const float t_OC[3], const float K[9], const int32_t res[3],
                       float voxelSize, float truncdist, float maxWeight,
                       const emf_image_t* invLambda, emf_stream_t stream);

/* The pixel-only factor of the integration (TSDF.cu:374-380): invLambda(x, y) =
 * 1 / |((x - cx) / fx, (y - cy) / fy, 1)|, f32 W x H, the very floats updateTSDF computes inline
 * per voxel from the rounded pixel.  Depends on K and the image size only: compute once. */
int emf_hip_computeInvLambda(const float K[9], emf_image_t* invLambda, emf_stream_t stream);

/* Replaces TSDF::updateGradients = tsdfGrads.setTo(0) + emf::cuda::TSDF::computeTSDFGrads
 * (TSDF.cpp:120-123, TSDF.cuh:132-134, TSDF.cu:429-464).  grads: N^3 x 3 f32; the last index
 * planes are written as zero by this call (no separate memset). */
int emf_hip_computeTSDFGrads(const float* tsdf, float* grads, const int32_t res[3],
                             emf_stream_t stream);

/* Replaces emf::cuda::TSDF::raycastTSDF (TSDF.cuh:154-162, TSDF.cu:466-601).
 * raylengths f32, vertices f32x3, normals f32x3, mask u8 (0/1), all W x H, must be PRE-ZEROED by
 * the caller exactly as the reference does (EMFusion.cpp:727-743): pixels without a hit are not
 * written, and a non-zero incoming raylength clips the march (TSDF.cu:496-500).
 *   grads   : N^3 x 3 gradient volume, or NULL -> the normal is blended from forward differences
 *             of `tsdf` on the fly (bit-identical to a volume made by emf_hip_computeTSDFGrads)
 *   fgVolMask: NULL, or N^3 u8 -- the march then sees weights `fgVolMask ? w : 0`, which replaces
 *             ObjTSDF::raycast's per-frame raycastWeights sweep (ObjTSDF.cpp:209-210)
 *   brickFlags: NULL, or the brick uniformity flags of `tsdf` (see EMF_BRICK): lookups whose
 *             eight corners lie in equally-uniform bricks are computed without touching `tsdf`
 *   rcpVoxel: 0, or the value emf_hip_voxelReciprocal returned for `voxelSize`: the march then
 *             divides by the voxel size in 3 instructions instead of 11, same results
 *   stats   : NULL, or 4 x u64 device counters this call ADDS to: [0] volume samples taken by the
 *             main march loop (the S of SURVEY.md section 8d), [1] hits, [2] samples that read
 *             the volume (the rest were answered by the brick flags), [3] samples fast-forwarded */
int emf_hip_raycastTSDF(const float* tsdf, const float* grads, const float* weights,
                        const uint8_t* fgVolMask, const uint8_t* brickFlags,
                        const emf_image_t* raylengths,
                        const emf_image_t* vertices, const emf_image_t* normals,
                        const emf_image_t* mask, const float R_CO[9], const float t_CO[3],
                        const float K[9], const int32_t res[3], float voxelSize, float truncdist,
                        float rcpVoxel, uint64_t* stats, emf_stream_t stream);

/* Plain device-to-device copy kernel (16 B per lane per iteration): the "attainable HBM bandwidth"
 * yardstick bench.py times beside the hot path.  16-byte aligned. */
int emf_hip_streamCopy(void* dst, const void* src, size_t bytes, emf_stream_t stream);

/* Reciprocal of a voxel size, CHECKED for use in place of the division x / voxelSize:
 * runs float inputs x through  q = x * r; q = fma(fma(-q, d, x), r, q)  (r = 1 / d) and through the
 * IEEE division on the device, and stores r in *rcp only if the two agree bit for bit for all x
 * with 1e-30 <= |x| <= 1e30 (0 otherwise; the march keeps its arguments inside that range, see
 * march_wave.hpp).  Swept: every mantissa of the binade [1, 2), both signs, and of the binade
 * that holds 1e-30 -- which decides every binade of the range because both forms commute with
 * scaling by 2^k there (argument and its device-checked premise: abi_common.hip,
 * k_check_reciprocal); ~20 microseconds instead of the 2.3 ms of all 2^32 inputs.
 * The verdict depends on the bit pattern of voxelSize alone and is remembered for the life of
 * the process: the first call for a size runs the check on a stream of its own and waits for THAT
 * (no allocation, no device-wide synchronisation), later calls for the same size return at once
 * without touching the device. */
int emf_hip_voxelReciprocal(float voxelSize, float* rcp);

/* The same check without any wait, for volumes created inside a frame (reference
 * EMFusion.cpp:495-560, initNewObjVolume): the march divides (rcpVoxel = 0, same results) until the
 * verdict is in.
 *   ...Cached: *rcp and EMF_OK if this size has been checked before in this process, else
 *              EMF_E_NOTREADY (nothing is enqueued);
 *   ...Begin : enqueues the check on `stream`; it first stores 0 to *mismatches, then adds the
 *              number of disagreeing inputs to it.  `mismatches` is the caller's (device memory, or
 *              host memory the device can write); nothing is allocated, nothing waited for;
 *   ...End   : the caller has seen the check complete (event, stream query) and read the count:
 *              records the verdict for the process and returns the reciprocal (0 if any input
 *              disagreed).  Pure host code. */
int emf_hip_voxelReciprocalCached(float voxelSize, float* rcp);
int emf_hip_voxelReciprocalBegin(float voxelSize, unsigned long long* mismatches, emf_stream_t stream);
int emf_hip_voxelReciprocalEnd(float voxelSize, unsigned long long mismatches, float* rcp);
/* Test aid: the same comparison over ALL 2^32 bit patterns (2.3 ms of the whole chip, blocking, nothing cached):
 * *mismatches_host = inputs of the guarded range on which the two forms differ.  The short form's verdict must be
 * "usable" exactly when this is 0 (tests/test_gpu_parity.py). */
int emf_hip_voxelReciprocalExhaustive(float voxelSize, unsigned long long* mismatches_host);

/* Measurement aid (bench.py): `iterations` independent 8-byte gather loads per lane from a footprint that stays in every
 * CU's vector L1, `workgroups` x 256 lanes; linesPerInstruction = distinct 128-byte lines one 64-lane instruction touches
 * (64, 4 or 1).  Calibrates the L1 rate the raycast's `roofline.frac` is quoted against.  buf: footprintBytes (power of
 * two) of readable device memory, sink: 8 writable bytes (never written in practice). */
int emf_hip_l1GatherProbe(const void* buf, size_t footprintBytes, int linesPerInstruction, int iterations, int workgroups,
                          void* sink, emf_stream_t stream);

/* ---- direct peer-write exchanges ("Collective implementation"; new design, the
 * reference is single-GPU) ---------------------------------------------------------------------------
 * The exchanges of the sharded path move 1-5 MB: latency decides.  Instead of a library collective
 * each rank stores its contribution straight into a slot of every peer's receive buffer (all xGMI
 * links at once), raises a flag on every peer, waits for the peers' flags and reduces the slots locally
 * in rank order.  emf_peer_t is what ONE rank knows about the group; the host maps the peers' buffers
 * once (same process: the pointers themselves; one process per GPU: hipIpcOpenMemHandle) --
 * emf::makePeerCommunicator.  Buffers: emf_hip_peerBufferBytes(world, slotBytes) bytes (two parities x
 * world slots) and `world` u32 flags per rank, zeroed before the first exchange; slotBytes % 16 == 0.
 * An exchange with sequence number seq (1, 2, 3 ... identical on all ranks) is
 *     scatter (ranks that contribute) -> signal + wait (every rank) -> reduce / copy out of the slots
 * enqueued on the caller's stream; nothing allocates or synchronises.  A wait that exceeds the group's bound
 * stores seq to *error (host-visible word of the caller's) and the exchange's consumer kernel leaves its outputs
 * untouched; the host classes turn a non-zero error word into EMF_E_PEER_TIMEOUT at their next synchronisation.
 * Three forms, same slots and flags:
 *   three launches    peerScatter -> peerSignalWait -> peerReduce* / peerCopyFromSlot            (round 3)
 *   two launches      peerScatter -> peerWaitReduce* / peerWaitCopyFromSlots: the consumer's first workgroup
 *                     signals, every workgroup waits, then reduces / copies                     (round 4)
 *   fused             the path's own kernels scatter and consume: emf_hip_estepBatchedPeer ->
 *                     peerNormalizeAssociation (E-step), emf_hip_packHitKeysPeer ->
 *                     emf_hip_compositeFromKeysPeer (raycast): one extra launch per exchange     (round 4) */
typedef struct emf_peer {
    int32_t rank, world;
    void* slots[EMF_MAX_PEERS];      /* receive buffer of peer p as addressable from THIS device */
    uint32_t* flags[EMF_MAX_PEERS];  /* flag page of peer p: 4096 bytes; words 0..world-1 are the flags */
    size_t slotBytes;                /* capacity of one sender's slot */
    uint32_t* error;                 /* this rank's error word */
    uint32_t timeoutMs;              /* bound of a wait in milliseconds (0: 5000) */
    uint32_t waitInFront;            /* != 0 (what emf::make*PeerCommunicator* set): every peerWait* / *Peer consumer entry
                                        enqueues the one-wave peerSignalWait in front of its kernel, which then does not
                                        poll.  0: the consumer's workgroups signal and poll themselves -- one launch less,
                                        but the polls of a whole grid on the same uncached words cost more than that
                                        launch (k_peer_normalize at 640 x 480, one rank: 5.4 + 5.9 us against 40 us with
                                        1200 polling workgroups, 20 us with 256), and when ranks share a GPU (rehearsals)
                                        grids of spinning workgroups can keep a lagging rank's producer from starting */
    uint32_t systemFences;           /* != 0: every flag store follows a system-scope release and every poll is followed by a
                                        system-scope acquire, in the wait launch and in consumers that wait themselves;
                                        peerScatter ends with one (6.6 us per exchange beside the background's sweep,
                                        measured).  The communicator sets it for ranks on DISTINCT devices; ranks sharing a
                                        device run without (slots and flags are fine-grained memory, peer_core.hpp
                                        "Memory ordering") */
} emf_peer_t;
size_t emf_hip_peerBufferBytes(int world, size_t slotBytes);
int emf_hip_peerScatter(const emf_peer_t* group, const void* src, size_t bytes, size_t dstOffset, uint32_t seq,
                        emf_stream_t stream);
int emf_hip_peerSignalWait(const emf_peer_t* group, uint32_t seq, uint32_t timeoutMs, emf_stream_t stream);
int emf_hip_peerReduceSumF32(const emf_peer_t* group, uint32_t seq, size_t count, float* out, emf_stream_t stream);
int emf_hip_peerReduceMinU64(const emf_peer_t* group, uint32_t seq, size_t count, uint64_t* out, emf_stream_t stream);
int emf_hip_peerCopyFromSlot(const emf_peer_t* group, uint32_t seq, int sender, size_t srcOffset, void* dst,
                             size_t bytes, emf_stream_t stream);
/* signal + wait + reduce in one launch (out := sum / min over the world slots in rank order) */
int emf_hip_peerWaitReduceSumF32(const emf_peer_t* group, uint32_t seq, size_t count, float* out, emf_stream_t stream);
int emf_hip_peerWaitReduceMinU64(const emf_peer_t* group, uint32_t seq, size_t count, uint64_t* out, emf_stream_t stream);
/* signal + wait + nparts copies dst[k][0, bytes[k]) := slot[senders[k]] + srcOffsets[k] in one launch (a broadcast:
 * one part on the receivers, none on the root; a band gather: one part per peer and image); nparts <= 16 */
int emf_hip_peerWaitCopyFromSlots(const emf_peer_t* group, uint32_t seq, int nparts, const int32_t* senders_host,
                                  const size_t* srcOffsets_host, void* const* dsts_host, const size_t* bytes_host,
                                  emf_stream_t stream);
/* Diagnostics behind the two arithmetic shortcuts of the tiled integration (device_core.hpp, on by
 * default, EMF_INT_FAST): the pixel of a voxel as round(x * rcp(z)) unless that lies next to a rounding
 * tie, and the side of the truncation band from the hardware square root unless the distance lies
 * next to +-truncdist.  Both rest on "v_rcp_f32 / v_sqrt_f32 are accurate to 1 ulp".
 *   ...sweepFastPathPremises: all 2^32 float bit patterns through both instructions against the
 *      correctly rounded double results; out4 (device, 4 x u64, zeroed by the call): [0] inputs with
 *      2^-126 <= |z| <= 2^126 whose reciprocal is off by more than 2^-23 relative, [1] inputs
 *      n >= 2^-126 whose square root is, [2] / [3] the largest relative errors seen (float bits);
 *   ...debugPixelRounding: fast[i] / exact[i] = the rounded quotient num[i] / den[i] by the shortcut
 *      and by the IEEE division -- the very device functions the kernels call;
 *   ...debugBandDecision: likewise for the branch (bits 0..3: 2 = behind the band, 3 = fuse; bit 4:
 *      inside the band) and the clamped sample of a voxel with depth d, pixel factor invLambda and
 *      squared distance n2. */
int emf_hip_sweepFastPathPremises(unsigned long long* out4_dev, emf_stream_t stream);
int emf_hip_debugPixelRounding(const float* num_dev, const float* den_dev, int n, int32_t* fast_dev,
                               int32_t* exact_dev, emf_stream_t stream);
int emf_hip_debugBandDecision(const float* d_dev, const float* invLambda_dev, const float* n2_dev, int n,
                              float truncdist, int32_t* kindFast_dev, float* sampleFast_dev,
                              int32_t* kindExact_dev, float* sampleExact_dev, emf_stream_t stream);

/* Diagnostic: one wave that stays resident on `stream` until *release != 0 (host memory the device
 * can read) or maxMilliseconds have passed.  While it runs the stream is "not ready", so a host call
 * that synchronised with the whole device cannot have returned before it ended: the tests use it
 * to show that a frame contains no device-wide synchronisation. */
int emf_hip_spinProbe(const volatile uint32_t* release, uint32_t maxMilliseconds, emf_stream_t stream);
/* Diagnostic: keeps `stream` busy for `microseconds` (one sleeping wave): the latency of a small
 * collective in single-GPU measurements of the exchange path (emf::makeDelayedCommunicator). */
int emf_hip_spinDelay(uint32_t microseconds, emf_stream_t stream);

/* Replaces emf::cuda::TSDF::getVolumeVals (TSDF.cuh:197-203, TSDF.cu:662-726).
 * vol: N^3 x channels f32 (channels 1..3, interleaved); points f32x3; vals f32 x channels.
 * The callee zero-fills vals for pixels without a lookup (vals.setTo(0), TSDF.cu:705). */
int emf_hip_getVolumeVals(const float* vol, int channels, const emf_image_t* points,
                          const float R_CO[9], const float t_CO[3], const int32_t res[3],
                          float voxelSize, const emf_image_t* vals, emf_stream_t stream);

/* Replaces emf::cuda::ObjTSDF::updateFgBgProbs (ObjTSDF.cuh:49-56, ObjTSDF.cu:29-107).
 * mask, occluded: u8 W x H read as bool; fgBgProbs: N^3 x 2 f32 read-modify-write. */
int emf_hip_updateFgBgProbs(const emf_image_t* mask, const emf_image_t* occluded,
                            const float* tsdf, const float* weights, float* fgBgProbs,
                            const float R_OC[9], const float t_OC[3], const float K[9],
                            const int32_t res[3], float voxelSize, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Level 2: one call per OpenCV-CUDA launch chain in the volume / orchestrator classes
 * ---------------------------------------------------------------------------------------------- */

/* Replaces ObjTSDF::computeFgProbs (ObjTSDF.cpp:218-226): split, add, divide (x/0 := 0),
 * compare(NE)+setTo(0), compare(GT 0.5).  fgProbs N^3 f32, fgVolMask N^3 u8 (0/255). */
int emf_hip_computeFgProbs(const float* fgBgProbs, float* fgProbs, uint8_t* fgVolMask,
                           const int32_t res[3], emf_stream_t stream);

/* Literal replacement of ObjTSDF::raycast's weight masking (ObjTSDF.cpp:209-210):
 * raycastWeights = fgVolMask ? weights : 0.  The native path passes fgVolMask to
 * emf_hip_raycastTSDF instead and never materialises this volume. */
int emf_hip_maskRaycastWeights(const float* weights, const uint8_t* fgVolMask,
                               float* raycastWeights, const int32_t res[3], emf_stream_t stream);

/* Replaces TSDF::computeAssociation (TSDF.cpp:125-136) incl. TSDF::computeLaplace
 * (TSDF.cpp:138-156) when fgProbs == NULL, and ObjTSDF::computeAssociation (ObjTSDF.cpp:181-201)
 * otherwise: trilinear SDF lookup, Laplace likelihood, optional foreground-probability factor,
 * mixture with the uniform prior, zero where the lookup is exactly 0.  out: f32 W x H,
 * UN-normalised, every pixel written. */
int emf_hip_computeAssociation(const float* tsdf, const float* fgProbs, const emf_image_t* points,
                               const float R_CO[9], const float t_CO[3], const int32_t res[3],
                               float voxelSize, float truncdist, float assocSigma, float alpha,
                               float uniPrior, const emf_image_t* out, emf_stream_t stream);

/* Replaces the normalisation half of EMFusion::computeAssociationWeights (EMFusion.cpp:653-665).
 * maps_host: HOST array of `nmaps` image views (device data), [0] = background then objects in
 * std::map (ascending ID) order; every map is divided in place by the normaliser; x/0 := 0.
 *   nsum    : the normaliser is the sequential sum of maps[0 .. nsum-1] (single GPU: nsum = nmaps)
 *   extraSum: NULL, or f32 W x H added LAST into the normaliser.  Multi-GPU: every rank
 *             passes nsum = 1 (its background replica) and extraSum = the all-reduced sum of all
 *             ranks' object maps (emf_hip_sumAssociation + RCCL all-reduce)
 *   norm    : NULL, or f32 W x H receiving associationNorm (required when nsum > 16)
 * 1 <= nmaps <= EMF_MAX_MODELS, 0 <= nsum <= nmaps, nsum == 0 requires extraSum. */
int emf_hip_normalizeAssociation(const emf_image_t* maps_host, int nmaps, int nsum,
                                 const emf_image_t* extraSum, const emf_image_t* norm,
                                 emf_stream_t stream);

/* Sum of `nmaps` association maps into `sum` (sequential order, maps_host[0] first): the local
 * partial a rank contributes to the normaliser all-reduce.  sum: f32 W x H, overwritten. */
int emf_hip_sumAssociation(const emf_image_t* maps_host, int nmaps, const emf_image_t* sum,
                           emf_stream_t stream);

/* Replaces the compositing part of EMFusion::raycast (EMFusion.cpp:760-794) in one pass.
 * Per-object inputs are HOST arrays of `nobj` image views in std::list (creation) order; ids_host
 * holds the object IDs written to the segmentation (saturated to u8 like cv::Scalar->uchar).
 *   diff     : f32 W x H, the persistent diffRaylengths buffer, only updated where bgMask != 0
 *   visCounts: device int32[nobj], overwritten with the number of pixels with seg == id inside
 *              [boundary, W-boundary) x [boundary, H-boundary)  (EMFusion.cpp:778-791)
 * Outputs ray/vert/norm/seg/noObj are fully overwritten (no pre-zeroing needed). */
int emf_hip_compositeRaycast(int nobj, const int32_t* ids_host, const emf_image_t* objRay_host,
                             const emf_image_t* objVert_host, const emf_image_t* objNorm_host,
                             const emf_image_t* objSeg_host, const emf_image_t* bgRay,
                             const emf_image_t* bgVert, const emf_image_t* bgNorm,
                             const emf_image_t* bgMask, const emf_image_t* ray,
                             const emf_image_t* vert, const emf_image_t* norm,
                             const emf_image_t* seg, const emf_image_t* diff,
                             const emf_image_t* noObj, int boundary, int32_t* visCounts,
                             emf_stream_t stream);

/* emf_hip_compositeRaycast + emf_hip_visibilityFlags in two launches instead of three: the launch that
 * writes the composite also counts (its last chunk, on the segmentation values it writes), the flag launch
 * clears the counts behind itself.  visCounts is scratch of the pair here: ZERO on entry, zero on return
 * (the numbers go to countsMirror, if given, and into the flags). */
int emf_hip_compositeVisibility(int nobj, const int32_t* ids_host, const emf_image_t* objRay_host,
                                const emf_image_t* objVert_host, const emf_image_t* objNorm_host,
                                const emf_image_t* objSeg_host, const emf_image_t* bgRay,
                                const emf_image_t* bgVert, const emf_image_t* bgNorm,
                                const emf_image_t* bgMask, const emf_image_t* ray,
                                const emf_image_t* vert, const emf_image_t* norm,
                                const emf_image_t* seg, const emf_image_t* diff,
                                const emf_image_t* noObj, int boundary, int32_t* visCounts,
                                int visibilityThresh, int32_t* visible_dev, int32_t* countsMirror,
                                emf_stream_t stream);

/* Replaces the occlusion mask of EMFusion::integrateMasks (EMFusion.cpp:897-900):
 * occluded = saturate_u8(objSeg - (seg == id ? 255 : 0)).  All u8 W x H. */
int emf_hip_occludedMask(const emf_image_t* objSeg, const emf_image_t* seg, int id,
                         const emf_image_t* occluded, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Level 3: batched, model-table driven launches used by the host classes (emf::EMFusion).
 * One launch covers the background and every object volume of this rank, replacing the
 * reference's one-stream-per-volume fan-out (EMFusion.h:471, EMFusion.cpp:636-668, 727-758,
 * 866-888).  Results are identical to calling the level-1/2 functions model by model.
 * ---------------------------------------------------------------------------------------------- */

/* Static description of one model, an array of which lives in DEVICE memory (models_dev).
 * Slot 0 is the background, slots 1.. the objects in creation order.  Image pointers are
 * continuous W x H buffers (pitch = width * elemsize). */
typedef struct emf_model {
    float* tsdf;            /* N^3 f32 */
    float* weights;         /* N^3 f32 */
    const float* grads;     /* N^3 x 3 f32 or NULL (on-the-fly differences) */
    const float* fgProbs;   /* N^3 f32, objects only, else NULL */
    const uint8_t* fgVolMask; /* N^3 u8, objects only, else NULL */
    uint8_t* brickFlags;    /* flag buffer (2 * B bytes, see EMF_BRICK) or NULL */
    float* assoc;           /* f32 association map of this model */
    float* raylengths;      /* f32   raycast outputs of this model */
    float* vertices;        /* f32x3 */
    float* normals;         /* f32x3 */
    uint8_t* hitMask;       /* u8 0/1 */
    uint8_t* signMaps;      /* emf_hip_signMapBytes(res) bytes or NULL: per 32x8x8 tile "holds a positive
                             * tsdf", then per tile "holds a negative tsdf"; kept by the tile integration
                             * launches (sticky), read by emf_hip_raycastFarBounds */
    uint32_t* relevantTiles; /* emf_hip_relevantTileBytes(res) bytes or NULL (emf_hip_updateRelevantTiles) */
    uint8_t* unseenTiles;   /* emf_hip_unseenTileBytes(res) bytes or NULL: per 32x8x8 tile "every weight is 0 (and
                             * every tsdf finite)"; set by the owner (a cleared volume: all 1;
                             * emf_hip_rebuildUnseenTiles), cleared by the tile integration launches, which
                             * integrate such a tile without reading it */
    int32_t res[3];
    int32_t id;             /* 0 = background */
    float voxelSize, truncdist, maxWeight;
    float assocC1;          /* -truncdist / assocSigma  (TSDF.cpp:151) */
    float assocC2;          /* 1 / (2 assocSigma)       (TSDF.cpp:154) */
    float alpha;            /*                          (TSDF.cpp:131) */
    float assocC3;          /* (1 - alpha) * uniPrior   (TSDF.cpp:133) */
    int32_t reserved;
    float rcpVoxel;         /* emf_hip_voxelReciprocal(voxelSize), or 0 = divide */
    int32_t pad_;
} emf_model_t;

/* Rigid transform passed by value with each launch (poses change every frame). */
typedef struct emf_pose {
    float R[9];
    float t[3];
} emf_pose_t;

/* E-step for all models in one launch (TSDF.cpp:125-156, ObjTSDF.cpp:181-201, EMFusion.cpp:635-670):
 * each (pixel, model) lane computes its likelihood, partial sums meet in LDS.
 *   poseCO_host[m]: camera -> volume m.  points: f32x3 W x H.
 *   normalize != 0: maps are written normalised, norm (f32 W x H, may be NULL) gets the
 *                   normaliser = sequential sum of all maps (+ nothing else): single-GPU form
 *   normalize == 0: maps are written UN-normalised and objSum (f32 W x H, or NULL: no sum) receives
 *                   the sequential sum of the object maps (slots 1..): the partial a rank feeds to
 *                   the all-reduce; finish with emf_hip_normalizeAssociation(nsum = 1, extraSum)
 * 1 <= nmodels <= EMF_MAX_BATCH.  A model list longer than that is served in chunks of the table
 * (models_dev + k, poseCO_host + k; normalize == 0, objSum NULL) followed by ONE
 * emf_hip_normalizeAssociation over all maps (nsum = nmaps): the same sequential sum, the same bits. */
int emf_hip_estepBatched(const emf_model_t* models_dev, const emf_pose_t* poseCO_host, int nmodels,
                         const emf_image_t* points, int normalize, const emf_image_t* norm,
                         const emf_image_t* objSum, emf_stream_t stream);

/* emf_hip_normalizeAssociation(nsum = nmaps) over the `assoc` maps of a whole model table (continuous W x H, slot 0 first)
 * in ONE launch: the sequential sum of all maps in table order, every map divided by it (x / 0 := 0), the sum to
 * norm_dev (continuous W x H f32, or NULL).  Finishes the chunked E-step of a model list longer than EMF_MAX_BATCH
 * (emf_hip_estepBatched per chunk with normalize == 0).  1 <= nmodels <= EMF_MAX_MODELS.  Same bits. */
int emf_hip_normalizeAssociationTable(const emf_model_t* models_dev, int nmodels, int width, int height, float* norm_dev,
                                      emf_stream_t stream);

/* emf_hip_computePoints + emf_hip_estepBatched in one launch, for the first E-step of a frame
 * (EMFusion.cpp:73, 79): each pixel's point is formed from `depth` with computePoints' arithmetic,
 * used, and stored to `points` (f32x3 W x H, every pixel written) for the frame's later stages. */
int emf_hip_estepBatchedFromDepth(const emf_model_t* models_dev, const emf_pose_t* poseCO_host, int nmodels,
                                  const emf_image_t* depth, const float K[9], const emf_image_t* points,
                                  int normalize, const emf_image_t* norm, const emf_image_t* objSum,
                                  emf_stream_t stream);

/* Raycast of all models in one launch (TSDF.cu:466-601 per model, ObjTSDF.cpp:203-216).
 * Unlike emf_hip_raycastTSDF the outputs need no pre-zeroing: every pixel of every model's
 * raylengths / vertices / normals / hitMask is written (zeros where there is no hit), which is
 * what the reference's setTo(0) + kernel leave behind (EMFusion.cpp:727-758).
 *   res_host: HOST int32[nmodels * 3], the resolutions stored in the table
 *   useBrickFlags != 0: march with the models' brick flags (fast-forward through uniform bricks);
 *   0: ignore them and use the wave-scheduled march (default; faster on the bench scene).
 * Both produce the same images.  Models whose table entry carries rcpVoxel != 0 divide by the
 * voxel size with the checked reciprocal (emf_hip_voxelReciprocal), same results.
 *   bgBandRow0, bgBandRows: multi-GPU split of the REPLICATED background (table slot 0): only the
 *   image rows [bgBandRow0, bgBandRow0 + bgBandRows) of slot 0 are marched and written, the others
 *   are left untouched for an all-gather of the ranks' bands (multiples of 16; 0, 0 = all rows).
 * This entry point always marches one lane per background ray: it does NOT read EMF_MARCH_ROWS (emf::EMFusion's
 * constructor does, and passes the lanes on).  A caller that wants 2 or 4 lanes uses emf_hip_raycastBatchedLanes. */
int emf_hip_raycastBatched(const emf_model_t* models_dev, const emf_pose_t* poseCO_host,
                           const int32_t* res_host, int nmodels, int width, int height,
                           const float K[9], int useBrickFlags, int bgBandRow0, int bgBandRows,
                           const float* farBounds_dev, const float* voxelSizes_host, uint64_t* stats,
                           emf_stream_t stream);
/* Free-viewpoint view of a whole model table in ONE launch (the reference's 3D view, EMFusion.cpp:162-231, ray-cast
 * instead of meshed): per pixel, every model is marched (TSDF.cu:466-601 arithmetic, fgVolMask-gated weights for
 * objects as in ObjTSDF.cpp:203-216), the hits are composited in table order with EMFusion.cpp:760-794's rule as
 * emf_hip_compositeRaycast applies it (diff starts at 0: no history), the labels in hideMask are hidden as
 * emf_hip_hideLabel does, and the result is Phong-shaded as emf_hip_renderPhong does (light at lightPos, viewer
 * frame).  Reads tsdf / weights / grads / fgVolMask only; writes nothing of the table.  Same bits as that chain.
 *   poseVO_dev: DEVICE emf_pose_t[nmodels], viewer -> volume of each slot (slot 0: the background)
 *   ids_host:   HOST int32[nmodels - 1], the labels of slots 1.. (compositeRaycast's ids); NULL if nmodels == 1
 *   colorMap:   label -> u8 x 3 colour;  hideMask: bit s (byte s / 8, bit s % 8) hides label s, or NULL: none
 *   rgb:        u8 x 3 width x height, required; raylengths (f32), segmentation (u8), vertices / normals (f32 x 3):
 *               width x height or NULL (not written).  Pitched images are accepted.
 *   stats_dev:  NULL or u64[4] accumulating samples / hits / gathered / 0 as the raycast counts them.
 * 1 <= nmodels <= EMF_MAX_MODELS in one launch (no EMF_MAX_BATCH chunking).  No far bounds, no brick flags; volumes
 * above 32-bit byte offsets take the 64-bit march. */
int emf_hip_renderView(const emf_model_t* models_dev, const emf_pose_t* poseVO_dev, const int32_t* ids_host,
                       int nmodels, int width, int height, const float K[9], const float lightPos[3],
                       const uint8_t colorMap[768], const uint8_t hideMask[32], const emf_image_t* rgb,
                       const emf_image_t* raylengths, const emf_image_t* segmentation, const emf_image_t* vertices,
                       const emf_image_t* normals, uint64_t* stats_dev, emf_stream_t stream);
/* emf_hip_raycastBatched with the BACKGROUND's rays marched by lanesPerBgRay = 1, 2 or 4 lanes each (march_quad,
 * march_wave.hpp: the lanes of a ray take consecutive samples speculatively; same images, same sample count; measured
 * slower beside the background's integration, hence not the default).  Ignored (1) with brick flags or volumes above
 * 4 GiB. */
int emf_hip_raycastBatchedLanes(const emf_model_t* models_dev, const emf_pose_t* poseCO_host,
                                const int32_t* res_host, int nmodels, int width, int height,
                                const float K[9], int useBrickFlags, int bgBandRow0, int bgBandRows,
                                const float* farBounds_dev, const float* voxelSizes_host, int lanesPerBgRay,
                                uint64_t* stats, emf_stream_t stream);
/* The same launch for a table chunk that holds OBJECTS ONLY (every slot, slot 0 included, is marched over its
 * footprint and zero-filled outside it): the later chunks of a model list longer than EMF_MAX_BATCH
 * (reference EMFusion.cpp:745-758 loops over any number of objects).  farBounds_dev: this chunk's part of the
 * bounds (emf_hip_raycastFarBounds called with the same chunk). */
int emf_hip_raycastBatchedObjects(const emf_model_t* models_dev, const emf_pose_t* poseCO_host,
                                  const int32_t* res_host, int nmodels, int width, int height,
                                  const float K[9], int useBrickFlags, const float* farBounds_dev,
                                  const float* voxelSizes_host, uint64_t* stats, emf_stream_t stream);
/* voxelSizes_host: NULL, or HOST float[nmodels], the voxel sizes stored in the table.  With them the
 * objects (slots 1..) get marching workgroups only for the 16x16-pixel tiles their volume box can project
 * to under poseCO_host; the rest of their images is zero-filled sixteen tiles per workgroup -- same
 * output, but four objects no longer put 4 x 1200 nearly empty workgroups in front of the background's
 * (whose dispatch alone took the first 200 us of the launch). */

/* Far bounds for emf_hip_raycastBatched (farBounds_dev; NULL = none).  A hit of the reference's march
 * (TSDF.cu:533-568) is a negative sample following a positive one, so it needs a negative and a positive
 * voxel close together.  From the models' sign maps (emf_model_t.signMaps) this call computes, per model
 * and per 8x8-pixel cell of the image, the largest raylength at which a ray of the cell can still
 * complete a hit (0: it cannot at all; +inf for models without sign maps); the march of a ray is cut
 * there.  Every sample still taken is taken exactly as before, the ones dropped could not have written
 * an output: results are bit-identical, the rays that used to run on through unseen space to the far
 * side of the volume -- the longest of the image -- stop behind the last surface.
 *   bounds_dev: emf_hip_raycastFarBoundBytes(nmodels, width, height) bytes
 * emf_hip_rebuildSignMaps recomputes a volume's maps from its values (needed after anything but the
 * tile integration launches wrote the tsdf: uploads, emf_hip_copyValues, the one-voxel-per-lane
 * kernels, emf_hip_updateTSDF). */
size_t emf_hip_signMapBytes(const int32_t res[3]);
int emf_hip_rebuildSignMaps(const float* tsdf, const int32_t res[3], uint8_t* signMaps, emf_stream_t stream);
/* Unseen-tile map (emf_model_t.unseenTiles).  A voxel nobody has fused into (weight 0) is set to 0, to
 * -1 or to its first sample by kernel_updateTSDF whatever it held (TSDF.cu:352-355, 369-372, 392-400), or
 * left alone (pixel outside the image, association weight 0): for a tile of such voxels the tile
 * integration launches compute the new values without loading the old ones (they load what a voxel
 * keeps) and store them -- behind surfaces and outside the truncation band, where depth drop-outs flip
 * unseen voxels between -1 and 0 from frame to frame, that is two thirds of the bytes the sweep moved. */
size_t emf_hip_unseenTileBytes(const int32_t res[3]);
int emf_hip_rebuildUnseenTiles(const float* tsdf, const float* weights, const int32_t res[3], uint8_t* unseenTiles,
                               emf_stream_t stream);
size_t emf_hip_raycastFarBoundBytes(int nmodels, int width, int height);
/* scanMask: bit m set = model m has every tile of its sign maps examined (a neighbourhood scan per tile:
 * fine for an object volume, ~50 us for a 512^3 one); clear = its relevant-tile list is walked
 * (emf_model_t.relevantTiles; a model with neither bit nor list keeps its whole range). */
int emf_hip_raycastFarBounds(const emf_model_t* models_dev, const emf_pose_t* poseCO_host,
                             const int32_t* res_host, int nmodels, int width, int height, const float K[9],
                             uint32_t scanMask, float* bounds_dev, emf_stream_t stream);
/* The tiles in which a hit can be completed, as a list per model (emf_model_t.relevantTiles:
 * emf_hip_relevantTileBytes(res) bytes: a count, then tile indices): rebuilt from the sign maps after an
 * integration -- off the frame's critical path -- so that emf_hip_raycastFarBounds, which needs the
 * camera pose of the frame and therefore sits right in front of the raycast, only has to project a
 * few thousand tiles.  Models whose relevantTiles is NULL are skipped. */
size_t emf_hip_relevantTileBytes(const int32_t res[3]);
int emf_hip_updateRelevantTiles(const emf_model_t* models_dev, const int32_t* res_host, int nmodels,
                                emf_stream_t stream);

/* Integration of all models in one launch (TSDF.cu:327-427 per model, EMFusion.cpp:865-875).
 *   poseOC_host[m]: volume m -> camera
 *   res_host    : HOST int32[nmodels * 3], the resolutions stored in the table (the launch grid is
 *                 sized from them).  Models with Nx % 4 == 0 run on 32x8x8 float4 tiles; others (an
 *                 object after ObjTSDF::resize is only guaranteed an even Nx) run one voxel per
 *                 lane in a second launch of the same call -- same arithmetic, same gate
 *   visible_dev : NULL, or device int32[nmodels]; models with visible_dev[m] == 0 are skipped
 *                 (EMFusion.cpp:869-872) -- evaluated on the device, no host round trip
 * Each model's `assoc` map weights its fusion; brickFlags are kept consistent when present.
 *   invLambda   : NULL, or emf_hip_computeInvLambda's table for K and the depth size
 *   maintainBrickFlags: 0 if no model of the table carries brick flags (skips the launch that
 *                 refreshes the dilated flags); non-zero otherwise
 *   stats       : NULL, or one u64 device counter this call ADDS the voxel count of every model
 *                 it actually sweeps to (work accounting for the byte model)
 */
int emf_hip_integrateBatched(const emf_model_t* models_dev, const emf_pose_t* poseOC_host,
                             const int32_t* res_host, int nmodels, const int32_t* visible_dev,
                             const emf_image_t* depth, const emf_image_t* invLambda,
                             const float K[9], int maintainBrickFlags, uint64_t* stats,
                             emf_stream_t stream);

/* The same integration with a two-level launch (models with Nx % 4 == 0 only, no brick flags upkeep):
 * boxes of 1x2x2 tiles (32 x 16 x 16 voxels) that lie outside the view cone are culled first (one lane per box), and only
 * the tiles of the surviving boxes get a workgroup -- the culled tiles of a large volume otherwise
 * cost a workgroup dispatch each.  Results are identical to emf_hip_integrateBatched.
 *   scratch_dev      : emf_hip_integrateCullScratchBytes(res_host, nmodels) bytes
 *   launchBoxes      : how many boxes the tile launch is sized for -- the survivor count of an earlier
 *                      frame plus a margin; 0 = all boxes.  Too few: the grid strides over the rest;
 *                      too many: the extra workgroups exit.
 *   survivors_out_dev: NULL, or where this call's survivor count (u32) is copied at the end */
size_t emf_hip_integrateCullScratchBytes(const int32_t* res_host, int nmodels);
int emf_hip_integrateBatchedCulled(const emf_model_t* models_dev, const emf_pose_t* poseOC_host,
                                   const int32_t* res_host, int nmodels, const int32_t* visible_dev,
                                   const emf_image_t* depth, const emf_image_t* invLambda,
                                   const float K[9], void* scratch_dev, uint32_t launchBoxes,
                                   uint32_t* survivors_out_dev, uint64_t* stats, emf_stream_t stream);

/* Out-of-place form of the same launch, for volumes that are kept TWICE (double-buffered) so that the
 * integration of a frame can run concurrently with the raycast of the same frame -- both read the state
 * the previous frame left; the reference runs them back to back (EMFusion.cpp:94, 103) -- and the
 * raycast never sees a half-integrated volume.  Model m is READ from models_dev[m].tsdf / .weights
 * and the integrated state is written to out_host[m].tsdf / .weights, the volume's second copy.  The
 * two copies are equal wherever the previous integration changed nothing, which the dirty maps track
 * per array at tile granularity (one byte per 32 x 8 x 8 voxel tile for the tsdf, then one per tile for
 * the weights: emf_hip_integrateDirtyMapBytes(res) bytes in all).  A set byte of dirtyPrev -- the
 * copies of that array differ in that tile -- makes this call write every voxel of the array in the
 * tile (integrated or copied), elsewhere it writes only what changes; dirtyNext (cleared by the call)
 * receives what this call changed and is the next call's dirtyPrev, with the roles of the copies
 * swapped.  A model whose visible_dev gate is closed is not integrated but still brought up to date.
 * Start with equal copies and clean maps.  Values are those of the in-place launch, bit for bit.
 * out_host == NULL: in place (= emf_hip_integrateBatchedCulled); otherwise every model of the call
 * needs its four pointers. */
typedef struct emf_volume_out {
    float* tsdf;
    float* weights;
    const uint8_t* dirtyPrev;
    uint8_t* dirtyNext;
} emf_volume_out_t;
size_t emf_hip_integrateDirtyMapBytes(const int32_t res[3]);
int emf_hip_integrateBatchedCulledOut(const emf_model_t* models_dev, const emf_pose_t* poseOC_host,
                                      const int32_t* res_host, int nmodels, const int32_t* visible_dev,
                                      const emf_image_t* depth, const emf_image_t* invLambda,
                                      const float K[9], const emf_volume_out_t* out_host, int prepared,
                                      void* scratch_dev, uint32_t launchBoxes, uint32_t* survivors_out_dev,
                                      uint64_t* stats, emf_stream_t stream);
/* prepared != 0: the caller has cleared the survivor counter (first word of scratch_dev) and the
 * dirtyNext maps already -- emf_hip_integratePrepareOut does exactly that and can be enqueued as soon as
 * the previous call on that scratch / those maps has run, i.e. off the frame's critical path (two fill
 * commands in front of the launch cost it ~40 us while the raycast's workgroups are being dispatched).
 * out_host may be NULL here (counter only). */
int emf_hip_integratePrepareOut(const emf_volume_out_t* out_host, const int32_t* res_host, int nmodels,
                                void* scratch_dev, emf_stream_t stream);

/* visible_dev[slot] = (slot == 0) ? 1 : (visCounts[slot - 1] > visibilityThresh)  for
 * slot < nmodels (EMFusion.cpp:778-791): turns compositeRaycast's counts into the gate above.
 * countsMirror: NULL, or nmodels - 1 int32 in device-visible HOST memory (hipHostMalloc) that receive
 * the counts as well -- the host's view of the visible set without a copy command in the stream. */
int emf_hip_visibilityFlags(const int32_t* visCounts, int nmodels, int visibilityThresh,
                            int32_t* visible_dev, int32_t* countsMirror, emf_stream_t stream);

/* Fill a brick flag buffer (2 * B bytes) for a freshly zeroed volume (all EMF_BRICK_ALL_ZERO). */
int emf_hip_resetBrickFlags(uint8_t* brickFlags, const int32_t res[3], emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-GPU compositing (object volumes sharded over ranks).  The reference
 * is single-GPU; these three calls bracket the ONE all-reduce(min, u64, W*H) that merges the
 * nearest raycast hit over the objects of all ranks with the reference's tie rule (first object in
 * creation order keeps the pixel, EMFusion.cpp:760-771):
 *   key = (float_bits(raylength) << 32) | listPosition,   no hit = all ones.
 * ---------------------------------------------------------------------------------------------- */

/* keys[pixel] = min key over this rank's objects.  listPos_host[k] = position of local object k in
 * the global creation-order list; objRay / objSeg: its raycast raylengths (f32) and hit mask (u8).
 * 0 <= nlocal <= EMF_MAX_BATCH; keys: u64 W x H, overwritten. */
int emf_hip_packHitKeys(int nlocal, const int32_t* listPos_host, const emf_image_t* objRay_host,
                        const emf_image_t* objSeg_host, uint64_t* keys, int width, int height,
                        emf_stream_t stream);

/* Finish the composite from all-reduced keys: segmentation id = ids_host[listPosition], raylength
 * from the key, vertex / normal from the winner's images when it lives on this rank (zeros
 * otherwise: they only feed rendering), then the background override, noObj mask, background
 * vertices / normals and per-object visibility counts exactly as emf_hip_compositeRaycast
 * (EMFusion.cpp:773-794).  ids_host: ids of ALL nall objects in creation order; visCounts: device
 * int32[nall], overwritten. */
int emf_hip_compositeFromKeys(const uint64_t* keys, int nall, const int32_t* ids_host, int nlocal,
                              const int32_t* listPos_host, const emf_image_t* objRay_host,
                              const emf_image_t* objVert_host, const emf_image_t* objNorm_host,
                              const emf_image_t* bgRay, const emf_image_t* bgVert,
                              const emf_image_t* bgNorm, const emf_image_t* bgMask,
                              const emf_image_t* ray, const emf_image_t* vert,
                              const emf_image_t* norm, const emf_image_t* seg,
                              const emf_image_t* diff, const emf_image_t* noObj, int boundary,
                              int32_t* visCounts, emf_stream_t stream);

/* visible_dev[slot] = (slot == 0) ? 1 : (visCounts[countIndex_host[slot]] > visibilityThresh):
 * emf_hip_visibilityFlags for a rank whose model slots map to arbitrary entries of a global count
 * array.  1 <= nmodels <= EMF_MAX_BATCH + 1 (the background + the objects one rank may own). */
int emf_hip_visibilityFlagsIndexed(const int32_t* visCounts, int nmodels,
                                   const int32_t* countIndex_host, int visibilityThresh,
                                   int32_t* visible_dev, emf_stream_t stream);

/* Depth pre-processing: replaces EMFusion::preprocessDepth
 * (EMFusion.cpp:294-305) = cv::cuda::bilateralFilter(kernelSize, sigmaDepth [m], sigmaSpatial [px],
 * reflected borders) + NaN -> 0 + "0 wherever the raw depth is 0", one launch.  f32 W x H images,
 * not in place; kernelSize odd, <= 15. */
int emf_hip_preprocessDepth(const emf_image_t* depthRaw, const emf_image_t* depth, int kernelSize,
                            float sigmaDepth, float sigmaSpatial, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Object creation / matching from instance masks (mesh-free part)
 * ---------------------------------------------------------------------------------------------- */

/* What EMFusion::initNewObjVolume needs of the masked points (EMFusion.cpp:498-535):
 * count = pixels with mask != 0 and a valid point (computeValidPoints: any coordinate != 0);
 * p10 / p90 = per axis, the elements at index int(count * .1f) and int(count * .9f) of the sorted
 * coordinates of those points after x' = R x + t (computePercentiles, EMFusion.cu:77-98). */
typedef struct emf_point_stats {
    uint32_t count;
    float p10[3];
    float p90[3];
} emf_point_stats_t;

size_t emf_hip_pointStatsScratchBytes(void);

/* filterPoints + transformPoints + computePercentiles (EMFusion.cu:63-98, EMFusion.cpp:408-415)
 * fused into a masked radix select: no compaction, no sort, bit-identical order statistics.
 * points f32x3, mask u8 (W x H); stats_dev and scratch_dev in device memory; 9 small launches. */
int emf_hip_maskedPointStats(const emf_image_t* points, const emf_image_t* mask, const float R[9],
                             const float t[3], void* scratch_dev, emf_point_stats_t* stats_dev,
                             emf_stream_t stream);

/* The statistics of EMFusion::updateObj (EMFusion.cpp:827-863): as emf_hip_maskedPointStats, but
 * over the masked points (already transformed into the object's frame by R, t) TOGETHER WITH the
 * vertex cloud of the object's marching-cubes mesh (TSDF.cu:855-1152, ObjTSDF.cpp:247-268): one
 * vertex per sign-changing edge of every cube whose 8 voxels have weight > 0 (and fgVolMask != 0 if
 * given), interpolated by vertexInterp.  The cloud does not depend on the triangle table, so no
 * mesh is built: the vertices are streamed into the same radix select. */
int emf_hip_objectExtentStats(const emf_image_t* points, const emf_image_t* mask, const float R[9],
                              const float t[3], const float* tsdf, const float* weights,
                              const uint8_t* fgVolMask, const int32_t res[3], float voxelSize,
                              void* scratch_dev, emf_point_stats_t* stats_dev, emf_stream_t stream);

/* Replaces emf::cuda::TSDF::copyValues (TSDF.cu:768-819) used by ObjTSDF::resize: dst (dstRes,
 * `channels` floats per voxel) receives src shifted by `offset` voxels -- dst(v) = src(v + offset)
 * inside the source, 0 elsewhere (the reference clears dst first; this call writes every voxel). */
int emf_hip_copyValues(const float* src, float* dst, int channels, const int32_t offset[3],
                       const int32_t srcRes[3], const int32_t dstRes[3], emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Meshes: cuda::TSDF::marchingCubes (TSDF.cu:855-1152) behind
 * TSDF::getMesh / ObjTSDF::getMesh (TSDF.cpp:356-373, ObjTSDF.cpp:247-268)
 * ---------------------------------------------------------------------------------------------- */

typedef struct emf_mesh_counts {
    uint32_t vertices;  /* = mesh.cloud.cols */
    uint32_t triangles; /* = mesh.polygons.cols / 4 */
} emf_mesh_counts_t;

/* Bytes of device scratch the two calls below share for a volume of this resolution (about
 * 36 bytes per 1000 voxels; the reference keeps 9 bytes per cube in cubeClasses / vertIdxBuffer / triIdxBuffer). */
size_t emf_hip_meshScratchBytes(const int32_t res[3]);

/* Pass 1 -- kernel_classifyCubes + the two sums + the two exclusive scans: counts the vertices and
 * triangles of the iso-surface over the cubes whose 8 voxels all have weights > 0 (and
 * fgVolMask != 0 when given: ObjTSDF::getMesh), and leaves the per-workgroup offsets in scratch.
 * counts_dev: device memory; read it back, allocate the outputs, then call emf_hip_meshEmit with
 * the same volume and the same scratch. */
int emf_hip_meshCount(const float* tsdf, const float* weights, const uint8_t* fgVolMask,
                      const int32_t res[3], void* scratch_dev, emf_mesh_counts_t* counts_dev,
                      emf_stream_t stream);

/* Pass 2 -- kernel_createTriangles: vertices and normals (3 floats each per vertex, volume frame)
 * and triangles (4 int32 each: 3, i0, i1, i2), element for element what the reference's mesh
 * holds.  grads: the N^3 x 3 gradient volume, or NULL to take the same forward differences on the
 * fly.  Normals are the interpolated gradients as they are -- the reference's normalisations are
 * no-ops (common.cuh:170-173). */
int emf_hip_meshEmit(const float* tsdf, const float* grads, const float* weights,
                     const uint8_t* fgVolMask, const int32_t res[3], float voxelSize,
                     const void* scratch_dev, float* vertices, float* normals, int32_t* triangles,
                     emf_stream_t stream);

/* The two passes over a TABLE of volumes (level 3): one count launch, one scan launch and one emit launch mesh every
 * model of models_dev[0 .. n) (tsdf, weights, grads, fgVolMask, res, voxelSize are read; NULL grads = on-the-fly
 * differences, NULL fgVolMask = no foreground gate).  1 <= n <= EMF_MAX_MODELS (no EMF_MAX_BATCH chunking).
 * res_host: HOST int32[3 n], the resolutions stored in the table.  Model m's mesh is written to the concatenated
 * outputs at its bases, and that slice is byte for byte what emf_hip_meshCount + emf_hip_meshEmit give for the volume
 * alone: the same order, triangle indices local to the model (its first vertex is 0).  The level-1 calls above are
 * the one-volume case of the same kernels.
 *   scratch: emf_hip_meshScratchBytesBatched(res_host, n) bytes (0 returned for bad arguments)
 *   counts_dev: n emf_mesh_counts_t
 *   bases_dev:  NULL, or 2 (n + 1) uint64: model m's first vertex and first triangle in the outputs, entry n = the
 *               totals (the size of the emit's outputs) */
size_t emf_hip_meshScratchBytesBatched(const int32_t* res_host, int n);
int emf_hip_meshCountBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, void* scratch_dev,
                             emf_mesh_counts_t* counts_dev, uint64_t* bases_dev, emf_stream_t stream);
/* vertices / normals: 3 floats per vertex of all models, triangles: 4 int32 per triangle of all models (sized by the
 * totals); the same scratch, table and res_host as the count. */
int emf_hip_meshEmitBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, const void* scratch_dev,
                            float* vertices, float* normals, int32_t* triangles, emf_stream_t stream);

/* The ignore_person block of EMFusion::render (EMFusion.cpp:139-150: compare, setTo, two masked
 * copyTo) in one launch: pixels labelled `id` get label 0 and the background's vertex / normal. */
int emf_hip_hideLabel(const emf_image_t* segmentation, int id, const emf_image_t* vertices,
                      const emf_image_t* normals, const emf_image_t* bgVertices, const emf_image_t* bgNormals,
                      emf_stream_t stream);

/* Replaces cuda::EMFusion::renderGPU (EMFusion.cu:100-186): Phong shading of the composited raycast
 * (vertices, normals f32x3; segmentation u8) into image (u8x3, RGB), coloured per label through
 * colorMap (256 x RGB, HOST memory, passed by value to the kernel).  Pixels without a vertex are
 * written as 0, so the reference's image.setTo(0) is not needed.  lightPos: the translation of
 * renderGPU's lightPose (EMFusion::render passes the identity, i.e. the camera centre). */
int emf_hip_renderPhong(const emf_image_t* vertices, const emf_image_t* normals,
                        const emf_image_t* segmentation, const uint8_t colorMap[768],
                        const float lightPos[3], const emf_image_t* image, emf_stream_t stream);

/* EMFusion::initObjsFromUnmatched's carving step (EMFusion.cpp:462-478): removes from the unmatched
 * instance mask `seg` (in place) the pixels the object `id` already claims -- its footprint in the
 * model segmentation, plus `matchMask` if a mask was matched to it (may be NULL) -- and counts the
 * mask's pixels before ([0]) and after ([1]).  The caller zeroes the mask if after / before < 0.5. */
int emf_hip_carveMask(const emf_image_t* seg, const emf_image_t* modelSeg, int id,
                      const emf_image_t* matchMask, uint32_t* counts_dev, emf_stream_t stream);

/* The two numbers of EMFusion::cleanUpObjs' association test (EMFusion.cpp:936-949):
 * count = |objSeg OR matchMask| (matchMask may be NULL), sum = sum of `assoc` over those pixels
 * (double accumulation like cv::cuda::sum, fixed order).  The object is spurious if
 * assocThresh * count > sum.  out_dev: emf_hip_maskAssociationMassBytes() bytes of device memory -- the answer in
 * out_dev[0], behind it the partials of the row bands (two launches; ABI 8: one emf_mask_mass_t used to suffice). */
typedef struct emf_mask_mass {
    double sum;
    uint32_t count;
    uint32_t pad_;
} emf_mask_mass_t;
size_t emf_hip_maskAssociationMassBytes(void);
int emf_hip_maskAssociationMass(const emf_image_t* objSeg, const emf_image_t* matchMask,
                                const emf_image_t* assoc, emf_mask_mass_t* out_dev,
                                emf_stream_t stream);

/* The association test of EMFusion::cleanUpObjs (EMFusion.cpp:922-980) over a model TABLE (level 3): the objects are
 * the slots [first, first + n) of models_dev (emf_model_t::hitMask = the object's raycast mask, ::assoc = its
 * association weights, both continuous width x height).  matchMasks_host: HOST array of n images, the mask matched
 * to object k this frame (data == NULL: none), or NULL = no masks.  One launch per EMF_MAX_BATCH objects (the masks
 * travel in the arguments), one finish launch for all.  out_dev[k] is byte for byte what emf_hip_maskAssociationMass
 * gives for object k alone (the level-1 entry is the one-object case of the same kernels).
 *   scratch_dev: emf_hip_maskAssociationMassScratchBytes(n) bytes (the row-band partials; 0 returned for a bad n)
 *   0 <= n <= EMF_MAX_MODELS - 1; n == 0 launches nothing unless verdicts are asked for.
 * Verdicts (verdict_dev != NULL): round_up(nall, 4) floats, all written: at listPos_host[k] (object k's position in
 * the job's creation-order list of nall objects) 1 if cleanUpObjs deletes it, else 0; 0 at every other position.  The
 * host rule (EMFusion.cpp:930-951): exLow_host[k] != 0 (existence probability below the threshold on a mask frame;
 * NULL = none) or visible_dev[first + k] == 0 (the integrate gate of the table, int32 per slot) or
 * double(assocThresh * float(count)) > sum.  Sharded ranks all-reduce (sum) the arrays: the joint verdicts. */
size_t emf_hip_maskAssociationMassScratchBytes(int n);
int emf_hip_maskAssociationMassBatched(const emf_model_t* models_dev, int first, int n, int width, int height,
                                       const emf_image_t* matchMasks_host, void* scratch_dev, emf_mask_mass_t* out_dev,
                                       float* verdict_dev, int nall, const int32_t* listPos_host,
                                       const int32_t* visible_dev, const uint8_t* exLow_host, float assocThresh,
                                       emf_stream_t stream);

/* The counts behind EMFusion::matchSegmentation (EMFusion.cpp:797-825) for ALL objects at once:
 * counts_dev[0] = pixels of `seg`; counts_dev[1 + id] = |seg AND (modelSeg == id)|;
 * counts_dev[257 + id] = |modelSeg == id|, id = 1..255 (513 uint32, cleared by the call).
 * IoU(id) = inter / (counts[0] + area - inter). */
int emf_hip_maskOverlap(const emf_image_t* seg, const emf_image_t* modelSeg, uint32_t* counts_dev,
                        emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Tracking: weighted Levenberg-Marquardt ICP on the TSDF
 * (TSDF.cpp:170-344, 375-395; EMFusion.cpp:672-724).  All LM state lives in device memory.
 * ---------------------------------------------------------------------------------------------- */

/* TSDFParams fields of the tracker (data.h:32-66) */
typedef struct emf_track_params {
    float huberThresh; /* 0.2  */
    float maxWeight;   /* maxTSDFWeight, 64 */
    float tau;         /* 1e3  */
    float eps1;        /* 1e-8 */
    float eps2;        /* 1e-8 */
    float nuInit;      /* 2    */
} emf_track_params_t;

/* Per-model Levenberg-Marquardt state (device memory; read it back after synchronising).
 * R, t = rel_pose_CO (camera -> volume), the quantity TSDF::prepareTracking sets up and
 * TSDF::syncTrack converts back: cam_pose = pose * rel_pose_CO. */
typedef struct emf_track_state {
    float R[9], t[3];
    float Rtrial[9], ttrial[3];
    float A[36], b[6], x[6];
    float mu, nu, rho, err, errNew;
    uint32_t maxIwBits;        /* float bits of max |min(intWeights, maxWeight)| at the current pose */
    uint32_t maxIwTrialBits;   /* ... at the trial pose */
    int32_t converged;         /* trackingConverged */
    int32_t firstIteration;
    int32_t evaluateGradient;
    int32_t haveTrial;
    int32_t iterations;        /* trial steps evaluated */
    int32_t accepted;          /* ... of which accepted (rho > 0) */
    int32_t iwSel;             /* which of the two weight images belongs to the current pose */
    /* bookkeeping of the fused step kernel (one launch per LM iteration, see emf_hip_trackIterate) */
    int32_t wSel;              /* which of the two per-pixel weight images belongs to the current pose */
    int32_t needAccum;         /* A, b, err must be summed at the current pose before the next solve */
    int32_t haveSpec;          /* spec[] holds them already (summed speculatively at the accepted trial pose) */
    float spec[28];            /* upper triangle of A (21), b (6), err -- moved into A, b, err by the next solve */
    int32_t checkB;            /* A, b are fresh: the max|b| < eps1 test is still to be made */
    int32_t pending;           /* what the last launch left in the partial sums: 0 nothing, 1 A/b/err at the
                                  current pose, 2 the trial step's error + A/b/err at the trial pose */
    int32_t body;              /* what the current launch does per pixel (same codes) */
    int32_t iterTarget;        /* `iterations` at which the current trackIterate call stops */
    /* |log| of the two poses (the step-size test of TSDF.cpp:292-296 needs the current pose's): kept with
     * the poses, so that no launch has to make them in front of its solve */
    float logCur, logTrial;
    /* factor on the current pose's per-pixel weight image: 1, or -- when a step was accepted whose weights had been
     * normalised by the previous pose's maximum although the accepted pose's is another -- the ratio of the two
     * maxima (see emf_hip_trackIterate) */
    float wFac;
} emf_track_state_t;

/* bytes of scratch per model for emf_hip_trackIterate on a width x height image */
size_t emf_hip_trackScratchBytes(int width, int height);

/* TSDF::prepareTracking for all models (TSDF.cpp:170-191): states[m] <- initial LM state with
 * rel_pose_CO = poseCO_host[m], which the caller has re-orthonormalised (the reference runs a
 * Householder QR of the rotation block on the host). */
int emf_hip_trackPrepare(emf_track_state_t* states_dev, const emf_pose_t* poseCO_host, int nmodels,
                         float nuInit, emf_stream_t stream);

/* `iterations` more LM iterations of every model in lock-step, as EMFusion::performTracking runs them
 * (EMFusion.cpp:673-684, 692-720), without host synchronisation: ONE launch per iteration.  Every
 * workgroup of a launch first finishes the previous launch in its own LDS copy of the state (adds the
 * partial sums in a fixed order, judges the pending trial step, solves for the next one -- the same
 * arithmetic in every workgroup, workgroup 0 stores the state), then evaluates the new trial pose per
 * pixel: its error under the current weights AND, speculatively, the Hessian sums the next iteration
 * needs if the step is accepted.  That speculation normalises the weights by the maximum integration
 * weight of the CURRENT pose (the trial pose's is known after the pass; it is the weight cap after a few
 * frames); when the two differ, the sums -- linear in the normaliser -- are multiplied by the ratio of the
 * maxima, and the accepted pose's weight image by the same factor where it is read (`wFac`): 2e-7 relative
 * from weights made anew.  (EMF_TRACK_RESCALE=0 in the environment: the sums are re-made at the accepted
 * pose by one extra launch, rounds 1-3.)  The call enqueues iterations + 3 launches (rounded up to even):
 * one spare for such an extra launch -- read `iterations` / `haveTrial` from the state to see how far a
 * model got; launches with nothing left to do return at once, as do converged models.  Each model's
 * `assoc` map supplies the association weights.
 * scratch_dev: nmodels * scratchBytesPerModel bytes (>= emf_hip_trackScratchBytes). */
int emf_hip_trackIterate(const emf_model_t* models_dev, emf_track_state_t* states_dev, int nmodels,
                         const emf_image_t* points, const emf_track_params_t* params,
                         void* scratch_dev, size_t scratchBytesPerModel, int iterations,
                         emf_stream_t stream);

/* The same loop, launch by launch, for a host that does not want to guess how many iterations a
 * stage needs: emf_hip_trackStep enqueues launch number `launch` (0, 1, 2, ... since the stage's
 * emf_hip_trackPrepare or since the last call of emf_hip_trackIterate; launch 0 also runs the weight-
 * maximum pass and lets every model do `iterations` more iterations) and has the device report to
 * `watch`, which must be host memory the device can write (hipHostMalloc, coherent):
 *   watch[0]      <- seq when the launch has begun (any nonzero number the caller increases per launch),
 *   watch[1 + m]  <- 1 when model m has converged, 2 when it has done its iterations, else 0 -- in the lower half;
 *                    the upper half is seq's (a stage tag, if the caller puts one there: launches of the previous stage
 *                    that are still queued write too).
 * These are hints to stop enqueuing (written with system-scope stores while the stream runs: keep a
 * few launches ahead of watch[0], stop when every watch[1 + m] != 0); the states are read as usual.
 * The number of launches of a stage must be even (the state alternates between the caller's array
 * and a shadow in the scratch): end with one more launch if it is not -- a launch with nothing to
 * do returns at once.  watch may be NULL.
 * finalStates (host memory the device can write, nmodels entries, or NULL): the launch that finds model m done
 * stores its state to finalStates[m] IN FRONT OF watch[1 + m] (system scope, release): a host that has seen the
 * word (and an acquire fence) reads the stage's result there -- no copy command, no wait for the stream. */
int emf_hip_trackStep(const emf_model_t* models_dev, emf_track_state_t* states_dev, int nmodels,
                      const emf_image_t* points, const emf_track_params_t* params,
                      void* scratch_dev, size_t scratchBytesPerModel, int launch, int iterations,
                      uint32_t* watch, uint32_t seq, emf_track_state_t* finalStates, emf_stream_t stream);

/* The two weight images a stage leaves behind, as the reference's debug output reads them at the end of a frame
 * (TSDF::getHuberWeights / getTrackingWeights, TSDF.cpp:346-354: `trackWeights` = min(huberThresh / |tsdf value|, 1)
 * with x / 0 := 0, TSDF.cpp:222-231; `intWeights` = that x the clamped, NORM_INF-normalised integration weights x the
 * association weights, TSDF.cpp:233-256) -- evaluated at the pose the stage ended with (states_dev[m].R / t), with the
 * body's own arithmetic (k_track_step): the tracker itself never materialises the Huber image and keeps only the
 * product.  Call it behind the stage's last launch and before anything overwrites the models' `assoc` maps.
 * huber_dev / track_dev: nmodels dense width x height float images each (either may be NULL). */
int emf_hip_trackWeightImages(const emf_model_t* models_dev, const emf_track_state_t* states_dev, int nmodels,
                              const emf_image_t* points, const emf_track_params_t* params,
                              const void* scratch_dev, size_t scratchBytesPerModel, float* huber_dev,
                              float* track_dev, emf_stream_t stream);

/* Level 1: replaces emf::cuda::TSDF::computePoseGradients (TSDF.cuh, TSDF.cu:603-660).
 * grads6: (W*H) x 6 f32, every row written (zeros where the reference leaves its setTo(0));
 * grads: N^3 x 3 gradient volume or NULL (forward differences blended on the fly, same values). */
int emf_hip_computePoseGradients(const float* tsdf, const float* grads, const emf_image_t* points,
                                 const float R_CO[9], const float t_CO[3], const int32_t res[3],
                                 float voxelSize, float* grads6, emf_stream_t stream);

/* ---- direct peer-write exchanges fused into the path's kernels (types: see the peer section above) ---- */
/* The E-step's exchange fused into the path (reference EMFusion.cpp:653-665; SURVEY 8e exchange 1):
 *   estepBatchedPeer          = emf_hip_estepBatched / ...FromDepth (depth != NULL) with normalize = 0 whose per-pixel
 *                               sum of the OBJECT maps goes straight into slot[me] (offset 0, W*H floats) of every peer;
 *   peerNormalizeAssociation  waits, sums the slots in rank order (-> objSum, optional), norm := maps[0] + that sum,
 *                               maps[k] := maps[k] / norm (x / 0 := 0): the values of peerWaitReduceSumF32 followed
 *                               by emf_hip_normalizeAssociation(maps, nmaps, 1, objSum, norm).  nmaps <= 16. */
int emf_hip_estepBatchedPeer(const emf_model_t* models_dev, const emf_pose_t* poseCO_host, int nmodels,
                             const emf_image_t* depth, const float K[9], const emf_image_t* points,
                             const emf_peer_t* group, uint32_t seq, emf_stream_t stream);
int emf_hip_peerNormalizeAssociation(const emf_peer_t* group, uint32_t seq, const emf_image_t* maps_host, int nmaps,
                                     const emf_image_t* objSum, const emf_image_t* norm, emf_stream_t stream);
/* The raycast's exchange fused into the path (reference EMFusion.cpp:760-794; SURVEY 8e exchange 2 + the row bands
 * of the replicated background's raycast).  Slot layout per sender: [W*H u64 hit keys][W*H f32 background
 * raylengths][W*H u8 background hit mask] -- emf_hip_peerRaycastSlotBytes(W, H).
 *   packHitKeysPeer          = emf_hip_packHitKeys whose keys go into slot[me] of every peer, together with rows
 *                              [bandRow0, bandRow0 + bandRows) of bgRay / bgMask (bandRows = 0: no bands);
 *   compositeFromKeysPeer    waits, takes the minimum key over the slots, fetches the foreign bands of bgRay / bgMask
 *                              from their owners' slots (rows of owner r: [r * bandRowsPerRank, ...); also stored into
 *                              the local images), then composites exactly as emf_hip_compositeFromKeys and counts
 *                              visibility into visCounts (which must be zero at the launch's start);
 *   visibilityFlagsMirror    the integrate gate from those counts (as visibilityFlagsIndexed), the nall counts mirrored
 *                              to host-visible memory, visCounts left cleared for the next frame. */
size_t emf_hip_peerRaycastSlotBytes(int width, int height);
int emf_hip_packHitKeysPeer(int nlocal, const int32_t* listPos_host, const emf_image_t* objRay_host,
                            const emf_image_t* objSeg_host, const emf_image_t* bgRay, const emf_image_t* bgMask,
                            int bandRow0, int bandRows, const emf_peer_t* group, uint32_t seq, emf_stream_t stream);
int emf_hip_compositeFromKeysPeer(const emf_peer_t* group, uint32_t seq, int bandRowsPerRank, int nall,
                                  const int32_t* ids_host, int nlocal, const int32_t* listPos_host,
                                  const emf_image_t* objRay_host, const emf_image_t* objVert_host,
                                  const emf_image_t* objNorm_host, const emf_image_t* bgRay, const emf_image_t* bgVert,
                                  const emf_image_t* bgNorm, const emf_image_t* bgMask, const emf_image_t* ray,
                                  const emf_image_t* vert, const emf_image_t* norm, const emf_image_t* seg,
                                  const emf_image_t* diff, const emf_image_t* noObj, int boundary, int32_t* visCounts,
                                  emf_stream_t stream);
int emf_hip_visibilityFlagsMirror(int32_t* visCounts, int nall, int nmodels, const int32_t* countIndex_host,
                                  int visibilityThresh, int32_t* visible_dev, int32_t* countsMirror, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-voxel colour (new behaviour: the reference hands its RGB frames to Mask R-CNN only).
 * A COLOUR VOLUME holds uint16_t[4] per voxel, in the voxel order of the tsdf: R, G, B as 8.8 fixed
 * point (q = rint(c * 256), c in [0, 255]) and the colour weight Wc as 8.8 fixed point.  Colour has a
 * weight of its own: a voxel collects TSDF weight from free-space updates long before a surface
 * reaches it, and 16 bits per channel because an 8-bit running average stalls near the weight cap.
 * ---------------------------------------------------------------------------------------------- */

/* Colour update of all models in one launch (level 3, 1 <= nmodels <= EMF_MAX_BATCH; longer tables in
 * chunks).  A voxel of model m is VISITED under exactly the gates of the TSDF update (TSDF.cu:345-380:
 * p_cam.z > 0, rounded pixel inside the image, depth > 0; same pose, same depth image, same
 * visible_dev gate) and COLOURED iff |sdf| < truncdist and aw = models_dev[m].assoc(py, px) > 0.
 * Then, in float32 without contraction, per channel k:
 *     W = Wc_q / 256.f;  c_old = C_q[k] / 256.f;  c = (float) rgb(py, px)[k];
 *     C_q[k] = (uint16_t) lrintf(((W * c_old + aw * c) / (W + aw)) * 256.f);
 *     Wc_q   = (uint16_t) lrintf(fminf(W + aw, maxWeight) * 256.f);     (maxWeight < 256)
 * with W read once, before any channel is written.  Every other voxel keeps its four values and is
 * neither read nor written.  Projection, pixel rounding and the band decision are the TSDF update's own
 * device functions.  Reads nothing the TSDF integration writes: it only has to follow the E-step that made
 * the association maps and whatever wrote visible_dev.
 *   colors_dev : DEVICE array of nmodels colour-volume pointers, parallel to models_dev (the model table
 *                keeps its layout); a NULL entry skips that model
 *   rgb        : u8 x 3 image of the depth image's size
 *   invLambda  : NULL, or emf_hip_computeInvLambda's table (same values)
 *   stats      : NULL, or one u64 device counter this call ADDS the number of coloured voxels to */
int emf_hip_integrateColorBatched(const emf_model_t* models_dev, uint16_t* const* colors_dev,
                                  const emf_pose_t* poseOC_host, const int32_t* res_host, int nmodels,
                                  const int32_t* visible_dev, const emf_image_t* depth, const emf_image_t* invLambda,
                                  const emf_image_t* rgb, const float K[9], uint64_t* stats, emf_stream_t stream);

/* emf_hip_copyValues for a colour volume (ObjTSDF::resize): dst(v) = src(v + offset) inside the source,
 * (0, 0, 0, 0) elsewhere; every voxel of dst is written. */
int emf_hip_copyColorValues(const uint16_t* src, uint16_t* dst, const int32_t offset[3], const int32_t srcRes[3],
                            const int32_t dstRes[3], emf_stream_t stream);

/* Vertex colours of a mesh: u8 x 3 per vertex, in the vertex order of emf_hip_meshEmit / emf_hip_meshEmitBatched for
 * the same volume(s) and the same scratch -- valid after the matching emf_hip_meshCount / ...Batched, before or after
 * the emit, which it does not disturb.  A vertex on the edge between voxels 1 and 2 takes, per channel,
 * rint(c1 + mu * (c2 - c1)) with c = C_q / 256.f and vertexInterp's mu (TSDF.cu:909-920) -- c1 or c2 outright in its
 * three early-return cases.  An endpoint with Wc_q == 0 contributes the other endpoint's colour; if both are
 * uncoloured the vertex is (0, 0, 0).
 *   color      : the volume's colour volume;  colors_dev: DEVICE array of n colour-volume pointers parallel to
 *                models_dev (a NULL entry: that model's vertices are (0, 0, 0))
 *   colors     : 3 bytes per vertex (all models concatenated like the emit's vertices) */
/* Coloured views: the colour under every pixel of a view, then the usual shading from it.
 *   sampleColor      per pixel with a vertex (vertices != 0; f32 x 3 in the VIEWER frame, as emf_hip_renderView writes
 *                    them) the colour of the voxel nearest to the vertex -- no interpolation -- in the model the
 *                    segmentation names (label 0: slot 0, label of ids_host[s - 1]: slot s, ids saturated to u8 as the
 *                    composite writes them), rounded from 8.8 fixed point to the nearest level; a voxel with
 *                    Wc_q == 0, a vertex outside its volume, a model without a colour volume (NULL entry, or colors_dev
 *                    NULL) and a label no slot carries fall back to colorMap[label].  Pixels without a vertex: 0.
 *                    poseVO_dev: DEVICE emf_pose_t[nmodels], viewer -> volume, the array emf_hip_renderView took.
 *                    Slots above 254 are not addressable by a u8 label and fall back too.
 *   renderPhongColor emf_hip_renderPhong with the diffuse colour of each pixel read from `colors` (u8 x 3) instead of
 *                    colorMap[segmentation]: the same terms, the same bits for the same colour. */
int emf_hip_sampleColor(const emf_model_t* models_dev, uint16_t* const* colors_dev, const emf_pose_t* poseVO_dev,
                        const int32_t* ids_host, int nmodels, const emf_image_t* vertices, const emf_image_t* segmentation,
                        const uint8_t colorMap[768], const emf_image_t* colors, emf_stream_t stream);
int emf_hip_renderPhongColor(const emf_image_t* vertices, const emf_image_t* normals, const emf_image_t* colors,
                             const float lightPos[3], const emf_image_t* image, emf_stream_t stream);
int emf_hip_meshColors(const float* tsdf, const float* weights, const uint8_t* fgVolMask, const uint16_t* color,
                       const int32_t res[3], const void* scratch_dev, uint8_t* colors, emf_stream_t stream);
int emf_hip_meshColorsBatched(const emf_model_t* models_dev, uint16_t* const* colors_dev, const int32_t* res_host, int n,
                              const void* scratch_dev, uint8_t* colors, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Welded meshes (new behaviour: the reference's marching cubes emits a triangle soup -- every cube its
 * own copy of every vertex it touches).  Opt-in; the soup entries above are untouched.
 * Soup vertex i was emitted by a cube for one of its 12 edges; it lies on the GRID EDGE joining two voxels
 * that differ in one coordinate.  Its EDGE KEY is
 *     (uint64_t) slot << 48  |  3 * linear(lower voxel) + axis,
 * linear = (z * Ny + y) * Nx + x, axis 0 / 1 / 2 for x / y / z, slot = the model's index in the table
 * (0 for a level-1 call) -- also when vertexInterp returned a corner outright: welding is by edge, never
 * by position.  WELDED vertex j is the first soup vertex, in soup order, of the j-th distinct key in order of
 * first occurrence: that copy's position, normal and colour, bit for bit.  WELDED triangles are the soup's,
 * same order and (3, i0, i1, i2) layout, every index replaced by the welded index of its vertex's key,
 * model-local in a table.  A pure function of the volume(s): no result depends on the order workgroups run in.
 * ---------------------------------------------------------------------------------------------- */

/* Edge keys of the soup of the last emf_hip_meshCount / ...Batched on the same volume(s) and scratch: one u64
 * per soup vertex, in the vertex order of the emit (all models concatenated).  Like emf_hip_meshColors it walks
 * the listed surface chunks once more, may run before or after the emit and does not disturb it. */
int emf_hip_meshEdgeKeys(const float* tsdf, const float* weights, const uint8_t* fgVolMask, const int32_t res[3],
                         const void* scratch_dev, uint64_t* keys, emf_stream_t stream);
int emf_hip_meshEdgeKeysBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, const void* scratch_dev,
                                uint64_t* keys, emf_stream_t stream);

/* Bytes of device scratch welding a soup of soupVertices needs: an open-addressing table of the smallest power
 * of two >= 2 * soupVertices (u64 key + u32 first index per slot), two u32 per soup vertex and the scan's
 * per-workgroup sums -- under 57 bytes per soup vertex plus 1 KiB, nothing sized by the volume.  0 if
 * soupVertices > 2^30 (the entries below then return EMF_E_LIMIT). */
size_t emf_hip_meshWeldScratchBytes(uint64_t soupVertices);

/* First occurrence and rank of every key.  Leaves in weld_scratch_dev what emf_hip_meshWeldEmit reads (the welded
 * index of every soup vertex) and writes, to device memory,
 *   welded_counts : n u32, the welded vertices of each model
 *   welded_bases  : NULL or n + 1 u64, each model's first welded vertex in the concatenated output and the total
 *   soup_bases    : DEVICE, what emf_hip_meshCountBatched wrote to bases_dev (2 (n + 1) u64: vertex and triangle bases
 *                   interleaved); the level-1 form is n == 1 with bases {0, 0, soupVertices, soupTriangles} implied.
 * soupVertices == 0 is valid: nothing is launched but the clearing of the outputs.  1 <= n <= EMF_MAX_MODELS.
 * Probing is bounded by the table's capacity; a table that cannot hold the keys (impossible with the documented
 * size) raises a flag in the scratch instead of spinning: see emf_hip_meshWeldStatus. */
int emf_hip_meshWeldCount(const uint64_t* keys, uint64_t soupVertices, void* weld_scratch_dev, uint32_t* welded_count,
                          emf_stream_t stream);
int emf_hip_meshWeldCountBatched(const uint64_t* keys, uint64_t soupVertices, const uint64_t* soup_bases_dev, int n,
                                 void* weld_scratch_dev, uint32_t* welded_counts, uint64_t* welded_bases,
                                 emf_stream_t stream);

/* Waits for the stream and returns EMF_OK, or EMF_E_LIMIT if the last emf_hip_meshWeldCount on this scratch ran out
 * of table (its outputs are then meaningless).  The one synchronising entry of the group: call it where the counts
 * are read back anyway. */
int emf_hip_meshWeldStatus(const void* weld_scratch_dev, uint64_t soupVertices, emf_stream_t stream);

/* Compact and remap: soup arrays in (as the emit / colour entries wrote them: 3 f32, 3 f32, 3 u8 per vertex, 4 i32
 * per triangle), welded arrays out.  colors / welded_colors: both NULL or both given.  triangles holds
 * soupTriangles (3, i0, i1, i2) records with model-local soup indices; welded_triangles may be the same buffer.
 * The vertex outputs must not alias the inputs.  The level-1 form takes no bases. */
int emf_hip_meshWeldEmit(const void* weld_scratch_dev, uint64_t soupVertices, uint64_t soupTriangles,
                         const float* vertices, const float* normals, const uint8_t* colors, const int32_t* triangles,
                         float* welded_vertices, float* welded_normals, uint8_t* welded_colors,
                         int32_t* welded_triangles, emf_stream_t stream);
int emf_hip_meshWeldEmitBatched(const void* weld_scratch_dev, uint64_t soupVertices, uint64_t soupTriangles,
                                const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                const float* vertices, const float* normals, const uint8_t* colors,
                                const int32_t* triangles, float* welded_vertices, float* welded_normals,
                                uint8_t* welded_colors, int32_t* welded_triangles, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh components (new behaviour: the reference has none).  Opt-in; the entries above are untouched.
 * The graph of one model's WELDED mesh has the model's welded vertices as nodes; two vertices are joined when a
 * triangle has both -- by index only: vertices of different grid edges that coincide at a voxel corner stay
 * unconnected.  A vertex's LABEL is the smallest model-local welded index in its component, a component's SIZE
 * its number of triangles (a vertex no triangle uses is a component of size 0).  Components never cross models.
 * FILTER: each model has (min_triangles, largest_only).  A component is kept if its size >= min_triangles
 * (min_triangles <= 1 keeps every size) and, with largest_only, only if it is also the model's largest by
 * triangles, a tie going to the smaller label.  The output holds the kept vertices in welded order (position,
 * normal and colour bits unchanged) and the kept triangles in order, (3, i0, i1, i2), re-indexed to the
 * compacted vertices, model-local; each model's slice is what the filter gives for that mesh alone, possibly
 * empty.  A pure function of the welded mesh: no result depends on the order workgroups run in.
 * The entries take the welded arrays as emf_hip_meshWeldEmit / ...Batched leave them: triangles hold
 * (3, i0, i1, i2) records with model-local welded indices; the table forms take soup_bases_dev (2 (n + 1) u64,
 * of which the TRIANGLE bases, the odd entries, are read) and welded_bases_dev (n + 1 u64), both on the device.
 * The level-1 forms are n == 1 with bases {0, weldedVertices} and {0, nTriangles} implied.
 * Limits: weldedVertices <= 2^30, nTriangles < 2^31, 1 <= n <= EMF_MAX_MODELS.
 * A triangle index outside its model's welded vertices is never dereferenced: the triangle joins nothing, is
 * dropped by the filter, and emf_hip_meshComponentsStatus reports EMF_E_ARG.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of device scratch: three u32 per welded vertex, one per triangle, the scans' per-workgroup sums and 4 KiB
 * of per-model cells -- under 13 bytes per welded vertex + 5 per triangle + 6 KiB.  0 beyond the limits. */
size_t emf_hip_meshComponentsScratchBytes(uint64_t weldedVertices, uint64_t nTriangles);

/* Labels every welded vertex and counts every component; leaves both in cc_scratch_dev for the entries below.
 *   labels : NULL or weldedVertices i32, model-local
 *   sizes  : NULL or weldedVertices u32, the size of the vertex's component
 * weldedVertices == 0 launches nothing. */
int emf_hip_meshComponentsLabel(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles, void* cc_scratch_dev,
                                int32_t* labels, uint32_t* sizes, emf_stream_t stream);
int emf_hip_meshComponentsLabelBatched(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                       const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                       void* cc_scratch_dev, int32_t* labels, uint32_t* sizes, emf_stream_t stream);

/* After emf_hip_meshComponentsLabel on the same arguments and scratch: keep flags and their ranks.
 *   min_triangles  : HOST, NULL (0 for every model) or n u32; read before the call returns
 *   largest_only   : HOST, NULL (off) or n u8
 * and, to device memory,
 *   kept_counts    : 2 n u32, the kept vertices and triangles of each model, interleaved
 *   kept_bases     : NULL or 2 (n + 1) u64, each model's first kept vertex and triangle in the concatenated output,
 *                    interleaved, and the totals (the layout of emf_hip_meshCountBatched's bases)
 *   components, kept_components : NULL or n u32 each
 * weldedVertices == 0 launches nothing but the clearing of the outputs. */
int emf_hip_meshComponentsFilterCount(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                      void* cc_scratch_dev, const uint32_t* min_triangles, const uint8_t* largest_only,
                                      uint32_t* kept_counts, uint32_t* components, uint32_t* kept_components,
                                      emf_stream_t stream);
int emf_hip_meshComponentsFilterCountBatched(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                             const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                             void* cc_scratch_dev, const uint32_t* min_triangles,
                                             const uint8_t* largest_only, uint32_t* kept_counts, uint64_t* kept_bases,
                                             uint32_t* components, uint32_t* kept_components, emf_stream_t stream);

/* Waits for the stream and returns EMF_OK, or EMF_E_ARG if the last emf_hip_meshComponentsLabel on this scratch met
 * a triangle index outside its model's welded vertices.  The one synchronising entry of the group: call it where
 * the counts are read back anyway. */
int emf_hip_meshComponentsStatus(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                                 emf_stream_t stream);

/* Compact: welded arrays in, kept arrays out (sized by the kept counts).  colors / kept_colors: both NULL or both
 * given.  No output may alias its input -- triangles move to lower positions, so not the triangles either. */
int emf_hip_meshComponentsEmit(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                               const float* vertices, const float* normals, const uint8_t* colors,
                               const int32_t* triangles, float* kept_vertices, float* kept_normals, uint8_t* kept_colors,
                               int32_t* kept_triangles, emf_stream_t stream);
int emf_hip_meshComponentsEmitBatched(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                                      const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                      const float* vertices, const float* normals, const uint8_t* colors,
                                      const int32_t* triangles, float* kept_vertices, float* kept_normals,
                                      uint8_t* kept_colors, int32_t* kept_triangles, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Simplified meshes (new behaviour: the reference has none).  Opt-in; the entries above are untouched.
 * Vertex clustering (Rossignac-Borrel) of an indexed mesh, or of a table of n meshes, in the form the filter takes:
 * vertices and normals 3 f32 each, optional colours 3 u8, triangles (3, i0, i1, i2) i32 with model-local indices,
 * tri_bases_dev (2 (n + 1) u64, of which the TRIANGLE bases, the odd entries, are read) and vertex_bases_dev
 * (n + 1 u64), both on the device and both NULL for one mesh (n == 1, bases {0, nVertices} and {0, nTriangles}).
 *   CELL of a vertex, per axis:  c = floor(((double)p - (double)origin) / (double)cell), in double, no reciprocal,
 *       no contraction; negative coordinates floor.  cell is the model's, in metres; a model with cell <= 0 is
 *       PASSED THROUGH: every vertex its own cluster, every vertex kept, every triangle with in-range indices kept
 *       (also one with two equal indices), so its arrays come out as they went in.
 *   KEY  (uint64_t) slot << 48 | (cz + 2^15) << 32 | (cy + 2^15) << 16 | (cx + 2^15), slot = the model's index in
 *       the table (0 for one mesh): clusters never cross models.
 *   CLUSTER j of a model is the j-th distinct key in order of first occurrence, i.e. by its smallest member index.
 *   CLUSTER VERTEX  one member: that member's position, normal and colour, bit for bit.  Several members:
 *       position per axis  q = llrint(ldexp((double)p, 20)) summed in int64, (float)(((double)sum / (double)count)
 *                          * 2^-20)
 *       normal             the same, a component that is not finite or has |n| >= 2^10 counting as 0 (the mean of
 *                          the raw gradients: it is not normalised)
 *       colour per channel (2 * sum + count) / (2 * count) in integers
 *       -- sums of integers, so no result depends on the order workgroups run in.
 *   TRIANGLES  every index is replaced by its cluster's; a triangle with two equal cluster indices is dropped; the
 *       kept ones stay in input order.  Two kept triangles over the same three clusters are both kept.
 *   VERTICES OUT  the clusters some kept triangle references, in cluster order; the triangles are re-indexed to them,
 *       model-local.  A model may come out empty.  Every output is a pure function of the input arrays.
 *   REFUSALS, reported by emf_hip_meshSimplifyStatus; nothing spins, nothing is dereferenced out of range:
 *       EMF_E_LIMIT  a coordinate of a clustered vertex that is NaN or infinite or has |p| >= 2^10 m, a cell coordinate
 *                    outside [-2^15, 2^15), a table that cannot hold the keys; the outputs are then meaningless
 *       EMF_E_ARG    a triangle index outside its model's vertices: the triangle is dropped (in a passed-through
 *                    model too) and the rest of the output is what the mesh without it gives
 *       with both, EMF_E_LIMIT is reported.
 * Limits: nVertices <= 2^30, nTriangles < 2^31, 1 <= n <= EMF_MAX_MODELS.
 * Not done: merging kept triangles that span the same three clusters (a 96-bit triple does not fit the table's
 * 64-bit key), quadric error placement, normalising the merged normal.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of device scratch: an open-addressing table of the smallest power of two >= 2 * vertices (u64 key + u32
 * first index per slot), 22 words of cluster cells per vertex, one word per triangle and the scans' per-workgroup
 * sums -- under 137 bytes per vertex + 5 per triangle + 8 KiB.  0 beyond the limits. */
size_t emf_hip_meshSimplifyScratchBytes(uint64_t vertices, uint64_t triangles);

/* Clusters, sums, kept flags and their ranks; leaves in simplify_scratch_dev what emf_hip_meshSimplifyEmit reads.
 *   colors        : NULL or the colours; the same choice goes to the emit
 *   cells         : HOST, n f32 (finite; <= 0 passes the model through); read before the call returns
 *   origin        : HOST, NULL (0, 0, 0) or 3 finite f32
 * and, to device memory,
 *   kept_counts   : 2 n u32, the vertices and triangles of each simplified model, interleaved
 *   kept_bases    : NULL or 2 (n + 1) u64, each model's first vertex and triangle in the concatenated output,
 *                   interleaved, and the totals (the layout of emf_hip_meshCountBatched's bases)
 *   clusters      : NULL or n u32, the clusters met in each model (referenced or not)
 * nVertices == 0 launches nothing but the clearing of the outputs. */
int emf_hip_meshSimplifyCount(const float* vertices, const float* normals, const uint8_t* colors,
                              const int32_t* triangles, uint64_t nVertices, uint64_t nTriangles,
                              const uint64_t* tri_bases_dev, const uint64_t* vertex_bases_dev, int n, const float* cells,
                              const float origin[3], void* simplify_scratch_dev, uint32_t* kept_counts,
                              uint64_t* kept_bases, uint32_t* clusters, emf_stream_t stream);

/* Waits for the stream and returns EMF_OK or the refusal of the last emf_hip_meshSimplifyCount on this scratch.  The
 * one synchronising entry of the group: call it where the counts are read back anyway. */
int emf_hip_meshSimplifyStatus(const void* simplify_scratch_dev, uint64_t nVertices, uint64_t nTriangles,
                               emf_stream_t stream);

/* Input arrays in (the ones the count saw), simplified arrays out (sized by the kept counts).  colors / kept_colors:
 * both NULL or both given.  No output may alias its input: EMF_E_ARG with nothing enqueued. */
int emf_hip_meshSimplifyEmit(const void* simplify_scratch_dev, uint64_t nVertices, uint64_t nTriangles,
                             const uint64_t* tri_bases_dev, const uint64_t* vertex_bases_dev, int n, const float* vertices,
                             const float* normals, const uint8_t* colors, const int32_t* triangles, float* kept_vertices,
                             float* kept_normals, uint8_t* kept_colors, int32_t* kept_triangles, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Packed buffers (new behaviour: the reference has no checkpoint).  A device buffer of nbytes (a positive
 * multiple of 4, at most 2^40, 16-byte aligned) is a sequence of 1024-byte CHUNKS of 256 32-bit words; the last
 * chunk may be ragged and only its valid words are read, compared or written.  Classification compares bits,
 * never floats:
 *     class 0  every word is 0x00000000
 *     class 1  every word equals the same non-zero word (-0.0f, a NaN pattern, the capped weight 64.0f ...)
 *     class 2  anything else (a LITERAL chunk)
 * The RANK of a class-1 / class-2 chunk is the number of chunks of its class before it, so the uniform words and
 * the literals are in chunk order on every run (placement is by scan, never by atomics).  The packed record the
 * host classes and emfusion_amd.ops.pack_buffer assemble from these arrays (little-endian):
 *     u64 nbytes; u32 nchunks; u32 nuniform; u32 nliteral; u32 0
 *     u8  class[nchunks]            zero-padded to a multiple of 8 bytes
 *     u32 uniform[nuniform]         chunk order, zero-padded to a multiple of 8 bytes
 *     u8  literal[nliteral][1024]   chunk order; a ragged last chunk is zero-padded
 * All byte offsets are 64-bit.  No entry allocates, copies synchronously or waits.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of device scratch emf_hip_packRank needs for a buffer of nbytes (8 per 256 chunks, plus 8); 0 if nbytes is 0
 * or above 2^40. */
size_t emf_hip_packScratchBytes(uint64_t nbytes);

/* classes[c] (u8) and words[c] (u32, the chunk's first word) for every chunk c; both hold nchunks =
 * ceil(nbytes / 1024) entries.  One wave per chunk, every byte of src read once. */
int emf_hip_packClassify(const void* src, uint64_t nbytes, uint8_t* classes, uint32_t* words, emf_stream_t stream);

/* From a class array (device) of a buffer of nbytes:
 *   ranks[c]           : nchunks u32, the rank of chunk c in its class (0 for class 0)
 *   uniform[r]         : the word of the class-1 chunk of rank r (words: what emf_hip_packClassify wrote);
 *                        words and uniform may both be NULL (restoring: the words come from the record)
 *   literal_chunks[r]  : the chunk index of the literal of rank r
 *   totals             : 2 u32 {nuniform, nliteral}
 * uniform and literal_chunks hold nchunks entries (the totals are not known before the call).  A class byte
 * above 2 counts as class 0 here and is skipped by the unpack entries. */
int emf_hip_packRank(const uint8_t* classes, const uint32_t* words, uint64_t nbytes, void* scratch_dev, uint32_t* ranks,
                     uint32_t* uniform, uint32_t* literal_chunks, uint32_t* totals, emf_stream_t stream);

/* Copies the literal chunks of ranks [first, first + count) to arena (count * 1024 bytes, 16-byte aligned), a ragged
 * last chunk zero-padded: a volume moves through a bounded arena, range by range.  first + count <= nchunks is
 * checked here; that it is <= nliteral is the caller's (entries of literal_chunks past nliteral are not chunk
 * indices; an index outside the buffer is skipped, never dereferenced).  count == 0 launches nothing. */
int emf_hip_packGather(const void* src, uint64_t nbytes, const uint32_t* literal_chunks, uint32_t first, uint32_t count,
                       void* arena, emf_stream_t stream);

/* Unpack is emf_hip_unpackFill once plus emf_hip_unpackLiterals per rank range; together they write every valid
 * word of dst exactly once -- no prior clear is needed and nothing past nbytes is written.
 * unpackFill writes the class-0 chunks (zeros) and the class-1 chunks (uniform[ranks[c]], nuniform entries; a rank
 * at or past nuniform writes nothing); unpackLiterals writes the literals of ranks [first, first + count) from
 * arena, laid out as emf_hip_packGather leaves it. */
int emf_hip_unpackFill(void* dst, uint64_t nbytes, const uint8_t* classes, const uint32_t* ranks, const uint32_t* uniform,
                       uint32_t nuniform, emf_stream_t stream);
int emf_hip_unpackLiterals(void* dst, uint64_t nbytes, const uint32_t* literal_chunks, uint32_t first, uint32_t count,
                           const void* arena, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Motion masks (new behaviour: the reference takes its instance masks from Mask R-CNN).  Opt-in; nothing above
 * is touched.  Instance proposals from geometry alone: connected regions of pixels whose measurement lies IN
 * FRONT of the background model's own raycast by more than a margin.
 * Inputs, both dense (no row padding), device memory:
 *   points        : w x h x 3 f32, the frame's points in the camera frame (emf_hip_computePoints)
 *   bg_raylengths : w x h f32, the background's raycast: the distance along the pixel's ray, 0 = the ray missed
 * With p the pixel's point, m = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z) (every operation rounded on its own) and
 * b its background ray length:
 *   1 candidates  a pixel is a CANDIDATE iff p.z > 0 and b > 0 and b - m > band.  A pixel whose background ray
 *                 missed is unknown, not novel: never a candidate.  NaN fails every comparison.
 *   2 erosion     `erode` passes of 3 x 3 binary erosion; outside the image counts as not-candidate.
 *   3 labels      4-connected components of the eroded candidates, two neighbours joined only if
 *                 |m_a - m_b| <= continuity.  A component's LABEL is the smallest linear index y * w + x in it.
 *   4 selection   components of at least min_pixels pixels, by area descending, ties to the smaller label, the
 *                 first max_masks of them: the PROPOSALS, their position in that order their RANK.
 *   5 outputs     labels : w x h i32, the rank of the pixel's proposal, -1 for every other pixel
 *                 masks  : max_masks planes of w x h u8, plane r = 1 inside proposal r, 0 elsewhere; planes at and
 *                          past the count are written as zeros
 *                 info   : max_masks emf_motion_info_t, entries at and past the count zeroed
 *                 count  : one i32, the number of proposals
 * Integer work and single comparisons on floats only: the outputs are a pure function of the inputs, whatever
 * order the workgroups run in.  Nothing allocates, copies to the host or waits.
 * Every rejected argument -- a NULL pointer included -- returns EMF_E_ARG with nothing enqueued; w * h <= 2^30.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_MOTION_MAX_MASKS 16

typedef struct emf_motion_params {
    float band;         /* m, >= 0: the candidate margin.  0.08 by default; the host classes use the background's
                           truncation distance, below which the TSDF itself cannot tell "in front" from noise */
    float continuity;   /* m, >= 0: the largest ray-length step across which neighbours still join.  0.05 */
    int32_t erode;      /* 0 .. 3 erosion passes.  1: removes the mixed pixels of a depth edge and one-pixel bridges */
    int32_t min_pixels; /* >= 0: the smallest component area kept.  200 */
    int32_t max_masks;  /* 1 .. EMF_MOTION_MAX_MASKS.  8 */
} emf_motion_params_t;

typedef struct emf_motion_info {
    int32_t label;          /* the smallest linear index of the proposal's pixels */
    int32_t area;           /* its pixels */
    int32_t x0, y0, x1, y1; /* its bounding box, both corners inclusive */
} emf_motion_info_t;

/* Bytes of device scratch for a w x h frame: 18 bytes per pixel plus the scan's per-workgroup sums, under
 * 19 bytes per pixel + 1 KiB.  0 for a size or a max_masks outside the limits. */
size_t emf_hip_motionMasksScratchBytes(int w, int h, int max_masks);

/* Stages 1-5 on `stream`: 9 + erode launches.  scratch_dev: emf_hip_motionMasksScratchBytes(w, h, max_masks)
 * bytes, 16-byte aligned, contents irrelevant before and meaningless after.  params is read before the call
 * returns. */
int emf_hip_motionMasks(const float* points, const float* bg_raylengths, int w, int h, const emf_motion_params_t* params,
                        void* scratch_dev, int32_t* labels, uint8_t* masks, emf_motion_info_t* info, int32_t* count,
                        emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rolling a volume (new behaviour: the reference's background never moves).  Opt-in; nothing above is touched.
 * One launch shifts a volume by whole voxels from one copy (src*) into a DIFFERENT copy (dst*), with the semantics
 * of emf_hip_copyValues at equal resolutions:
 *     dst(v) = src(v + shift) where v + shift lies inside the volume, 0 elsewhere
 * for the tsdf, the weights and, when both colour pointers are given, the u16 x 4 colour volume (both or neither).
 * Words are moved, never interpreted: the copy is bit for bit (-0.0f, NaN patterns).  |shift_i| >= res_i on any
 * axis gives an all-zero volume.  Every destination array must be disjoint from every source array and from the
 * other destination arrays: EMF_E_ARG otherwise, with nothing enqueued.
 *   Tile-granular roll  (emf_hip_rollVolumeIsTiled: every res_i and every shift_i a multiple of the integration
 *     tile 32 x 8 x 8)  one workgroup per destination tile, 16-byte accesses (all arrays 16-byte aligned:
 *     EMF_E_ARG otherwise), no index division.  With the four map pointers given (all or none) the same launch
 *     writes the destination's sign maps (emf_hip_signMapBytes) and unseen-tile map (emf_hip_unseenTileBytes) by
 *     moving the source's per-tile entries; a tile whose source lies outside the volume gets "no sign, unseen".
 *     PRECONDITION: the source maps describe the source values (the caller refreshes stale ones first).  When they
 *     are what emf_hip_rebuildSignMaps / emf_hip_rebuildUnseenTiles compute from the source, the written maps equal,
 *     byte for byte, what those entries compute from the destination.  The destination maps must not overlap the
 *     source maps.
 *   Any other shift or resolution  one voxel per lane, same values.  The map pointers are ignored and nothing is
 *     written through them: the caller rebuilds the maps with the two rebuild entries.
 * Nothing allocates, copies to the host or waits.
 * ---------------------------------------------------------------------------------------------- */

/* 1 if (res, shift) takes the tile-granular path of emf_hip_rollVolume (and so writes the maps), else 0.  No device. */
int emf_hip_rollVolumeIsTiled(const int32_t res[3], const int32_t shift[3]);

int emf_hip_rollVolume(const float* srcTsdf, const float* srcWeights, const uint16_t* srcColor, const uint8_t* srcSignMaps,
                       const uint8_t* srcUnseenTiles, float* dstTsdf, float* dstWeights, uint16_t* dstColor,
                       uint8_t* dstSignMaps, uint8_t* dstUnseenTiles, const int32_t res[3], const int32_t shift[3],
                       emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Storing and restoring tiles (new behaviour: the reference's background never moves).  Opt-in; nothing above is
 * touched.  Whole integration tiles (32 x 8 x 8 voxels) of a volume whose resolution is a multiple of the tile on
 * every axis and whose arrays are 16-byte aligned (EMF_E_ARG otherwise) are taken out of a volume, and written back
 * into one, as the bytes they are.  Words are moved and compared as bits, never interpreted.  Each ARRAY of a tile
 * (0 tsdf, 1 weights, 2 colour) gets a packed-buffer class of its own:
 *     class 0  every word is 0x00000000
 *     class 1  every element equals the same non-zero element; an element is a u32 for tsdf and weights and the
 *              8-byte voxel for colour (-0.0f, -1.0f under weight 0, the capped weight 64.0f ...)
 *     class 2  anything else: a LITERAL, 8 KiB for tsdf or weights, 16 KiB for colour, in TILE ORDER: voxel
 *              (z * 8 + y) * 32 + x of the tile, x fastest
 * Per tile c:  classes[c][3] u8;  words[c][4] u32 = the first tsdf word, the first weight word, the first colour
 * voxel's two words (whatever the class; zeros without a colour volume);  lits[c][3] u32 = where array k's literal
 * starts in the ARENA, in units of 8 KiB (0 for an array that is not a literal).
 * Nothing allocates, copies to the host or waits.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of device scratch emf_hip_spillTiles needs for a box of ntiles tiles (4 per 256 tiles, plus 4); 0 above 2^30. */
size_t emf_hip_spillScratchBytes(uint64_t ntiles);

/* Classify and gather the box of tiles [box_lo, box_lo + box_size) (in TILES, inside the volume: EMF_E_ARG otherwise).
 * Candidates are numbered x fastest inside the box; classes / words / lits hold one entry per candidate and totals[0]
 * (one u32) the arena units used.  Literals are placed in candidate order, within a candidate tsdf, weights, colour,
 * by a scan and never by atomics: two spills of one box give the same bytes.  color may be NULL (classes[c][2] = 0).
 *   arena == NULL   count only: everything but the arena is written.
 *   arena != NULL   arena_units (8 KiB each) must cover the box's worst case, box tiles x (colour ? 4 : 2):
 *                   EMF_E_LIMIT otherwise, with nothing enqueued -- the host moves a big box in several calls.
 * words must be 16-byte aligned.  A box of zero tiles writes totals[0] = 0 and nothing else.  The source is only
 * read: once by the classify pass, its literals once more by the gather. */
int emf_hip_spillTiles(const float* tsdf, const float* weights, const uint16_t* color, const int32_t res[3],
                       const int32_t box_lo[3], const int32_t box_size[3], void* scratch_dev, uint8_t* classes,
                       uint32_t* words, uint32_t* lits, uint32_t* totals, void* arena, uint64_t arena_units,
                       emf_stream_t stream);

/* The inverse, for a list of n destination tiles: coords[i][3] i32 (tile coordinates in the destination volume, on
 * the device) with classes / words / lits as above (device) and an arena of arena_units units.  One workgroup per
 * listed tile writes every word of its tsdf and weights, and of its colour when color is given, from zero, the
 * repeated element or the literal; a tile stored without colour (class 0) gets zero colour, colour data for a
 * destination without a colour volume is ignored.  Tiles not listed are not touched; a tile must not be listed twice.
 * With signMaps and unseenTiles given (both or neither: EMF_E_ARG) the tile's three map entries are written from the
 * values just written -- positive: any tsdf > 0; negative: any tsdf < 0; unseen: every weight == 0.f and every
 * |tsdf| <= 3.0e38f -- byte for byte what emf_hip_rebuildSignMaps / emf_hip_rebuildUnseenTiles compute.
 * classes_host: the same n x 3 class bytes in host memory (the caller assembled the list there), read before the
 * call returns: a class above 2 is EMF_E_ARG with nothing enqueued.  What only the device can see is skipped, never
 * dereferenced: a tile whose coordinate lies outside the volume, whose device class byte is above 2 or whose literal
 * does not lie inside the arena is left untouched.  n == 0 launches nothing. */
int emf_hip_fillTiles(float* tsdf, float* weights, uint16_t* color, uint8_t* signMaps, uint8_t* unseenTiles,
                      const int32_t res[3], const int32_t* coords, const uint8_t* classes, const uint8_t* classes_host,
                      const uint32_t* words, const uint32_t* lits, const void* arena, uint64_t arena_units, uint32_t n,
                      emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Meshing a set of tiles (new behaviour: DESIGN.md 5.16).  Opt-in; nothing above is touched.  Marching cubes over a
 * SPARSE set of integration tiles (32 x 8 x 8 voxels) on one integer lattice instead of a dense volume: the result is
 * the mesh of the dense volume that holds exactly these tiles and is unobserved (tsdf 0, weight 0) everywhere else.
 *   ownership   the cube anchored at voxel v belongs to the tile that contains v
 *   validity    all 8 corners have weights > 0 (no foreground mask)
 *   geometry    class, edge order, vertexInterp, triangle table and the (3, i0, i1, i2) records of emf_hip_meshEmit
 *   normals     the interpolated raw forward differences of the corner voxels; the difference reads the next voxel in
 *               whatever tile it lies and 0 where there is none -- a tile set has no "last plane"
 *   positions   a corner is (float(lattice voxel) - half) * voxelSize per axis; the caller passes half
 *   colours     the rule of emf_hip_meshColors; an array absent from a tile (class 0) counts as uncoloured
 *   order       tiles in table order; within a tile its 2048 cubes in (z, y, x) order of their anchor; within a cube
 *               vertices in edge-bit order and triangles in table order.  Triangle indices are GLOBAL u32.
 * The table: n emf_mesh_tile_t sorted by lattice tile coordinate, strictly ascending in (z, y, x).  Per array (0 tsdf,
 * 1 weights, 2 colour) a class: 0, 1, 2 as in "Storing and restoring tiles" (1: words[]; 2: at[k] = the literal's
 * arena unit of 8 KiB), and
 *     class 3  in place in a dense volume: at[k] = the element offset of the tile's first voxel in
 *              emf_mesh_tiles_source_t's arrays (a multiple of 4), rows and planes row_stride / plane_stride apart
 * nbr[k - 1], k = 1 .. 7: the table index of the tile at +(k & 1, k >> 1 & 1, k >> 2) tiles, or -1.  The host fills
 * them; a tile that is not listed is unobserved.
 * What the host can see is refused before any launch (emf_hip_meshTilesCount reads tiles_host, the same n entries in
 * host memory): a class above 3, a coordinate that is not strictly ascending, a neighbour index outside [-1, n) or
 * one that names a tile at another coordinate (EMF_E_ARG); an arena or a volume array that is not 16-byte aligned, a
 * stride that is not a multiple of 4 (EMF_E_ARG); literals without an arena or class 3 without a volume (EMF_E_NULL);
 * a tile with a lattice VOXEL coordinate outside [-2^19, 2^19) or n > 2^17 (EMF_E_LIMIT).  What only the device sees
 * skips the tile -- it counts as not listed, as an owner and as a neighbour -- and is never dereferenced: a literal
 * outside the arena, an in-place offset (not a multiple of 4, or) whose tile does not lie inside volume_elements, a
 * class above 3, a neighbour whose coordinate is not the one the index stands for.  A tile is skipped as a whole
 * when ANY of its three arrays fails: a colour literal outside the arena removes the tile's geometry too, also from
 * a mesh made without colours -- the same tiles count in every pass, so the passes always agree on the vertex slots.
 * ---------------------------------------------------------------------------------------------- */

typedef struct emf_mesh_tile {
    int32_t coord[3];  /* lattice tile coordinate (x, y, z) */
    uint8_t cls[3];    /* class of tsdf, weights, colour */
    uint8_t reserved0;
    uint32_t words[4]; /* class 1: the tsdf word, the weight word, the colour voxel's two words */
    int32_t nbr[7];
    int32_t reserved1;
    uint64_t at[3];    /* class 2: arena unit; class 3: element offset */
} emf_mesh_tile_t;     /* 88 bytes */

typedef struct emf_mesh_tiles_source {
    const void* arena;        /* literals (device), or NULL */
    uint64_t arena_units;     /* its size in units of 8 KiB */
    const float* tsdf;        /* the dense volume of class 3 (device), or NULL */
    const float* weights;
    const uint16_t* color;    /* u16 x 4 per voxel, or NULL */
    uint64_t volume_elements; /* voxels each of the three arrays holds */
    uint64_t row_stride;      /* voxels from (x, y, z) to (x, y + 1, z) */
    uint64_t plane_stride;    /* voxels from (x, y, z) to (x, y, z + 1) */
} emf_mesh_tiles_source_t;

/* Bytes of device scratch the four calls below share for a table of n tiles (12 per tile, plus 8); 0 above 2^17.
 * After emf_hip_meshTilesCount it holds three u32 arrays: [n + 1] the first vertex of every tile and the total,
 * [n + 1] the same for triangles, [n] the surface cubes each tile owns. */
size_t emf_hip_meshTilesScratchBytes(uint32_t n);

/* Pass 1: one workgroup per listed tile counts its vertices and triangles; one workgroup scans the per-tile totals
 * (mesh_scan.hpp: no atomics) and writes the totals to counts_dev (device).  n == 0 writes zero counts. */
int emf_hip_meshTilesCount(const emf_mesh_tile_t* tiles_dev, const emf_mesh_tile_t* tiles_host, uint32_t n,
                           const emf_mesh_tiles_source_t* source, void* scratch_dev, emf_mesh_counts_t* counts_dev,
                           emf_stream_t stream);

/* Pass 2, after the count on the same table, source and scratch: 3 floats per vertex twice and 4 int32 per triangle,
 * sized by the counts.  half: HOST float[3]. */
int emf_hip_meshTilesEmit(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                          const float half[3], float voxelSize, const void* scratch_dev, float* vertices, float* normals,
                          int32_t* triangles, emf_stream_t stream);

/* u8 x 3 per vertex, in the emit's vertex order (the same scratch). */
int emf_hip_meshTilesColors(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                            const void* scratch_dev, uint8_t* colors, emf_stream_t stream);

/* One u64 per vertex, in the emit's vertex order: the key of the grid edge the vertex lies on,
 *     3 * (((z + 2^19) << 40) | ((y + 2^19) << 20) | (x + 2^19)) + axis
 * of the edge's lower LATTICE voxel (x, y, z).  It is below 2^62, hence never the weld table's empty key; the keys and
 * the soup go unchanged into emf_hip_meshWeldCount / ...Emit and emf_hip_meshComponents* as one model. */
int emf_hip_meshTilesEdgeKeys(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                              const void* scratch_dev, uint64_t* keys, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Distance field (new behaviour: DESIGN.md 5.18).  Opt-in; nothing above is touched.  Three steps from the volumes of
 * a scene to "how far is the nearest obstacle", all over a BOX of voxels [box_lo, box_lo + box_size) of a volume of
 * resolution res (res, box_lo, box_size: x, y, z).  The result is that of the cropped arrays: what lies outside the
 * box does not exist.  Box arrays are dense, one element per voxel of the box in (z, y, x) order, x fastest.
 *   1 classes   one u8 per voxel from the volume's (tsdf, weights), single float comparisons only:
 *                   EMF_OCC_FREE      0   weights > 0 && tsdf > 0
 *                   EMF_OCC_OCCUPIED  1   weights > 0 && !(tsdf > 0)      (-0.0 and NaN count as occupied)
 *                   EMF_OCC_UNKNOWN   2   !(weights > 0)                  (0, negative and NaN weights)
 *   2 stamping  objects mark EMF_OCC_OCCUPIED where they are solid.  For the voxel v (volume coordinates) of the
 *               background and one object, every operation a single float32 operation in this order:
 *                   p_b = (float(v) - half_b) * voxel_b            half = (res - 1) / 2.f per axis
 *                   p_o = R p_b + t                                rows of R summed left to right; R, t: the object's
 *                                                                  frame <- the background volume's frame
 *                   q   = p_o / voxel_o + half_o
 *                   i   = rint(q) per axis, ties to even           a NaN coordinate is outside
 *               the voxel becomes OCCUPIED iff i lies inside the object's resolution, the object's weights[i] > 0,
 *               fgVolMask[i] != 0 (unless fgVolMask is NULL) and !(tsdf[i] > 0).  Nothing else is written: an object
 *               never turns a voxel free.  Each object is evaluated over its own sub-box [lo, lo + size) of the
 *               background lattice (emf_hip_occupancyObjectBox computes a covering one), clipped to the box.  Plain
 *               stores of one value, no atomics: the result does not depend on the order of objects or workgroups.
 *   3 distance  d2, one i32 per voxel: the exact squared Euclidean distance, in voxels, to the nearest SITE of the
 *               box -- a voxel whose class bit is set in site_mask (bit 0 FREE, bit 1 OCCUPIED, bit 2 UNKNOWN; a
 *               class byte above 2 is never a site) -- 0 at a site, EMF_DF_FAR where the box holds no site.  With
 *               cap > 0 every d2 > cap * cap becomes EMF_DF_FAR.  Integer arithmetic only: a pure function of the
 *               inputs, bit for bit.
 * Limits: every box axis in 1 .. EMF_DF_MAX_AXIS and at most 2^31 - 1 voxels in a box (EMF_E_LIMIT above; a zero or
 * negative axis and a box that leaves the volume are EMF_E_ARG).  Every rejected argument -- a NULL pointer
 * included -- returns EMF_E_ARG or EMF_E_LIMIT with nothing enqueued.  Nothing allocates, copies to the host or waits.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_OCC_FREE 0
#define EMF_OCC_OCCUPIED 1
#define EMF_OCC_UNKNOWN 2
#define EMF_DF_FAR 0x7fffffff
#define EMF_DF_MAX_AXIS 2048

typedef struct emf_occ_object {
    const float* tsdf;        /* the object's volume (device) */
    const float* weights;
    const uint8_t* fgVolMask; /* or NULL: no foreground gate */
    int32_t res[3];           /* its resolution (x, y, z), every axis >= 1 */
    float voxelSize;          /* > 0 */
    float R[9], t[3];         /* object frame <- background volume frame, row-major */
    int32_t lo[3], size[3];   /* the sub-box of the BACKGROUND lattice the object is evaluated over (volume coordinates);
                                 a size <= 0 on any axis: nowhere */
} emf_occ_object_t;           /* 112 bytes */

/* Step 1.  tsdf, weights: the whole volume (device); classes: box_size[0] * [1] * [2] bytes.  Rows whose first voxel
 * is 16-byte aligned in both arrays are read with 16-byte loads, four voxels per lane; other rows voxel by voxel. */
int emf_hip_occupancyClasses(const float* tsdf, const float* weights, const int32_t res[3], const int32_t box_lo[3],
                             const int32_t box_size[3], uint8_t* classes, emf_stream_t stream);

/* Host only, no device: sets object->lo / size to a sub-box of a background of resolution res and voxel size
 * voxel_size that covers every voxel step 2 can map into the object (the object's corners taken through the inverse of
 * (R, t) in double precision, one voxel of margin, clipped to the volume; the whole volume when R is singular or a
 * value is not finite). */
int emf_hip_occupancyObjectBox(emf_occ_object_t* object, const int32_t res[3], float voxel_size);

/* Step 2 on the classes of the box.  objects: n entries in HOST memory, read before the call returns (passed to the
 * kernels by value); n >= 0, EMF_MAX_BATCH per launch, longer lists in several launches.  A launch covers only the
 * objects' sub-boxes. */
int emf_hip_occupancyStampObjects(uint8_t* classes, const int32_t res[3], float voxel_size, const int32_t box_lo[3],
                                  const int32_t box_size[3], const emf_occ_object_t* objects, int32_t n,
                                  emf_stream_t stream);

/* Occupancy of a set of tiles (new behaviour: DESIGN.md 5.28).  Step 1 over a SPARSE set of integration tiles on one
 * integer lattice instead of a dense volume: the result is emf_hip_occupancyClasses of the dense volume that holds
 * exactly the listed tiles and is unobserved (tsdf 0, weight 0) everywhere else, cropped to the box.  box_lo and
 * box_size are in LATTICE voxels (x, y, z); box_lo may be negative and nothing needs to be aligned to a tile.  A voxel
 * in no listed tile is EMF_OCC_UNKNOWN; the three single float comparisons are those above, NaN and -0.0 included.
 * Only the tsdf and the weights of a tile are read; its colour class counts for the skip rule alone.
 * The table, tiles_dev / tiles_host and source are those of "Meshing a set of tiles": sorted strictly ascending in
 * (z, y, x), classes 0 / 1 / 2 / 3 per array; what the host can see is refused from tiles_host before any launch with
 * the codes of emf_hip_meshTilesCount, and what only the device sees skips the tile as a whole -- it then counts as
 * not listed and is never dereferenced.  nbr[] is neither used nor checked.
 * Limits: every box axis in 1 .. EMF_DF_MAX_AXIS and at most 2^31 - 1 voxels (EMF_E_LIMIT above; a zero or negative
 * axis and a NULL box or classes are EMF_E_ARG); every lattice voxel of the box in [-2^19, 2^19) (EMF_E_LIMIT); n at
 * most 2^17 (EMF_E_LIMIT).  n == 0 writes an all-unknown box.  One launch: a workgroup per tile-aligned cell the box
 * overlaps finds its tile by a search of the sorted table; every byte of the box is written exactly once by a plain
 * store.  Nothing allocates, copies to the host or waits. */
int emf_hip_occupancyTiles(const emf_mesh_tile_t* tiles_dev, const emf_mesh_tile_t* tiles_host, uint32_t n,
                           const emf_mesh_tiles_source_t* source, const int32_t box_lo[3], const int32_t box_size[3],
                           uint8_t* classes, emf_stream_t stream);

/* Step 3.  classes: size[0] * [1] * [2] bytes, only read; d2: as many i32.  site_mask in 1 .. 7; cap >= 0 in voxels,
 * 0 = none.  metres: NULL, or as many f32, written by the last pass as sqrtf(float(d2)) * voxel_size (two roundings;
 * voxel_size > 0 then) and +inf where d2 is EMF_DF_FAR.  Three separable passes, x (wave ballots and bit scans, no
 * LDS), then y and z in place in d2 (bundles of whole lines staged in LDS); no atomics, no scratch buffer. */
int emf_hip_distanceTransform(const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap, int32_t* d2,
                              float* metres, float voxel_size, emf_stream_t stream);

/* Step 3 with the nearest site.  For a box of class bytes, a site_mask and a cap exactly as above,
 * nearest, one i32 per voxel v: the linear index (z' * ny + y') * nx + x' of the site nearest to v.
 *   ties     where several sites share the minimal squared distance, the one with the smallest linear index
 *   no site  EMF_DF_NONE exactly where d2[v] == EMF_DF_FAR: no site in the box, or cap > 0 and the nearest one beyond it
 *   a site   nearest[v] == v
 * (at most 2^31 - 1 voxels: the index fits.)  d2 and metres are those of emf_hip_distanceTransform byte for byte, from
 * the same three passes in one run: pass x writes the index of the row's winner (the left site where both sides are
 * equally far), passes y and z break ties toward the smaller y' and z' and gather the winner's index from the previous
 * pass's index array into the other one of (nearest, scratch); no pass reads an index array it writes.
 * scratch: emf_hip_nearestSiteScratchBytes(size) bytes (one i32 per voxel; 0 for a size beyond the limits), contents
 * undefined afterwards.  d2, nearest and scratch are three different arrays, 4-byte aligned; a NULL nearest or scratch
 * is EMF_E_ARG. */
#define EMF_DF_NONE (-1)
size_t emf_hip_nearestSiteScratchBytes(const int32_t size[3]);
int emf_hip_distanceTransformNearest(const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap,
                                     int32_t* d2, float* metres, int32_t* nearest, void* scratch, float voxel_size,
                                     emf_stream_t stream);

/* A gather of n box voxels (voxels: n x (x, y, z) i32 on the device) from the arrays of a box of shape size: per point
 * the class byte, d2 and the nearest site.  Any of the three inputs may be NULL together with its output (an input
 * without its output or the reverse is EMF_E_ARG).  A voxel outside the box yields class 255, EMF_DF_FAR and
 * EMF_DF_NONE.  One lane per point, plain loads and stores; n == 0 enqueues nothing. */
int emf_hip_distanceQuery(const uint8_t* classes, const int32_t* d2, const int32_t* nearest, const int32_t size[3],
                          const int32_t* voxels, int32_t n, uint8_t* out_class, int32_t* out_d2, int32_t* out_nearest,
                          emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Frontiers (new behaviour: DESIGN.md 5.19).  Opt-in; nothing above is touched.  "Where does the known map end": the
 * free voxels that touch unknown space, grouped into clusters, over a box of class bytes of shape size (x, y, z) as
 * the steps above produce them.  Arrays are dense, (z, y, x) order, x fastest; what lies outside the box does not exist.
 *   frontier voxel  a voxel v with class EMF_OCC_FREE of which at least one of the six face neighbours INSIDE the box
 *                   is EMF_OCC_UNKNOWN (a class byte above 2 is neither free nor unknown) and, where a d2 array of the
 *                   same shape (emf_hip_distanceTransform's output) is passed with min_d2 > 0, d2[v] >= min_d2
 *                   (EMF_DF_FAR passes): the clearance gate.  d2 == NULL or min_d2 <= 0: no gate.
 *   cluster         a 26-connected component of frontier voxels (3 x 3 x 3 neighbourhoods).  Its label is the smallest
 *                   linear index (z * ny + y) * nx + x among its members.
 *   label volume    one i32 per voxel: the label of the voxel's cluster, -1 where the voxel is no frontier voxel.
 *   record          emf_frontier_cluster_t: label, count, the inclusive bounding box lo / hi, the sums of the members'
 *                   x, y, z (box coordinates) and a representative voxel rep -- a MEMBER of the cluster (the centroid
 *                   of a curved frontier can lie in unknown or occupied space): with the rounded centroid
 *                   c = (2 * sum + count) / (2 * count) per axis (integer division), the member that minimises the
 *                   integer |v - c|^2, ties to the smallest linear index -- the minimum of the 64-bit key
 *                   (dist^2 << 31) | linear (dist^2 <= 3 * 2047^2 < 2^24, linear < 2^31).
 *   filter, order   clusters with count < min_voxels (>= 1) are dropped; the kept records are written in ascending
 *                   label order, placed by scan, at most capacity of them.  counters (3 x u32):
 *                   [EMF_FRONTIER_KEPT] kept clusters, [EMF_FRONTIER_CLUSTERS] all clusters, [EMF_FRONTIER_VOXELS]
 *                   frontier voxels -- always the full numbers, whatever capacity is.
 * Integer arithmetic and integer atomics only: every output is a pure function of the inputs, bit for bit.
 * Limits as for the distance field: every axis in 1 .. EMF_DF_MAX_AXIS, at most 2^31 - 1 voxels (EMF_E_LIMIT above).
 * Every rejected argument -- a NULL pointer, a non-positive axis, min_voxels < 1, a negative capacity -- returns
 * EMF_E_ARG or EMF_E_LIMIT with nothing enqueued.  Nothing allocates, copies to the host or waits.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_FRONTIER_KEPT 0
#define EMF_FRONTIER_CLUSTERS 1
#define EMF_FRONTIER_VOXELS 2

typedef struct emf_frontier_cluster {
    int32_t label;         /* the smallest linear index of the cluster */
    int32_t count;         /* voxels */
    int32_t lo[3], hi[3];  /* inclusive bounding box (x, y, z), box coordinates */
    uint64_t sum[3];       /* sums of the members' x, y, z */
    int32_t rep[3];        /* the representative voxel (x, y, z) */
    int32_t reserved;      /* 0 */
} emf_frontier_cluster_t;  /* 72 bytes */

/* Labels.  classes: size[0] * [1] * [2] bytes, only read; d2: NULL or as many i32, only read; labels: as many i32.
 * Writes counters[EMF_FRONTIER_CLUSTERS] and [EMF_FRONTIER_VOXELS] and zeroes [EMF_FRONTIER_KEPT].  Flags (one wave per
 * row, wave ballots), hooks (lock-free union-find over the label volume itself, 13 neighbours of smaller index per
 * frontier voxel), flatten, count. */
int emf_hip_frontierLabel(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2,
                          int32_t* labels, uint32_t* counters, emf_stream_t stream);

/* Host only, no device: the bytes of scratch emf_hip_frontierClusters needs for a box of this size that holds
 * n_clusters clusters -- 4 bytes per 256 voxels + under 65 bytes per cluster + under 1 KiB.  0 for a size beyond the limits. */
size_t emf_hip_frontierScratchBytes(const int32_t size[3], uint32_t n_clusters);

/* Records of a label volume as emf_hip_frontierLabel leaves it.  n_clusters: counters[EMF_FRONTIER_CLUSTERS] as the
 * host read it after the labelling -- the one number the host needs to size the per-cluster tables; a smaller value
 * drops the clusters of the largest labels, a larger one only wastes scratch (no index ever leaves the tables).
 * scratch_dev: emf_hip_frontierScratchBytes(size, n_clusters) bytes, 16-byte aligned; records: capacity entries (NULL
 * with capacity 0).  Writes the first min(kept, capacity) records and counters[EMF_FRONTIER_KEPT]; with n_clusters == 0
 * only the counter is cleared.  Roots by scan in index order, a voxel finds its cluster's slot by binary search of its
 * label; per-slot statistics by integer atomics, merged per row and per workgroup before they touch global memory. */
int emf_hip_frontierClusters(const int32_t* labels, const int32_t size[3], int32_t min_voxels, uint32_t n_clusters,
                             void* scratch_dev, emf_frontier_cluster_t* records, int32_t capacity, uint32_t* counters,
                             emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Planning (new behaviour: DESIGN.md 5.20).  Opt-in; nothing above is touched.  "Can the robot get there, by which way,
 * at what cost": a multi-source shortest-path (cost-to-go) field over the traversable voxels of a box of class bytes,
 * and the paths from any number of goals back to the start.  Arrays are dense, (z, y, x) order, x fastest; size[3] =
 * (nx, ny, nz) as in the frontier entries; what lies outside the box does not exist.
 *   traversable set T   a voxel v is in T if either holds:
 *                       gate    (1u << class[v]) & traverse_mask is non-zero (the bit convention of site_mask; a class
 *                               byte above 2 is in no mask) and, where a d2 array is passed with min_d2 > 0,
 *                               d2[v] >= min_d2 (EMF_DF_FAR passes): the frontier gate;
 *                       bubble  class[v] != EMF_OCC_OCCUPIED and v lies within seed_radius voxels of a used seed s
 *                               (integer |v - s|^2 <= seed_radius^2, seed_radius >= 0).  The bubble ignores class and
 *                               clearance: the robot is standing there, and a sensor cannot see its own near field.
 *                               With radius 0 the bubble is the seed voxel itself.
 *   seeds               n_seeds >= 1 voxels (x, y, z), a device array of 3 * n_seeds i32.  A seed outside the box, or
 *                       one whose class is EMF_OCC_OCCUPIED, is ignored; counters[EMF_PLAN_SEEDS] is the number of
 *                       seeds of the list that were used.
 *   moves               26-connected, between two voxels that are both in T.  Integer chamfer weights: 3 for a face
 *                       move, 4 for an edge move, 5 for a corner move.  No extra corner-cutting rule: the clearance is
 *                       what keeps paths off walls.
 *   cost field (u32)    0 at a used seed; at any other voxel of T the least total weight of a move sequence from any
 *                       used seed; EMF_PLAN_UNREACHED for a voxel of T that no seed reaches or whose cost exceeds
 *                       max_cost (when max_cost > 0); EMF_PLAN_BLOCKED for a voxel outside T.  A truncated field equals
 *                       the untruncated one wherever it is finite (costs are non-negative: every prefix of a path
 *                       within the cap is within it).
 *   paths               for each goal voxel g with a finite cost the path g = p0, p1, ..., pk with cost[pk] == 0, where
 *                       p(i+1) is the neighbour n of pi with cost[n] + w(n, pi) == cost[pi], ties to the smallest
 *                       linear index (z * ny + y) * nx + x.  At the fixed point such a neighbour always exists.
 *                       paths[n_goals][capacity] i32: linear indices, the goal first, truncated to capacity, untouched
 *                       beyond; lengths[n_goals] i32: the full k + 1, 0 for a goal that is unreached, blocked or out of
 *                       the box, minus the steps taken where the walk found no such neighbour (only on a field that
 *                       did not converge; where that happens at the goal itself this is 0 too, and a goal_cost that is
 *                       finite tells it from a goal without a path); goal_cost[n_goals] u32 (EMF_PLAN_BLOCKED for a goal out of the box).
 * Limits: every axis in 1 .. EMF_DF_MAX_AXIS and at most 2^29 voxels, so that 5 * voxels < EMF_PLAN_BLOCKED and no cost
 * can overflow (EMF_E_LIMIT above, checked first, from the sizes alone).  Every rejected argument -- a NULL pointer,
 * n_seeds < 1, a negative radius or capacity -- returns EMF_E_ARG or EMF_E_LIMIT with nothing enqueued.
 * Integer arithmetic only: every output but counters[0..1] of a run that was cut off is a pure function of the inputs.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_PLAN_UNREACHED 0xffffffffu
#define EMF_PLAN_BLOCKED 0xfffffffeu
#define EMF_PLAN_CONVERGED 0 /* counters (4 x u32): 1 if a round found no active tile, else 0 */
#define EMF_PLAN_ROUNDS 1    /* rounds enqueued */
#define EMF_PLAN_FINITE 2    /* voxels with a finite cost */
#define EMF_PLAN_SEEDS 3     /* seeds used */

/* Host only, no device: the bytes of scratch emf_hip_planCost needs for a box of this size -- two bytes per tile of
 * 32 x 8 x 8 voxels + under 128 bytes.  0 for a size beyond the limits. */
size_t emf_hip_planScratchBytes(const int32_t size[3]);

/* The cost field.  classes: size[0] * [1] * [2] bytes, only read; d2: NULL or as many i32, only read; seeds: device,
 * 3 * n_seeds i32, only read; cost: as many u32 as voxels; scratch_dev: emf_hip_planScratchBytes(size) bytes, 16-byte
 * aligned; counters: device, 4 x u32 (EMF_PLAN_*).  max_cost: 0 for none.  max_rounds <= 0: voxels + 1, which a
 * converging run never reaches.  A tiled label-correcting iteration: k_pl_init, then rounds of k_pl_relax -- one
 * workgroup per active tile, the tile and a one-voxel halo relaxed in LDS, the tiles whose halo changed flagged for
 * the next launch -- enqueued on the stream in batches; like emf_hip_frontierLabel's caller this entry WAITS on the
 * stream, once per batch, to read the rounds' activity counters, and stops at the first round with no active tile or
 * at max_rounds.  A run that was cut off (counters[EMF_PLAN_CONVERGED] == 0) leaves costs that are >= the true ones. */
int emf_hip_planCost(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2, uint32_t traverse_mask,
                     const int32_t* seeds, int32_t n_seeds, int32_t seed_radius, uint32_t max_cost, int32_t max_rounds,
                     uint32_t* cost, void* scratch_dev, uint32_t* counters, emf_stream_t stream);

/* Paths over a cost field as emf_hip_planCost leaves it.  goals: device, 3 * n_goals i32 (x, y, z); paths: n_goals *
 * capacity i32 (NULL with capacity 0); lengths, goal_cost: n_goals each.  One wave per goal, at most
 * max(capacity, cost / 3 + 1) steps.  Nothing allocates, copies to the host or waits. */
int emf_hip_planPaths(const uint32_t* cost, const int32_t size[3], const int32_t* goals, int32_t n_goals, int32_t capacity,
                      int32_t* paths, int32_t* lengths, uint32_t* goal_cost, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Voxel rays (new behaviour: DESIGN.md 5.22).  Opt-in; nothing above is touched.  "Can I go, or look, straight from a
 * to b, and what would I pass on the way": a straight walk through a box of class bytes of shape size = (nx, ny, nz)
 * that stops at the first voxel that blocks.  Arrays are dense, (z, y, x) order, x fastest; what lies outside the box
 * does not exist.  The ray is an INTEGER walk on the voxel lattice, not a floating-point march.
 *   the walk     a ray goes from voxel a to voxel b (x, y, z, i32).  d_k = |b_k - a_k|, s_k = sign(b_k - a_k) per axis.
 *                It makes exactly n = d_x + d_y + d_z face steps v_1 .. v_n, v_n = b.  With i_k the steps already made
 *                along axis k, the next step goes along the axis that still has steps left (i_k < d_k) and has the
 *                smallest crossing parameter (2 i_k + 1) / (2 d_k), compared by cross-multiplication in integers,
 *                (2 i_p + 1) * d_q < (2 i_q + 1) * d_p; TIES GO TO THE LOWER AXIS INDEX, x before y before z.  These
 *                are the voxels the centre-to-centre segment passes through, with a fixed rule where it passes
 *                exactly through an edge or a corner; sorting all crossings by (parameter as a fraction, axis) gives
 *                the same sequence.  The walk is NOT symmetric: a -> b and b -> a visit different voxel sets for most
 *                rays (integer segments hit edges often, and the tie rule is stated per axis, not per direction).
 *   limits       d_k <= EMF_RAY_MAX_DELTA on every axis: the products stay below 2^26 and no ray takes more than
 *                3 * EMF_RAY_MAX_DELTA steps.
 *   what stops   a itself is never tested and never counted: the robot or sensor stands there.  A voxel v PASSES if it
 *                lies in the box, (1u << class[v]) & pass_mask is non-zero (the bit convention of site_mask and
 *                traverse_mask; a class byte above 2 is in no mask and blocks) and, where a d2 array is passed with
 *                min_d2 > 0, d2[v] >= min_d2 (EMF_DF_FAR passes): the clearance gate of the frontiers and the plan.
 *                The first voxel that does not pass ends the ray.
 *   per ray      emf_ray_result_t.  status: EMF_RAY_REACHED (steps == n; a == b is REACHED with 0 steps),
 *                EMF_RAY_BLOCKED (stop is the blocking voxel), EMF_RAY_LEFT (stepped out of the box), EMF_RAY_OUTSIDE
 *                (a is not in the box, nothing walked; tested first), EMF_RAY_INVALID (a d_k above the limit, nothing
 *                walked).  weighted gives a far voxel the weight of the solid angle it stands for, so that rays that
 *                share their first voxels do not dominate a sum.
 *   per group    with group > 0 every run of group consecutive rays is one group, the last one may be short:
 *                ceil(n / group) records emf_ray_group_t, the integer sums over the group's rays; invalid counts the
 *                OUTSIDE and the INVALID rays.  Integer sums: no dependence on the order of waves or workgroups.
 * Limits of the box as for the distance field: every axis in 1 .. EMF_DF_MAX_AXIS, at most 2^31 - 1 voxels
 * (EMF_E_LIMIT above).  Every rejected argument -- a NULL pointer, a mask above 7, a negative n or group, group > 0
 * without groups or the reverse, neither results nor groups -- returns EMF_E_ARG or EMF_E_LIMIT with nothing enqueued.
 * Integer arithmetic only: every output is a pure function of the inputs, bit for bit.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_RAY_MAX_DELTA 4095
#define EMF_RAY_REACHED 0
#define EMF_RAY_BLOCKED 1
#define EMF_RAY_LEFT 2
#define EMF_RAY_OUTSIDE 3
#define EMF_RAY_INVALID 4

typedef struct emf_ray_result {
    int32_t stop;      /* linear index of the blocking voxel, EMF_DF_NONE if none */
    int32_t steps;     /* voxels entered and passed */
    uint32_t counted;  /* passed voxels whose class bit is in count_mask */
    uint32_t status;   /* EMF_RAY_* */
    uint64_t weighted; /* sum over the counted voxels of the integer |v - a|^2 */
} emf_ray_result_t;    /* 24 bytes */

typedef struct emf_ray_group {
    uint64_t counted, weighted;               /* sums of the rays' fields */
    uint32_t reached, blocked, left, invalid; /* rays by status; invalid: OUTSIDE + INVALID */
} emf_ray_group_t;                            /* 32 bytes */

/* classes: size[0] * [1] * [2] bytes, only read; d2: NULL or as many i32, only read; from, to: device, 3 * n i32
 * each, only read; results: n records, or NULL when only the groups are wanted; groups: ceil(n / group) records with
 * group > 0, NULL with group == 0 (zeroed by a memset on the stream, then one integer atomic per non-zero quantity and
 * run of lanes).  pass_mask, count_mask in 0 .. 7.  n == 0 enqueues nothing.  One lane per ray, one loop bounded by
 * 3 * EMF_RAY_MAX_DELTA; a voxel outside the box is never dereferenced.  Nothing allocates, copies to the host or waits. */
int emf_hip_castVoxelRays(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2, uint32_t pass_mask,
                          uint32_t count_mask, const int32_t* from, const int32_t* to, int32_t n, emf_ray_result_t* results,
                          int32_t group, emf_ray_group_t* groups, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Object shapes (new behaviour: DESIGN.md 5.23).  Opt-in; nothing above is touched.  Where in its volume a model is,
 * how large it is, how it is oriented and how much of its surface has been seen: a per-voxel pass over a model table
 * that reduces to a few dozen integers per model, and a second pass that measures the model along given axes.
 * WHAT IS MEASURED IS THE OBSERVED SOLID BAND, NOT THE BODY: a TSDF observes a band around the surface, the interior
 * of an object has weight 0.  Nothing here is a volume in cubic metres and nothing must be presented as one.
 * Volumes are dense, (z, y, x) order, x fastest, resolution res = (nx, ny, nz); a voxel is v = (x, y, z).  Single float
 * comparisons only:
 *   solid(v)     weights[v] > 0 && (fgVolMask == NULL || fgVolMask[v] != 0) && !(tsdf[v] > 0): exactly the rule by which
 *                emf_hip_occupancyStampObjects calls an object solid.  A tsdf of -0.0 or NaN is solid; a NaN, zero or
 *                negative weight is not.
 *   observed(v)  weights[v] > 0.
 *   faces        for each of the up to six face neighbours n of a solid voxel that lie INSIDE the volume: n is FREE if
 *                weights[n] > 0 && tsdf[n] > 0, UNKNOWN if !(weights[n] > 0), and neither otherwise.  A neighbour
 *                outside the volume does not exist.  The mask plays no part in a neighbour's kind.
 * emf_shape_moments_t, per model, integers only: the counts, the sums of the solid voxels' coordinates and of their
 * products, the ordered pairs (solid voxel, face neighbour) by the neighbour's kind -- faces_free is the seen surface in
 * voxel faces, faces_unknown is where the solid band ends against space nobody has seen -- and the axis-aligned bounds
 * of the solid voxels (lo = res and hi = -1 without one).
 * Limits: every axis in 1 .. EMF_DF_MAX_AXIS and at most 2^31 - 1 voxels per model (EMF_E_LIMIT above; a zero or
 * negative axis is EMF_E_ARG), so that every sum stays below 2^53; the models of one call together at most 2^24 - 1
 * tiles of 32 x 8 x 8 voxels, partial ones included (EMF_E_LIMIT above).
 *
 * Extents along given axes: per model a frame emf_shape_axes_t -- three row vectors A and a centre c, f32, in voxel
 * coordinates -- and for every solid voxel, each line a single float32 operation without contraction, rows summed left
 * to right (the discipline of the stamping arithmetic):
 *     p_j = float(v_j) - c_j
 *     e_k = A_k0 * p_0 + A_k1 * p_1 + A_k2 * p_2
 * emf_shape_extents_t holds the minimum and the maximum of e_k over the solid voxels (lo = +inf, hi = -inf without
 * one).  They are taken on the order-preserving map of the f32 bits to u32 (key = bits ^ 0x80000000 for a clear sign
 * bit, ~bits for a set one): for numbers that is the float order with -0 below +0, a NaN with a clear sign bit lies
 * above +inf and one with a set sign bit below -inf.  Minimum and maximum do not depend on the order of the voxels:
 * both records are pure functions of the inputs, bit for bit.
 *
 * The frame of a model from its moments (emf_fusion_shape_frame of include/emf_fusion.h; on the host, without a
 * device).  Everything in float64, every line a single operation in this order, no contraction:
 *     m_j  = double(sum_j) / double(solid)
 *     C_jk = double(solid * sum2_jk - sum_j * sum_k) / (double(solid) * double(solid))
 *            the integer numerator exact in 128 bits and rounded to double once (ties to even)
 *     cyclic Jacobi on S = C with V = I: EMF_SHAPE_JACOBI_SWEEPS sweeps over the pairs (p, q) = (0,1), (0,2), (1,2);
 *     a pair with S_pq == 0 exactly is skipped, else
 *         theta = (S_qq - S_pp) / (2 * S_pq)
 *         t = 1 / (|theta| + sqrt(theta * theta + 1)), negated where theta < 0
 *         c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * S_pq
 *         S_pp = S_pp - h;  S_qq = S_qq + h;  S_pq = S_qp = 0
 *         with r the third index: (S_rp, S_rq) = (c * S_rp - s * S_rq, s * S_rp + c * S_rq), mirrored
 *         for every row i of V:    (V_ip, V_iq) = (c * V_ip - s * V_iq, s * V_ip + c * V_iq)
 *     eigenvalue j = S_jj, its vector column j of V; sorted by eigenvalue, descending, ties to the lower index
 *     axes 0 and 1 are negated where their component of largest magnitude (ties to the lowest index) is negative;
 *     axis 2 = axis 0 x axis 1, each component one difference of two products: the frame is right-handed
 *     A = float(axes), c = float(m): rounded to f32 once, for the extents pass
 * solid == 0 gives valid = 0 and nothing else is written.
 * The box of a model from its frame and extents (emf_fusion_shape_box), float64 in this order, sums left to right:
 *     mid_k    = (double(lo_k) + double(hi_k)) / 2
 *     centre_j = m_j + (A_0j * mid_0 + A_1j * mid_1 + A_2j * mid_2)         A: the float64 axes
 *     half_k   = (double(hi_k) - double(lo_k)) / 2 + (|A_k0| + |A_k1| + |A_k2|) / 2
 *                the second term is the half-width of a voxel cube along the axis
 *     completeness = double(faces_free) / (double(faces_free) + double(faces_unknown)), NaN when both are 0
 *     metres, in the model's own frame:  centre_obj_j = (centre_j - (double(res_j) - 1) / 2) * double(voxel_size),
 *                half_m_k = half_k * double(voxel_size)
 *     corner i (bit k of i set: +half_m_k, clear: -half_m_k):  p_j = ((centre_obj_j + h_0 * A_0j) + h_1 * A_1j) + h_2 * A_2j
 *     world, with the model's pose (R, t; f32 taken to double):  x_i = (R_i0 * p_0 + R_i1 * p_1 + R_i2 * p_2) + t_i;
 *                world axis k, component i = R_i0 * A_k0 + R_i1 * A_k1 + R_i2 * A_k2
 * ---------------------------------------------------------------------------------------------- */
#define EMF_SHAPE_JACOBI_SWEEPS 8 /* the smallest count after which another sweep changes no bit on the fixtures, + 2 */

typedef struct emf_shape_moments {
    uint64_t solid, observed;           /* counts */
    uint64_t sum[3];                    /* sum of x, y, z over the solid voxels */
    uint64_t sum2[6];                   /* sums of xx, yy, zz, xy, xz, yz */
    uint64_t faces_free, faces_unknown; /* ordered pairs (solid voxel, face neighbour inside the volume) */
    int32_t lo[3], hi[3];               /* bounds of the solid voxels; res and -1 without one */
} emf_shape_moments_t;                  /* 128 bytes */

typedef struct emf_shape_axes {
    float A[9]; /* three row vectors */
    float c[3]; /* the centre, voxel coordinates */
} emf_shape_axes_t; /* 48 bytes */

typedef struct emf_shape_extents {
    float lo[3], hi[3]; /* minimum and maximum of e_k; +inf and -inf without a solid voxel */
} emf_shape_extents_t;  /* 24 bytes */

typedef struct emf_shape_frame {
    int32_t valid, reserved; /* valid == 0 (solid == 0): nothing else is written */
    double centroid[3];      /* m, voxel coordinates */
    double covariance[6];    /* C: xx, yy, zz, xy, xz, yz (voxels^2) */
    double eigenvalues[3];   /* descending (voxels^2) */
    double axes[9];          /* three row vectors, right-handed */
    emf_shape_axes_t f32;    /* the same frame rounded once: what the extents pass takes */
} emf_shape_frame_t;         /* 224 bytes */

typedef struct emf_shape_box {
    double center_vox[3], half_vox[3]; /* voxel coordinates, along the frame's axes */
    double completeness;               /* faces_free / (faces_free + faces_unknown), NaN without either */
    double center_obj[3], half_m[3];   /* metres, the model's own frame */
    double corners_obj[24];            /* 8 x 3 */
    double center_world[3], axes_world[9], corners_world[24];
} emf_shape_box_t;                     /* 584 bytes */

/* Both run over the slots [first, first + n) of a device model table, 1 <= n, first >= 0, first + n <= EMF_MAX_MODELS,
 * in ONE launch for the whole range (plus the small launches that initialise and finish the records).  res_host: HOST
 * int32[3 n], the resolutions of those slots as the table stores them.  Of a model tsdf, weights, fgVolMask (NULL: no
 * gate), res and unseenTiles are read; nothing of a model is written.  A workgroup whose 32 x 8 x 8 tile the model's
 * unseenTiles map (NULL: none) marks "every weight is 0" adds nothing of its own and is skipped; its voxels are still
 * read as the neighbours of other tiles' solid voxels.
 *   moments_dev  n records (record k: slot first + k), initialised by the call on the stream, then one integer atomic
 *                per non-zero quantity and workgroup
 *   frames_dev   n emf_shape_axes_t, only read;  extents_dev: n records, initialised by the call on the stream
 * A second call into the same buffers gives the same bytes.  Every rejected argument -- a NULL pointer, n <= 0,
 * first < 0, first + n > EMF_MAX_MODELS, an axis outside the limits -- returns EMF_E_ARG or EMF_E_LIMIT with nothing
 * enqueued.  Nothing allocates, copies to the host or waits. */
int emf_hip_shapeMoments(const emf_model_t* models_dev, const int32_t* res_host, int32_t first, int32_t n,
                         emf_shape_moments_t* moments_dev, emf_stream_t stream);
int emf_hip_shapeExtents(const emf_model_t* models_dev, const int32_t* res_host, int32_t first, int32_t n,
                         const emf_shape_axes_t* frames_dev, emf_shape_extents_t* extents_dev, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Ground map (new behaviour: DESIGN.md 5.24).  Opt-in; nothing above is touched.  A box of class bytes, as
 * emf_hip_occupancyClasses + emf_hip_occupancyStampObjects leave it, is projected along a given "up" onto a 2-D lattice
 * of ground cells with a column of height bins per cell; every column reduces to a floor level, its headroom and a
 * 2-D class, so that a robot that drives on a floor can use the 2-D paths of the entries above (size = (W, H, 1)).
 * After one float mapping per voxel everything is integer: the results are pure functions of the inputs, bit for bit.
 *
 * Input: classes, dense, (z, y, x) order, x fastest, size = (nx, ny, nz), and an emf_ground_frame_t BY VALUE from host
 * memory: G, a 3 x 4 row-major map from box voxel to ground coordinates (row 0: u in cells, row 1: v in cells, row 2:
 * h in height bins), map = (W, H), each in 1 .. EMF_DF_MAX_AXIS, and bins = B in 1 .. EMF_GROUND_MAX_BINS.
 *
 * Slot of the voxel (x, y, z), every line a single float32 operation in this order, never contracted:
 *     q_j = ((G_j0 * float(x) + G_j1 * float(y)) + G_j2 * float(z)) + G_j3        j = u, v, h
 *     i_j = floorf(q_j)
 * The voxel is dropped unless 0 <= i_u < W, 0 <= i_v < H and 0 <= i_h < B, compared in float before any cast: a NaN or
 * an infinity drops the voxel (-0.0 is cell 0).
 *
 * Bit columns: per cell c = i_v * W + i_u two bit planes occ and fre of words = (B + 63) / 64 u64 words each, word w
 * of cell c at index c * words + w, bit i_h & 63 of word i_h >> 6.  An EMF_OCC_OCCUPIED voxel sets its bit of occ, an
 * EMF_OCC_FREE voxel its bit of fre; EMF_OCC_UNKNOWN and class bytes above 2 set nothing.  EVERY voxel counts, nothing
 * is sampled: a thin obstacle inside a coarse cell is never missed.  OR does not depend on the order of the voxels.
 * Slot state: OCC if the occ bit is set; FREE if it is clear and the fre bit is set; UNK otherwise.
 *
 * Cell records emf_ground_cell_t for a robot height of R >= 1 bins:
 *     level k is standable iff slot k is OCC, k + R <= B - 1 and the slots k + 1 .. k + R are all FREE
 *     floor   the lowest standable level, or -1          top     the highest OCC slot, or -1
 *     clear   the number of consecutive FREE slots directly above floor, or 0 without one
 *     levels  the number of standable levels
 *
 * 2-D classes, one byte per cell, (1, H, W) order, u fastest, for a largest step of S >= 0 bins:
 *     floor >= 0   EMF_OCC_FREE, unless one of the eight neighbours INSIDE the map has floor_n >= 0 and
 *                  |floor - floor_n| > S: then EMF_OCC_OCCUPIED.  A neighbour without a floor constrains nothing.
 *     floor < 0    EMF_OCC_OCCUPIED if top >= 0, else EMF_OCC_UNKNOWN
 * The array is a valid input of every class-volume entry above with size = (W, H, 1).
 *
 * Holes: the ground lattice is rotated against the voxel lattice; a closed ball of radius sqrt(3) / 2 always holds a
 * lattice point, so with cells and bins of at least 2 voxels every slot that lies wholly inside the box receives a voxel
 * centre.  Narrower slots can stay empty and break a FREE run by a spurious UNK unless up is along a box axis.  The
 * entries take any frame; the layers above refuse narrower slots on a tilted frame.
 *
 * The frame on the host (emf_fusion_ground_frame of include/emf_fusion.h; no device): float64, every line a single
 * operation in this order, sums left to right, no contraction.  Inputs: the query box (lo, the background's resolution
 * res, voxel size vs and pose R, t: volume -> world, f32 taken to double), up, cell and bin in metres, a reference world
 * point ref and a band (lo_m, hi_m) in metres relative to ref along up.  The world point of the box voxel b (any real
 * b) is that of QueryBox::worldPoint:  p_i = (R_i0 * o_0 + R_i1 * o_1 + R_i2 * o_2) + t_i  with
 * o_j = ((double(lo_j) + b_j) - (double(res_j) - 1) / 2) * vs.
 *     1  h = up / sqrt(up_0 * up_0 + up_1 * up_1 + up_2 * up_2)            (a zero or non-finite up: EMF_E_ARG)
 *     2  a = column 0 of R;  d = a_0 * h_0 + a_1 * h_1 + a_2 * h_2;  w_i = a_i - d * h_i;
 *        n2 = w_0 * w_0 + w_1 * w_1 + w_2 * w_2;  if n2 < 1e-6 the same with a = column 2 of R;  u = w / sqrt(n2)
 *     3  v = h x u, each component one difference of two products
 *     4  with E = (u, v, h) as rows:  M_jk = (E_j0 * R_0k + E_j1 * R_1k + E_j2 * R_2k) * vs      per voxel step
 *        c_j = ((double(lo_j)) - (double(res_j) - 1) / 2) * vs;   p0_i = (R_i0 * c_0 + R_i1 * c_1 + R_i2 * c_2) + t_i
 *        g_j = E_j0 * p0_0 + E_j1 * p0_1 + E_j2 * p0_2                   ground metres of box voxel (0, 0, 0)
 *     5  rows j = 0, 1:  A_jk = M_jk / cell,  a_j = g_j / cell;  over the eight corners b_k in {-0.5, size_k - 0.5}, the
 *        corner index counting x fastest:  s = ((A_j0 * b_0 + A_j1 * b_1) + A_j2 * b_2) + a_j,  mn_j and mx_j their
 *        minimum and maximum;  G_j3 = a_j - mn_j;  W (j = 0) or H (j = 1) = floor(mx_j - mn_j) + 1, above
 *        EMF_DF_MAX_AXIS: EMF_E_LIMIT
 *     6  row 2:  A_2k = M_2k / bin;  z0 = (h_0 * ref_0 + h_1 * ref_1 + h_2 * ref_2) + lo_m;  G_23 = (g_2 - z0) / bin
 *     7  B = ceil((hi_m - lo_m) / bin); below 1 EMF_E_ARG, above EMF_GROUND_MAX_BINS EMF_E_LIMIT
 *     8  G = float(A | G_j3): rounded to f32 once
 * The ground pose "ground coordinates in metres -> world" has the rotation (u, v, h) as COLUMNS and the translation
 * o_i = u_i * (mn_0 * cell) + v_i * (mn_1 * cell) + h_i * z0 (left to right): the ground point (cu, cv, ch) metres --
 * cu = (i_u + 0.5) * cell for the centre of cell i_u, ch = (i_h + 1) * bin for the top face of bin i_h -- is the world
 * point  ((o_i + u_i * cu) + v_i * cv) + h_i * ch.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_GROUND_MAX_BINS 256

typedef struct emf_ground_frame {
    float G[12];    /* 3 x 4 row-major: box voxel -> (u in cells, v in cells, h in bins) */
    int32_t map[2]; /* W, H */
    int32_t bins;   /* B */
} emf_ground_frame_t; /* 60 bytes */

typedef struct emf_ground_cell {
    int16_t floor, top, clear, levels;
} emf_ground_cell_t; /* 8 bytes */

/*   groundColumns  classes_dev: the box, only read.  occ_dev, fre_dev: W * H * words u64 each, 8-byte aligned, distinct;
 *                  zeroed by the call on the stream, then 64-bit integer atomicOr, issued only for known voxels, the
 *                  lanes of a wave that share a destination word combined first.
 *   groundCells    one lane per cell; robot_bins = R >= 1.  cells_dev: W * H records.
 *   groundClasses  one lane per cell; max_step = S >= 0.  classes2d_dev: W * H bytes, distinct from nothing it reads.
 * A second call into the same buffers gives the same bytes.  Every rejected argument -- a NULL pointer, a misaligned
 * plane, an axis, a map side or a bin count outside its limits (below 1: EMF_E_ARG, above: EMF_E_LIMIT), more than
 * 2^31 - 1 voxels (EMF_E_LIMIT), R < 1, S < 0 -- returns its code with nothing enqueued.  Nothing allocates, copies to
 * the host or waits. */
int emf_hip_groundColumns(const uint8_t* classes_dev, const int32_t size[3], emf_ground_frame_t frame, uint64_t* occ_dev,
                          uint64_t* fre_dev, emf_stream_t stream);
int emf_hip_groundCells(const uint64_t* occ_dev, const uint64_t* fre_dev, const int32_t map[2], int32_t bins,
                        int32_t robot_bins, emf_ground_cell_t* cells_dev, emf_stream_t stream);
int emf_hip_groundClasses(const emf_ground_cell_t* cells_dev, const int32_t map[2], int32_t max_step,
                          uint8_t* classes2d_dev, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Planes (new behaviour: DESIGN.md 5.25).  Opt-in; nothing above is touched.  What the scene is made of: the dominant
 * planes -- floor, walls, table tops -- of a box [box_lo, box_lo + box_size) of a volume, by a three-stage vote on the
 * TSDF gradients of its surface voxels: direction, then offset, then assignment with integer moments for a least-squares
 * refit.  Every float step below is a single float32 operation in the stated order, never contracted whatever the build;
 * everything after it is integer.  Every output is a pure function of the inputs, bit for bit.
 * Volumes and boxes are dense, (z, y, x) order, x fastest; a box voxel is b = (x, y, z), its linear index
 * (z * by + y) * bx + x with box_size = (bx, by, bz).  Box limits are those of emf_hip_occupancyClasses.
 * WHAT A PLANE IS: the plane of the SHELL's voxel centres.  A solid voxel with a free face neighbour lies less than one
 * voxel behind the zero crossing, so a plane fitted to these records sits up to one voxel behind the surface.  Nothing
 * here corrects that.
 *
 * Stage 1, surface records.  The rules of emf_hip_shapeMoments without a mask:
 *     solid(v)    weights[v] > 0 && !(tsdf[v] > 0)                 free(n)   weights[n] > 0 && tsdf[n] > 0
 *     surface(v)  solid(v) and at least one of the six face neighbours INSIDE THE VOLUME is free
 *     normal(v)   surface(v), all six face neighbours lie inside the volume and have weights > 0, the three differences
 *                 g_j = tsdf[v + e_j] - tsdf[v - e_j] (one float32 subtraction each) are finite and not all zero
 * Neighbours come from the volume, not from the box: the records of a box are exactly those of the whole volume that
 * fall into it, re-indexed.  g points from solid to free space.
 * Output: the voxels with a normal as emf_plane_voxel_t, in this fixed order: tiles of 32 x 8 x 8 voxels anchored at the
 * box origin, partial ones included, in (z, y, x) order of the tiles, then the voxels inside a tile in (z, y, x) order.
 * Positions come from a count per tile, an exclusive scan and a second pass; no atomic decides a position.  At most
 * `capacity` records are written: the first `capacity` of that order.
 *     counters (device, 4 x u32): [0] surface voxels, [1] those with a normal, [2] records written = min([1], capacity),
 *     [3] 0.  Zeroed and written by the call on the stream.
 *     scratch: emf_hip_planeSurfaceScratchBytes(box_size) bytes, one u32 per tile (0 for a size beyond the limits);
 *     contents undefined afterwards.  At most 2^24 - 1 tiles (EMF_E_LIMIT above).
 *     unseenTiles: NULL or the VOLUME's unseen-tile map (emf_hip_unseenTileBytes(res)).  A workgroup whose voxels all lie
 *     in tiles marked "every weight is 0" leaves at once; a surface voxel is observed, so that is exact: the bytes are
 *     the same with the map and without it.
 *     capacity == 0: records may be NULL, only the counters are written.  capacity <= 2^31 - 1.
 *
 * Stage 2a, direction votes.  A cube map with K cells per face side, K in 1 .. EMF_PLANE_MAX_K: 6 K^2 bins of u32.  For
 * a record with gradient g (a record whose g has a component that is not finite, or is all zero, votes for nothing;
 * stage 1 writes none):
 *     m    = the index of the largest |g_j|, ties to the lowest index
 *     face = 2 m + (g_m < 0)
 *     u    = g_((m + 1) % 3) / |g_m|,  v = g_((m + 2) % 3) / |g_m|          one IEEE division each
 *     cell(u) = min(int(floorf((u + 1.f) * h)), K - 1)   with h = float(K) / 2.f formed once on the host
 *     bin  = (face * K + cell(v)) * K + cell(u)
 * The bins are zeroed by the call; the histogram is kept in LDS per workgroup and flushed with integer atomics.
 *
 * Stage 2b, offset votes.  D unit directions n_k (f32, box voxel coordinates), D in 1 .. EMF_PLANE_MAX_DIRS, with cos2 in
 * [0, 1], inv_bin, one shift_k per direction and S slots, S in 1 .. EMF_PLANE_MAX_SLOTS.  With (x, y, z) the record's box
 * voxel as floats:
 *     a  = (n0 * g0 + n1 * g1) + n2 * g2        gg = (g0 * g0 + g1 * g1) + g2 * g2
 *     ALIGNED with k iff  a > 0 && a * a >= cos2 * gg   as computed; a NaN aligns with nothing
 *     slot = floorf(((n0 * x + n1 * y) + n2 * z) * inv_bin + shift_k)
 * An aligned record votes for hist[k * S + slot] iff 0 <= slot < S, compared in float before any cast, in every
 * direction it is aligned with.  hist: D * S u32 in device memory, zeroed by the call.  One atomic per run of
 * neighbouring lanes of a wave with the same destination.
 *
 * Stage 3, assignment.  P planes (n_k, d_k) in f32, P in 1 .. EMF_PLANE_MAX_PLANES, with cos2 and a band >= 0 in voxels.
 *     e_k = ((n0 * x + n1 * y) + n2 * z) - d_k
 * A record belongs to the plane of smallest |e_k| among those it is ALIGNED with (as above) and for which
 * |e_k| <= band; ties go to the lowest k.  labels: one i16 per record written by stage 1 (-1: none); labels past
 * counters[2] are not written.  moments: P records emf_plane_moments_t of integers only, initialised by the call
 * (count 0, lo = box_size, hi = -1), then per run of equal labels in a wave one integer atomic per quantity.
 * A second call of any entry into the same buffers gives the same bytes.
 *
 * The three entries of stages 2 and 3 read the record count counters[2] on the device, bounded by `capacity` (the
 * capacity given to stage 1, 1 .. 2^31 - 1): the host does not wait in between.  dirs_host (3 D f32), shift_host (D f32)
 * and planes_host (4 P f32: n0, n1, n2, d) are HOST arrays, read before the call returns.
 * Every rejected argument -- a NULL pointer, a misaligned array (records: 16 bytes, moments: 8), a count below 1
 * (EMF_E_ARG) or above its limit (EMF_E_LIMIT), cos2 outside [0, 1] or NaN, a negative or NaN band -- returns its code
 * with nothing enqueued.  Nothing allocates, copies to the host or waits.
 *
 * Stage 4, patches.  A plane of stage 3 is infinite: two tables of one height are one plane.  This stage
 * splits every plane into its connected surfaces.  Inputs: records (stage 1's output in stage 1's order), labels (stage
 * 3's output), counters (n = min(counters[2], capacity) is read on the device, as stages 2 and 3 do), box_size and a
 * reach in 1 .. EMF_PLANE_MAX_REACH.
 *     Two records are LINKED iff their labels are equal and >= 0 and the Chebyshev distance of their box voxels (from
 *     `index`) is <= reach.  Only the record list matters: a voxel without a record links nothing.
 *     A PATCH is a connected component of the link graph; its id is the smallest RECORD INDEX among its members.  Record
 *     order is the fixed tile order of stage 1, so the id is a pure function of the inputs.
 *     patch: one i32 per record, the id, or -1 where labels[i] < 0.  Entries past n are not written.
 *     patch_counters (device, 3 x u32): [EMF_PATCH_KEPT] patches of at least min_count members (written by
 *     emf_hip_planePatches, zeroed by emf_hip_planePatchLabel), [EMF_PATCH_PATCHES] all patches, [EMF_PATCH_MEMBERS]
 *     records with a label >= 0.  Always the full numbers, whatever the capacities.
 * How a neighbour is found: there is NO dense volume; scratch is O(records + patches).  Stage 1's order is strictly
 * increasing in the key  tile(v) * 2048 + within(v)  with, for the 32 x 8 x 8 tiles anchored at the box origin,
 *     tile(v)   = ((z / 8) * ceil(by / 8) + y / 8) * ceil(bx / 32) + x / 32
 *     within(v) = ((z % 8) * 8 + y % 8) * 32 + x % 32
 * so the record of a voxel is found by a binary search of the voxel's key among the n records' own keys, recomputed
 * from `index`.  One lane per member visits the HALF neighbourhood of the offsets (dx, dy, dz) that precede (0, 0, 0) in
 * (z, y, x) order -- dz < 0, or dz == 0 and dy < 0, or dz == dy == 0 and dx < 0 -- with |dx|, |dy|, |dz| <= reach: 13
 * offsets at reach 1, 62 at reach 2; a neighbour outside the box is skipped, the others are searched, their label compared
 * and the two records united in a lock-free union-find over record indices whose roots are minimal indices.
 * Records that are NOT in stage 1's order give unspecified patches, but no access leaves the arrays: the search is
 * bounded by n, a record whose index lies outside [0, bx * by * bz) has no voxel (it links nothing), no array is indexed
 * by a voxel, and a slot is used only where it holds the record's patch.
 *
 * Patch records emf_plane_patch_t: id, plane (the members' label), count, sum and sum2 in the layout of
 * emf_plane_moments_t, the bounds lo, hi of the members, and ulo, uhi, vlo, vhi: the minimum and maximum over the members of
 *     e_u = (u0 * x + u1 * y) + u2 * z        e_v = (v0 * x + v1 * y) + v2 * z
 * each line a single float32 operation, never contracted, with (u, v) the two in-plane axes of the member's PLANE from
 * axes_host (HOST, 6 P f32: u0, u1, u2, v0, v1, v2 per plane, read before the call returns).  They are reduced on the
 * order-preserving u32 key of emf_hip_shapeExtents, so they do not depend on the order of lanes or workgroups.  A member
 * whose label is >= P contributes to everything but the four floats (+inf, -inf without a contribution).
 * Roots are ranked by a scan in record order; a record finds its patch's slot by binary search; the integer sums are
 * aggregated per run of equal patch within a wave, then one integer atomic per quantity and run.  Patches of fewer than
 * min_count (>= 1) members are dropped; the kept ones are written in ascending id order, placed by scan, at most
 * capacity_patches (>= 0; 0: out may be NULL) of them.
 *     n_patches: patch_counters[EMF_PATCH_PATCHES] as the host read it after emf_hip_planePatchLabel -- the one wait, with
 *     the contract of emf_hip_frontierClusters: a smaller value drops the patches of the largest ids (from the records
 *     and from EMF_PATCH_KEPT), a larger one only wastes scratch; 0 writes EMF_PATCH_KEPT = 0 and nothing else.
 *     scratch: emf_hip_planePatchScratchBytes(capacity, n_patches) bytes, 16-byte aligned (0 for a capacity outside
 *     1 .. 2^31 - 1); contents undefined afterwards.
 * Every buffer is initialised by a launch of the entry's own: a second call into dirty buffers gives the same bytes.
 * Every rejected argument -- a NULL pointer, a reach below 1 (EMF_E_ARG) or above EMF_PLANE_MAX_REACH (EMF_E_LIMIT),
 * min_count < 1, P outside 1 .. EMF_PLANE_MAX_PLANES, a negative capacity_patches, a misaligned array (records and
 * scratch: 16 bytes, out: 8, patch and counters: 4, labels: 2) -- returns its code with nothing enqueued.  Nothing
 * allocates, copies to the host or waits.
 * ---------------------------------------------------------------------------------------------- */
#define EMF_PLANE_MAX_K 31
#define EMF_PLANE_MAX_REACH 2
#define EMF_PATCH_KEPT 0
#define EMF_PATCH_PATCHES 1
#define EMF_PATCH_MEMBERS 2
#define EMF_PLANE_MAX_DIRS 16
#define EMF_PLANE_MAX_SLOTS 4096
#define EMF_PLANE_MAX_PLANES 64

typedef struct emf_plane_voxel {
    int32_t index; /* linear index in the box */
    float g[3];    /* tsdf[v + e_j] - tsdf[v - e_j] */
} emf_plane_voxel_t; /* 16 bytes */

typedef struct emf_plane_moments {
    uint64_t count;
    uint64_t sum[3];     /* sum of x, y, z over the members, BOX voxel coordinates */
    uint64_t sum2[6];    /* sums of xx, yy, zz, xy, xz, yz: the layout of emf_shape_moments_t */
    int32_t lo[3], hi[3]; /* bounds of the members; box_size and -1 without one */
} emf_plane_moments_t;   /* 104 bytes */

typedef struct emf_plane_patch {
    int32_t id, plane;        /* the smallest record index of the members; their label */
    uint64_t count;
    uint64_t sum[3];          /* as emf_plane_moments_t */
    uint64_t sum2[6];
    int32_t lo[3], hi[3];     /* bounds of the members, box voxels */
    float ulo, uhi, vlo, vhi; /* extents along the plane's two in-plane axes, voxels */
} emf_plane_patch_t;          /* 128 bytes */

/* The host steps between the stages (emf_fusion_plane_directions / _offsets / _fit of include/emf_fusion.h; no device).
 * Float64, every line a single operation in this order, sums left to right, no contraction:
 *   directions  bins sorted by count descending, ties to the lower bin.  Greedy: a bin of at least min_votes becomes a
 *               direction unless its dot with an already chosen one exceeds cos(separation * pi / 180); at most
 *               EMF_PLANE_MAX_DIRS.  The direction of bin b (face, iv, iu as above, m = face / 2) is the normalised centre
 *               of its cell: c_m = +1 or -1, c_((m+1)%3) = (iu + 0.5) / (K / 2) - 1, c_((m+2)%3) = (iv + 0.5) / (K / 2) - 1,
 *               n = c / sqrt((c0 * c0 + c1 * c1) + c2 * c2).
 *   offsets     per direction, over the eight corners b_j in {-0.5, size_j - 0.5} of the box's voxel cubes (x fastest):
 *               s = (n0 * b0 + n1 * b1) + n2 * b2, lo and hi their minimum and maximum; S = floor((hi - lo) / bin) + 1
 *               (above EMF_PLANE_MAX_SLOTS: EMF_E_LIMIT), inv_bin = 1 / bin, shift = -lo * inv_bin; inv_bin and shift are
 *               rounded to f32 once for stage 2b.  Peaks of a direction's S slots: slots by votes descending, ties to the
 *               lower slot; a slot of at least min_votes is a peak unless a chosen one lies within peak_gap slots.  The
 *               offset of a peak is the centre of its slot, d = lo + (slot + 0.5) * bin.  Seed planes ordered by votes,
 *               ties by (direction, slot), at most max_planes <= EMF_PLANE_MAX_PLANES.
 *   fit         from a plane's emf_plane_moments_t: centroid m, covariance and Jacobi frame are those of
 *               emf_fusion_shape_frame (count -> solid, sum, sum2), called, not restated.  n = the axis of the smallest
 *               eigenvalue, negated where its dot with the seed normal is negative, so that it points into free space;
 *               d = (n0 * m0 + n1 * m1) + n2 * m2; thickness = sqrt(max(eigenvalue, 0)) in voxels; the two in-plane axes
 *               and all three eigenvalues are kept.  A plane of fewer than 3 members keeps its seed (fitted = 0).
 *   rounds      (refine + 1) times: stage 3 with the current planes rounded to f32 once, then the fit of every plane.
 *   gate        cos2 = float(c * c) with c = cos(angle * pi / 180). */
typedef struct emf_plane_params {
    int32_t K;          /* cells per cube-map face side, 1 .. EMF_PLANE_MAX_K */
    int32_t refine;     /* >= 0 */
    int32_t max_planes; /* 1 .. EMF_PLANE_MAX_PLANES */
    int32_t peak_gap;   /* slots, >= 0 */
    double angle_deg;      /* the alignment gate, (0, 90] */
    double separation_deg; /* between directions; <= 0: angle_deg */
    double bin_vox;        /* the width of an offset slot in voxels, > 0 */
    double band_vox;       /* the assignment band in voxels, >= 0 */
    int64_t min_votes;     /* <= 0: max(50, records / 200) */
} emf_plane_params_t; /* 56 bytes */

typedef struct emf_plane {
    double n[3], d;        /* box voxel coordinates: n . b = d; n points into free space */
    double centroid[3];    /* of the members (fitted != 0) */
    double thickness;      /* sqrt of the smallest eigenvalue, voxels */
    double axes[6];        /* the two in-plane axes, larger eigenvalue first */
    double eigenvalues[3]; /* descending, voxels^2 */
    uint64_t count;        /* members */
    int32_t lo[3], hi[3];  /* their bounds, box voxels */
    int32_t fitted, label; /* label: the plane's value in the label array */
} emf_plane_t; /* 176 bytes */

/* The host steps behind stage 4 (emf_fusion_plane_patch_rect of include/emf_fusion.h; no device).  Float64, every line a
 * single operation in this order, sums left to right, no contraction.  Inputs: the patch and its PLANE (n, d, axes
 * u = axes[0..2], v = axes[3..5], box voxel coordinates).
 *   fit         emf_fusion_plane_fit CALLED on the patch's count, sum, sum2, lo, hi with the plane's (n, d) as the seed:
 *               the patch's own centroid, normal, d and thickness; below 3 members it keeps the seed (fitted = 0).
 *   rectangle   the extents widened by half a voxel on each side:
 *                   a0 = double(ulo) - 0.5   a1 = double(uhi) + 0.5   b0 = double(vlo) - 0.5   b1 = double(vhi) + 0.5
 *                   cu = (a0 + a1) * 0.5     hu = (a1 - a0) * 0.5     cv = (b0 + b1) * 0.5     hv = (b1 - b0) * 0.5
 *               center_j = (d * n_j + u_j * cu) + v_j * cv, and the corners k = 0 .. 3 with (su, sv) = (-1, -1), (+1, -1),
 *               (+1, +1), (-1, +1):  eu = cu + su * hu,  ev = cv + sv * hv,  corner_kj = (d * n_j + u_j * eu) + v_j * ev
 *               (each product formed first, then added), with the PLANE's n and d: the rectangle lies in the plane.
 *   fill        count / (((double(uhi) - double(ulo)) + 1) * ((double(vhi) - double(vlo)) + 1) * max |n_j|), the
 *               products left to right: near 1 for a full rectangle, lower for an L shape or one with holes.  A ratio
 *               of two estimates. */
typedef struct emf_plane_patch_rect {
    emf_plane_t fit;    /* the patch's own fit */
    double center[3];   /* box voxel coordinates */
    double half[2];     /* hu, hv in voxels */
    double corners[12]; /* 4 x 3 */
    double fill;
} emf_plane_patch_rect_t; /* 320 bytes */

size_t emf_hip_planeSurfaceScratchBytes(const int32_t box_size[3]);
int emf_hip_planeSurface(const float* tsdf, const float* weights, const int32_t res[3], const int32_t box_lo[3],
                         const int32_t box_size[3], const uint8_t* unseenTiles, emf_plane_voxel_t* records, uint32_t capacity,
                         uint32_t* counters, void* scratch, emf_stream_t stream);
int emf_hip_planeDirections(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity, int32_t K,
                            uint32_t* bins, emf_stream_t stream);
int emf_hip_planeOffsets(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity,
                         const int32_t box_size[3], const float* dirs_host, const float* shift_host, int32_t D, float cos2,
                         float inv_bin, int32_t S, uint32_t* hist, emf_stream_t stream);
int emf_hip_planeAssign(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity,
                        const int32_t box_size[3], const float* planes_host, int32_t P, float cos2, float band,
                        int16_t* labels, emf_plane_moments_t* moments, emf_stream_t stream);
int emf_hip_planePatchLabel(const emf_plane_voxel_t* records, const int16_t* labels, const uint32_t* counters, uint32_t capacity,
                            const int32_t box_size[3], int32_t reach, int32_t* patch, uint32_t* patch_counters,
                            emf_stream_t stream);
size_t emf_hip_planePatchScratchBytes(uint32_t capacity, uint32_t n_patches);
int emf_hip_planePatches(const emf_plane_voxel_t* records, const int16_t* labels, const int32_t* patch, const uint32_t* counters,
                         uint32_t capacity, const int32_t box_size[3], const float* axes_host, int32_t P, int64_t min_count,
                         uint32_t n_patches, void* scratch, emf_plane_patch_t* out, int32_t capacity_patches,
                         uint32_t* patch_counters, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Object contacts (new behaviour: DESIGN.md 5.27).  Opt-in; nothing above is touched.  Whether two models touch, how
 * far apart their surfaces are and whether they interpenetrate, read from their signed-distance volumes: a surface
 * voxel of model a, taken through the relative pose into model b's volume and sampled there trilinearly, reads b's
 * signed distance at a point of a's surface.
 * IT MEASURES WHAT THE VOLUMES SAY:
 *   - a tsdf is clamped to +-1, so min_s == 1 means "at least one truncation distance apart" and is not a distance;
 *   - nothing is fused deeper than one truncation distance behind a surface, so a deeper penetration reads UNKNOWN,
 *     not a larger depth;
 *   - a surface voxel lies up to one voxel behind a's zero crossing, so clearances read up to one probe voxel large.
 * An ordered PAIR is (probe a, field b): two different slots of a device model table, R[9], t[3] (f32, b's frame <-
 * a's frame, row-major) and touch (f32, in units of b's stored tsdf, i.e. fractions of b's truncation distance).
 * Volumes are dense, (z, y, x) order, x fastest, res = (nx, ny, nz); a voxel is v = (x, y, z).  Every float step below
 * is a single float32 operation without contraction, in this order; everything else is integer.
 *   solid(v), free(n)  exactly the rules of emf_hip_shapeMoments: solid(v) = weights[v] > 0 && (fgVolMask == NULL ||
 *                fgVolMask[v] != 0) && !(tsdf[v] > 0) with a's mask; free(n) = weights[n] > 0 && tsdf[n] > 0, the mask
 *                plays no part.  A neighbour outside the volume does not exist.
 *   surface(v)   solid(v) and at least one of the face neighbours inside a's volume is free.
 *   sample point of a surface voxel (the stamping arithmetic of emf_hip_occupancyStampObjects with the roles named;
 *                half_j = float(N_j - 1) / 2.f; rows of R summed left to right):
 *                    p_a_j = (float(v_j) - half_a_j) * voxelSize_a
 *                    p_b_i = ((R_i0 * p_a_0 + R_i1 * p_a_1) + R_i2 * p_a_2) + t_i
 *                    q_i   = p_b_i / voxelSize_b + half_b_i
 *                    l_i = int(q_i),  f_i = q_i - float(l_i)
 *   classes, first match wins:
 *     OUTSIDE    some q_j is NaN, q_j < 0 or q_j + 1 >= float(N_j) of b: the pad-1 rule of the raycast's lookups.  All
 *                eight corners l + {0, 1}^3 of every other cell lie inside b's volume.
 *     UNKNOWN    one of the eight corners has !(weights_b > 0), or the blended value s is NaN
 *     MASKED     b has an fgVolMask and it is 0 at the voxel (rint(q_0), rint(q_1), rint(q_2)), ties to even (inside
 *                the volume by the rule above)
 *     SAMPLED    everything else
 *   s            b's tsdf blended over the cell in the reference's order: x pairs, then y, then z, each
 *                (1 - f) * c0 + f * c1 as one difference, two products and one sum
 *   INSIDE       SAMPLED and s < 0.   TOUCHING: SAMPLED and s <= touch (it contains INSIDE when touch >= 0; never with a
 *                NaN touch).
 *   normal of a touching voxel: all six face neighbours of v lie inside a's volume with weights > 0 and the three
 *                g_j = tsdf[v + e_j] - tsdf[v - e_j] are finite; then gq_j = int(rintf(min(max(g_j * 4096.f, -8192.f),
 *                8192.f))).  The clamp changes nothing for a tsdf within +-1 and bounds every sum for any other:
 *                2^31 voxels of +-8192 stay below 2^53.
 * emf_contact_t, per pair, integers except min_s:
 *     surface = outside + unknown + masked + sampled;  inside, touching <= sampled;  normals <= touching
 *     sum       the sums of x, y, z of the TOUCHING voxels in a's lattice;  gsum: of gq over those with a normal
 *     lo, hi    bounds of the touching voxels; res_a and -1 without one
 *     min_s     the minimum of s over SAMPLED, taken on the order-preserving u32 key of emf_hip_shapeExtents (-0 below
 *               +0); +inf when sampled == 0
 * Every field is a pure function of the inputs, bit for bit, whatever order lanes and workgroups run in.
 * Limits: 1 <= n_models <= EMF_MAX_MODELS, 1 <= n_pairs <= EMF_CONTACT_MAX_PAIRS; of every slot a pair names, each
 * axis in 1 .. EMF_DF_MAX_AXIS and at most 2^31 - 1 voxels; the probes of a call (each distinct probe once) together at
 * most 2^24 - 1 tiles of 32 x 8 x 8 voxels.
 *
 * The host stage (include/emf_fusion.h emf_fusion_contact_pose / _touch / _summary; no device, no handle).  Float64,
 * every line a single operation in this order, sums left to right, no contraction; f32 inputs are taken to double.
 *   pose (what a pair carries), from the poses (world <- model) of a and b:
 *       R_ij = float((Rb_0i * Ra_0j + Rb_1i * Ra_1j) + Rb_2i * Ra_2j)
 *       d_k  = ta_k - tb_k;   t_i = float((Rb_0i * d_0 + Rb_1i * d_1) + Rb_2i * d_2)
 *   touch:  float(touch_m / double(truncdist_b)), touch_m a double in metres
 *   summary of the unordered pair {a, b} from the record a -> b and, where b was a probe as well, b -> a:
 *       state, first match wins: PENETRATING some inside > 0, TOUCHING some touching > 0, APART some sampled > 0, else
 *             UNSEEN
 *       d_ab = double(min_s_ab) * double(truncdist_b),  d_ba = double(min_s_ba) * double(truncdist_a)
 *       distance_m = d_ba < d_ab ? d_ba : d_ab (d_ab alone without a second record); saturated: the deciding min_s == 1
 *       direction: the record with more touching voxels, ties to a -> b; -1 when neither has one (point, normal and
 *             corners are zeros then).  With p its probe (res, voxelSize, pose R, t):
 *           m_j = double(sum_j) / double(touching);  h_j = (double(res_j) - 1) / 2;  o_j = (m_j - h_j) * double(voxelSize)
 *           point_i = ((R_i0 * o_0 + R_i1 * o_1) + R_i2 * o_2) + t_i
 *           normal: len = sqrt((g_0 * g_0 + g_1 * g_1) + g_2 * g_2) with g = double(gsum); has_normal = normals > 0 &&
 *                 len > 0; u_j = g_j / len; normal_i = (R_i0 * u_0 + R_i1 * u_1) + R_i2 * u_2: out of the probe
 *           corner c (bit j of c set: hi_j, clear: lo_j) goes the way of m_j: the box of the contact region in the world
 * ---------------------------------------------------------------------------------------------- */
#define EMF_CONTACT_MAX_PAIRS 65535
#define EMF_CONTACT_UNSEEN 0
#define EMF_CONTACT_APART 1
#define EMF_CONTACT_TOUCHING 2
#define EMF_CONTACT_PENETRATING 3

typedef struct emf_contact_pair {
    int32_t a, b;     /* probe and field: slots of the model table */
    float R[9], t[3]; /* b's frame <- a's frame, row-major */
    float touch;      /* in units of b's stored tsdf */
    int32_t reserved;
} emf_contact_pair_t; /* 64 bytes */

typedef struct emf_contact {
    uint64_t surface, outside, unknown, masked, sampled, inside, touching, normals; /* counts */
    uint64_t sum[3];        /* sums of x, y, z of the touching voxels */
    int64_t gsum[3];        /* sums of gq over the touching voxels with a normal */
    int32_t lo[3], hi[3];   /* bounds of the touching voxels; res_a and -1 without one */
    float min_s;            /* minimum of s over SAMPLED; +inf without one */
    int32_t reserved;       /* 0 */
} emf_contact_t;            /* 144 bytes */

typedef struct emf_contact_side {
    int32_t res[3];
    float voxelSize, truncdist;
    float R[9], t[3]; /* world <- model */
} emf_contact_side_t; /* 68 bytes */

typedef struct emf_contact_summary {
    int32_t state;      /* EMF_CONTACT_* */
    int32_t saturated;  /* the deciding min_s == 1: at least one truncation distance apart, not a distance */
    int32_t direction;  /* 0: a -> b, 1: b -> a, -1: no touching voxel */
    int32_t has_normal;
    double distance_m;  /* +inf when nothing was sampled */
    double point[3], normal[3], corners[24]; /* world; zeros without a touching voxel (the normal: without has_normal) */
} emf_contact_summary_t; /* 264 bytes */

/* models_dev: the device table, n_models slots; res_host: HOST int32[3 n_models], the resolutions as the table stores
 * them (only the slots a pair names are looked at).  Of a model tsdf, weights, fgVolMask (NULL: no gate), res,
 * voxelSize and, of a probe, unseenTiles are read; nothing of a model is written.  pairs_dev / pairs_host: the same
 * n_pairs pairs in device and in host memory; the host copy serves the argument checks and the launch geometry only
 * and is read before the call returns.  The kernel walks, per probe, the pairs between the first and the last that
 * name it: a list grouped by probe is the fast one, any order gives the same bytes.
 * records_dev: n_pairs records (record k: pair k), initialised by a launch of the call's own on the stream; a second
 * call into the same buffers gives the same bytes.  One workgroup per 32 x 8 x 8 tile of a probe; a tile the probe's
 * unseenTiles map marks holds no surface voxel and is skipped.  One integer atomic per non-zero quantity and wave.
 * Every rejected argument -- a NULL pointer, n_pairs <= 0, a slot outside the table, a == b, an axis outside
 * 1 .. EMF_DF_MAX_AXIS, more than 2^24 - 1 probe tiles -- returns EMF_E_ARG or EMF_E_LIMIT with nothing enqueued.
 * Nothing allocates, copies to the host or waits. */
int emf_hip_contactProbe(const emf_model_t* models_dev, const int32_t* res_host, int32_t n_models,
                         const emf_contact_pair_t* pairs_dev, const emf_contact_pair_t* pairs_host, int32_t n_pairs,
                         emf_contact_t* records_dev, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Absorbing a volume (new behaviour: DESIGN.md 5.29).  Opt-in; nothing above is touched.  The signed-distance band of
 * a SOURCE volume is resampled through a rigid pose into a DESTINATION volume and fused there by the destination's own
 * running average: the one operation that moves geometry from one lattice onto another (roll, spill, fill and
 * copyValues move whole voxels on one lattice).
 * IT CARRIES THE BAND, NOT THE FREE SPACE AROUND IT: a saturated source sample (|s| == 1) only says "at least one
 * source truncation distance away", which with another truncation distance is no value the destination can fuse; such
 * a voxel is left alone.  emf_hip_absorbVolume does not touch colour; emf_hip_absorbVolumeColor (below) carries the
 * voxel's colour entry with the band.
 * Volumes are dense, (z, y, x) order, x fastest, res = (nx, ny, nz); a voxel is v = (x, y, z).  R[9], t[3] (f32,
 * row-major): the source's volume frame <- the destination's volume frame.  Per destination voxel v of the box
 * [box_lo, box_lo + box_size), every float step a single float32 operation without contraction, in this order;
 * everything else is integer.  half_j = float(N_j - 1) / 2.f; rows of R summed left to right; the classes in this
 * order, the first match wins, and only a FUSED voxel is written:
 *   sample point (the stamping arithmetic of emf_hip_occupancyStampObjects, the sample point of "Object contacts"):
 *                    p_d_j = (float(v_j) - half_d_j) * voxelSize_d
 *                    p_s_i = ((R_i0 * p_d_0 + R_i1 * p_d_1) + R_i2 * p_d_2) + t_i
 *                    q_i   = p_s_i / voxelSize_s + half_s_i
 *                    l_i = int(q_i),  f_i = q_i - float(l_i)
 *     OUTSIDE    some q_j is NaN, q_j < 0 or q_j + 1 >= float(N_j) of the source: the pad-1 rule of "Object contacts".
 *     UNKNOWN    one of the eight corners l + {0, 1}^3 has !(weights_s > 0), or the blended value s is NaN; s is the
 *                source's tsdf blended over the cell in x pairs, then y, then z, each (1 - f) * c0 + f * c1 as one
 *                difference, two products and one sum
 *     MASKED     the source has an fgVolMask and it is 0 at (rint(q_0), rint(q_1), rint(q_2)), ties to even
 *     SATURATED  !(fabsf(s) < 1)
 *     FUSED      everything else.  With ratio = truncdist_s / truncdist_d (one float32 division, made once on the host),
 *                w_o the minimum of the eight corner weights (exact, whatever the order) and pw, pt the destination's
 *                weight and tsdf at v:
 *                    u = min(max(s * ratio, -1), 1)                       equal truncation distances: u == s, bit for bit
 *                    !(pw > 0):  nt = u,  nw = min(w_o, maxWeight)        FRESH; a select, pt takes no part
 *                    else:       nt = (pw * pt + w_o * u) / (pw + w_o),  nw = min(pw + w_o, maxWeight)
 *                SOLID: FUSED and !(nt > 0).  Of tsdf[v] and weights[v] only the words whose bits change are stored.
 * emf_absorb_t: visited = outside + unknown + masked + saturated + fused (the voxels of the box); fresh, solid <= fused;
 * lo, hi: the inclusive bounds of the FUSED voxels in the destination, res_d and -1 without one.  Every destination
 * voxel reads and writes only itself: the pass is in place, and the bytes are a pure function of the inputs whatever
 * order lanes and workgroups run in.
 * ---------------------------------------------------------------------------------------------- */
typedef struct emf_absorb_source {
    const float* tsdf;          /* the source volume (device), only read */
    const float* weights;
    const uint8_t* fgVolMask;   /* or NULL: no gate */
    const uint8_t* unseenTiles; /* or NULL: the source's unseen-tile map (emf_hip_unseenTileBytes(res)); a sample whose
                                   first corner lies in a tile marked "every weight is 0" is UNKNOWN unread: the bytes are
                                   the same with the map and without it */
    int32_t res[3];
    float voxelSize;
    float truncdist;
    int32_t reserved;           /* 0 */
} emf_absorb_source_t;          /* 56 bytes */

typedef struct emf_absorb {
    uint64_t visited, outside, unknown, masked, saturated, fused, fresh, solid; /* counts */
    int32_t lo[3], hi[3];       /* bounds of the fused voxels; res_d and -1 without one */
} emf_absorb_t;                 /* 88 bytes */

/* dst_tsdf, dst_weights: the whole destination volume (device), written in place; any resolution from 1 x 1 x 1, no slot
 * of a model table.  record_dev: one record (device, 8-byte aligned), set to the neutral record by a launch of the
 * call's own on the stream and then counted into with one integer atomic per non-zero quantity and wave.  One workgroup
 * of 256 lanes per 32 x 8 x 8 destination tile that meets the box; a box with a size of 0 on some axis is empty:
 * EMF_OK, the neutral record, nothing else written.  The covering box of a whole source is what
 * emf_hip_occupancyObjectBox computes from (res_s, voxelSize_s, R, t).
 * Refused with EMF_E_ARG or EMF_E_LIMIT and nothing enqueued: a NULL or misaligned pointer; a destination array that
 * shares a byte with the other, with an array of the source or with the record (dst == src included); an axis below 1
 * or above EMF_DF_MAX_AXIS or more than 2^31 - 1 voxels, of either volume (EMF_E_LIMIT above, EMF_E_ARG below); a voxel
 * size, a truncation distance, maxWeight or the ratio of the truncation distances that is not finite and > 0; a
 * negative box size or a box that leaves the destination.  Nothing allocates, copies to the host or waits. */
int emf_hip_absorbVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                         float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                         const int32_t box_lo[3], const int32_t box_size[3], emf_absorb_t* record_dev, emf_stream_t stream);

/* Colour with the band.  emf_hip_absorbVolumeColor is emf_hip_absorbVolume -- the same walk, the same
 * classes, and for the same inputs byte for byte the same tsdf, weights and emf_absorb_t -- that also carries the colour
 * ENTRY of "Per-voxel colour" (uint16_t[4] per voxel: R, G, B, Wc in 8.8 fixed point, in the voxel order of the tsdf) of
 * every FUSED voxel; the entry of every other voxel is neither read nor written.  All colour arithmetic is integer and
 * exact: contraction cannot touch it.
 *   SOURCE ENTRY  S = (Sc[3], Sw): src_color at (rint(q_0), rint(q_1), rint(q_2)), ties to even -- the voxel MASKED
 *                 addresses, and the "nearest voxel, no interpolation" rule of emf_hip_sampleColor.  src_color == NULL:
 *                 every source entry is (0, 0, 0, 0).
 *   WEIGHT CAP    capq, made once on the host from max_weight: 65535 if max_weight * 256 >= 65535, otherwise
 *                 lrintf(max_weight * 256.f), and at least 1.
 *   With D = (Dc[3], Dw) the destination's entry at v, read once before any channel is written, and De = 0 if the voxel
 *   is FRESH (!(pw > 0): an unobserved voxel's entry is not evidence), otherwise De = Dw:
 *     UNCOLOURED  Sw == 0: the entry becomes (0, 0, 0, 0) if the voxel is FRESH and stays as it is otherwise.
 *     COLOURED    Sw > 0, per channel:  Dc' = (De * Dc + Sw * Sc + (De + Sw) / 2) / (De + Sw), floor division, exact for
 *                 every u16 input (the products and their sum do not fit 32 bits);  Dw' = min(De + Sw, capq).  With
 *                 De == 0 this is a copy of Sc.
 * emf_color_moved_t: a second device record, neutral at (0, 0) and set by the call's own init launch;
 * colored + uncolored == fused.  An entry whose four values do not change need not be stored. */
typedef struct emf_color_moved {
    uint64_t colored, uncolored;
} emf_color_moved_t;            /* 16 bytes */

/* The arguments of emf_hip_absorbVolume plus dst_color (the destination's colour volume, written in place), src_color
 * (the source's, only read, or NULL) and color_record_dev (device, 8-byte aligned).  Refused with nothing enqueued,
 * on top of everything emf_hip_absorbVolume refuses and with its codes: dst_color NULL (the plain entry is the one to
 * call) or color_record_dev NULL; a colour pointer or the colour record not 8-byte aligned; dst_color or the colour
 * record sharing a byte with any other array of the call.  An empty box: EMF_OK and both neutral records. */
int emf_hip_absorbVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                              float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const uint16_t* src_color,
                              const float R[9], const float t[3], const int32_t box_lo[3], const int32_t box_size[3],
                              emf_absorb_t* record_dev, emf_color_moved_t* color_record_dev, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Lifting a volume (new behaviour: DESIGN.md 5.30).  Opt-in; nothing above is touched.  The opposite direction of
 * "Absorbing a volume", in two passes: a new object is SEEDED from what the background already holds of it, and the
 * background RELEASES what the object then holds as foreground.  Everything "Absorbing a volume" lays down holds here
 * word for word: dense (z, y, x) volumes, x fastest, res = (nx, ny, nz); R[9], t[3] (f32, row-major) = the SOURCE's (the
 * claimant's) volume frame <- the DESTINATION's volume frame; per destination voxel v of the box [box_lo, box_lo +
 * box_size) the sample-point arithmetic p_d, p_s, q, l, f; the pad-1 OUTSIDE rule; the blend in x pairs, then y, then z;
 * every float step a single float32 operation without contraction, everything else integer; the classes in the order
 * given, the first match wins; of tsdf[v] and weights[v] only the words whose bits change are stored.  pw, pt: the
 * destination's weight and tsdf at v.  Colour is not touched by either pass; emf_hip_seedVolumeColor and
 * emf_hip_releaseVolumeColor (below) carry it.
 *
 * emf_hip_seedVolume: THE DESTINATION TAKES THE SOURCE'S BAND ONLY WHERE IT HAS NO OBSERVATION OF ITS OWN.
 *     KEPT       pw > 0.  Decided before anything of the source is read; the voxel is not written.  (A new object has
 *                integrated the frame that the source integrated too: a running average there would count one
 *                measurement twice.)
 *     OUTSIDE, UNKNOWN, MASKED    exactly as in "Absorbing a volume" (source->fgVolMask, source->unseenTiles included:
 *                the bytes are the same with the unseen-tile map and without it)
 *     SATURATED  !(fabsf(s) < 1) or !(fabsf(u) < 1) with u = s * ratio, ratio = truncdist_s / truncdist_d (one float32
 *                division, made once on the host): only values inside the destination's own band are carried, which is
 *                what its own integration would have produced.  No clamped +-1 is ever written.
 *     SEEDED     nt = u, nw = min(w_o, maxWeight), w_o the minimum of the eight corner weights
 *                SOLID: SEEDED and !(nt > 0).
 * emf_seed_t: visited = kept + outside + unknown + masked + saturated + seeded (the voxels of the box); solid <= seeded;
 * lo, hi: the inclusive bounds of the SEEDED voxels in the destination, res_d and -1 without one.
 *
 * emf_hip_releaseVolume: THE DESTINATION GIVES UP THE BAND VOXELS THAT THE CLAIMANT HOLDS.  claim_mask: a u8 volume of
 * claim_res on the claimant's lattice (an object's fgVolMask), or NULL: everything inside the claimant's cube.
 *     EMPTY      !(pw > 0)
 *     FREE       !(fabsf(pt) < 1): free space and NaN stay; it releases the band, not the free space around it
 *     OUTSIDE    the pad-1 rule on q against claim_res
 *     UNCLAIMED  claim_mask is not NULL and is 0 at (rint(q_0), rint(q_1), rint(q_2)), ties to even: the addressing of
 *                MASKED
 *     RELEASED   tsdf[v] and weights[v] become the bits of +0.0f, what an unseen voxel holds after a reset
 *                SOLID: RELEASED and !(pt > 0) of the old value.
 * emf_release_t: visited = empty + free_space + outside + unclaimed + released; solid <= released; lo, hi: the inclusive
 * bounds of the RELEASED voxels.  EMPTY and FREE come first: most voxels of a covering box cost 8 bytes and no transform.
 *
 * In both, every destination voxel reads and writes only itself: the passes are in place, and the bytes are a pure
 * function of the inputs whatever order lanes and workgroups run in.  A second seed finds its seeded voxels KEPT, a second
 * release finds its released voxels EMPTY.
 * ---------------------------------------------------------------------------------------------- */
typedef struct emf_seed {
    uint64_t visited, kept, outside, unknown, masked, saturated, seeded, solid; /* counts */
    int32_t lo[3], hi[3];       /* bounds of the seeded voxels; res_d and -1 without one */
} emf_seed_t;                   /* 88 bytes */

typedef struct emf_release {
    uint64_t visited, empty, free_space, outside, unclaimed, released, solid;   /* counts */
    int32_t lo[3], hi[3];       /* bounds of the released voxels; res_d and -1 without one */
} emf_release_t;                /* 80 bytes */

/* The arguments, the record, the launch shape (one workgroup of 256 lanes per 32 x 8 x 8 destination tile that meets the
 * box, after a launch that sets the neutral record), the empty box (EMF_OK, the neutral record, nothing else written)
 * and the refusals are those of emf_hip_absorbVolume.  Refused with EMF_E_ARG or EMF_E_LIMIT and nothing enqueued: a NULL
 * or misaligned pointer; a destination array that shares a byte with the other, with an array of the source or with the
 * record; an axis below 1 or above EMF_DF_MAX_AXIS or more than 2^31 - 1 voxels, of either volume; a voxel size, a
 * truncation distance, maxWeight or the ratio of the truncation distances that is not finite and > 0; a negative box
 * size or a box that leaves the destination.  Nothing allocates, copies to the host or waits. */
int emf_hip_seedVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                       float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                       const int32_t box_lo[3], const int32_t box_size[3], emf_seed_t* record_dev, emf_stream_t stream);

/* claim_mask may be NULL, claim_res may not.  The refusals are those above with the claimant's mask in the source's
 * place; there is no truncation distance and no maxWeight to refuse. */
int emf_hip_releaseVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size,
                          const uint8_t* claim_mask, const int32_t claim_res[3], float claim_voxel_size, const float R[9],
                          const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_release_t* record_dev,
                          emf_stream_t stream);

/* Colour with the band: the two passes as emf_hip_absorbVolumeColor states them -- the same walk, for
 * the same inputs byte for byte the same tsdf, weights and geometry record as the plain entry, the colour entry, the
 * SOURCE ENTRY S = (Sc[3], Sw) at the nearest voxel, capq and emf_color_moved_t of "Absorbing a volume", integer and
 * exact.  Only the entry of a SEEDED (RELEASED) voxel is written; every other voxel's is neither read nor written.
 *   SEED      a SEEDED voxel's entry becomes (Sc, min(Sw, capq)) if Sw > 0 (COLOURED), else (0, 0, 0, 0) (UNCOLOURED);
 *             colored + uncolored == seeded.  A second seed finds the voxel KEPT and changes no colour byte.
 *   RELEASE   a RELEASED voxel's entry becomes (0, 0, 0, 0), what TSDF::reset leaves.  COLOURED counts the entries that
 *             held a non-zero value, UNCOLOURED those already zero; colored + uncolored == released.
 * The arguments of the plain entries plus dst_color, src_color (the seed; may be NULL: every source entry is
 * (0, 0, 0, 0)) and color_record_dev; the additional refusals are those of emf_hip_absorbVolumeColor. */
int emf_hip_seedVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                            float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const uint16_t* src_color,
                            const float R[9], const float t[3], const int32_t box_lo[3], const int32_t box_size[3],
                            emf_seed_t* record_dev, emf_color_moved_t* color_record_dev, emf_stream_t stream);
int emf_hip_releaseVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                               const uint8_t* claim_mask, const int32_t claim_res[3], float claim_voxel_size, const float R[9],
                               const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_release_t* record_dev,
                               emf_color_moved_t* color_record_dev, emf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Merging a volume (new behaviour: DESIGN.md 5.32).  Opt-in; nothing above is touched.  An absorption whose DESTINATION
 * IS AN OBJECT: a signed-distance volume plus the per-voxel (fg, bg) counts its foreground mask is derived from.
 * Everything "Absorbing a volume" lays down holds here word for word: dense (z, y, x) volumes, x fastest, res = (nx, ny,
 * nz); R[9], t[3] (f32, row-major) = the SOURCE's volume frame <- the DESTINATION's volume frame; per destination voxel
 * v of the box the sample-point arithmetic p_d, p_s, q, l, f; the pad-1 OUTSIDE rule; the blend in x pairs, then y, then
 * z; every float step a single float32 operation without contraction, everything else integer; the classes OUTSIDE,
 * UNKNOWN, MASKED, SATURATED, FUSED in that order, the first match wins; only the words whose bits change are stored.
 * The tsdf and the weights of a FUSED voxel are the absorption's (u, w_o, FRESH, the running average, the cap at
 * maxWeight): for the same inputs the tsdf, the weights and the whole emf_absorb_t of emf_hip_mergeVolume equal
 * emf_hip_absorbVolume's byte for byte.
 * source->fgVolMask IS REQUIRED: a source voxel the source itself calls background is no evidence about the destination.
 * COUNTS.  dst_fgbg, src_fgbg: res_d (res_s) pairs of f32, interleaved (fg, bg), in the voxel order of the tsdf -- the
 * layout of emf_hip_updateFgBgProbs -- a pair read and written as one 8-byte word.  Only the pair of a FUSED voxel is
 * read or written.  With (sf, sb) the source's pair at (rint(q_0), rint(q_1), rint(q_2)), ties to even (the addressing of
 * MASKED), and (df, db) the destination's own at v, read once before either is written:
 *     FRESH (!(pw > 0)):  (nf, nb) = (sf, sb)            an unobserved voxel's counts are not evidence
 *     else:               (nf, nb) = (df + sf, db + sb)  one float32 sum each
 * and the pair is stored only where its bits change.
 * emf_merge_counts_t: a second device record, neutral at (0, 0) and set by the call's own init launch.  foreground: the
 * FUSED voxels with nf > nb; gained: those of them that were FRESH or had !(df > db).  gained <= foreground <= fused.
 * ---------------------------------------------------------------------------------------------- */
typedef struct emf_merge_counts {
    uint64_t foreground, gained;
} emf_merge_counts_t;           /* 16 bytes */

/* The arguments of emf_hip_absorbVolume plus dst_fgbg (written in place), src_fgbg (only read) and counts_dev (device,
 * 8-byte aligned).  The record, the launch shape and the empty box (EMF_OK, both neutral records, nothing else written)
 * are those of emf_hip_absorbVolume.  Refused with nothing enqueued, on top of everything emf_hip_absorbVolume refuses and
 * with its codes: source->fgVolMask, dst_fgbg, src_fgbg or counts_dev NULL; a count volume or the count record not
 * 8-byte aligned; an array the call writes (the destination's three, the two records) sharing a byte with any other
 * array of the call. */
int emf_hip_mergeVolume(float* dst_tsdf, float* dst_weights, float* dst_fgbg, const int32_t dst_res[3], float dst_voxel_size,
                        float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const float* src_fgbg, const float R[9],
                        const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_absorb_t* record_dev,
                        emf_merge_counts_t* counts_dev, emf_stream_t stream);

/* Colour with the band: the colour entry of every FUSED voxel exactly as emf_hip_absorbVolumeColor carries it (SOURCE
 * ENTRY, capq, UNCOLOURED / COLOURED, emf_color_moved_t), on top of the above; for the same inputs tsdf, weights, counts
 * and both other records equal the plain entry's.  dst_color, src_color (or NULL) and color_record_dev as there, with
 * its additional refusals; an empty box: EMF_OK and the three neutral records. */
int emf_hip_mergeVolumeColor(float* dst_tsdf, float* dst_weights, float* dst_fgbg, uint16_t* dst_color, const int32_t dst_res[3],
                             float dst_voxel_size, float dst_truncdist, float max_weight, const emf_absorb_source_t* source,
                             const float* src_fgbg, const uint16_t* src_color, const float R[9], const float t[3], const int32_t box_lo[3],
                             const int32_t box_size[3], emf_absorb_t* record_dev, emf_merge_counts_t* counts_dev,
                             emf_color_moved_t* color_record_dev, emf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EMF_HIP_H */
