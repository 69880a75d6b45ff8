// Switches.hpp -- the one declaration of the run-time switches: every environment variable the host classes read.
//
// EMF_SWITCH_TABLE below is the table; the struct emf::Switches, the introspection (emf_fusion_describe_switches) and
// the parsing are all generated from it, so a variable that is not a row here is not read (nothing else under core/
// calls getenv).  One row:
//
//   X(field, C type, "NAME", kind, rule, default, selects a path, "one line of documentation")
//
// kind  Product: read by every build.  Demoted: an A/B switch whose measurement is on record as lost (DESIGN.md
//       section 6): read only by builds with -DEMF_DEBUG_SWITCHES (libemf_fusion_dbg.so, `make dbg`); the product build
//       keeps the default and says so on stderr, once per variable and process, when the variable is set.
// rule  how the variable's text becomes the value -- SwitchRule.  The rules are the ones the call sites applied before
//       they had one home and are kept as they were, oddities included: "no" does not switch an OffOnZero switch
//       off, "yes" does not switch an OnOnOne switch on.
// path  the switch selects between execution paths of the one-rank frame on a device depth map, which must produce the
//       same bytes: tests/test_switches_cpu.py holds the product rows marked so against the list that
//       tests/test_gpu_switch_pairs.py sets two at a time.  (Not marked: switches of the sharded path, the host upload
//       and the tracking driver's host loops, which have tests of their own, and sizes / priorities / logs.)
//
// When they are read: emf::EMFusion reads the whole table once per construction (Switches::fromEnvironment(), in front
// of its first member that needs a value) and keeps it as `sw`; a variable set later does not reach a live instance.
// TSDF (voxelRcp at volume creation, unseenTiles and brickFlags at describe()), the peer communicator (at its creation)
// and the device-buffer pool (poolMiB, once per process at first use) read their rows through switchValue().
#pragma once

#include <cstddef>
#include <string>

namespace emf {

enum class SwitchKind { Product, Demoted };

enum class SwitchRule {
    OffOnZero,  // on/off: off iff the text starts with '0'; unset, "" and any other text leave it on
    OnOnOne,    // on/off: on iff the text starts with '1'; unset, "" and any other text leave it off
    Present,    // on/off: on iff the variable is set, to anything (also to "")
    Int,        // small integer: atoi of the text ("abc" and "" give 0); unset gives the default
    IntMin1,    // small integer: max(1, atoi)
    Lanes,      // enumerated: atoi must give 1, 2 or 4 -- any other text, "" included, is refused with EMF_E_ARG
    Flags012,   // enumerated: text starting with '2' gives 2, with '1' gives 1, anything else 0
    Priority,   // enumerated: h / + / 1 give +1 (high), l / - give -1 (low), unset and "" the default, any other text 0
    MiB,        // size: strtoull, base 10
};

// clang-format off
#define EMF_SWITCH_TABLE(X) \
    X(perVolume,      bool,   "EMF_PER_VOLUME",         Product, OnOnOne,   0,     true,  "1: the per-volume path (one stream and launch per volume, host visibility gate) instead of the batched one") \
    X(bgBands,        bool,   "EMF_BG_BANDS",           Product, OffOnZero, 1,     false, "0: sharded path, every rank raycasts the whole replicated background instead of a row band") \
    X(cullBoxes,      bool,   "EMF_INT_CULL",           Product, OffOnZero, 1,     true,  "0: one-level integration launch, every tile gets a workgroup and culls itself") \
    X(bgOverlap,      bool,   "EMF_BG_OVERLAP",         Product, OffOnZero, 1,     true,  "0: the background is integrated in place after the raycast, as the reference does, not beside it") \
    X(useFarBounds,   bool,   "EMF_FAR_BOUNDS",         Product, OffOnZero, 1,     true,  "0: no far bounds, every ray is marched to the end of its range") \
    X(marchLanes,     int,    "EMF_MARCH_ROWS",         Product, Lanes,     1,     true,  "lanes per background ray: 1, 2 or 4; read once, by the constructor, anything else is refused") \
    X(asyncUpload,    bool,   "EMF_ASYNC_UPLOAD",       Product, OffOnZero, 1,     false, "0: processFrame(RGBD) copies from the caller's pageable memory on the frame's stream, no pinned staging") \
    X(useLambdaTable, bool,   "EMF_LAMBDA_TABLE",       Product, OffOnZero, 1,     true,  "0: the integration computes 1 / lambda inline instead of reading the per-pixel table") \
    X(forceSharded,   bool,   "EMF_FORCE_SHARDED",      Product, OnOnOne,   0,     false, "1: a one-rank communicator uses the sharded path's exchanges too") \
    X(voxelRcp,       bool,   "EMF_VOXEL_RCP",          Product, OffOnZero, 1,     true,  "0: the march divides by the voxel size instead of multiplying by its checked reciprocal") \
    X(unseenTiles,    bool,   "EMF_UNSEEN_TILES",       Product, OffOnZero, 1,     true,  "0: the integration does not use the unseen-tile maps") \
    X(poolMiB,        size_t, "EMF_POOL_MIB",           Product, MiB,       16384, false, "cap of the pool of released device buffers in MiB; once per process, at first use") \
    X(peerTimeoutMs,  int,    "EMF_PEER_TIMEOUT_MS",    Product, IntMin1,   5000,  false, "bound of a peer exchange's wait in milliseconds; read when the communicator is created") \
    X(objCull,        bool,   "EMF_OBJ_CULL",           Demoted, OnOnOne,   0,     true,  "1: the two-level integration launch for chunks of objects alone too") \
    X(trackChunk,     int,    "EMF_TRACK_CHUNK",        Demoted, Int,       8,     false, "LM iterations enqueued between two polls of the convergence flags (0: never poll)") \
    X(trackWindow,    int,    "EMF_TRACK_WINDOW",       Demoted, Int,       4,     false, "tracking launches kept ahead of the device's progress report (0: poll in chunks)") \
    X(fusePoints,     bool,   "EMF_FUSE_POINTS",        Demoted, OffOnZero, 1,     true,  "0: the points get a launch of their own instead of being made by the frame's first E-step") \
    X(fuseVisibility, bool,   "EMF_FUSE_VISIBILITY",    Demoted, OffOnZero, 1,     true,  "0: the visibility counts get a launch of their own behind the composite") \
    X(earlyFarBounds, bool,   "EMF_EARLY_FAR_BOUNDS",   Demoted, OffOnZero, 1,     true,  "0: the far bounds wait for the main stream, not for the previous raycast only") \
    X(useFootprints,  bool,   "EMF_RAY_FOOTPRINTS",     Demoted, OffOnZero, 1,     true,  "0: every object gets a marching workgroup for every tile of the image") \
    X(peerFused,      bool,   "EMF_PEER_FUSED",         Demoted, OffOnZero, 1,     false, "0: sharded path over a peer transport keeps the transport's own two-launch collectives") \
    X(farScan,        bool,   "EMF_FAR_SCAN",           Demoted, OnOnOne,   0,     true,  "1: volumes too small for a relevant-tile list have their sign maps scanned for far bounds") \
    X(brickFlags,     int,    "EMF_BRICK_FLAGS",        Demoted, Flags012,  0,     true,  "brick uniformity flags: 0 not kept, 1 the raycast skips deep-uniform bricks, 2 uniform look-ups answered from them") \
    X(peerWaitInFront,bool,   "EMF_PEER_WAIT_IN_FRONT", Demoted, OffOnZero, 1,     false, "0: an exchange's consumers poll themselves (never when ranks share a device); read at communicator creation") \
    X(trackLog,       bool,   "EMF_TRACK_LOG",          Demoted, Present,   0,     false, "set: the tracking driver logs launches and verdicts on stderr") \
    X(prioMain,       int,    "EMF_PRIO_MAIN",          Demoted, Priority,  1,     false, "queue priority class of the frame's main stream") \
    X(prioCopy,       int,    "EMF_PRIO_COPY",          Demoted, Priority,  1,     false, "queue priority class of the depth upload's copy stream") \
    X(prioAux,        int,    "EMF_PRIO_AUX",           Demoted, Priority,  -1,    false, "queue priority class of the background integration's stream") \
    X(prioLists,      int,    "EMF_PRIO_LISTS",         Demoted, Priority,  -1,    false, "queue priority class of the far bounds' and list rebuilds' stream")
// clang-format on

/** One id per row, in table order. */
enum class Switch {
#define X(field, type, name, kind, rule, dflt, path, doc) field,
    EMF_SWITCH_TABLE(X)
#undef X
};

/**
 * The value of one row as parsed from the environment NOW (a demoted row in a product build: its default, and the
 * line on stderr if the variable is set).  Throws HipError(EMF_E_ARG) where the rule refuses the text.
 */
long long switchValue(Switch id);

/** Every row's value, typed. */
struct Switches {
#define X(field, type, name, kind, rule, dflt, path, doc) type field;
    EMF_SWITCH_TABLE(X)
#undef X
    static Switches fromEnvironment();
};

/** The table as JSON, values as fromEnvironment() gives them: what emf_fusion_describe_switches returns. */
std::string describeSwitches();

}  // namespace emf
