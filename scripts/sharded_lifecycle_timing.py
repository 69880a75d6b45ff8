"""Cost of the object life cycle with clean-up on, unsharded and on the sharded path:
  - clean-up masses on the device (HIP events): the level-1 entry once per object (2 launches each, what cleanUpObjs
    did before the batched entry) against emf_hip_maskAssociationMassBatched over the same objects, at 5 and 65 models;
  - a dynamic synthetic sequence (spawning from instance masks every 3rd frame, matching, clean-up every frame) run
    unsharded and on ONE rank with the sharded path forced (EMF_FORCE_SHARDED=1, a 1-rank rehearsal communicator):
    host wall ms per frame and the exchanges each frame issues (Communicator.exchanges()).
Under `rocprofv3 --kernel-trace --stats -- python scripts/sharded_lifecycle_timing.py` the kernel statistics give the
k_mask_mass / k_mask_mass_finish launches and their durations.
python scripts/sharded_lifecycle_timing.py [frames]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")

from emfusion_amd import ops, pipeline  # noqa: E402
from emfusion_amd.devmem import DeviceArray, Event, synchronize  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
W, H = 640, 480


def timed(fn, reps=20):
    fn()
    synchronize()
    a, b = Event(), Event()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) * 1e3 / reps


def masses(n):
    rng = np.random.default_rng(n)
    hm = [DeviceArray.from_numpy((rng.uniform(size=(H, W)) < 0.1).astype(np.uint8)) for _ in range(n)]
    ad = [DeviceArray.from_numpy(rng.uniform(0, 1, (H, W)).astype(np.float32)) for _ in range(n)]
    md = [None if k % 2 else DeviceArray.from_numpy((rng.uniform(size=(H, W)) < 0.05).astype(np.uint8))
          for k in range(n)]
    # device time only: the wrappers' read-backs are outside the timed launches
    import ctypes as C
    from emfusion_amd import _lib
    L = _lib.load()
    out1 = DeviceArray.zeros((int(L.emf_hip_maskAssociationMassBytes()) // 8,), np.float64)
    views = [(ops.image_view(h), None if m is None else ops.image_view(m), ops.image_view(a)) for h, a, m in zip(hm, ad, md)]

    def level1():
        for s, m, a in views:
            L.emf_hip_maskAssociationMass(C.byref(s), None if m is None else C.byref(m), C.byref(a),
                                          C.c_void_p(out1.ptr), None)
    models = [_lib.EmfModel()]
    for h, a in zip(hm, ad):
        mo = _lib.EmfModel()
        mo.hitMask, mo.assoc = h.ptr, a.ptr
        models.append(mo)
    table = ops.upload_models(models)
    imgs = (_lib.EmfImage * n)()
    for k, m in enumerate(md):
        if m is not None:
            imgs[k] = ops.image_view(m)
    scratch = DeviceArray.zeros((int(L.emf_hip_maskAssociationMassScratchBytes(n)) // 8,), np.float64)
    out = DeviceArray.zeros((n, 2), np.float64)
    verdict = DeviceArray.zeros(((n + 3) // 4 * 4,), np.float32)
    vis = DeviceArray.from_numpy(np.ones(n + 1, np.int32))
    pos = (C.c_int32 * n)(*range(n))

    def batched():
        L.emf_hip_maskAssociationMassBatched(C.c_void_p(table.ptr), 1, n, W, H, imgs, C.c_void_p(scratch.ptr),
                                             C.c_void_p(out.ptr), C.c_void_p(verdict.ptr), n, pos, C.c_void_p(vis.ptr),
                                             None, 0.2, None)
    t1, tb = timed(level1), timed(batched)
    print(f"clean-up masses, {n} objects at {W}x{H}: level-1 loop {2 * n} launches {t1:.1f} us; "
          f"batched {(n + 31) // 32 + 1} launches {tb:.1f} us", flush=True)


def sequence(sharded):
    os.environ["EMF_FORCE_SHARDED"] = "1" if sharded else "0"
    prm = pipeline.make_params(W, H, 256, 0.02, 64, mask_frames=3)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 4, seed=0xE3F5)
    comm = pipeline.Communicator.local_group(1)[0] if sharded else None
    fus = pipeline.Fusion(prm, comm)
    fus.set_cleanup(True)
    inputs = []
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        inst = [DeviceArray.from_numpy((sid == k).astype(np.uint8)) for k in range(1, 5)] if f % 3 == 0 else None
        inputs.append((DeviceArray.from_numpy(depth), R, t, inst))
    synchronize()
    walls, xs, created, deleted = [], [], [], []
    for d, R, t, inst in inputs:
        if inst is not None:
            fus.queue_instance_masks([ops.image_view(m) for m in inst])
        x0 = comm.exchanges() if comm else 0
        t0 = time.perf_counter()
        fus.process_frame(ops.image_view(d), R, t, {}, {}, False)
        fus.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        xs.append(comm.exchanges() - x0 if comm else 0)
        created += [i for i in fus.last_created() if i > 0]
        deleted += fus.last_deleted()
    ids = fus.object_ids()
    fus.close()
    synth.close()
    if comm:
        comm.close()
    os.environ.pop("EMF_FORCE_SHARDED", None)
    mask_frames = [k for k in range(frames) if k % 3 == 0]
    other = [k for k in range(1, frames) if k % 3]
    print(f"{'sharded (1 rank, forced)' if sharded else 'unsharded':26s}: {np.median(walls[1:]):.2f} ms/frame median "
          f"(mask frames {np.median([walls[k] for k in mask_frames[1:]]):.2f}, others "
          f"{np.median([walls[k] for k in other]):.2f}); exchanges per frame {xs}; created {created}, deleted {deleted}, "
          f"live {ids}", flush=True)


for n in (5, 65):
    masses(n)
for sh in (False, True):
    sequence(sh)
