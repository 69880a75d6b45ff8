"""The object life cycle on the sharded path (EMFusion.cpp:95-108, 329-372, 495-557, 827-863, 922-980 with the
objects spread over ranks): creation, matching, carving, resizing and clean-up decided identically on every rank,
with the owner-only facts (volume IoU, existence probability, association mass) joined by fixed exchanges.

Ranks are threads on one GPU joined by the rehearsal communicators (tests/test_gpu_rehearsal.py): a rank that
issued a different sequence of collectives would time out instead of finishing.  The batched clean-up kernel
(emf_hip_maskAssociationMassBatched) is checked against the level-1 entry first."""
import threading

import numpy as np
import pytest

from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

JOIN_S = 240
EYE = np.eye(3, dtype=np.float32).reshape(-1)


# ---- 1. batched masses and verdicts against the level-1 entry ---------------------------------------------------

def host_rule(thr, count, total, visible, ex_low):
    """cleanUpObjs' delete decision: double(float(thr) * float(count)) > sum, or invisible, or low existence."""
    need = np.float32(thr) * np.float32(count)
    return bool(ex_low) or not visible or float(need) > float(total)


@pytest.mark.parametrize("n", [0, 1, 5, 40])
def test_batched_masses_and_verdicts_equal_level1(dev, n):
    from emfusion_amd import ops
    W, H = 160, 120
    rng = np.random.default_rng(100 + n)
    segs, assocs, matches, hm, ad, md = [], [], [], [], [], []
    for k in range(n):
        seg = (rng.uniform(size=(H, W)) < rng.uniform(0.05, 0.4)).astype(np.uint8)
        a = rng.uniform(0, 1, (H, W)).astype(np.float32)
        m = None if k % 3 == 1 else (rng.uniform(size=(H, W)) < 0.1).astype(np.uint8) * 255
        if k == 2:  # the exact tie: float(thr * count) == sum -> NOT spurious
            a[:] = 0.5
        segs.append(seg)
        assocs.append(a)
        matches.append(m)
        hm.append(to_dev(seg))
        ad.append(to_dev(a))
        md.append(None if m is None else to_dev(m))
    nall = n + 3
    pos = rng.permutation(nall)[:n].tolist()
    visible = [int(k % 4 != 3) for k in range(n)]
    ex_low = [int(k % 5 == 4) for k in range(n)]
    thr = 0.5  # (object 2's weights are all 0.5: thr * count == sum exactly)
    counts, sums, verdicts = ops.mask_association_masses(
        hm, ad, md, verdict=dict(nall=nall, list_pos=pos, visible=visible, ex_low=ex_low, assoc_thresh=thr))
    assert verdicts.shape == ((nall + 3) // 4 * 4,)
    want_v = np.zeros_like(verdicts)
    for k in range(n):
        c1, s1 = ops.mask_association_mass(hm[k], md[k], ad[k])
        inside = (segs[k] != 0) if matches[k] is None else ((segs[k] != 0) | (matches[k] != 0))
        assert c1 == int(inside.sum())
        # byte-identical to the level-1 entry (same row bands, lane order and block order)
        assert int(counts[k]) == c1, k
        assert np.float64(sums[k]).tobytes() == np.float64(s1).tobytes(), (k, sums[k], s1)
        want_v[pos[k]] = 1.0 if host_rule(thr, c1, s1, visible[k], ex_low[k]) else 0.0
    assert np.array_equal(verdicts, want_v), (verdicts, want_v)
    if n >= 3:
        assert float(np.float32(thr) * np.float32(counts[2])) == float(sums[2])  # the tie really is one
        assert verdicts[pos[2]] == (0.0 if visible[2] and not ex_low[2] else 1.0)
        assert 0 < verdicts.sum() < n  # both answers occur
    # the same masses without verdicts
    c2, s2, v2 = ops.mask_association_masses(hm, ad, md)
    assert v2 is None and np.array_equal(c2, counts) and np.array_equal(s2, sums)


# ---- the thread-rank harness -------------------------------------------------------------------------------

def run_ranks(world, body, transport="host"):
    """body(rank, fusion, comm) on `world` thread-ranks (world 1: unsharded, no communicator); returns the results."""
    from emfusion_amd import pipeline
    comms = pipeline.Communicator.local_group(world, transport, max_bytes=1 << 22) if world > 1 else [None]
    out, errors = [None] * world, []
    ready = threading.Barrier(world)

    def main(r):
        try:
            out[r] = body(r, comms[r], ready)
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((r, repr(e)))
            ready.abort()

    threads = [threading.Thread(target=main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=JOIN_S)
    assert not any(th.is_alive() for th in threads), "a rank hangs"
    assert not errors, errors
    for c in comms:
        if c is not None:
            c.close()
    return out


def close(a, b, what):  # the sharded normaliser sums in another order: ulps, and a handful of flipped pixels
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = np.isclose(a, b, rtol=1e-4, atol=1e-6)
    assert ok.mean() > 0.995, (what, ok.mean())


# ---- 2. a dynamic scene ---------------------------------------------------------------------------------------

WD, HD, NFRAMES = 320, 240, 14


def dynamic_inputs():
    from scipy.ndimage import binary_dilation

    from emfusion_amd import pipeline
    prm = pipeline.make_params(WD, HD, 128, 0.04, 32, visibility_thresh=400, boundary=10, mask_frames=2)
    synth = pipeline.SyntheticStream(WD, HD, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    disc = np.hypot(*np.mgrid[-9:10, -9:10]) <= 9.0
    frames = []
    for f in range(NFRAMES):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        s1, s2 = (sid == 1).astype(np.uint8), (sid == 2).astype(np.uint8)
        inst = None
        if f == 0:  # both spheres and a spurious blob on the wall
            blob = np.zeros_like(s1)
            blob[12:60, 12:90] = 1
            blob &= (sid == 0) & (depth > 0)
            inst = [s1, s2, blob]
        elif f == 2:  # sphere 1 twice: an eroded duplicate goes the unmatched way and is carved (Q20 path)
            dup = s1.copy()
            dup[:, : WD // 2 - 10] = 0
            inst = [s1, s2, dup]
        elif f == 4:  # sphere 1 reported too generously: its volume grows (updateObj -> resize)
            inst = [(binary_dilation(s1, disc) & (sid != 2)).astype(np.uint8), s2]
        elif f % 2 == 0 or f >= 5:  # the blob is never reported again: its existence probability 1 / (1 + misses)
            inst = [s1]             # drops below existenceThresh (0.1) at the 10th miss, frame 12
        frames.append((depth, R, t, inst))
    synth.close()
    return prm, frames


def run_dynamic(world, transport="host"):
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm, frames = dynamic_inputs()
    far = np.array([0, 0, -30], np.float32)

    def body(r, comm, ready):
        fus = pipeline.Fusion(prm, comm)
        fus.set_cleanup(True)
        keep, log = [], []
        ready.wait(timeout=JOIN_S)
        for f, (depth, R, t, inst) in enumerate(frames):
            d = to_dev(depth)
            keep.append(d)
            if inst is not None:
                dm = [to_dev(m) for m in inst]
                keep.append(dm)
                fus.queue_instance_masks([image_view(m) for m in dm])
            poses = {2: (EYE, far)} if f >= 6 else {}  # object 2 leaves the view: deleted as invisible
            fus.process_frame(image_view(d), R, t, poses, {}, False)
            fus.synchronize()
            log.append(dict(assigned=fus.last_mask_assignment(), created=fus.last_created(),
                            deleted=fus.last_deleted(), ids=fus.object_ids(), vis=sorted(fus.visible_objects())))
        mine = [i for i in fus.object_ids() if fus.owns_object(i)]
        res = dict(log=log, mine=mine, seg=fus.image("segmentation"), bg_tsdf=fus.volume("tsdf", 0),
                   bg_w=fus.volume("weights", 0), bg_ray=fus.image("bg_raylengths"),
                   obj={i: (fus.volume("tsdf", i), fus.volume("weights", i), fus.pose(i)) for i in mine})
        fus.close()
        return res

    return run_ranks(world, body, transport)


@pytest.fixture(scope="module")
def dynamic_single(dev):
    return run_dynamic(1)[0]


def test_dynamic_scene_single_gpu_covers_the_life_cycle(dynamic_single):
    log = dynamic_single["log"]
    assert log[0]["created"][:2] == [1, 2]
    assert log[2]["assigned"][:2] == [1, 2] and log[2]["assigned"][2] == -1  # the duplicate is not matched
    deleted = [i for fr in log for i in fr["deleted"]]
    assert 2 in deleted  # moved out of view
    assert log[0]["created"][2] == 3 and log[12]["deleted"] == [3]  # the blob: created, then dropped as spurious
    assert 1 in log[-1]["ids"]
    assert dynamic_single["obj"][1][0].shape[0] > 32  # grown by the generous mask


@pytest.mark.parametrize("world,transport", [(2, "host"), (3, "host"), (2, "peer")])
def test_dynamic_scene_on_thread_ranks_equals_single_gpu(dynamic_single, world, transport):
    single = dynamic_single
    ranks = run_dynamic(world, transport)
    for f in range(NFRAMES):
        want = single["log"][f]
        for r, res in enumerate(ranks):
            got = res["log"][f]
            for k in ("assigned", "created", "deleted", "ids", "vis"):
                assert got[k] == want[k], (f, r, k, got[k], want[k])
    assert sorted(i for r in ranks for i in r["mine"]) == single["mine"]
    r0 = ranks[0]
    for r in ranks:
        for k in ("seg", "bg_tsdf", "bg_w", "bg_ray"):
            assert np.array_equal(r[k], r0[k]), k  # the replicas do not drift apart
        assert (r["seg"] == single["seg"]).mean() > 0.995
        close(r["bg_tsdf"], single["bg_tsdf"], "bg tsdf")
        for i in r["mine"]:
            t, w, (Ro, to) = r["obj"][i]
            ts, ws, (Rs, tss) = single["obj"][i]
            close(t, ts, f"tsdf of object {i}")
            assert ((w > 0) == (ws > 0)).mean() > 0.999
            assert np.allclose(to, tss, atol=2e-3) and np.allclose(Ro, Rs, atol=2e-3), i


# ---- 3 / 4. calls between frames --------------------------------------------------------------------------------

def two_sphere_frames():
    from emfusion_amd import pipeline
    prm = pipeline.make_params(WD, HD, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(WD, HD, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    frames = [synth.render(f) + synth.camera_pose(f) for f in range(2)]
    synth.close()
    return prm, frames


def test_remote_overlap_blocks_a_new_object(dev):
    """Object 1 lives on rank 0; rank 1 cannot see its geometry, yet both refuse a mask that overlaps it."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm, frames = two_sphere_frames()
    depth, sid, R, t = frames[0]

    def body(r, comm, ready):
        fus = pipeline.Fusion(prm, comm)
        ready.wait(timeout=JOIN_S)
        d, m1, m2 = to_dev(depth), to_dev((sid == 1).astype(np.uint8)), to_dev((sid == 2).astype(np.uint8))
        fus.queue_new_object_masks([image_view(m1)])
        fus.process_frame(image_view(d), R, t, {}, {}, False)
        fus.synchronize()
        x0 = comm.exchanges() if comm else 0
        again = fus.create_object_from_mask(image_view(to_dev((sid == 1).astype(np.uint8))))
        other = fus.create_object_from_mask(image_view(m2))
        res = dict(created=fus.last_created(), again=again, other=other, owns1=fus.owns_object(1),
                   x=(comm.exchanges() - x0) if comm else 0, ids=fus.object_ids())
        fus.close()
        return res

    single = run_ranks(1, body)[0]
    ranks = run_ranks(2, body)
    assert single["created"] == [1] and single["again"] == -1 and single["other"] == 2
    assert ranks[0]["owns1"] and not ranks[1]["owns1"]
    for r in ranks:
        assert r["created"] == [1] and r["again"] == -1 and r["other"] == 2 and r["ids"] == [1, 2], r
        assert r["x"] == 2  # one 16-byte all-reduce per IoU test


def test_update_object_on_every_rank(dev):
    from scipy.ndimage import binary_dilation

    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm, frames = two_sphere_frames()
    disc = np.hypot(*np.mgrid[-9:10, -9:10]) <= 9.0

    def body(r, comm, ready):
        fus = pipeline.Fusion(prm, comm)
        ready.wait(timeout=JOIN_S)
        keep = []
        for f, (depth, sid, R, t) in enumerate(frames):
            d = to_dev(depth)
            keep.append(d)
            if f == 0:
                new = [to_dev((sid == k).astype(np.uint8)) for k in (1, 2)]
                keep.append(new)
                fus.queue_new_object_masks([image_view(m) for m in new])
            fus.process_frame(image_view(d), R, t, {}, {}, False)
        fus.synchronize()
        depth, sid = frames[-1][:2]
        big = to_dev((binary_dilation(sid == 1, disc) & (sid != 2)).astype(np.uint8))
        mine = [i for i in fus.object_ids() if fus.owns_object(i)]
        before = {i: fus.volume("tsdf", i) for i in mine}
        off = fus.update_object(1, image_view(big))
        fus.synchronize()
        res = dict(off=np.asarray(off, np.float32), mine=mine, before=before,
                   after={i: fus.volume("tsdf", i) for i in mine}, pose={i: fus.pose(i) for i in mine})
        fus.close()
        return res

    single = run_ranks(1, body)[0]
    ranks = run_ranks(2, body)
    assert np.any(single["off"] != 0) or single["after"][1].shape != single["before"][1].shape  # a resize happened
    for r in ranks:
        assert np.allclose(r["off"], single["off"], atol=1e-6), (r["off"], single["off"])
        assert np.array_equal(r["off"], ranks[0]["off"])  # every rank returns the owner's bits
        for i in r["mine"]:
            if i == 1:
                close(r["after"][1], single["after"][1], "resized volume")
                assert np.allclose(r["pose"][1][1], single["pose"][1][1], atol=1e-5)
            else:
                assert np.array_equal(r["after"][i], r["before"][i]), i  # untouched
    assert ranks[0]["mine"] == [1] and ranks[1]["mine"] == [2]


# ---- 5. exchange accounting -------------------------------------------------------------------------------------

def test_exchanges_per_frame(dev):
    """Clean-up adds exactly one exchange per frame; a mask that reaches the IoU test adds one; the counts are the
    same on every rank, the one that owns no object included (world 3, two objects)."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm = pipeline.make_params(WD, HD, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(WD, HD, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    frames = [synth.render(f) + synth.camera_pose(f) for f in range(4)]
    synth.close()

    def job(cleanup, extra_mask):
        def body(r, comm, ready):
            fus = pipeline.Fusion(prm, comm)
            fus.set_cleanup(cleanup)
            ready.wait(timeout=JOIN_S)
            keep, per_frame, deleted = [], [], []
            for f, (depth, sid, R, t) in enumerate(frames):
                d = to_dev(depth)
                masks = {i: to_dev((sid == i).astype(np.uint8)) for i in fus.object_ids()}
                keep += [d, masks]
                if f == 0:
                    new = [to_dev((sid == k).astype(np.uint8)) for k in (1, 2)]
                    keep.append(new)
                    fus.queue_new_object_masks([image_view(m) for m in new])
                if f == 3 and extra_mask:  # sphere 1 again (blocked by the IoU test) and a mask with too few points
                    tiny = np.zeros((HD, WD), np.uint8)
                    tiny[100:105, 100:105] = 1
                    new = [to_dev((sid == 1).astype(np.uint8)), to_dev(tiny)]
                    keep.append(new)
                    fus.queue_new_object_masks([image_view(m) for m in new])
                x0 = comm.exchanges()
                fus.process_frame(image_view(d), R, t, {}, {i: image_view(m) for i, m in masks.items()}, True)
                fus.synchronize()
                per_frame.append(comm.exchanges() - x0)
                deleted.append(fus.last_deleted())
            res = dict(x=per_frame, deleted=deleted, ids=fus.object_ids(),
                       owned=[i for i in fus.object_ids() if fus.owns_object(i)], created=fus.last_created())
            fus.close()
            return res
        return run_ranks(3, body)

    off, on, extra = job(False, False), job(True, False), job(True, True)
    assert on[2]["owned"] == [] and on[0]["ids"] == [1, 2]  # rank 2 owns nothing
    for runs in (off, on, extra):
        assert all(r["x"] == runs[0]["x"] for r in runs)
    assert all(fr == [] for fr in on[0]["deleted"])
    assert [b - a for a, b in zip(off[0]["x"], on[0]["x"])] == [1] * len(frames)
    assert [b - a for a, b in zip(on[0]["x"], extra[0]["x"])] == [0, 0, 0, 1]
    assert extra[0]["created"] == [-1, -1]


# ---- 6. uneven ownership, more objects than two launch chunks ---------------------------------------------------

def test_uneven_ownership_many_objects(dev):
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 80, 60
    prm = pipeline.make_params(Wf, Hf, 32, 0.08, 8, visibility_thresh=20, boundary=2)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 1, seed=0xE3F5)
    depth, _ = synth.render(0)
    R, t = synth.camera_pose(0)
    centre = synth.sphere(0, 0)[0]
    synth.close()
    behind = np.array([0, 0, -30], np.float32)

    def body(r, comm, ready):
        fus = pipeline.Fusion(prm, comm)
        fus.set_cleanup(True)
        ready.wait(timeout=JOIN_S)
        d = to_dev(depth)
        log = []
        for f in range(4):  # spawn and delete until the ids pass 3 x world
            for _ in range(3):
                fus.add_object(behind, 0.5)
            fus.process_frame(image_view(d), R, t, {}, {}, False)
            fus.synchronize()
            log.append(fus.last_deleted())
        rng = np.random.default_rng(7)
        for k in range(70):  # > 2 x EMF_MAX_BATCH, several of them out of view
            c = behind if k % 9 == 4 else centre + rng.uniform(-0.2, 0.2, 3).astype(np.float32)
            fus.add_object(c, 0.4)
        for f in range(3):
            fus.process_frame(image_view(d), R, t, {}, {}, False)
            fus.synchronize()
            log.append(fus.last_deleted())
        res = dict(log=log, ids=fus.object_ids(), n=len([i for i in fus.object_ids() if fus.owns_object(i)]))
        fus.close()
        return res

    single = run_ranks(1, body)[0]
    assert max(i for fr in single["log"][:4] for i in fr) > 9
    assert sum(len(fr) for fr in single["log"][4:]) >= 7  # at least the ones behind the camera
    ranks = run_ranks(3, body)
    for r in ranks:
        assert r["log"] == single["log"] and r["ids"] == single["ids"], (r["log"], single["log"])
    assert sum(r["n"] for r in ranks) == len(single["ids"])
