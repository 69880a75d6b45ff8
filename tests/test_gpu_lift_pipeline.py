"""Lifting objects out of the background on live sessions, at the scale of test_gpu_absorb_pipeline.py:
128^3 background, 32^3 objects, 320 x 240.  The round trip: two objects are seen, the camera turns away (both are absorbed),
and it turns back later, from another viewpoint, on a frame with masks (two new ids).  With the switch on each new object
equals, byte for byte, tests/lift_reference.py's seed applied to a twin's volumes (switch off, same frames) with the twin's
background, the background equals the release applied in the log's order with the live session's foreground masks, and
the log holds the restatement's records.  Derived state: two more frames equal those of a session resumed from a
checkpoint.  lift_object on a live object; the switch set and cleared against never set; a rejected mask; the refusals;
--lift-objects on both apps."""
import subprocess
import sys

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import lift_reference as lr
from tests.parity_util import to_dev
from tests.test_gpu_absorb_pipeline import BG, H, TURN, W, background, digest, params
from tests.test_gpu_frontier_pipeline import APP, ROOT, listing

pytestmark = pytest.mark.gpu

f32 = np.float32
BACK = 45  # the stream's frame at which the camera looks at the objects again: half its orbit (10 cm) from where it began


class Run:
    """One session over the two-sphere stream of test_gpu_absorb_pipeline.Run: objects spawned from their masks, poses
    handed in, no tracking.  frame(new=True) queues a new-object mask per sphere; frame(turned=True) looks the other way."""

    def __init__(self, absorb=True, lift=False, pose_log=False, exp_lifted=False):
        from emfusion_amd import pipeline
        self.prm = params()
        self.synth = pipeline.SyntheticStream(W, H, np.array(self.prm.K, f32), 2, seed=0xE3F5)
        self.fus = pipeline.Fusion(self.prm, None)
        self.fus.set_cleanup(True)
        if pose_log:
            self.fus.setup_output(False, False, exp_lifted=exp_lifted)
        if absorb:
            self.fus.set_absorb_objects(True)
        if lift:
            self.fus.set_lift_objects(True)
        self.centers, self.sphere, self.keep, self.f = {}, {}, [], 0

    def frame(self, turned=False, new=None, blank_new=False):
        from emfusion_amd.ops import image_view
        fus, f = self.fus, self.f
        new = f == 0 if new is None else new
        depth, sid = self.synth.render(f)
        R, t = self.synth.camera_pose(f)
        if turned:  # the camera looks the other way: x and z of its frame flip
            R = (R.reshape(3, 3) @ np.diag([-1, 1, -1]).astype(f32)).reshape(-1)
        d = to_dev(depth)
        live = [i for i in self.centers if i in fus.object_ids()]
        masks = {} if turned else {i: to_dev((sid == self.sphere[i]).astype(np.uint8)) for i in live}
        self.keep += [d, masks]
        if new:  # blank_new: masks of three pixels, below the visibility threshold: initNewObjVolume rejects them
            fresh = [to_dev(((sid == k + 1) & (not blank_new or np.arange(sid.size).reshape(sid.shape) % 4001 == 0)).astype(np.uint8))
                     for k in range(2)]
            self.keep.append(fresh)
            fus.queue_new_object_masks([image_view(m) for m in fresh])
        poses = {i: (np.eye(3, dtype=f32).reshape(-1), self.centers[i]) for i in live}
        fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, not turned)
        fus.synchronize()
        if new:
            for k, i in enumerate(fus.last_created()):
                if i >= 0:
                    self.centers[i], self.sphere[i] = fus.pose(i)[1], k + 1
        self.f += 1

    def close(self):
        self.fus.close()
        self.synth.close()


def volumes(fus, oid):
    info = fus.object_info(oid)
    return dict(tsdf=fus.volume("tsdf", oid), weights=fus.volume("weights", oid), voxel_size=info["voxel_size"],
                truncdist=info["truncdist"])


def expected(twin, live, events):
    """The restatement in the log's order: per event the object's (tsdf, weights, seed record), and the background's
    (tsdf, weights) with the release records."""
    from emfusion_amd import ops, pipeline
    prm = twin.params
    bg, trunc = background(twin)
    bg_pose = twin.background_pose()
    src = ar.src_vol(bg["tsdf"], bg["weights"], None, prm.bg_voxel_size, trunc)
    objs, released = {}, []
    tsdf, weights = bg["tsdf"], bg["weights"]
    for e in events:
        i = e["id"]
        v, pose = volumes(twin, i), twin.pose(i)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pose, live.pose(i)))
        R, t = pipeline.absorb_pose(pose, bg_pose)  # the destination first: background frame <- object frame
        assert R.tobytes() == e["seed_R"].tobytes() and t.tobytes() == e["seed_t"].tobytes()
        dst = ar.dst_vol(v["tsdf"], v["weights"], v["voxel_size"], v["truncdist"], prm.max_tsdf_weight)
        objs[i] = lr.seed(dst, src, (R, t))
        lr.check_identities(objs[i][2])
        R, t = pipeline.absorb_pose(bg_pose, pose)
        assert R.tobytes() == e["release_R"].tobytes() and t.tobytes() == e["release_t"].tobytes()
        res = v["tsdf"].shape[::-1]
        box = ops.absorb_box((BG, BG, BG), prm.bg_voxel_size, res, v["voxel_size"], (R, t))
        assert box == (e["lo"], e["size"])
        claim = lr.claim_of(live.volume("fgmask", i), res, v["voxel_size"])
        tsdf, weights, rec = lr.release(ar.dst_vol(tsdf, weights, prm.bg_voxel_size, trunc), claim, (R, t), box)
        lr.check_identities(rec)
        released.append(rec)
    return objs, (tsdf, weights), released


@pytest.fixture(scope="module")
def round_trip(dev, tmp_path_factory):
    """The live session and its twin (absorb on in both) through the frame at which the camera sees the objects again; a
    checkpoint of the live session right after it.  The live session's switch goes on while the camera looks away: up to
    there the two sessions are one, and the twin's volumes are what the live session's passes started from."""
    live, twin = Run(lift=False, pose_log=True, exp_lifted=True), Run(lift=False, pose_log=True)
    for r in (live, twin):
        for _ in range(TURN):
            r.frame()
        assert r.fus.object_ids() == [1, 2]
        r.frame(turned=True)
        assert r.fus.object_ids() == [] and [e["id"] for e in r.fus.absorbed()] == [1, 2]
    assert live.fus.lifted() == [] and live.fus.volume("tsdf", 0).tobytes() == twin.fus.volume("tsdf", 0).tobytes()
    live.fus.set_lift_objects(True)
    for r in (live, twin):
        r.f = BACK
        r.frame(new=True)
    path = tmp_path_factory.mktemp("lift") / "after.ckpt"
    live.fus.save_checkpoint(path)
    yield dict(live=live, twin=twin, ckpt=path)
    live.close()
    twin.close()


def read_lifted(path):
    """The event lines of a lifted.txt, each checked for its shape and the count identities."""
    lines = path.read_text().splitlines()
    assert lines[0].startswith("# id frame clipped box_lo(3) box_size(3) seed: visited kept outside unknown masked saturated seeded solid")
    for row in (ln.split() for ln in lines[1:]):
        assert len(row) == 36 + 24
        n = [int(v) for v in row[:36]]
        assert n[2] in (0, 1) and n[9] == sum(n[10:16]) and n[16] <= n[15]      # the seed
        assert n[23] == sum(n[24:29]) and n[29] <= n[28] and n[23] == n[6] * n[7] * n[8]  # the release: the voxels of the box
        [float(v) for v in row[36:]]
    return lines[1:]


def test_a_returning_object_is_seeded_and_the_background_releases_it(round_trip, tmp_path):
    live, twin = round_trip["live"].fus, round_trip["twin"].fus
    ids = live.object_ids()
    assert ids == twin.object_ids() == live.last_created() == [3, 4] and live.last_deleted() == []
    log = live.lifted()
    assert [e["id"] for e in log] == ids and all(e["frame"] == TURN + 1 and not e["clipped"] for e in log) and twin.lifted() == []
    objs, (tsdf, weights), released = expected(twin, live, log)
    for e, rec in zip(log, released):
        i = e["id"]
        print(i, e["lo"], e["size"], objs[i][2], rec)
        assert e["seed"].dtype == lr.SEED and e["seed"].tobytes() == objs[i][2].tobytes(), (e["seed"], objs[i][2])
        assert e["release"].dtype == lr.RELEASE and e["release"].tobytes() == rec.tobytes(), (e["release"], rec)
        got_t, got_w = live.volume("tsdf", i), live.volume("weights", i)
        assert got_t.tobytes() == objs[i][0].tobytes() and got_w.tobytes() == objs[i][1].tobytes()
        # seeded voxels under the frame's instance mask are foreground at once
        seeded = got_w.view(np.uint32) != twin.volume("weights", i).view(np.uint32)
        fg = live.volume("fgmask", i)
        print("seeded", int(seeded.sum()), "of them foreground", int((fg[seeded] == 255).sum()), "released", int(rec["released"]))
        assert seeded.sum() == objs[i][2]["seeded"] > 0 and (fg[seeded] == 255).sum() > 0
        assert rec["released"] > 0 and rec["solid"] > 0
    got_t, got_w = live.volume("tsdf", 0), live.volume("weights", 0)
    assert got_t.tobytes() == tsdf.tobytes() and got_w.tobytes() == weights.tobytes()
    # every reader of the background: no occupied voxel among the released ones, where the twin keeps the ghost
    gone = got_w.view(np.uint32) != twin.volume("weights", 0).view(np.uint32)
    assert gone.sum() == sum(int(r["released"]) for r in released)
    occ_live = live.distance_field(metres=False, exclude=ids)["classes"] == 1
    occ_twin = twin.distance_field(metres=False, exclude=ids)["classes"] == 1
    print("occupied among the released: live", int(occ_live[gone].sum()), "twin", int(occ_twin[gone].sum()))
    assert occ_live[gone].sum() == 0 and occ_twin[gone].sum() == sum(int(r["solid"]) for r in released) > 0
    for rec in released:
        lo, hi = rec["lo"], rec["hi"]
        cut = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
        assert occ_twin[cut].sum() > occ_live[cut].sum()
    # the kept meshes of the absorbed objects are the twin's; lifted.txt is lifted_line() of the events
    from emfusion_amd import pipeline
    live.write_results(tmp_path / "live", volumes=False)
    twin.write_results(tmp_path / "twin", volumes=False)
    a, b = listing(tmp_path / "live"), listing(tmp_path / "twin")
    assert set(a) - set(b) == {"lifted.txt"} and set(b) <= set(a) and {"mesh_1.ply", "mesh_2.ply", "mesh_bg.ply"} <= set(b)
    assert a["mesh_1.ply"] == b["mesh_1.ply"] and a["mesh_2.ply"] == b["mesh_2.ply"] and a["mesh_bg.ply"] != b["mesh_bg.ply"]
    lines = read_lifted(tmp_path / "live" / "lifted.txt")
    assert lines == [pipeline.lifted_line(e) for e in log] and len(lines) == 2
    for line, e, rec in zip(lines, log, released):
        row = line.split()
        assert [int(v) for v in row[:3]] == [e["id"], TURN + 1, 0] and tuple(int(v) for v in row[3:9]) == e["lo"] + e["size"]
        assert [int(v) for v in row[9:17]] == [int(objs[e["id"]][2][k]) for k in lr.SEED_COUNTS]
        assert [int(v) for v in row[23:30]] == [int(rec[k]) for k in lr.RELEASE_COUNTS]
        poses = np.array([np.float32(v) for v in row[36:]], f32)  # %.9g carries a float32 exactly
        assert poses.tobytes() == b"".join(e[k].astype(f32).tobytes() for k in ("seed_R", "seed_t", "release_R", "release_t"))


def test_two_more_frames_equal_those_of_a_resumed_session(round_trip, tmp_path):
    from emfusion_amd import pipeline
    live = round_trip["live"]
    resumed = pipeline.Fusion.from_checkpoint(round_trip["ckpt"])
    try:
        assert resumed.lifted() == [] and len(live.fus.lifted()) == 2  # the log is session state: not in the file
        resumed.save_checkpoint(tmp_path / "again.ckpt")  # ... and the file's bytes do not depend on it
        assert (tmp_path / "again.ckpt").read_bytes() == round_trip["ckpt"].read_bytes()
        other = Run.__new__(Run)
        other.prm, other.synth, other.fus, other.centers, other.sphere, other.keep, other.f = \
            live.prm, live.synth, resumed, dict(live.centers), dict(live.sphere), [], live.f
        for _ in range(2):
            f = live.f
            live.frame()
            other.f = f
            other.frame()
            for which in ("bg_raylengths", "segmentation", "vertices", "normals"):
                assert live.fus.image(which).tobytes() == resumed.image(which).tobytes(), (f, which)
            for i in [0] + live.fus.object_ids():
                for which in ("tsdf", "weights", "bricks"):
                    assert live.fus.volume(which, i).tobytes() == resumed.volume(which, i).tobytes(), (f, which, i)
        assert live.fus.object_ids() == resumed.object_ids() == [3, 4] and sorted(live.fus.visible_objects()) == [3, 4]
    finally:
        resumed.close()


def test_lift_object_on_a_live_object(dev):
    """The switch is off: the objects of frame 0 start empty although the background fused the spheres itself on that
    frame.  lift_object(2) between frames seeds and releases; the object stays live."""
    from emfusion_amd import pipeline
    run, twin = Run(absorb=False), Run(absorb=False)
    try:
        for _ in range(3):
            run.frame()
            twin.frame()
        fus = run.fus
        other = fus.volume("tsdf", 1)
        event = fus.lift_object(2)
        assert fus.object_ids() == [1, 2] and event["id"] == 2 and event["frame"] == 3 and not event["clipped"]
        objs, (tsdf, weights), released = expected(twin.fus, fus, [event])
        assert event["seed"].tobytes() == objs[2][2].tobytes() and event["release"].tobytes() == released[0].tobytes()
        assert released[0]["released"] > 0
        assert fus.volume("tsdf", 2).tobytes() == objs[2][0].tobytes() and fus.volume("weights", 2).tobytes() == objs[2][1].tobytes()
        assert fus.volume("tsdf", 0).tobytes() == tsdf.tobytes() and fus.volume("weights", 0).tobytes() == weights.tobytes()
        assert fus.volume("tsdf", 1).tobytes() == other.tobytes()
        log = fus.lifted()
        assert len(log) == 1 and log[0]["seed"].tobytes() == event["seed"].tobytes() and log[0]["lo"] == event["lo"]
        run.frame()  # the session goes on with both objects
        assert fus.object_ids() == [1, 2] and sorted(fus.visible_objects()) == [1, 2]
        for bad in (3, 7, 0, -1):
            with pytest.raises(pipeline.FusionError) as err:
                fus.lift_object(bad)
            assert err.value.code == -4, bad
        assert len(fus.lifted()) == 1
        fus.reset()
        assert fus.lifted() == []
    finally:
        run.close()
        twin.close()


def test_the_switch_set_and_cleared_is_the_switch_never_set(dev, tmp_path):
    runs = [Run(), Run()]
    try:
        runs[1].fus.set_lift_objects(True)
        runs[1].fus.set_lift_objects(False)
        for f in range(TURN + 3):
            got = []
            for k, r in enumerate(runs):
                r.frame(turned=f == TURN, new=f in (0, TURN + 1))
                got.append(digest(r, tmp_path, f"{k}.ckpt"))
            assert got[0] == got[1], f
        assert runs[0].fus.object_ids() == [3, 4] and runs[1].fus.lifted() == []
    finally:
        for r in runs:
            r.close()


def test_a_rejected_mask_lifts_nothing(dev):
    """Frame 1 queues two masks of a handful of pixels, below the visibility threshold: initNewObjVolume returns -1 for
    both, nothing is launched, and the session is the one that was handed no new mask."""
    runs = [Run(lift=True), Run(lift=True)]
    try:
        for k, r in enumerate(runs):
            r.frame()
            r.frame(new=k == 0, blank_new=True)
            assert r.fus.object_ids() == [1, 2] and [e["id"] for e in r.fus.lifted()] == [1, 2]  # frame 0 only
        assert runs[0].fus.last_created() == [-1, -1] and runs[1].fus.last_created() == []
        for i in (0, 1, 2):
            for which in ("tsdf", "weights"):
                assert runs[0].fus.volume(which, i).tobytes() == runs[1].fus.volume(which, i).tobytes(), (i, which)
    finally:
        for r in runs:
            r.close()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.set_lift_objects(True), lambda: fus.lift_object(1)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        fus.set_lift_objects(False)  # clearing what was never set is no error
        assert fus.lifted() == []
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 2, [-4] * 2]


def test_the_apps_write_lifted_txt_only_with_the_switch(dev, tmp_path):
    """emfusion_synth --autonomous spawns its objects from instance masks and TRACKS the camera and the objects, so a lift
    changes what later frames track against: the runs are compared for finishing and for the shape of their files."""
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = ["--frames", "5", "--objects", "2", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120", "--autonomous"]
    outs, stdout = {}, {}
    for name, extra in (("plain", []), ("lift", ["--lift-objects"])):
        p = subprocess.run([str(APP), *small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name], stdout[name] = listing(tmp_path / name), p.stdout
    assert set(outs["lift"]) - set(outs["plain"]) == {"lifted.txt"} and set(outs["plain"]) <= set(outs["lift"])
    rows = [ln.split() for ln in read_lifted(tmp_path / "lift" / "lifted.txt")]
    count = [ln for ln in stdout["lift"].splitlines() if ln.startswith("lifted out of the background:")]
    assert len(count) == 1 and int(count[0].split()[5]) == len(rows) >= 1  # one line per event
    assert not any(ln.startswith("lifted out of the background:") for ln in stdout["plain"].splitlines())
    # refused before any device is touched: no --out; the synthetic stream with given poses, where no mask creates an object
    for cmd, word in (([str(APP), "--autonomous", "--lift-objects"], "--out"),
                      ([str(APP), "--lift-objects", "--out", str(tmp_path / "no")], "--autonomous"),
                      ([str(APP), "--lift-objects", "--turn-away", "3", "--out", str(tmp_path / "no")], "--autonomous")):
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (cmd, p.returncode, p.stderr[-500:])
    assert not (tmp_path / "no").exists()
    # the dataset app takes the same switch
    from tests import tum_staging as T
    seq, masks, _ = T.stage(tmp_path)
    tum = [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]
    p = subprocess.run([*tum, "--out", str(tmp_path / "tum"), "--lift-objects"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    read_lifted(tmp_path / "tum" / "lifted.txt")
