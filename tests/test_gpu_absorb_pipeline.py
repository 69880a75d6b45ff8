"""Absorbing objects into the background on live sessions: 128^3 background, 32^3 objects, 320 x 240, on
the pattern of test_gpu_lifecycle.py::test_invisible_objects_are_cleaned_up -- but the objects leave view because the
CAMERA turns away.  With the switch on the background after the deleting frame equals, byte for byte,
tests/absorb_reference.py applied to a twin's background (switch off, same frames), the objects' volumes from before the
frame and absorb_pose of the poses; the log holds the restatement's records; the distance field sees the absorbed
objects.  Derived state: two more frames equal those of a session resumed from a checkpoint.  Spurious objects and a
person under ignore_person are not absorbed.  absorb_object on a live object; the switch set and cleared against never
set; the refusals; --absorb-objects on both apps."""
import hashlib
import subprocess
import sys

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests.parity_util import to_dev
from tests.test_gpu_frontier_pipeline import APP, ROOT, listing

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, BG, VOX, OBJ = 320, 240, 128, 0.04, 32
TURN = 3  # the frame at which the camera looks the other way


def params():
    from emfusion_amd import pipeline
    return pipeline.make_params(W, H, BG, VOX, OBJ, visibility_thresh=400, boundary=10)


class Run:
    """One session over the two-sphere stream: objects spawned from their masks on frame 0, poses handed in, no
    tracking; at `turn` the camera pose is rotated by half a turn about its y axis, so that no object is seen."""

    def __init__(self, absorb=False, spheres=2, pose_log=False, exp_vols=False, exp_absorbed=False):
        from emfusion_amd import pipeline
        self.prm = params()
        self.synth = pipeline.SyntheticStream(W, H, np.array(self.prm.K, f32), spheres, seed=0xE3F5)
        self.fus = pipeline.Fusion(self.prm, None)
        self.fus.set_cleanup(True)
        if pose_log:
            self.fus.setup_output(False, exp_vols, exp_absorbed=exp_absorbed)
        if absorb:
            self.fus.set_absorb_objects(True)
        self.spheres, self.centers, self.keep, self.f = spheres, {}, [], 0

    def frame(self, turned=False, masks_for=None, run_masks=True):
        from emfusion_amd.ops import image_view
        fus, f = self.fus, self.f
        depth, sid = self.synth.render(f)
        R, t = self.synth.camera_pose(f)
        if turned:  # the camera looks the other way: x and z of its frame flip
            R = (R.reshape(3, 3) @ np.diag([-1, 1, -1]).astype(f32)).reshape(-1)
        d = to_dev(depth)
        ids = [i for i in self.centers if i in fus.object_ids()] if masks_for is None else masks_for
        masks = {} if turned else {i: to_dev((sid == i).astype(np.uint8)) for i in ids}
        self.keep += [d, masks]
        if f == 0:
            new = [to_dev((sid == k + 1).astype(np.uint8)) for k in range(self.spheres)]
            self.keep.append(new)
            fus.queue_new_object_masks([image_view(m) for m in new])
        poses = {i: (np.eye(3, dtype=f32).reshape(-1), c) for i, c in self.centers.items() if i in fus.object_ids()}
        fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, run_masks and not turned)
        fus.synchronize()
        if f == 0:
            self.centers = {k: fus.pose(k)[1] for k in fus.last_created()}
        self.f += 1

    def close(self):
        self.fus.close()
        self.synth.close()


def model(fus, oid):
    """What the restatement needs of one live object: its volumes as a source, and its pose."""
    info = fus.object_info(oid)
    return (ar.src_vol(fus.volume("tsdf", oid), fus.volume("weights", oid), fus.volume("fgmask", oid), info["voxel_size"],
                       info["truncdist"]), fus.pose(oid))


def background(fus):
    """The background as a destination; voxel size and truncation distance as object_contacts reports them."""
    ids = fus.object_ids()
    side = fus.object_contacts(ids=ids[:1])["sides"][0] if ids else None
    trunc = float(side["truncdist"]) if ids else None
    return ar.dst_vol(fus.volume("tsdf", 0), fus.volume("weights", 0), fus.params.bg_voxel_size, trunc or 1.0,
                      fus.params.max_tsdf_weight), trunc


def expected(bg_tsdf, bg_weights, trunc, prm, bg_pose, sources, events):
    """The restatement applied in the log's order: (tsdf, weights, records)."""
    from emfusion_amd import ops, pipeline
    tsdf, weights, records = bg_tsdf, bg_weights, []
    for (src, pose), e in zip(sources, events):
        R, t = pipeline.absorb_pose(bg_pose, pose)
        Rn, tn = ar.absorb_pose_np(bg_pose[0], bg_pose[1], pose[0], pose[1])
        assert R.tobytes() == Rn.tobytes() == e["R"].tobytes() and t.tobytes() == tn.tobytes() == e["t"].tobytes()
        box = ops.absorb_box((BG, BG, BG), prm.bg_voxel_size, src["tsdf"].shape[::-1], src["voxel_size"], (R, t))
        assert box == (e["lo"], e["size"])
        dst = ar.dst_vol(tsdf, weights, prm.bg_voxel_size, trunc, prm.max_tsdf_weight)
        tsdf, weights, rec = ar.absorb(dst, src, (R, t), box)
        ar.check_identities(rec)
        records.append(rec)
    return tsdf, weights, records


@pytest.fixture(scope="module")
def turned(dev, tmp_path_factory):
    """The live session (switch on) and its twin (off) through the frame at which the camera turns away; what the
    restatement needs, read before that frame; a checkpoint of the live session right after it."""
    live, twin = Run(absorb=True, pose_log=True, exp_absorbed=True), Run(absorb=False, pose_log=True)
    for _ in range(TURN):
        live.frame()
        twin.frame()
    ids = live.fus.object_ids()
    assert ids == twin.fus.object_ids() == [1, 2] and sorted(live.fus.visible_objects()) == [1, 2]
    # In this scene the background saw the spheres itself on frame 0, before the objects existed.  Two rolls, 96 voxels up
    # and 64 down along x, wipe that part of it in both sessions and leave the background 32 voxels from where it
    # started: the objects then stand in a region it knows nothing of, and the pose used is one after rolls.
    for r in (live, twin):
        r.fus.roll_background((96, 0, 0), keep_retired=False)
        r.fus.roll_background((-64, 0, 0), keep_retired=False)
        assert r.fus.background_origin() == (32, 0, 0)
    sources = [model(live.fus, i) for i in ids]
    _, trunc = background(live.fus)
    assert live.fus.volume("tsdf", 0).tobytes() == twin.fus.volume("tsdf", 0).tobytes() and live.fus.absorbed() == []
    live.frame(turned=True)
    twin.frame(turned=True)
    path = tmp_path_factory.mktemp("absorb") / "after.ckpt"
    live.fus.save_checkpoint(path)
    yield dict(live=live, twin=twin, sources=sources, trunc=trunc, ids=ids, ckpt=path)
    live.close()
    twin.close()


def read_absorbed(path):
    """The event lines of an absorbed.txt, each checked for its shape and the count identity."""
    lines = path.read_text().splitlines()
    assert lines[0].startswith("# id frame clipped box_lo(3) box_size(3) visited outside unknown masked saturated fused fresh solid")
    assert "the band only" in lines[0]
    for row in (ln.split() for ln in lines[1:]):
        n = [int(v) for v in row[:23]]
        assert len(row) == 23 + 12 and n[2] in (0, 1) and n[9] == sum(n[10:15]) and n[15] <= n[14] and n[16] <= n[14]
        assert n[9] == n[6] * n[7] * n[8]  # visited: the voxels of the box
    return lines[1:]


def test_objects_that_leave_view_are_absorbed(turned, tmp_path):
    live, twin = turned["live"].fus, turned["twin"].fus
    assert live.last_deleted() == twin.last_deleted() == [1, 2] and live.object_ids() == twin.object_ids() == []
    log = live.absorbed()
    assert [e["id"] for e in log] == [1, 2] and all(e["frame"] == TURN and not e["clipped"] for e in log) and twin.absorbed() == []
    assert live.background_pose()[0].tobytes() == twin.background_pose()[0].tobytes()
    tsdf, weights, records = expected(twin.volume("tsdf", 0), twin.volume("weights", 0), turned["trunc"], live.params,
                                      twin.background_pose(), turned["sources"], log)
    for e, rec in zip(log, records):
        print(e["id"], e["lo"], e["size"], rec)
        assert e["record"].dtype == ar.ABSORB and e["record"].tobytes() == rec.tobytes(), (e["record"], rec)
        assert rec["fused"] == rec["fresh"] > 0 and rec["solid"] > 0  # into a region the background does not know
    got_t, got_w = live.volume("tsdf", 0), live.volume("weights", 0)
    assert got_t.tobytes() == tsdf.tobytes() and got_w.tobytes() == weights.tobytes()
    assert got_t.tobytes() != twin.volume("tsdf", 0).tobytes()
    # every reader of the background sees them: occupied voxels inside the records' bounds where the twin has none
    occ_live, occ_twin = live.distance_field(metres=False)["classes"] == 1, twin.distance_field(metres=False)["classes"] == 1
    for rec in records:
        lo, hi = rec["lo"], rec["hi"]
        cut = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
        print("occupied in the bounds: live", int(occ_live[cut].sum()), "twin", int(occ_twin[cut].sum()), "live only",
              int((occ_live[cut] & ~occ_twin[cut]).sum()), "twin only", int((occ_twin[cut] & ~occ_live[cut]).sum()))
        assert occ_live[cut].sum() == rec["solid"] and occ_twin[cut].sum() == 0
    # the kept meshes of the deleted objects are the twin's (the pose log is on); the background's mesh is not
    live.write_results(tmp_path / "live", volumes=False)
    twin.write_results(tmp_path / "twin", volumes=False)
    a, b = listing(tmp_path / "live"), listing(tmp_path / "twin")
    assert set(a) - set(b) == {"absorbed.txt"} and set(b) <= set(a) and {"mesh_1.ply", "mesh_2.ply", "mesh_bg.ply"} <= set(b)
    assert all(a[k] == b[k] for k in b if k != "mesh_bg.ply") and a["mesh_bg.ply"] != b["mesh_bg.ply"]
    # absorbed.txt (the live session's exp_absorbed): one line per event, the line absorbed_line() makes of the event, and
    # in it the restatement's record and the pose and the box the restatement was given
    from emfusion_amd import pipeline
    lines = read_absorbed(tmp_path / "live" / "absorbed.txt")
    assert lines == [pipeline.absorbed_line(e) for e in log] and len(lines) == 2
    for line, e, rec in zip(lines, log, records):
        row = line.split()
        assert [int(v) for v in row[:3]] == [e["id"], TURN, 0] and tuple(int(v) for v in row[3:9]) == e["lo"] + e["size"]
        assert [int(v) for v in row[9:17]] == [int(rec[k]) for k in ar.COUNTS]
        assert [int(v) for v in row[17:23]] == [int(v) for v in rec["lo"]] + [int(v) for v in rec["hi"]]
        pose = np.array([np.float32(v) for v in row[23:]], f32)  # %.9g carries a float32 exactly
        assert pose.tobytes() == e["R"].astype(f32).tobytes() + e["t"].astype(f32).tobytes()


def test_two_more_frames_equal_those_of_a_resumed_session(turned):
    from emfusion_amd import pipeline
    live = turned["live"]
    resumed = pipeline.Fusion.from_checkpoint(turned["ckpt"])
    try:
        assert resumed.absorbed() == []  # the log is session state: not in the file
        assert resumed.volume("tsdf", 0).tobytes() == live.fus.volume("tsdf", 0).tobytes()
        other = Run.__new__(Run)
        other.prm, other.synth, other.fus, other.spheres, other.centers, other.keep, other.f = \
            live.prm, live.synth, resumed, live.spheres, dict(live.centers), [], live.f
        for _ in range(2):
            f = live.f
            live.frame()
            other.f = f
            other.frame()
            for which in ("bg_raylengths", "segmentation", "vertices", "normals"):
                assert live.fus.image(which).tobytes() == resumed.image(which).tobytes(), (f, which)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(live.fus.pose(0), resumed.pose(0)))
            for which in ("tsdf", "weights", "bricks"):
                assert live.fus.volume(which, 0).tobytes() == resumed.volume(which, 0).tobytes(), (f, which)
        assert (live.fus.image("bg_raylengths") > 0).sum() > 1000
    finally:
        resumed.close()


def test_a_spurious_object_is_not_absorbed(dev):
    """Object 2 gets no mask on eleven mask frames: its existence probability falls below existenceThresh (0.1) and the
    clean-up deletes it as spurious while it is still in view."""
    runs = [Run(absorb=True), Run(absorb=False)]
    try:
        deleted = None
        for f in range(13):
            for r in runs:
                r.frame(masks_for=[1] if f else None)
            assert runs[0].fus.last_deleted() == runs[1].fus.last_deleted()
            if runs[0].fus.last_deleted():
                deleted = (f, runs[0].fus.last_deleted())
                break
            assert 2 in runs[0].fus.visible_objects()
        assert deleted is not None and deleted[1] == [2] and runs[0].fus.object_ids() == [1]
        assert runs[0].fus.absorbed() == []
        for which in ("tsdf", "weights"):
            assert runs[0].fus.volume(which, 0).tobytes() == runs[1].fus.volume(which, 0).tobytes()
    finally:
        for r in runs:
            r.close()


def test_a_person_under_ignore_person_is_not_absorbed(dev):
    """One object whose accumulated class scores say "person" (test_gpu_lifecycle.py); the camera turns away."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    person = np.zeros(81)
    person[1] = 0.9
    out = []
    for absorb in (True, False):
        prm = params()
        synth = pipeline.SyntheticStream(W, H, np.array(prm.K, f32), 1, seed=0xE3F5)
        fus = pipeline.Fusion(prm, None)
        fus.set_cleanup(True)
        fus.set_ignore_person(True)
        if absorb:
            fus.set_absorb_objects(True)
        centers, keep = {}, []
        for f in range(3):
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            turned_now = f == 2
            if turned_now:
                R = (R.reshape(3, 3) @ np.diag([-1, 1, -1]).astype(f32)).reshape(-1)
            d = to_dev(depth)
            inst = [to_dev((sid == 1).astype(np.uint8))]
            keep += [d, inst]
            if not turned_now:
                fus.queue_instance_masks([image_view(m) for m in inst])
                fus.queue_instance_scores([person])
            poses = {i: (np.eye(3, dtype=f32).reshape(-1), c) for i, c in centers.items()}
            fus.process_frame(image_view(d), R, t, poses, {}, False)
            fus.synchronize()
            if f == 0:
                centers = {1: fus.pose(1)[1]}
            if f == 1:
                assert fus.object_class(1) == 1 and fus.object_ids() == [1]
        assert fus.last_deleted() == [1] and fus.absorbed() == []
        out.append((fus.volume("tsdf", 0), fus.volume("weights", 0)))
        fus.close()
        synth.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_absorb_object_on_a_live_object(dev, tmp_path):
    run, twin = Run(absorb=False, pose_log=True), Run(absorb=False, pose_log=True)
    try:
        from emfusion_amd import pipeline
        for _ in range(3):
            run.frame()
            twin.frame()
        twin.fus.write_results(tmp_path / "twin", volumes=False)
        fus = run.fus
        src = model(fus, 2)
        bg, trunc = background(fus)
        other = fus.volume("tsdf", 1)
        event = fus.absorb_object(2)
        assert fus.object_ids() == [1] and event["id"] == 2 and event["frame"] == 3 and not event["clipped"]
        tsdf, weights, records = expected(bg["tsdf"], bg["weights"], trunc, fus.params, fus.background_pose(), [src], [event])
        assert event["record"].tobytes() == records[0].tobytes() and records[0]["fused"] > 0
        assert fus.volume("tsdf", 0).tobytes() == tsdf.tobytes() and fus.volume("weights", 0).tobytes() == weights.tobytes()
        log = fus.absorbed()
        assert len(log) == 1 and log[0]["record"].tobytes() == event["record"].tobytes() and log[0]["lo"] == event["lo"]
        assert fus.volume("tsdf", 1).tobytes() == other.tobytes()
        fus.write_results(tmp_path / "live", volumes=False)  # the kept mesh (pose log on): the one the live object gave
        a, b = listing(tmp_path / "live"), listing(tmp_path / "twin")
        assert a["mesh_2.ply"] == b["mesh_2.ply"] and a["mesh_1.ply"] == b["mesh_1.ply"] and len(a["mesh_2.ply"]) > 1000
        run.frame()  # the session goes on with one object
        assert fus.object_ids() == [1] and 1 in fus.visible_objects()
        # the refusals
        for bad in (2, 7, 0, -1):
            with pytest.raises(pipeline.FusionError) as err:
                fus.absorb_object(bad)
            assert err.value.code == -4, bad
        assert len(fus.absorbed()) == 1
        fus.reset()
        assert fus.absorbed() == []
    finally:
        run.close()
        twin.close()


def digest(run, tmp_path, name):
    h = hashlib.sha256()
    fus = run.fus
    for which in ("bg_raylengths", "segmentation", "vertices", "normals"):
        h.update(fus.image(which).tobytes())
    for which in ("tsdf", "weights", "bricks"):
        h.update(fus.volume(which, 0).tobytes())
    for i in fus.object_ids():
        h.update(fus.volume("tsdf", i).tobytes() + fus.volume("weights", i).tobytes())
    h.update(repr((fus.last_deleted(), fus.object_ids(), sorted(fus.visible_objects()))).encode())
    fus.save_checkpoint(tmp_path / name)
    h.update((tmp_path / name).read_bytes())
    return h.hexdigest()


def test_the_switch_set_and_cleared_is_the_switch_never_set(dev, tmp_path):
    runs = [Run(absorb=False), Run(absorb=False)]
    try:
        runs[1].fus.set_absorb_objects(True)
        runs[1].fus.set_absorb_objects(False)
        for f in range(TURN + 2):
            got = []
            for k, r in enumerate(runs):
                r.frame(turned=f == TURN)
                got.append(digest(r, tmp_path, f"{k}.ckpt"))
            assert got[0] == got[1], f
        assert runs[0].fus.object_ids() == [] and runs[1].fus.absorbed() == []
    finally:
        for r in runs:
            r.close()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.set_absorb_objects(True), lambda: fus.absorb_object(1)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        fus.set_absorb_objects(False)  # clearing what was never set is no error
        assert fus.absorbed() == []
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 2, [-4] * 2]


def test_the_apps_write_absorbed_txt_only_with_the_switch(dev, tmp_path):
    """emfusion_synth with --turn-away 3: the camera handed in looks the other way from frame 3 on and the clean-up runs,
    so both objects leave view there -- deleted in the plain run, absorbed first with --absorb-objects."""
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = ["--frames", "5", "--objects", "2", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120",
             "--turn-away", "3"]
    outs, stdout = {}, {}
    for name, extra in (("plain", []), ("absorb", ["--absorb-objects"])):
        p = subprocess.run([str(APP), *small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name], stdout[name] = listing(tmp_path / name), p.stdout
    assert set(outs["absorb"]) - set(outs["plain"]) == {"absorbed.txt"} and set(outs["plain"]) <= set(outs["absorb"])
    assert {"mesh_1.ply", "mesh_2.ply"} <= set(outs["plain"])  # both objects were deleted with the log on: their meshes are kept
    # everything but the background's own files is the plain run's, byte for byte
    same = [k for k in outs["plain"] if outs["absorb"][k] == outs["plain"][k]]
    assert {"mesh_1.ply", "mesh_2.ply", "poses-cam.txt", "poses-1.txt", "poses-2.txt"} <= set(same)
    assert outs["absorb"]["mesh_bg.ply"] != outs["plain"]["mesh_bg.ply"]
    rows = [ln.split() for ln in read_absorbed(tmp_path / "absorb" / "absorbed.txt")]
    count = [ln for ln in stdout["absorb"].splitlines() if ln.startswith("absorbed into the background:")]
    assert len(count) == 1 and int(count[0].split()[4]) == len(rows) == 2  # one line per event
    assert [int(r[0]) for r in rows] == [1, 2] and all(int(r[1]) == 3 and int(r[14]) > 0 for r in rows)  # ids, frame, fused
    assert not any(ln.startswith("absorbed into the background:") for ln in stdout["plain"].splitlines())
    # refused before any device is touched: no --out; the plain synthetic stream, where nothing is ever deleted
    for cmd, word in (([str(APP), "--absorb-objects"], "--out"),
                      ([str(APP), "--absorb-objects", "--out", str(tmp_path / "no")], "--turn-away"),
                      ([str(APP), "--turn-away", "0", "--out", str(tmp_path / "no")], "--turn-away"),
                      ([str(APP), "--turn-away", "3", "--autonomous", "--out", str(tmp_path / "no")], "--turn-away")):
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (cmd, p.returncode, p.stderr[-500:])
    assert not (tmp_path / "no").exists()
    # the dataset app takes the same switch; whether an object leaves view there is the sequence's business
    from tests import tum_staging as T
    seq, masks, _ = T.stage(tmp_path)
    tum = [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]
    p = subprocess.run([*tum, "--out", str(tmp_path / "tum"), "--absorb-objects"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    read_absorbed(tmp_path / "tum" / "absorbed.txt")
