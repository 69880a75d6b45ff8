"""Merging an object into another object on live sessions, at the scale of test_gpu_lift_pipeline.py: 128^3
background, 32^3 objects, 320 x 240.  One sphere is cut by two half masks into two objects.  After merge_objects the
destination's tsdf, weights, counts and foreground mask equal, byte for byte, tests/merge_reference.py applied to a twin's
volumes (same frames, no merge) -- the growth included: the union of both bands, the resize, the shift -- the source's id is
gone, the bookkeeping is the sum and the log holds the restatement's records; object_shapes() reports one object whose
band covers both halves; the next frames run and raycast the merged object.  The max_res cap leaves the destination as
it is and says `clipped`; a coloured session carries colour; a checkpoint does not depend on the log; the refusals, the
sharded path among them.  Automatic: a true duplicate -- the same sphere as two objects -- is merged at the next mask frame
after set_merge_objects, the older id kept, `automatic` set, the overlaps those of the restatement's ordering on a twin's
probe; two abutting halves are not merged at the default threshold; the switch set and cleared equals never set, by
per-frame digests; both apps write merged.txt only with the switch and give the usage errors."""
import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import merge_reference as mr
from tests.parity_util import to_dev
from tests.test_gpu_absorb_pipeline import H, W, params

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAMES = 3  # frames before the merge: the creating one and two more with both half masks
VOL_PAD = 2.0  # Params::volPad of core/data.hpp


class Run:
    """One session over the one-sphere stream: the sphere's mask is cut at its middle column into two half masks, queued
    as two new objects on frame 0 and handed to them on every later frame; poses handed in, no tracking.  Once the halves
    are merged the whole mask goes to the object that is left."""

    def __init__(self, color=False):
        from emfusion_amd import pipeline
        self.prm = params()
        self.synth = pipeline.SyntheticStream(W, H, np.array(self.prm.K, f32), 1, seed=0xE3F5)
        self.fus = pipeline.Fusion(self.prm, None)
        self.fus.set_cleanup(True)
        self.color = color
        if color:
            self.fus.enable_color()
        self.centers, self.keep, self.f = {}, [], 0

    def frame(self):
        from emfusion_amd.ops import image_view
        fus, f = self.fus, self.f
        depth, sid = self.synth.render(f)
        R, t = self.synth.camera_pose(f)
        cols = np.nonzero((sid == 1).any(axis=0))[0]
        left = (sid == 1) & (np.arange(W)[None, :] < (cols.min() + cols.max() + 1) // 2)
        halves = [left, (sid == 1) & ~left]
        d = to_dev(depth)
        live = fus.object_ids()
        masks = {i: to_dev((halves[i - 1] if len(live) == 2 else sid == 1).astype(np.uint8)) for i in live}
        self.keep += [d, masks]
        if f == 0:
            new = [to_dev(h.astype(np.uint8)) for h in halves]
            self.keep.append(new)
            fus.queue_new_object_masks([image_view(m) for m in new])
        if self.color:
            rgb = np.zeros((H, W, 3), np.uint8)
            rgb[..., 0], rgb[..., 1], rgb[..., 2] = 40 + sid * 90, np.arange(W)[None, :] % 256, np.arange(H)[:, None] % 256
            c = to_dev(rgb)
            self.keep.append(c)
            fus.set_color_image(image_view(c))
        poses = {i: (np.eye(3, dtype=f32).reshape(-1), self.centers[i]) for i in live}
        fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, True)
        fus.synchronize()
        if f == 0:
            self.centers = {k: fus.pose(k)[1] for k in fus.last_created()}
        self.f += 1

    def close(self):
        self.fus.close()
        self.synth.close()


def model(fus, oid, color=False):
    info = fus.object_info(oid)
    v = dict(tsdf=fus.volume("tsdf", oid), weights=fus.volume("weights", oid), fgbg=fus.volume("fgbg", oid),
             fg=fus.volume("fgmask", oid), voxel_size=f32(info["voxel_size"]), truncdist=f32(info["truncdist"]))
    if color:
        v["color"] = fus.volume("color", oid)
    return v


def expected(twin, e, max_res=256, color=False):
    """The restatement of merge_objects(1, 2) on the twin's volumes: the growth, then the device stage through the poses
    the event names; returns (grown, merge_reference.merge(_color)'s tuple, the foreground mask)."""
    from emfusion_amd import ops, pipeline
    prm = twin.params
    d, s = model(twin, 1, color), model(twin, 2, color)
    shapes = {r["id"]: r for r in twin.object_shapes([1, 2])}
    res_d, res_s = d["tsdf"].shape[::-1], s["tsdf"].shape[::-1]
    assert np.array_equal(mr.fg_mask_of(d["fgbg"]), d["fg"]) and np.array_equal(mr.fg_mask_of(s["fgbg"]), s["fg"])
    # grow: destination frame <- source frame, the union, the resize
    R, t = pipeline.absorb_pose(twin.pose(2), twin.pose(1))
    args = (shapes[1]["bounds_vox"], res_d, d["voxel_size"], shapes[2]["bounds_vox"], res_s, s["voxel_size"])
    union = mr.union_np(*args, R, t)
    got = pipeline.merge_union(*args, (R, t))
    assert union[0].tobytes() == got[0].tobytes() and union[1].tobytes() == got[1].tobytes()
    grown = mr.grow(res_d, d["voxel_size"], union[0], union[1], VOL_PAD, max_res)
    Rd, td = twin.pose(1)
    if grown is not None:
        n, offset, centre = grown
        for k in ("tsdf", "weights", "fgbg") + (("color",) if color else ()):
            d[k] = mr.shifted(d[k], n, offset)
        td = td + np.asarray(Rd, f32).reshape(3, 3) @ centre
    assert e["res_before"] == res_d[0] and e["res_after"] == d["tsdf"].shape[0]
    assert np.array_equal(e["dst_R"].reshape(-1), np.asarray(Rd, f32).reshape(-1)) and np.allclose(e["dst_t"], td, atol=1e-6)
    assert all(a.tobytes() == np.asarray(b, f32).tobytes() for a, b in zip((e["src_R"].reshape(-1), e["src_t"]), twin.pose(2)))
    # merge: through the poses as the event holds them (the destination's after the growth)
    R, t = pipeline.absorb_pose((e["dst_R"], e["dst_t"]), (e["src_R"], e["src_t"]))
    Rn, tn = ar.absorb_pose_np(e["dst_R"], e["dst_t"], e["src_R"], e["src_t"])
    assert R.tobytes() == Rn.tobytes() == e["R"].tobytes() and t.tobytes() == tn.tobytes() == e["t"].tobytes()
    box = ops.absorb_box(d["tsdf"].shape[::-1], d["voxel_size"], res_s, s["voxel_size"], (R, t))
    assert box == (e["lo"], e["size"])
    dst = dict(ar.dst_vol(d["tsdf"], d["weights"], d["voxel_size"], d["truncdist"], prm.max_tsdf_weight), fgbg=d["fgbg"])
    src = dict(ar.src_vol(s["tsdf"], s["weights"], s["fg"], s["voxel_size"], s["truncdist"]), fgbg=s["fgbg"])
    if color:
        dst["color"], src["color"] = d["color"], s["color"]
    want = (mr.merge_color if color else mr.merge)(dst, src, (R, t), box)
    mr.check_identities(want[2], want[4])
    return grown, want, mr.fg_mask_of(want[3])


def compare(live, e, want, mask, color=False):
    assert e["record"].tobytes() == want[2].tobytes(), (e["record"], want[2])
    assert e["counts"].tobytes() == want[4].tobytes(), (e["counts"], want[4])
    assert live.volume("tsdf", 1).tobytes() == want[0].tobytes() and live.volume("weights", 1).tobytes() == want[1].tobytes()
    assert live.volume("fgbg", 1).tobytes() == want[3].tobytes() and live.volume("fgmask", 1).tobytes() == mask.tobytes()
    if color:
        assert e["color"].tobytes() == want[6].tobytes() and live.volume("color", 1).tobytes() == want[5].tobytes()
    else:
        assert int(e["color"]["colored"]) == int(e["color"]["uncolored"]) == 0


@pytest.fixture(scope="module")
def split(dev):
    """The live session and its twin through FRAMES frames: the two halves are objects 1 and 2 in both."""
    live, twin = Run(), Run()
    for r in (live, twin):
        for _ in range(FRAMES):
            r.frame()
        assert r.fus.object_ids() == [1, 2] and sorted(r.fus.visible_objects()) == [1, 2]
    assert live.fus.merged() == []
    yield dict(live=live, twin=twin)
    live.close()
    twin.close()


def world_bounds(shape):
    """The corners of an object's band bounds in the world frame: (lo, hi)."""
    lo, hi = shape["bounds_vox"]
    res, R, t = np.asarray(shape["res"], np.float64), shape["pose"][0].astype(np.float64), shape["pose"][1].astype(np.float64)
    pts = []
    for k in range(8):
        v = np.array([(lo, hi)[(k >> j) & 1][j] for j in range(3)], np.float64)
        pts.append(R @ ((v - (res - 1) / 2) * shape["voxel_size"]) + t)
    return np.min(pts, axis=0), np.max(pts, axis=0)


def test_two_halves_of_a_sphere_become_one_object(split):
    live, twin = split["live"].fus, split["twin"].fus
    books = mr.bookkeeping_np(twin.object_bookkeeping(1), twin.object_bookkeeping(2))
    assert live.object_bookkeeping(1)[:2] == twin.object_bookkeeping(1)[:2] and books[0] > twin.object_bookkeeping(1)[0] > 0
    e = live.merge_objects(1, 2)
    assert (e["dst"], e["src"], e["frame"], e["automatic"]) == (1, 2, FRAMES, False) and list(e["overlap"]) == [0.0, 0.0]
    grown, want, mask = expected(twin, e)
    print("grown", grown, "box", e["lo"], e["size"], "clipped", e["clipped"], want[2], want[4])
    assert grown is not None and e["res_after"] > e["res_before"] and not e["clipped"]
    compare(live, e, want, mask)
    assert want[2]["fused"] > want[2]["fresh"] > 0 and want[4]["gained"] > 0
    # the source is gone, the destination keeps its id; the log holds the event; the existence counts are the sums
    assert live.object_ids() == [1] and twin.object_ids() == [1, 2]
    log = live.merged()
    assert len(log) == 1 and all(np.asarray(log[0][k]).tobytes() == np.asarray(e[k]).tobytes() for k in e)
    got = live.object_bookkeeping(1)
    assert got[:2] == books[:2] and got[2].tobytes() == books[2].tobytes()  # the sums of both, scores element-wise
    assert live.object_info(1)["existence"] == np.float32(books[0]) / np.float32(books[0] + books[1])
    with pytest.raises(Exception):
        live.object_info(2)
    # one object whose band covers both halves
    shape = live.object_shapes([1])[0]
    halves = {r["id"]: r for r in twin.object_shapes([1, 2])}
    lo, hi = world_bounds(shape)
    vox = shape["voxel_size"]
    for i in (1, 2):
        hlo, hhi = world_bounds(halves[i])
        print("half", i, hlo, hhi, "merged", lo, hi)
        assert (lo <= hlo + 2 * vox).all() and (hi >= hhi - 2 * vox).all()
    assert shape["solid"] > max(halves[1]["solid"], halves[2]["solid"])
    # the next frames run and raycast the merged object; its pose moved with the volume's centre, as in any resize
    split["live"].centers[1] = live.pose(1)[1]
    for _ in range(2):
        split["live"].frame()
    assert live.object_ids() == [1] and sorted(live.visible_objects()) == [1]
    seg = live.image("segmentation")
    _, sid = split["live"].synth.render(split["live"].f - 1)
    inside = seg[sid == 1]
    print("segmentation under the sphere:", np.unique(inside, return_counts=True))
    assert (inside != 0).mean() > 0.8 and len(np.unique(inside[inside != 0])) == 1


def test_the_cap_leaves_the_destination_and_says_clipped(dev):
    live, twin = Run(), Run()
    try:
        for r in (live, twin):
            for _ in range(FRAMES):
                r.frame()
        live.fus.set_merge_objects(False, max_res=32)  # the parameters are kept with the switch off
        e = live.fus.merge_objects(1, 2)
        grown, want, mask = expected(twin.fus, e, max_res=32)
        assert grown is None and e["res_after"] == e["res_before"] == 32 and e["clipped"]
        compare(live.fus, e, want, mask)
        assert live.fus.object_ids() == [1]
        # reset() empties the log
        live.fus.reset()
        assert live.fus.merged() == []
    finally:
        live.close()
        twin.close()


def test_a_coloured_session_carries_colour_and_a_checkpoint_does_not_depend_on_the_log(dev, tmp_path):
    live, twin = Run(color=True), Run(color=True)
    try:
        for r in (live, twin):
            for _ in range(FRAMES):
                r.frame()
        e = live.fus.merge_objects(1, 2)
        grown, want, mask = expected(twin.fus, e, color=True)
        compare(live.fus, e, want, mask, color=True)
        assert grown is not None and want[6]["colored"] > 0
        # two more frames equal those of a session resumed from a checkpoint, whose log is empty
        live.centers[1] = live.fus.pose(1)[1]  # the pose moved with the volume's centre
        live.fus.save_checkpoint(tmp_path / "merged.ckpt")
        resumed = Run(color=True)
        try:
            resumed.fus.load_checkpoint(tmp_path / "merged.ckpt")
            assert resumed.fus.merged() == [] and resumed.fus.object_ids() == [1]
            resumed.f, resumed.centers = live.f, dict(live.centers)
            for _ in range(2):
                live.frame()
                resumed.frame()
            for which in ("tsdf", "weights", "fgbg", "color"):
                assert live.fus.volume(which, 1).tobytes() == resumed.fus.volume(which, 1).tobytes(), which
            assert live.fus.volume("tsdf", 0).tobytes() == resumed.fus.volume("tsdf", 0).tobytes()
            assert live.fus.image("segmentation").tobytes() == resumed.fus.image("segmentation").tobytes()
        finally:
            resumed.close()
    finally:
        live.close()
        twin.close()


def test_the_refusals(split):
    from emfusion_amd.pipeline import FusionError
    twin = split["twin"].fus
    for dst, src in ((0, 1), (1, 0), (1, 1), (1, 9), (9, 2), (-1, 2)):
        with pytest.raises(FusionError):
            twin.merge_objects(dst, src)
    for bad in (dict(max_res=1), dict(min_overlap=float("nan")), dict(touch=float("nan")), dict(min_surface=-1)):
        with pytest.raises(FusionError):
            twin.set_merge_objects(True, **bad)
    assert twin.merged() == [] and twin.object_ids() == [1, 2]


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.set_merge_objects(True), lambda: fus.merge_objects(1, 2)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        fus.set_merge_objects(False)  # clearing what was never set is no error
        assert fus.merged() == []
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 2, [-4] * 2]


class Twice:
    """One session over the one-sphere stream with the SAME sphere as two objects from the start -- a true duplicate: two
    volumes added at the sphere's place before the first frame (add_object asks no box IoU, as a raised volIOUThresh would
    not), the sphere's mask handed to both on every frame; poses handed in, no tracking, no clean-up."""

    def __init__(self, exp_merged=False):
        from emfusion_amd import pipeline
        self.prm = params()
        self.synth = pipeline.SyntheticStream(W, H, np.array(self.prm.K, f32), 1, seed=0xE3F5)
        self.fus = pipeline.Fusion(self.prm, None)
        self.fus.setup_output(False, False, exp_merged=exp_merged)
        c, _, size = self.synth.sphere(0, 0)
        self.ids = [self.fus.add_object(c, size), self.fus.add_object(c, size)]
        self.center, self.keep, self.f = c, [], 0

    def frame(self):
        from emfusion_amd.ops import image_view
        depth, sid = self.synth.render(self.f)
        R, t = self.synth.camera_pose(self.f)
        d, live = to_dev(depth), self.fus.object_ids()
        masks = {i: to_dev((sid == 1).astype(np.uint8)) for i in live}
        self.keep += [d, masks]
        poses = {i: (np.eye(3, dtype=f32).reshape(-1), self.fus.pose(i)[1]) for i in live}
        self.fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, True)
        self.fus.synchronize()
        self.f += 1

    def close(self):
        self.fus.close()
        self.synth.close()


def probe(fus):
    """{(a, b): (surface, touching)} of the probe the automatic merge runs: all ordered object pairs, no background, half a
    truncation distance."""
    ids = fus.object_ids()
    c = fus.object_contacts(ids=ids, background=False, touch=0.5 * fus.object_info(ids[0])["truncdist"])
    return {(p["a"], p["b"]): (p["surface"], p["touching"]) for p in c["pairs"]}


def test_a_true_duplicate_is_merged_at_the_next_mask_frame_and_abutting_halves_are_not(dev, tmp_path):
    live, twin = Twice(exp_merged=True), Twice()
    try:
        for r in (live, twin):
            for _ in range(2):
                r.frame()
            assert r.fus.object_ids() == [1, 2]
        live.fus.set_merge_objects(True)
        live.frame()
        twin.frame()
        # what decided: the restatement's ordering on the twin's probe after the same frame
        records = probe(twin.fus)
        pairs = mr.merge_pairs_np(records)
        print("probe", records, "pairs", pairs)
        assert pairs == mr.merge_pairs_py(records) and len(pairs) == 1 and pairs[0][:2] == (1, 2)
        log = live.fus.merged()
        assert len(log) == 1 and live.fus.object_ids() == [1] and live.fus.last_deleted() == [2] and twin.fus.object_ids() == [1, 2]
        e = log[0]
        assert (e["dst"], e["src"], e["frame"], e["automatic"]) == (1, 2, 2, True)  # the older id is kept
        assert tuple(e["overlap"]) == pairs[0][2:] and max(e["overlap"]) >= 0.5
        grown, want, mask = expected(twin.fus, e)
        compare(live.fus, e, want, mask)
        assert want[2]["fused"] > 0 and want[2]["fresh"] < want[2]["fused"]
        got, books = live.fus.object_bookkeeping(1), mr.bookkeeping_py(twin.fus.object_bookkeeping(1), twin.fus.object_bookkeeping(2))
        assert got[:2] == books[:2] and list(got[2]) == books[2]
        # the next frame runs with one object and merges nothing more; merged.txt is merged_line of the log
        live.frame()
        assert live.fus.object_ids() == [1] and len(live.fus.merged()) == 1
        from emfusion_amd import pipeline
        live.fus.write_results(tmp_path / "live", volumes=False)
        twin.fus.write_results(tmp_path / "twin", volumes=False)
        lines = (tmp_path / "live" / "merged.txt").read_text().splitlines()
        assert lines[0].startswith("# dst src frame clipped automatic") and lines[1:] == [pipeline.merged_line(e)]
        assert not (tmp_path / "twin" / "merged.txt").exists()
    finally:
        live.close()
        twin.close()
    # two halves that abut: with the default threshold nothing is merged
    halves = Run()
    try:
        halves.fus.set_merge_objects(True)
        for _ in range(FRAMES):
            halves.frame()
        records = probe(halves.fus)
        print("halves", records, {k: mr.overlap_py(*v) for k, v in records.items()})
        assert halves.fus.object_ids() == [1, 2] and halves.fus.merged() == [] and mr.merge_pairs_np(records) == []
    finally:
        halves.close()


def test_the_switch_set_and_cleared_equals_never_set(dev, tmp_path):
    from tests.test_gpu_absorb_pipeline import digest
    a, b = Run(), Run()
    try:
        a.fus.set_merge_objects(True, min_overlap=0.25, max_res=64)
        a.fus.set_merge_objects(False)
        for f in range(FRAMES):
            a.frame()
            b.frame()
            assert digest(a, tmp_path, "a.ckpt") == digest(b, tmp_path, "b.ckpt"), f
        assert a.fus.merged() == [] and a.fus.object_ids() == [1, 2]
    finally:
        a.close()
        b.close()


def test_the_apps_write_merged_txt_only_with_the_switch(dev, tmp_path):
    import subprocess
    import sys
    from tests.test_gpu_frontier_pipeline import APP, ROOT, listing
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = ["--frames", "5", "--objects", "2", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120", "--autonomous"]
    outs, stdout = {}, {}
    for name, extra in (("plain", []), ("merge", ["--merge-objects", "--merge-overlap", "0.4", "--merge-max-res", "128"])):
        p = subprocess.run([str(APP), *small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name], stdout[name] = listing(tmp_path / name), p.stdout
    assert set(outs["merge"]) - set(outs["plain"]) == {"merged.txt"} and set(outs["plain"]) <= set(outs["merge"])
    lines = (tmp_path / "merge" / "merged.txt").read_text().splitlines()
    assert lines[0].startswith("# dst src frame clipped automatic") and all(len(ln.split()) == 69 for ln in lines[1:])
    count = [ln for ln in stdout["merge"].splitlines() if ln.startswith("merged into other objects:")]
    assert len(count) == 1 and int(count[0].split()[4]) == len(lines) - 1
    assert not any(ln.startswith("merged into other objects:") for ln in stdout["plain"].splitlines())
    # refused before any device is touched
    for cmd, word in (([str(APP), "--autonomous", "--merge-objects"], "--out"),
                      ([str(APP), "--merge-objects", "--out", str(tmp_path / "no")], "--autonomous"),
                      ([str(APP), "--autonomous", "--merge-overlap", "0.4", "--out", str(tmp_path / "no")], "--merge-objects"),
                      ([str(APP), "--autonomous", "--merge-max-res", "64", "--out", str(tmp_path / "no")], "--merge-objects")):
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (cmd, p.returncode, p.stderr[-500:])
    assert not (tmp_path / "no").exists()
    # the dataset app takes the same switch
    from tests import tum_staging as T
    seq, masks, _ = T.stage(tmp_path)
    tum = [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]
    p = subprocess.run([*tum, "--out", str(tmp_path / "tum"), "--merge-objects"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert (tmp_path / "tum" / "merged.txt").read_text().startswith("# dst src frame clipped automatic")
    p = subprocess.run([*tum, "--out", str(tmp_path / "tum2"), "--merge-overlap", "0.4"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--merge-objects" in p.stderr
