"""Colour through absorb, seed and release on live sessions, on the round-trip scene of
test_gpu_lift_pipeline.py -- 128^3 background, 32^3 objects, 320 x 240 -- with the colour images of tests/color_scene.py:
two objects are seen, absorbed when the camera turns away, and seen again on a mask frame.  Against twins with the
hand-over switches off (one with both off for the absorptions; one that absorbs but does not lift for the seeds and the
releases, whose background is what the live session's passes started from), as bytes: the background's colour volume after
the absorptions, each new object's colour volume, the background's entries at the released voxels, absorbed_colors() and
lifted_colors(), the vertex colours of mesh(0), absorbed.txt and lifted.txt.  A colourless session with the switches on
against the plain entries called through ops; two more frames after a checkpoint and a resume; the apps."""
import subprocess
import sys

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import color_scene as cs
from tests import lift_reference as lr
from tests import transfer_color_reference as tc
from tests.mesh_color_reference import vertex_colours
from tests.parity_util import to_dev
from tests.test_gpu_absorb_pipeline import BG, H, TURN, W, background, model, params, read_absorbed
from tests.test_gpu_frontier_pipeline import APP, ROOT, listing
from tests.test_gpu_lift_pipeline import BACK, Run, read_lifted, volumes

pytestmark = pytest.mark.gpu

f32 = np.float32


class ColourRun(Run):
    """test_gpu_lift_pipeline.Run with colour on: every frame goes with the seeded RGB noise image of its number."""

    def __init__(self, color=True, **kw):
        super().__init__(**kw)
        self.color = color
        if color:
            self.fus.enable_color()

    def frame(self, **kw):
        from emfusion_amd.ops import image_view
        if self.color:
            rgb = to_dev(cs.rgb_noise(self.f, W, H))
            self.keep.append(rgb)
            self.fus.set_color_image(image_view(rgb))
        super().frame(**kw)


def split_lines(lines, extra):
    """The lines of a coloured session's file: (the line a colourless session writes, the trailing colour counts)."""
    rows = [ln.split() for ln in lines]
    return [" ".join(r[:-extra]) for r in rows], [[int(v) for v in r[-extra:]] for r in rows]


@pytest.fixture(scope="module")
def round_trip(dev, tmp_path_factory):
    live = ColourRun(absorb=True)
    live.fus.setup_output(False, False, exp_absorbed=True, exp_lifted=True)
    absorbing, off = ColourRun(absorb=True), ColourRun(absorb=False)
    runs = (live, absorbing, off)
    for r in runs:
        for _ in range(TURN):
            r.frame()
        assert r.fus.object_ids() == [1, 2]
    sources = []
    for i in (1, 2):  # what the absorptions read: the objects before the frame that loses them
        src, pose = model(live.fus, i)
        sources.append((dict(src, color=live.fus.volume("color", i)), pose))
        assert sources[-1][0]["color"].tobytes() == off.fus.volume("color", i).tobytes()
    _, trunc = background(live.fus)
    for r in runs:
        r.frame(turned=True)
        assert r.fus.object_ids() == []
    after_turn = {k: live.fus.volume(k, 0) for k in ("tsdf", "weights", "color")}
    live.fus.set_lift_objects(True)
    for r in (live, absorbing):
        r.f = BACK
        r.frame(new=True)
    path = tmp_path_factory.mktemp("transfer_color") / "after.ckpt"
    live.fus.save_checkpoint(path)
    yield dict(live=live, absorbing=absorbing, off=off, sources=sources, trunc=trunc, after_turn=after_turn, ckpt=path)
    for r in runs:
        r.close()


def test_absorbed_objects_keep_their_colour(round_trip):
    from emfusion_amd import ops, pipeline
    live, off = round_trip["live"].fus, round_trip["off"].fus
    prm, log, colors = live.params, live.absorbed(), live.absorbed_colors()
    assert [e["id"] for e in log] == [1, 2] and len(colors) == 2 and off.absorbed() == [] and off.absorbed_colors() == []
    bg_pose = off.background_pose()
    tsdf, weights, color = off.volume("tsdf", 0), off.volume("weights", 0), off.volume("color", 0)
    kinds = {}
    for (src, pose), e, crec in zip(round_trip["sources"], log, colors):
        R, t = pipeline.absorb_pose(bg_pose, pose)
        assert R.tobytes() == e["R"].tobytes() and t.tobytes() == e["t"].tobytes()
        box = ops.absorb_box((BG, BG, BG), prm.bg_voxel_size, src["tsdf"].shape[::-1], src["voxel_size"], (R, t))
        assert box == (e["lo"], e["size"])
        dst = dict(ar.dst_vol(tsdf, weights, prm.bg_voxel_size, round_trip["trunc"], prm.max_tsdf_weight), color=color)
        tsdf, weights, rec, color, want = tc.absorb_color(dst, src, (R, t), box, kinds=kinds)
        tc.check_identities(rec, want, "fused")
        print(e["id"], rec, want, crec)
        assert e["record"].tobytes() == rec.tobytes() and crec.dtype == tc.COLOR_MOVED and crec.tobytes() == want.tobytes()
    print(kinds)
    got = round_trip["after_turn"]
    assert got["tsdf"].tobytes() == tsdf.tobytes() and got["weights"].tobytes() == weights.tobytes()
    assert got["color"].tobytes() == color.tobytes()
    moved = (got["color"] != off.volume("color", 0)).any(axis=3)
    assert sum(int(c["colored"]) for c in colors) > 0 and moved.sum() > 0  # the objects' colours are in the background now


def expected_lift(twin, live, events):
    """test_gpu_lift_pipeline.expected with colour: per event the object's (tsdf, weights, record, color, colour
    record) of the seed, and the background's after the releases in the log's order with their records."""
    from emfusion_amd import ops, pipeline
    prm = twin.params
    bg, trunc = background(twin)
    bg_pose = twin.background_pose()
    src = dict(ar.src_vol(bg["tsdf"], bg["weights"], None, prm.bg_voxel_size, trunc), color=twin.volume("color", 0))
    objs, released = {}, []
    tsdf, weights, color = bg["tsdf"], bg["weights"], src["color"]
    for e in events:
        i = e["id"]
        v, pose = volumes(twin, i), twin.pose(i)
        R, t = pipeline.absorb_pose(pose, bg_pose)
        assert R.tobytes() == e["seed_R"].tobytes() and t.tobytes() == e["seed_t"].tobytes()
        dst = dict(ar.dst_vol(v["tsdf"], v["weights"], v["voxel_size"], v["truncdist"], prm.max_tsdf_weight), color=twin.volume("color", i))
        objs[i] = tc.seed_color(dst, src, (R, t))
        tc.check_identities(objs[i][2], objs[i][4], "seeded")
        R, t = pipeline.absorb_pose(bg_pose, pose)
        res = v["tsdf"].shape[::-1]
        box = ops.absorb_box((BG, BG, BG), prm.bg_voxel_size, res, v["voxel_size"], (R, t))
        assert box == (e["lo"], e["size"])
        claim = lr.claim_of(live.volume("fgmask", i), res, v["voxel_size"])
        dst = dict(ar.dst_vol(tsdf, weights, prm.bg_voxel_size, trunc), color=color)
        tsdf, weights, rec, color, crec = tc.release_color(dst, claim, (R, t), box)
        tc.check_identities(rec, crec, "released")
        released.append((rec, crec))
    return objs, (tsdf, weights, color), released


def test_returning_objects_are_seeded_with_colour_and_the_ghost_loses_it(round_trip, tmp_path):
    from emfusion_amd import pipeline
    live, twin = round_trip["live"].fus, round_trip["absorbing"].fus
    ids = live.object_ids()
    assert ids == twin.object_ids() == [3, 4]
    log, colors = live.lifted(), live.lifted_colors()
    assert [e["id"] for e in log] == ids and len(colors) == 2 and twin.lifted_colors() == []
    objs, (tsdf, weights, color), released = expected_lift(twin, live, log)
    for e, pair, (rec, crec) in zip(log, colors, released):
        i = e["id"]
        print(i, objs[i][2], objs[i][4], rec, crec)
        assert e["seed"].tobytes() == objs[i][2].tobytes() and e["release"].tobytes() == rec.tobytes()
        assert pair[0].tobytes() == objs[i][4].tobytes() and pair[1].tobytes() == crec.tobytes()
        assert live.volume("tsdf", i).tobytes() == objs[i][0].tobytes() and live.volume("weights", i).tobytes() == objs[i][1].tobytes()
        assert live.volume("color", i).tobytes() == objs[i][3].tobytes()
        assert objs[i][2]["seeded"] > 0 and rec["released"] > 0
    got = {k: live.volume(k, 0) for k in ("tsdf", "weights", "color")}
    assert got["tsdf"].tobytes() == tsdf.tobytes() and got["weights"].tobytes() == weights.tobytes()
    assert got["color"].tobytes() == color.tobytes()
    # the background's entries at the released voxels are zero where the twin's are not
    gone = got["weights"].view(np.uint32) != twin.volume("weights", 0).view(np.uint32)
    ghost = twin.volume("color", 0)[gone].any(axis=1)
    assert gone.sum() == sum(int(r["released"]) for r, _ in released) and not got["color"][gone].any()
    assert ghost.sum() == sum(int(c["colored"]) for _, c in released)
    assert sum(int(o[4]["colored"]) for o in objs.values()) + int(ghost.sum()) > 0
    # what users look at: the vertex colours of the background's mesh are those of the session's own volumes
    v, n, t, c = live.mesh(0, colors=True)
    want = vertex_colours(got["tsdf"], got["weights"], got["color"])
    assert len(v) == len(want) > 1000 and c.tobytes() == want.tobytes()
    # absorbed.txt and lifted.txt: the line functions with the colour counts, the colourless line in front
    live.write_results(tmp_path / "live", volumes=False)
    lines = (tmp_path / "live" / "absorbed.txt").read_text().splitlines()
    assert lines[0].startswith("# id frame clipped") and "colored uncolored" in lines[0]
    events, acolors = live.absorbed(), live.absorbed_colors()
    assert lines[1:] == [pipeline.absorbed_line(e, color=k) for e, k in zip(events, acolors)] and len(lines) == 3
    plain, counts = split_lines(lines[1:], 2)
    assert plain == [pipeline.absorbed_line(e) for e in events]
    assert counts == [[int(k["colored"]), int(k["uncolored"])] for k in acolors]
    (tmp_path / "plain").mkdir()
    (tmp_path / "plain" / "absorbed.txt").write_text("\n".join([lines[0]] + plain) + "\n")
    read_absorbed(tmp_path / "plain" / "absorbed.txt")  # the shape and the identities of the colourless part
    lines = (tmp_path / "live" / "lifted.txt").read_text().splitlines()
    assert "seed: colored uncolored release: colored uncolored" in lines[0]
    assert lines[1:] == [pipeline.lifted_line(e, color=k) for e, k in zip(log, colors)] and len(lines) == 3
    plain, counts = split_lines(lines[1:], 4)
    assert plain == [pipeline.lifted_line(e) for e in log]
    assert counts == [[int(a["colored"]), int(a["uncolored"]), int(b["colored"]), int(b["uncolored"])] for a, b in colors]
    (tmp_path / "plain" / "lifted.txt").write_text("\n".join([lines[0]] + plain) + "\n")
    read_lifted(tmp_path / "plain" / "lifted.txt")


def test_two_more_frames_equal_those_of_a_resumed_session(round_trip):
    from emfusion_amd import pipeline
    live = round_trip["live"]
    resumed = pipeline.Fusion.from_checkpoint(round_trip["ckpt"])
    try:
        assert resumed.lifted_colors() == [] and resumed.absorbed_colors() == [] and len(live.fus.lifted_colors()) == 2
        other = ColourRun.__new__(ColourRun)
        other.prm, other.synth, other.fus, other.centers, other.sphere, other.keep, other.f, other.color = \
            live.prm, live.synth, resumed, dict(live.centers), dict(live.sphere), [], live.f, True
        for _ in range(2):
            f = live.f
            live.frame()
            other.f = f
            other.frame()
            for i in [0] + live.fus.object_ids():
                for which in ("tsdf", "weights", "color"):
                    assert live.fus.volume(which, i).tobytes() == resumed.volume(which, i).tobytes(), (f, which, i)
        assert live.fus.object_ids() == resumed.object_ids() == [3, 4]
    finally:
        resumed.close()


def test_a_colourless_session_calls_the_plain_entries(dev, tmp_path):
    """Colour off, both switches on: the session is the parent's -- its volumes are those the plain entries give through
    ops on the twin's volumes, the colour counts are zero and the files have no new field."""
    from emfusion_amd import ops, pipeline
    live, twin = ColourRun(color=False, absorb=True), ColourRun(color=False, absorb=False)
    try:
        live.fus.setup_output(False, False, exp_absorbed=True, exp_lifted=True)
        live.fus.set_lift_objects(True)
        twin.fus.set_lift_objects(True)
        for r in (live, twin):
            for _ in range(TURN):
                r.frame()
        sources = [model(live.fus, i) for i in (1, 2)]
        _, trunc = background(live.fus)
        for r in (live, twin):
            r.frame(turned=True)
        prm, log = live.fus.params, live.fus.absorbed()
        assert [e["id"] for e in log] == [1, 2] and len(live.fus.lifted()) == 2  # the objects of frame 0 were lifted
        d_bg = dict(tsdf=to_dev(twin.fus.volume("tsdf", 0)), weights=to_dev(twin.fus.volume("weights", 0)), voxel_size=prm.bg_voxel_size,
                    truncdist=trunc, max_weight=prm.max_tsdf_weight)
        for (src, pose), e in zip(sources, log):
            d_src = dict(tsdf=to_dev(src["tsdf"]), weights=to_dev(src["weights"]), fg_mask=to_dev(src["fg"]), voxel_size=src["voxel_size"],
                         truncdist=src["truncdist"])
            rec = ops.absorb_volume(d_bg, d_src, (e["R"].reshape(9), e["t"]), box=(e["lo"], e["size"]))
            assert rec.tobytes() == e["record"].tobytes() and rec["fused"] > 0
        assert live.fus.volume("tsdf", 0).tobytes() == d_bg["tsdf"].numpy().tobytes()
        assert live.fus.volume("weights", 0).tobytes() == d_bg["weights"].numpy().tobytes()
        zero = tc.moved().tobytes()
        assert [c.tobytes() for c in live.fus.absorbed_colors()] == [zero] * 2
        assert [a.tobytes() + b.tobytes() for a, b in live.fus.lifted_colors()] == [zero * 2] * 2
        live.fus.write_results(tmp_path / "out", volumes=False)
        assert read_absorbed(tmp_path / "out" / "absorbed.txt") == [pipeline.absorbed_line(e) for e in log]
        assert read_lifted(tmp_path / "out" / "lifted.txt") == [pipeline.lifted_line(e) for e in live.fus.lifted()]
        assert "colored" not in (tmp_path / "out" / "absorbed.txt").read_text() + (tmp_path / "out" / "lifted.txt").read_text()
    finally:
        live.close()
        twin.close()


def test_the_apps_run_in_colour_with_the_switches(dev, tmp_path):
    """--color with --absorb-objects and --lift-objects is the feature: no new flag.  Both apps on the staged sequence with
    RGB images of test_gpu_voxel_color_app.py (the synthetic stream has no colour images); the comment lines name the
    colour counts and every event line parses, the colourless part by the readers of the colourless tests."""
    from tests.test_gpu_voxel_color_app import _stage_with_colour
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    T, seq, masks, _ = _stage_with_colour(tmp_path)
    switches = ["--color", "--absorb-objects", "--lift-objects"]
    for name, cmd in (("synth", [str(APP), "--sequence", seq, "--masks", masks]),
                      ("tum", [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks)])):
        p = subprocess.run([*cmd, "--out", str(tmp_path / name), *switches, *T.SMALL], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        events = 0
        for file, fields, read in (("absorbed.txt", 2, read_absorbed), ("lifted.txt", 4, read_lifted)):
            lines = (tmp_path / name / file).read_text().splitlines()
            assert "colored uncolored" in lines[0], (name, file)
            plain, counts = split_lines(lines[1:], fields)
            (tmp_path / name / file).write_text("\n".join([lines[0]] + plain) + "\n")
            for row, c in zip((ln.split() for ln in read(tmp_path / name / file)), counts):
                if fields == 2:
                    assert c[0] + c[1] == int(row[14])  # colored + uncolored == fused
                else:
                    assert c[0] + c[1] == int(row[15]) and c[2] + c[3] == int(row[28])  # == seeded, == released
                events += 1
        print(name, "events", events)  # whether an object is created or leaves view is the sequence's business
