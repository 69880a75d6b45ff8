"""The background follows the camera (Fusion.set_background_follow).  The stream of
tests/roll_reference.py makes the policy fire at the end of frame 6 (x only) and of frame 9 (y and z together).  A twin
session with follow off replays the same frames and rolls explicitly at those frames: it supplies the volumes and the
mesh just BEFORE each roll, which a following session never shows.
  (i)   the frames after a roll integrate like the oracle continuing from the rolled state
  (ii)  every retired slab is the mesh of the numpy-sliced sub-box as a volume of its own, soup and welded
  (iii) triangles before a roll = the roll's slabs + triangles after it
  (iv)  origins accumulate; write_results writes bg_retired/ in the frame of the initial pose
  (v)   with follow off nothing changes, checkpoint file included
  (vi)  save after a roll, resume, continue: the bytes of the uninterrupted session
  (vii) refused on the sharded path"""
import hashlib

import numpy as np
import pytest

from tests import roll_reference as rr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu
f32 = np.float32


def run(follow=False, explicit=None, weld=False, color=False, first=0, last=rr.FRAMES, fus=None, touch=None):
    """Frames [first, last) on a new session (or on `fus`).  follow: the policy; explicit: {frame: shift} rolled by hand
    at the END of that frame.  Per frame: the volumes, the background pose and origin, the association weights, and
    around an explicit roll the volumes and the mesh before and after it."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    if fus is None:
        fus = pipeline.Fusion(rr.params())
        if color:
            fus.enable_color(True)
        fus.enable_pose_log(True)
        fus.set_mesh_weld(weld)
        if follow:
            fus.set_background_follow(True, step=rr.STEP, look_ahead=rr.LOOK)
        if touch:
            touch(fus)
    log, keep = [], []
    for f in range(first, last):
        d = to_dev(rr.render(f))
        keep.append(d)
        if color:
            c = to_dev(rr.color_image(f))
            keep.append(c)
            fus.set_color_image(image_view(c))
        fus.process_frame(image_view(d), rr.EYE, rr.camera_t(f), {}, {}, False)
        fus.synchronize()
        rec = dict(assoc=fus.image("bg_assoc"))
        if explicit and f in explicit:
            rec["pre"] = dict(tsdf=fus.volume("tsdf", 0), weights=fus.volume("weights", 0), mesh=fus.mesh(0),
                              origin=fus.background_origin())
            if color:
                rec["pre"]["color"] = fus.volume("color", 0)
            fus.roll_background(explicit[f])
            rec["post_mesh"] = fus.mesh(0)
        rec.update(tsdf=fus.volume("tsdf", 0), weights=fus.volume("weights", 0), pose=fus.background_pose(),
                   origin=fus.background_origin(), ray=fus.image("bg_raylengths"))
        log.append(rec)
    return fus, log


@pytest.fixture(scope="module")
def following(dev):
    fus, log = run(follow=True)
    yield fus, log
    fus.close()


@pytest.fixture(scope="module")
def twin(dev):
    fus, log = run(explicit=rr.ROLLS)
    yield fus, log
    fus.close()


def test_policy_fires_as_planned_and_equals_explicit_rolls(following, twin):
    (_, a), (_, b) = following, twin
    origin = np.zeros(3, np.int64)
    for f in range(rr.FRAMES):
        origin += rr.ROLLS.get(f, (0, 0, 0))
        assert a[f]["origin"] == tuple(int(v) for v in origin), f  # (iv) origins accumulate
        assert b[f]["origin"] == a[f]["origin"]
        assert a[f]["tsdf"].tobytes() == b[f]["tsdf"].tobytes() and a[f]["weights"].tobytes() == b[f]["weights"].tobytes(), f
        assert a[f]["pose"][1].tobytes() == b[f]["pose"][1].tobytes() and a[f]["ray"].tobytes() == b[f]["ray"].tobytes(), f
    assert tuple(origin) == (32, 8, -8)
    for f, shift in rr.ROLLS.items():  # the rolled state is the numpy shift at the resize pose
        pre = b[f]["pre"]
        assert a[f]["tsdf"].view(np.uint32).tobytes() == rr.rolled(pre["tsdf"], shift).view(np.uint32).tobytes()
        assert a[f]["weights"].view(np.uint32).tobytes() == rr.rolled(pre["weights"], shift).view(np.uint32).tobytes()
        R, t = a[f - 1]["pose"]
        assert a[f]["pose"][1].tobytes() == rr.rolled_pose_t(R, t, shift, rr.VOX).tobytes()


def test_frames_after_a_roll_integrate_like_the_oracle_from_the_rolled_state(oracle, following):
    """(i) As tests/test_gpu_lifecycle.py does after an object's resize: the oracle's integration of the frame's depth
    with the session's association weights into the previous state, at the shifted pose; equal arrays."""
    _, log = following
    prm = rr.params()
    K = np.array(prm.K, f32)
    trunc = float(f32(f32(prm.bg_rel_truncdist) * f32(rr.VOX)))
    checked = 0
    for roll_frame in rr.ROLLS:
        for f in (roll_frame + 1, roll_frame + 2):
            tsdf, wts = log[f - 1]["tsdf"].copy(), log[f - 1]["weights"].copy()
            Rb, tb = log[f - 1]["pose"]  # no roll at the end of these frames: the pose the frame integrated at
            assert f not in rr.ROLLS and np.array_equal(Rb, np.eye(3, dtype=f32))
            tc = rr.camera_t(f)
            t_oc = (tb + (-tc)).astype(f32)  # camera^-1 * background pose, both rotations the identity
            oracle.update_tsdf(rr.render(f), log[f]["assoc"], tsdf, wts, rr.EYE, t_oc, K, float(f32(rr.VOX)), trunc,
                               float(prm.max_tsdf_weight))
            assert np.array_equal(log[f]["weights"], wts), f
            assert np.array_equal(log[f]["tsdf"], tsdf), f
            checked += 1
    assert checked == 4


def slab_groups(slabs):
    """Slabs by the frame of their roll, in order."""
    out = {}
    for s in slabs:
        out.setdefault(s["frame"], []).append(s)
    return out


@pytest.mark.parametrize("weld", [False, True], ids=["soup", "welded"])
def test_retired_slabs_are_the_meshes_of_the_sliced_boxes(dev, twin, following, weld):
    """(ii) and the layout of the sub-boxes: x first over all y, z, then y over the x that stays, then z."""
    from emfusion_amd import ops
    if weld:
        fus, _ = run(follow=True, weld=True, color=True)
        slabs = fus.retired_slabs(colors=True)
        cfus, ref = run(explicit=rr.ROLLS, color=True)  # the coloured twin: its pre-roll colour volumes
        cfus.close()
    else:
        fus, ref = following[0], twin[1]
        slabs = fus.retired_slabs()
    groups = slab_groups(slabs)
    assert sorted(groups) == sorted(rr.ROLLS)
    for f, shift in rr.ROLLS.items():
        pre = ref[f]["pre"]
        boxes = rr.retired_boxes((rr.BG,) * 3, shift)
        assert len(groups[f]) == len(boxes) == sum(k != 0 for k in shift)
        for s, (lo, size) in zip(groups[f], boxes):
            assert s["origin"] == tuple(o + l for o, l in zip(pre["origin"], lo)) and s["res"] == size
            sl = (slice(lo[2], lo[2] + size[2]), slice(lo[1], lo[1] + size[1]), slice(lo[0], lo[0] + size[0]))
            t, w = to_dev(np.ascontiguousarray(pre["tsdf"][sl])), to_dev(np.ascontiguousarray(pre["weights"][sl]))
            c = to_dev(np.ascontiguousarray(pre["color"][sl])) if weld else None
            want = ops.extract_mesh(t, w, float(f32(rr.VOX)), weld=weld, color=c)
            assert len(want[2]) > 0, (f, lo, size)  # the wall does cross every slab
            assert s["vertices"].tobytes() == want[0].tobytes() and s["normals"].tobytes() == want[1].tobytes()
            assert s["triangles"].tobytes() == want[2].tobytes()
            if weld:
                assert s["colors"].tobytes() == want[3].tobytes() and s["colors"].any()
    if weld:
        fus.close()


def test_triangles_before_a_roll_are_the_slabs_plus_what_stays(twin):
    """(iii) Exactly: the entering region is unobserved, the sub-boxes are disjoint and cover every cube with a
    leaving voxel -- for the two-axis roll as well."""
    fus, log = twin
    groups = slab_groups(fus.retired_slabs())
    for f in rr.ROLLS:
        before, after = len(log[f]["pre"]["mesh"][2]), len(log[f]["post_mesh"][2])
        retired = sum(len(s["triangles"]) for s in groups[f])
        assert retired > 0 and after > 0 and before == retired + after, (f, before, retired, after)


def read_ply(path):
    lines = path.read_text().splitlines()
    end = lines.index("end_header")
    nv = int([l for l in lines[:end] if l.startswith("element vertex")][0].split()[-1])
    return np.array([l.split()[:3] for l in lines[end + 1:end + 1 + nv]], np.float64).reshape(nv, 3)


def test_write_results_writes_the_retired_slabs_in_the_initial_frame(twin, tmp_path):
    """(iv) bg_retired/%04d.ply + origins.txt; every vertex of a slab's file is a vertex of the mesh before its roll,
    both taken to the frame of the initial pose."""
    from scipy.spatial import cKDTree
    fus, log = twin
    fus.write_results(str(tmp_path), volumes=False)
    slabs = fus.retired_slabs()
    rows = np.loadtxt(tmp_path / "bg_retired" / "origins.txt", dtype=np.int64).reshape(-1, 7)
    assert len(rows) == len(slabs) == 3
    for k, s in enumerate(slabs):
        assert tuple(rows[k]) == (s["frame"],) + s["origin"] + s["res"]
    # Tolerance.  Coordinates stay below extent = (96 / 2 + 40) * 0.02 m < 2 m, where float32 values are 2^-23 * 2 apart
    # at most (np.spacing below).  The pre-roll vertex and the slab's vertex are each one rounded interpolation in their
    # own frames (<= 1 spacing each after the offsets are added), the translation is done in double and rounded once
    # (1/2 spacing), and the PLY's "%f" keeps six decimals (1/2 * 1e-6): 3 spacings + 0.5e-6, per axis.
    extent = (rr.BG / 2 + 40) * rr.VOX
    tol = 3 * float(np.spacing(f32(extent))) + 0.5e-6
    assert tol < 1.3e-6
    k = 0
    for f in rr.ROLLS:
        pre = log[f]["pre"]
        world = pre["mesh"][0].astype(np.float64) + np.array(pre["origin"], np.float64) * float(f32(rr.VOX))
        tree = cKDTree(world)
        for s in [s for s in slabs if s["frame"] == f]:
            v = read_ply(tmp_path / "bg_retired" / f"{k:04d}.ply")
            assert len(v) == len(s["vertices"]) > 0
            dist, idx = tree.query(v, p=np.inf)
            assert dist.max() <= tol, (k, dist.max(), tol)
            k += 1
    assert k == 3 and not (tmp_path / "bg_retired" / "0003.ply").exists()


def digest_outputs(fus, log, tmp_path, name):
    h = hashlib.sha256()
    for rec in log:
        for key in ("tsdf", "weights", "ray", "assoc"):
            h.update(rec[key].tobytes())
    out = tmp_path / name
    fus.write_results(str(out), volumes=True)
    for p in sorted(out.rglob("*")):
        if p.is_file():
            h.update(str(p.relative_to(out)).encode() + p.read_bytes())
    ck = tmp_path / (name + ".ckpt")
    fus.save_checkpoint(ck)
    return h.hexdigest(), hashlib.sha256(ck.read_bytes()).hexdigest(), ck


def test_follow_off_changes_nothing(dev, tmp_path):
    """(v) By digest against a session whose setter was never called: outputs, files and the checkpoint, which stays
    version 1."""
    from emfusion_amd import pipeline

    def on_and_off(fus):
        fus.set_background_follow(True, step=rr.STEP, look_ahead=rr.LOOK)
        fus.set_background_follow(False)

    n = 8  # past the frame at which a following session rolls
    plain, plain_log = run(last=n)
    touched, touched_log = run(last=n, touch=on_and_off)
    a, b = digest_outputs(plain, plain_log, tmp_path, "plain"), digest_outputs(touched, touched_log, tmp_path, "touched")
    assert a[0] == b[0] and a[1] == b[1]
    assert not (tmp_path / "plain" / "bg_retired").exists() and not (tmp_path / "touched" / "bg_retired").exists()
    info = pipeline.checkpoint_info(a[2])
    assert info["version"] == 1 and info["background_origin"] == [0, 0, 0]
    assert touched.background_origin() == (0, 0, 0) and touched.retired_slabs() == []
    plain.close()
    touched.close()


def test_save_after_a_roll_resume_and_continue(dev, following, tmp_path):
    """(vi) The resumed session continues with the bytes of the uninterrupted one; checkpoint_info shows the origin."""
    from emfusion_amd import pipeline
    cut = 8  # after the first roll, before the second
    fus, log = run(follow=True, last=cut)
    ck = tmp_path / "rolled.ckpt"
    fus.save_checkpoint(ck)
    fus.close()
    info = pipeline.checkpoint_info(ck)
    assert info["version"] == 2 and info["background_origin"] == [32, 0, 0] and info["retired_slabs"] == 1
    resumed = pipeline.Fusion.from_checkpoint(ck)
    assert resumed.background_origin() == (32, 0, 0) and resumed.frame_index() == cut
    assert resumed.background_pose()[1].tobytes() == log[-1]["pose"][1].tobytes()
    resumed.enable_pose_log(True)
    _, rest = run(first=cut, fus=resumed)  # the follow switch and its parameters came back with the file
    whole = following[1]
    for f in range(cut, rr.FRAMES):
        a, b = rest[f - cut], whole[f]
        assert a["origin"] == b["origin"] and a["pose"][1].tobytes() == b["pose"][1].tobytes(), f
        for key in ("tsdf", "weights", "ray", "assoc"):
            assert a[key].tobytes() == b[key].tobytes(), (f, key)
    want, got = following[0].retired_slabs(), resumed.retired_slabs()
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert (a["frame"], a["origin"], a["res"]) == (b["frame"], b["origin"], b["res"])
        assert a["vertices"].tobytes() == b["vertices"].tobytes() and a["triangles"].tobytes() == b["triangles"].tobytes()
    resumed.close()


def test_refusals(dev):
    """(vii) A communicator of world 2 (thread ranks) refuses the switch and the session goes on; bad steps are refused."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(rr.params(), comm)
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.set_background_follow(True, step=rr.STEP)
        assert err.value.code == -4
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path"):
            fus.roll_background((32, 0, 0))
        fus.set_background_follow(False)  # switching it off is no error anywhere
        ready.wait(timeout=JOIN_S)
        for f in range(2):
            d = to_dev(rr.render(f))
            fus.process_frame(image_view(d), rr.EYE, rr.camera_t(f), {}, {}, False)
            fus.synchronize()
        hits = int((fus.image("bg_raylengths") > 0).sum())
        origin = fus.background_origin()
        fus.close()
        return hits, origin

    for hits, origin in run_ranks(2, body):
        assert hits > rr.W * rr.H // 4 and origin == (0, 0, 0)
    fus = pipeline.Fusion(rr.params())
    for bad in ((48, 8, 8), (32, 12, 8), (32, 8, 0), (-32, 8, 8)):
        with pytest.raises(pipeline.FusionError) as err:
            fus.set_background_follow(True, step=bad)
        assert err.value.code == -4, bad
    fus.close()


def test_an_explicit_roll_retires_only_if_asked(dev):
    """roll_background(shift, keep_retired): False only re-centres, True retires, None follows the session's setting
    (on by default; off after set_background_follow(..., keep_retired=False))."""
    fus, _ = run(last=3)
    fus.roll_background((32, 0, 0), keep_retired=False)
    assert fus.retired_slabs() == [] and fus.background_origin() == (32, 0, 0)
    fus.roll_background((-32, 0, 0), keep_retired=True)
    assert [s["res"] for s in fus.retired_slabs()] == [(33, rr.BG, rr.BG)]
    fus.roll_background((0, 8, 0))
    assert len(fus.retired_slabs()) == 2
    fus.set_background_follow(False, keep_retired=False)
    fus.roll_background((0, -8, 0))
    assert len(fus.retired_slabs()) == 2
    fus.roll_background((0, 0, 8), keep_retired=True)
    assert len(fus.retired_slabs()) == 3 and fus.background_origin() == (0, 0, 8)
    assert all(s["frame"] == 2 for s in fus.retired_slabs())
    fus.close()
