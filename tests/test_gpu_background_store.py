"""The background store in a session (Fusion.set_background_store): what rolls out of the background
comes back when the camera does.  tests/store_reference.py restates the spill, the fill and the store in numpy; its
stream walks out along x until the policy rolls by +32 (end of frame 6) and back until it rolls by -32 (end of frame
12).  A twin session with follow off rolls explicitly at those frames and shows the volumes just before each roll.
Everything is compared as bytes."""
import hashlib
import os

import numpy as np
import pytest

from tests import roll_reference as rr
from tests import store_reference as sr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu
f32 = np.float32
OUT, BACK = (32, 8, -8), (-32, -8, 8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype).tobytes()


def volumes(fus, color):
    return (fus.volume("tsdf", 0), fus.volume("weights", 0)) + ((fus.volume("color", 0),) if color else (None,))


def new_session(store=True, budget=None, follow=False, color=False, touch=None):
    from emfusion_amd import pipeline
    fus = pipeline.Fusion(rr.params())
    if color:
        fus.enable_color(True)
    fus.enable_pose_log(True)
    if follow:
        fus.set_background_follow(True, step=rr.STEP, look_ahead=rr.LOOK)
    if store:
        fus.set_background_store(True) if budget is None else fus.set_background_store(True, max_bytes=budget)
    if touch:
        touch(fus)
    return fus


def frames(fus, first, last, color=False, explicit=None, camera=sr.camera_t, render=sr.render):
    """Frames [first, last) of the out-and-back stream; explicit: {frame: shift} rolled by hand at the END of that
    frame.  Per frame: volumes, pose, origin, ray lengths, association weights, store counters, and around an explicit
    roll the volumes before it."""
    from emfusion_amd.ops import image_view
    log, keep = [], []
    for f in range(first, last):
        d = to_dev(render(f))
        keep.append(d)
        if color:
            c = to_dev(rr.color_image(f))
            keep.append(c)
            fus.set_color_image(image_view(c))
        fus.process_frame(image_view(d), rr.EYE, camera(f), {}, {}, False)
        fus.synchronize()
        rec = dict(assoc=fus.image("bg_assoc"))
        if explicit and f in explicit:
            rec["pre"] = volumes(fus, color)
            fus.roll_background(explicit[f])
        t, w, c = volumes(fus, color)
        rec.update(tsdf=t, weights=w, color=c, pose=fus.background_pose(), origin=fus.background_origin(),
                   ray=fus.image("bg_raylengths"), info=fus.background_store_info())
        log.append(rec)
    return log


# ---- round trip ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_a_roll_out_and_back_returns_the_bytes(dev, color):
    """A few frames, roll_background((32, 8, -8)), then (-32, -8, 8): with the store on the volumes equal the bytes
    before the first roll; with it off the returned region is zeros (today's behaviour: this test fails without the
    store)."""
    got = {}
    for store in (True, False):
        fus = new_session(store=store, color=color)
        frames(fus, 0, 3, color=color, camera=rr.camera_t, render=rr.render)
        before = volumes(fus, color)
        assert (before[1] > 0).sum() > 1000
        pose0 = fus.background_pose()
        fus.roll_background(OUT)
        mid = fus.background_store_info()
        fus.roll_background(BACK)
        got[store] = (before, volumes(fus, color), mid, fus.background_store_info(), pose0, fus.background_pose(),
                      fus.background_origin(), len(fus.retired_slabs()))
        fus.close()
    before, after, mid, info, pose0, pose1, origin, slabs = got[True]
    for a, b in zip(before, after):
        if a is not None:
            assert bits(a) == bits(b)
    assert origin == (0, 0, 0) and pose1[0].tobytes() == pose0[0].tobytes()
    # the restatement: what the first roll spills, what the second restores, and nothing left that belongs inside
    store = sr.DictStore()
    a = sr.roll_with_store(store, before[0], before[1], before[2], (0, 0, 0), OUT)
    assert mid == store.info() and mid["tiles_held"] == mid["tiles_spilled"] > 0 and mid["tiles_restored"] == 0
    b = sr.roll_with_store(store, a[0], a[1], a[2], OUT, BACK)
    assert bits(b[0]) == bits(before[0]) and bits(b[1]) == bits(before[1])
    assert info == store.info() and info["tiles_restored"] == mid["tiles_spilled"] and info["tiles_evicted"] == 0
    nt = sr.tiles_of((rr.BG,) * 3)
    assert all(not all(0 <= k[i] < nt[i] for i in range(3)) for k in store.tiles)  # lattice origin (0, 0, 0) again
    assert info["tiles_held"] == len(store.tiles)
    assert slabs == 6  # the log is chronological: three slabs out, three slabs back
    # store off: the region that returned is zeros, the part that stayed is what it was
    before, after = got[False][0], got[False][1]
    want = rr.rolled(rr.rolled(before[0], OUT), BACK), rr.rolled(rr.rolled(before[1], OUT), BACK)
    assert bits(after[0]) == bits(want[0]) and bits(after[1]) == bits(want[1]) and bits(after[1]) != bits(before[1])
    assert got[False][3] == dict(tiles_held=0, bytes_held=0, tiles_spilled=0, tiles_restored=0, tiles_evicted=0)


# ---- the policy on the out-and-back stream -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def following(dev):
    fus = new_session(follow=True)
    log = frames(fus, 0, sr.FRAMES)
    yield fus, log
    fus.close()


@pytest.fixture(scope="module")
def twin(dev):
    """Follow off, store on, the policy's rolls by hand: the volumes just before each roll."""
    fus = new_session()
    log = frames(fus, 0, sr.FRAMES, explicit=sr.ROLLS)
    yield fus, log
    fus.close()


def test_the_policy_fires_both_ways_and_every_roll_equals_the_restatement(following, twin):
    (_, a), (_, b) = following, twin
    origin, store = np.zeros(3, np.int64), sr.DictStore()
    for f in range(sr.FRAMES):
        if f in sr.ROLLS:
            pre = b[f]["pre"]
            want = sr.roll_with_store(store, pre[0], pre[1], None, tuple(int(v) for v in origin), sr.ROLLS[f])
            assert bits(a[f]["tsdf"]) == bits(want[0]) and bits(a[f]["weights"]) == bits(want[1]), f
            assert a[f]["info"] == store.info(), f
            origin += sr.ROLLS[f]
        assert a[f]["origin"] == b[f]["origin"] == tuple(int(v) for v in origin), f
        assert bits(a[f]["tsdf"]) == bits(b[f]["tsdf"]) and bits(a[f]["weights"]) == bits(b[f]["weights"]), f
        assert a[f]["ray"].tobytes() == b[f]["ray"].tobytes() and a[f]["info"] == b[f]["info"], f
    assert tuple(origin) == (0, 0, 0)
    info = a[-1]["info"]
    assert info["tiles_restored"] > 0 and info["tiles_evicted"] == 0
    # the low-x slab that left at frame 6 is back: the returned region holds observed voxels
    assert (a[12]["weights"][:, :, :32] > 0).sum() > 1000
    assert not (rr.rolled(b[12]["pre"][1], sr.ROLLS[12])[:, :, :32] > 0).any()  # which a roll alone leaves empty


def test_frames_after_the_return_integrate_like_the_oracle_from_the_restored_state(oracle, following):
    """As test_frames_after_a_roll_integrate_like_the_oracle_from_the_rolled_state: the oracle's integration of the
    frame's depth with the session's association weights into the previous (restored) state; equal arrays."""
    _, log = following
    prm = rr.params()
    K = np.array(prm.K, f32)
    trunc = float(f32(f32(prm.bg_rel_truncdist) * f32(rr.VOX)))
    for f in (13, 14):
        tsdf, wts = log[f - 1]["tsdf"].copy(), log[f - 1]["weights"].copy()
        Rb, tb = log[f - 1]["pose"]
        assert f not in sr.ROLLS and np.array_equal(Rb, np.eye(3, dtype=f32))
        t_oc = (tb + (-sr.camera_t(f))).astype(f32)
        oracle.update_tsdf(sr.render(f), log[f]["assoc"], tsdf, wts, rr.EYE, t_oc, K, float(f32(rr.VOX)), trunc,
                           float(prm.max_tsdf_weight))
        assert np.array_equal(log[f]["weights"], wts), f
        assert np.array_equal(log[f]["tsdf"], tsdf), f


def test_the_frame_after_the_return_hits_the_restored_wall(oracle, following, twin):
    """The raycast of the frame after the return (13) against that of the frame before the outward roll (6).  The count
    asserted on: pixels whose ray hits (ray length > 0) at a world x in [-0.96, -0.32) -- the low-x slab of the volume
    at origin 0 (voxels 0 .. 31 of 96 at 0.02 m, centred on x = 0), the region that leaves at the end of frame 6 and
    returns at the end of frame 12; a hit's world x is the camera's x plus ray length times the pixel's unit
    direction.  hits(13) >= hits(6) > 0, first on the restatement -- the oracle's raycast of the numpy volumes, the
    one frame 6 sees and the restated roll-and-fill at the end of frame 12 -- then on the session's own ray lengths."""
    (_, a), (_, b) = following, twin
    prm = rr.params()
    K = np.array(prm.K, f32)
    trunc = float(f32(f32(prm.bg_rel_truncdist) * f32(rr.VOX)))
    Kd = K.astype(np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(rr.W), np.arange(rr.H))
    d = np.stack([(xs - Kd[0, 2]) / Kd[0, 0], (ys - Kd[1, 2]) / Kd[1, 1], np.ones(xs.shape)], axis=2)
    d /= np.linalg.norm(d, axis=2, keepdims=True)

    def hits(ray, f):
        x = float(sr.camera_t(f)[0]) + ray.astype(np.float64) * d[:, :, 0]
        return int(((ray > 0) & (x >= -0.96) & (x < -0.32)).sum())

    def restated(tsdf, wts, f, bg_t):
        t_co = (sr.camera_t(f) + (-bg_t)).astype(f32)  # background pose^-1 * camera, both rotations the identity
        return oracle.raycast_tsdf(tsdf, None, wts, None, rr.W, rr.H, rr.EYE, t_co, K, float(f32(rr.VOX)), trunc)[0]

    store = sr.DictStore()
    pre6, pre12 = b[6]["pre"], b[12]["pre"]
    sr.roll_with_store(store, pre6[0], pre6[1], None, (0, 0, 0), sr.ROLLS[6])
    back = sr.roll_with_store(store, pre12[0], pre12[1], None, (32, 0, 0), sr.ROLLS[12])
    assert b[5]["origin"] == b[12]["origin"] == (0, 0, 0)
    r6 = hits(restated(b[5]["tsdf"], b[5]["weights"], 6, b[5]["pose"][1]), 6)      # what frame 6 is given to raycast
    r13 = hits(restated(back[0], back[1], 13, b[12]["pose"][1]), 13)               # what frame 13 is given
    bare = rr.rolled(pre12[0], sr.ROLLS[12]), rr.rolled(pre12[1], sr.ROLLS[12])
    assert r13 >= r6 > 0, (r6, r13)
    assert hits(restated(bare[0], bare[1], 13, b[12]["pose"][1]), 13) < r6  # a roll alone does not get there
    h6, h13 = hits(a[6]["ray"], 6), hits(a[13]["ray"], 13)
    assert h13 >= h6 > 0, (h6, h13)


# ---- the maps --------------------------------------------------------------------------------------------------------

def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("env", [{"EMF_UNSEEN_TILES": "0", "EMF_FAR_BOUNDS": "0"}, {"EMF_BG_OVERLAP": "0"}],
                         ids=["blind", "in-place"])
def test_restored_map_entries_serve_the_frames_like_no_maps_at_all(dev, following, env):
    """A wrong restored entry shows in the frames after the return: a seen tile called unseen is integrated as a first
    sample, a tile without its sign drops out of the relevant-tile list and the far bounds stop rays in front of it.
    A session that uses neither the unseen maps nor the far bounds cannot see the maps, and one that keeps the
    background once rebuilds nothing out of place: equal volumes, ray lengths and association weights after every step."""
    def session():
        fus = new_session(follow=True)
        try:
            return frames(fus, 0, sr.FRAMES)
        finally:
            fus.close()

    other = with_env(env, session)
    _, log = following
    for f, (a, b) in enumerate(zip(log, other)):
        for key in ("tsdf", "weights", "ray", "assoc"):
            assert a[key].tobytes() == b[key].tobytes(), (f, key)
        assert a["origin"] == b["origin"] and a["info"] == b["info"], f


# ---- the budget --------------------------------------------------------------------------------------------------------

def test_a_budget_below_the_second_spill_evicts_the_first(dev):
    """Two rolls out, (32, 0, 0) then (0, 8, 0), with a budget that holds either spill but not both: the first spill is
    evicted when the second arrives.  On the way back the y slab returns exactly and the x slab returns as zeros."""
    probe = new_session()
    frames(probe, 0, 3, camera=rr.camera_t, render=rr.render)
    before = volumes(probe, False)
    probe.close()
    ref = sr.DictStore()
    a = sr.roll_with_store(ref, before[0], before[1], None, (0, 0, 0), (32, 0, 0))
    first = ref.bytes_held
    b = sr.roll_with_store(ref, a[0], a[1], None, (32, 0, 0), (0, 8, 0))
    second = ref.bytes_held - first
    assert first > 0 and second > 0
    budget = max(first, second) + 1
    assert budget < first + second

    store = sr.DictStore(budget=budget)
    fus = new_session(budget=budget)
    frames(fus, 0, 3, camera=rr.camera_t, render=rr.render)
    vols, origin = volumes(fus, False), (0, 0, 0)
    assert bits(vols[0]) == bits(before[0])
    for shift in ((32, 0, 0), (0, 8, 0), (0, -8, 0), (-32, 0, 0)):
        vols = sr.roll_with_store(store, vols[0], vols[1], None, origin, shift)
        origin = tuple(o + s for o, s in zip(origin, shift))
        fus.roll_background(shift)
        got = volumes(fus, False)
        assert bits(got[0]) == bits(vols[0]) and bits(got[1]) == bits(vols[1]), shift
        assert fus.background_store_info() == store.info(), shift
    info = fus.background_store_info()
    fus.close()
    assert info["tiles_evicted"] > 0 and info["tiles_restored"] > 0
    # the evicted x slab is zeros; everything else is what it was
    assert not vols[1][:, :, :32].view(np.uint32).any() and (before[1][:, :, :32] > 0).any()
    assert bits(vols[0][:, :, 32:]) == bits(before[0][:, :, 32:]) and bits(vols[1][:, :, 32:]) == bits(before[1][:, :, 32:])


# ---- store off changes nothing -------------------------------------------------------------------------------------

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


def test_store_off_changes_nothing(dev, tmp_path):
    """As test_follow_off_changes_nothing: a following session whose store setter was never called against one that
    switched the store on and off again before the first frame -- volumes, images, result files and the checkpoint,
    which stays version 2."""
    from emfusion_amd import pipeline

    def on_and_off(fus):
        fus.set_background_store(True, max_bytes=1 << 20)
        fus.set_background_store(False)

    n = 9  # past the outward roll
    plain = new_session(store=False, follow=True)
    plain_log = frames(plain, 0, n)
    touched = new_session(store=False, follow=True, touch=on_and_off)
    touched_log = frames(touched, 0, n)
    a, b = digest_outputs(plain, plain_log, tmp_path, "plain"), digest_outputs(touched, touched_log, tmp_path, "touched")
    assert a[0] == b[0] and a[1] == b[1]
    info = pipeline.checkpoint_info(a[2])
    assert info["version"] == 2 and info["background_origin"] == [32, 0, 0] and info["stored_tiles"] == 0
    assert touched.background_store_info()["tiles_spilled"] == 0
    plain.close()
    touched.close()
    never = new_session(store=False)
    frames(never, 0, 2)
    ck = tmp_path / "never.ckpt"
    never.save_checkpoint(ck)
    never.close()
    assert pipeline.checkpoint_info(ck)["version"] == 1


# ---- checkpoint ------------------------------------------------------------------------------------------------------

def test_save_after_the_outward_roll_resume_and_return(dev, following, tmp_path):
    from emfusion_amd import pipeline
    cut = 9  # after the outward roll, before the return
    fus = new_session(follow=True)
    log = frames(fus, 0, cut)
    ck = tmp_path / "stored.ckpt"
    fus.save_checkpoint(ck)
    held = fus.background_store_info()
    fus.close()
    info = pipeline.checkpoint_info(ck)
    assert info["version"] == 3 and info["background_origin"] == [32, 0, 0]
    assert info["stored_tiles"] == held["tiles_held"] > 0 and info["stored_bytes"] == held["bytes_held"]
    resumed = pipeline.Fusion.from_checkpoint(ck)
    assert resumed.background_store_info() == held and resumed.background_origin() == (32, 0, 0)
    # damaged files are refused with the session untouched: the file cut short, and a tile section longer than its tiles
    good = ck.read_bytes()
    at = good.rindex(b"TILE")
    n = int.from_bytes(good[at + 16:at + 24], "little")
    assert at + 24 + n + 24 == len(good)  # the section, then the end marker
    longer = good[:at + 16] + (n + 8).to_bytes(8, "little") + good[at + 24:at + 24 + n] + bytes(8) + good[at + 24 + n:]
    state = volumes(resumed, False)
    for name, data in (("cut", good[:-4096]), ("longer", longer)):
        bad = tmp_path / (name + ".ckpt")
        bad.write_bytes(data)
        with pytest.raises(pipeline.FusionError) as err:
            resumed.load_checkpoint(bad)
        assert err.value.code == -4, name
        now = volumes(resumed, False)
        assert bits(now[0]) == bits(state[0]) and bits(now[1]) == bits(state[1]), name
        assert resumed.background_store_info() == held and resumed.background_origin() == (32, 0, 0), name
    resumed.enable_pose_log(True)
    rest = frames(resumed, cut, sr.FRAMES)  # the follow and store switches came back with the file
    whole = following[1]
    for f in range(cut, sr.FRAMES):
        a, b = rest[f - cut], whole[f]
        assert a["origin"] == b["origin"] and a["pose"][1].tobytes() == b["pose"][1].tobytes() and a["info"] == b["info"], f
        for key in ("tsdf", "weights", "ray", "assoc"):
            assert a[key].tobytes() == b[key].tobytes(), (f, key)
    # and the two sessions write the same checkpoint at the end
    end_a, end_b = tmp_path / "a.ckpt", tmp_path / "b.ckpt"
    resumed.save_checkpoint(end_a)
    following[0].save_checkpoint(end_b)
    assert end_a.read_bytes() == end_b.read_bytes()
    resumed.close()


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_refusals(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(rr.params(), comm)
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.set_background_store(True)
        assert err.value.code == -4
        fus.set_background_store(False)  # switching it off is no error anywhere
        ready.wait(timeout=JOIN_S)
        info = fus.background_store_info()
        fus.close()
        return info

    for info in run_ranks(2, body):
        assert info["tiles_held"] == 0
    # a shift that is no tile multiple, with the store on: refused before anything changes
    fus = new_session()
    frames(fus, 0, 2, camera=rr.camera_t, render=rr.render)
    before, pose = volumes(fus, False), fus.background_pose()
    with pytest.raises(pipeline.FusionError, match="multiples of the tile") as err:
        fus.roll_background((3, -5, 2))
    assert err.value.code == -4
    after = volumes(fus, False)
    assert bits(after[0]) == bits(before[0]) and bits(after[1]) == bits(before[1])
    assert fus.background_origin() == (0, 0, 0) and fus.retired_slabs() == []
    assert fus.background_pose()[1].tobytes() == pose[1].tobytes()
    assert fus.background_store_info()["tiles_spilled"] == 0
    fus.set_background_store(False)
    fus.roll_background((3, -5, 2))  # with the store off any shift rolls, as before
    assert fus.background_origin() == (3, -5, 2)
    fus.close()


def test_the_apps_refuse_the_store_without_follow(dev):
    """--follow-store without --follow-camera: both apps say so and stop before they open a device."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    for cmd in ([sys.executable, str(root / "apps" / "run_tum.py"), "no-such-sequence", "--follow-store"],
                [str(root / "apps" / "emfusion_synth"), "--follow-store"]):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (cmd, p.stderr)
        assert "--follow-store needs --follow-camera" in p.stderr, (cmd, p.stderr)
