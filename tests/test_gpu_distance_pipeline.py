"""Fusion.distance_field on a live session: a 64^3 background with one object for a few frames.  The
field equals tests/distance_reference.py applied to Fusion.volume(...) and the poses the call reports, byte for byte;
exclude, signed, the camera box, a roll, the outputs of write_results and of apps/emfusion_synth, and the refusal on a
sharded session."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import distance_reference as dr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
APP = ROOT / "apps" / "emfusion_synth"
W, H, BG, VOX, OBJ = 160, 120, 64, 0.04, 32


def params():
    from emfusion_amd import pipeline
    return pipeline.make_params(W, H, BG, VOX, OBJ, visibility_thresh=100, boundary=5)


def new_session(frames=3):
    """The scene of the entry point's smoke run: one moving sphere in front of the synthetic background."""
    from emfusion_amd import devmem, ops, pipeline
    prm = params()
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 1)
    fus = pipeline.Fusion(prm)
    c, _, vs = synth.sphere(0, 0)
    oid = fus.add_object(c, vs)
    for f in range(frames):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        masks = {oid: devmem.DeviceArray.from_numpy((sid == 1).astype(np.uint8))} if f == 0 else {}
        d_depth = devmem.DeviceArray.from_numpy(depth)
        fus.process_frame(ops.image_view(d_depth), R, t, {oid: (np.eye(3, dtype=np.float32), synth.sphere(0, f)[0])},
                          {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
        fus.synchronize()
    synth.close()
    return fus, oid


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def reference(fus, got, site_mask, cap_voxels=0):
    """(classes, d2) of the restatement on the session's volumes, the box and the object poses the call reports."""
    tsdf, wts = fus.volume("tsdf", 0), fus.volume("weights", 0)
    res = tsdf.shape[::-1]
    objs = [(fus.volume("tsdf", i), fus.volume("weights", i), fus.volume("fgmask", i), fus.object_info(i)["voxel_size"], R, t)
            for i, R, t in got["objects"]]
    classes = dr.stamp(dr.classes_of(tsdf, wts, got["box"]), res, got["voxel_size"], got["box"], objs)
    return classes, dr.distance_transform(classes, site_mask, cap_voxels)


def check(fus, got, site_mask=2, cap_voxels=0):
    classes, d2 = reference(fus, got, site_mask, cap_voxels)
    assert got["classes"].tobytes() == classes.tobytes()
    assert got["d2"].tobytes() == d2.tobytes()
    if "metres" in got:
        assert got["metres"].tobytes() == dr.metres_of(d2, got["voxel_size"]).tobytes()
    return classes, d2


def box_pose(fus, lo):
    """The background's pose composed with the box origin, in float64."""
    R, t = fus.background_pose()
    corner = (np.array(lo, np.float64) - (BG - 1) / 2.0) * float(np.float32(VOX))
    return R, t.astype(np.float64) + R.astype(np.float64) @ corner


def test_whole_background_equals_the_reference(session):
    fus, oid = session
    before = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid))
    got = fus.distance_field()
    assert got["box"] == ((0, 0, 0), (BG, BG, BG)) and got["classes"].shape == (BG, BG, BG)
    classes, d2 = check(fus, got)
    assert {0, 1, 2} == set(np.unique(classes)) and (d2 == 0).sum() > 500 and (d2 != dr.FAR).all()
    # the object's pose is object <- background, composed from the two poses the session reports
    (i, R, t), = got["objects"]
    assert i == oid
    Ro, to = fus.pose(oid)
    Rb, tb = fus.background_pose()
    want_R = Ro.astype(np.float64).T @ Rb.astype(np.float64)
    want_t = Ro.astype(np.float64).T @ (tb.astype(np.float64) - to.astype(np.float64))
    assert np.abs(R - want_R).max() < 1e-6 and np.abs(t - want_t).max() < 1e-5
    # the object does add obstacle voxels of its own (few: the background has fused the same sphere from the same depth)
    no_obj = dr.classes_of(before[0], before[1])
    assert ((classes == dr.OCCUPIED) & (no_obj != dr.OCCUPIED)).any()
    Rp, tp = got["pose"]
    wR, wt = box_pose(fus, (0, 0, 0))
    assert Rp.tobytes() == wR.tobytes() and np.abs(tp - wt).max() < 1e-5
    # nothing of the session changed
    after = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert fus.distance_field()["d2"].tobytes() == got["d2"].tobytes()


def test_unknown_as_obstacle_cap_and_no_metres(session):
    fus, _ = session
    got = fus.distance_field(unknown_is_obstacle=True, cap=0.2, metres=False)  # 0.2 m = 5 voxels
    assert "metres" not in got
    _, d2 = check(fus, got, site_mask=6, cap_voxels=5)
    assert (d2 == dr.FAR).any() and d2[d2 != dr.FAR].max() <= 25
    got = fus.distance_field(cap=0.21)  # rounded up to 6 voxels
    check(fus, got, cap_voxels=6)


def test_exclude_removes_the_objects_voxels(session):
    fus, oid = session
    with_obj = fus.distance_field()
    got = fus.distance_field(exclude=(oid,))
    assert got["objects"] == []
    classes, _ = check(fus, got)
    assert classes.tobytes() == dr.classes_of(fus.volume("tsdf", 0), fus.volume("weights", 0)).tobytes()
    differ = with_obj["classes"] != classes
    assert differ.any() and (with_obj["classes"][differ] == dr.OCCUPIED).all() and (with_obj["d2"] <= got["d2"]).all()


def test_signed(session):
    fus, _ = session
    got = fus.distance_field(signed=True)
    classes, d2 = check(fus, got)
    inside = dr.distance_transform(classes, 7 ^ 2)
    assert got["d2_inside"].tobytes() == inside.tobytes()
    m_in = dr.metres_of(inside, got["voxel_size"])
    assert got["metres_inside"].tobytes() == m_in.tobytes()
    want = dr.signed_metres(dr.metres_of(d2, got["voxel_size"]), m_in)
    assert got["signed"].tobytes() == want.tobytes()
    occ = classes == dr.OCCUPIED
    assert (want[occ] < 0).all() and (want[~occ] > 0).all() and want[occ].max() == -np.float32(VOX)


def test_camera_box_is_clipped_at_the_border(session):
    fus, _ = session
    R, t = fus.background_pose()
    q = R.astype(np.float64).T @ (fus.pose(0)[1].astype(np.float64) - t.astype(np.float64))
    centre = np.rint(q / float(np.float32(VOX)) + (BG - 1) / 2.0).astype(int)
    got = fus.distance_field(box="camera", size=24)
    lo, size = got["box"]
    for a in range(3):
        assert lo[a] == max(centre[a] - 12, 0) and lo[a] + size[a] == min(centre[a] + 12, BG)
    assert min(size) >= 1 and min(size) < 24  # the camera stands at the volume's near face: the box is cut there
    assert got["classes"].shape == size[::-1]
    check(fus, got)
    wR, wt = box_pose(fus, lo)
    assert np.abs(got["pose"][1] - wt).max() < 1e-5
    # an explicit box with odd offsets, and the refusals
    check(fus, fus.distance_field(box=((3, 5, 7), (33, 20, 11)), unknown_is_obstacle=True), site_mask=6)
    from emfusion_amd import pipeline
    with pytest.raises(pipeline.FusionError) as err:
        fus.distance_field(box=((40, 0, 0), (25, 8, 8)))
    assert err.value.code == -4
    with pytest.raises(ValueError):
        fus.distance_field(box="camera")


def test_follows_a_roll(dev):
    fus, oid = new_session()
    before = fus.distance_field()
    shift = (8, 0, -8)
    fus.roll_background(shift, keep_retired=False)
    got = fus.distance_field()
    classes, _ = check(fus, got)
    # the contents moved with the roll: voxel v now holds what v + shift held (objects are stamped where they are)
    assert got["classes"][8:, :, :-8].tobytes() == before["classes"][:-8, :, 8:].tobytes()
    wR, wt = box_pose(fus, (0, 0, 0))
    assert np.abs(got["pose"][1] - wt).max() < 1e-5
    moved = got["pose"][1].astype(np.float64) - before["pose"][1].astype(np.float64)
    assert np.abs(moved - got["pose"][0].astype(np.float64) @ (np.array(shift) * float(np.float32(VOX)))).max() < 1e-5
    fus.close()


def read_volume_file(path, dtype):
    raw = Path(path).read_bytes()
    res = np.frombuffer(raw, np.int32, 3, 0)
    elem = int(np.frombuffer(raw, np.uint64, 1, 12)[0])
    voxel = float(np.frombuffer(raw, np.float32, 1, 20)[0])
    assert elem == np.dtype(dtype).itemsize and len(raw) == 24 + elem * int(np.prod(res.astype(np.int64)))
    return np.frombuffer(raw, dtype, offset=24).reshape(res[2], res[1], res[0]), voxel


def listing(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(Path(root).rglob("*")) if p.is_file()}


def test_write_results_writes_the_two_files_only_with_the_switch(dev, tmp_path):
    out = {}
    for on in (False, True):
        fus, _ = new_session()
        if on:
            fus.setup_output(False, False, exp_distance_field=True, distance_cap=0.4)
        else:
            fus.setup_output(False, False)
        fus.write_results(tmp_path / str(on), volumes=False)
        if on:
            got = fus.distance_field(cap=0.4)
        fus.close()
        out[on] = listing(tmp_path / str(on))
    new = set(out[True]) - set(out[False])
    assert new == {"distance.bin", "occupancy.bin"} and set(out[False]) <= set(out[True])
    assert all(out[True][k] == v for k, v in out[False].items())
    metres, voxel = read_volume_file(tmp_path / "True" / "distance.bin", np.float32)
    classes, _ = read_volume_file(tmp_path / "True" / "occupancy.bin", np.uint8)
    assert voxel == np.float32(VOX)
    assert metres.tobytes() == got["metres"].tobytes() and classes.tobytes() == got["classes"].tobytes()


def test_the_app_writes_the_two_files_and_nothing_else_changes(dev, tmp_path):
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = ["--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    outs = {}
    for name, extra in (("plain", []), ("field", ["--distance-field", "--distance-cap", "0.5", "--distance-unknown-obstacle"])):
        p = subprocess.run([str(APP), *small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = listing(tmp_path / name)
    assert set(outs["field"]) - set(outs["plain"]) == {"distance.bin", "occupancy.bin"}
    assert all(outs["field"][k] == v for k, v in outs["plain"].items()) and len(outs["plain"]) > 3
    metres, voxel = read_volume_file(tmp_path / "field" / "distance.bin", np.float32)
    classes, _ = read_volume_file(tmp_path / "field" / "occupancy.bin", np.uint8)
    assert classes.shape == (64, 64, 64) and {0, 1, 2} == set(np.unique(classes))
    cap = int(np.ceil(np.float32(0.5) / np.float32(voxel)))
    assert metres.tobytes() == dr.metres_of(dr.distance_transform(classes, 6, cap), voxel).tobytes()
    tsdf, _ = read_volume_file(tmp_path / "field" / "tsdfs" / "bg_tsdf.bin", np.float32)
    assert (tsdf[classes == dr.FREE] > 0).all()  # an object can only add obstacles


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.distance_field()
        code = err.value.code
        ready.wait(timeout=JOIN_S)
        fus.close()
        return code

    assert list(run_ranks(2, body)) == [-4, -4]
