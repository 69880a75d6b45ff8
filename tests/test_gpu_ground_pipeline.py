"""Fusion.ground_map and Fusion.ground_plan on a live session: the 64^3 background with one object the
frontier pipeline test uses, looked at with "up" towards the camera so that the wall the camera sees is the floor.
ground_map() equals tests/ground_reference.py applied to the classes Fusion.distance_field() reports for the same box,
with the object stamped and with it excluded, byte for byte, under the frame pipeline.ground_frame restates; ground_plan()
equals tests/plan_reference.py and tests/frontier_reference.py run on the returned 2-D classes; the world points equal
the numpy frame exactly; write_results writes ground.bin and ground.txt only with the switch and changes no other byte;
the sharded path refuses; a checkpoint written after the calls equals one written without them."""
import hashlib

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import frontier_reference as fr
from tests import ground_reference as rf
from tests import plan_reference as pl
from tests.test_gpu_frontier_pipeline import BG, VOX, listing, new_session, params

pytestmark = pytest.mark.gpu

WALL = dict(up=(0.0, 0.0, -1.0), band=(-3.0, 0.2), robot_height=0.2, max_step=0.1)  # the wall in front of the camera as floor
TILTED = dict(up=(0.1, -0.2, -1.0), band=(-3.0, 0.2), robot_height=0.2, max_step=0.1)


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def check_map(fus, got, exclude=(), **kw):
    """got = fus.ground_map(exclude=exclude, **kw) against the restatement on the classes of distance_field()."""
    from emfusion_amd import pipeline
    df = fus.distance_field(box=got["box"], exclude=exclude, metres=False)
    classes = df["classes"]
    vs = float(np.float32(VOX))
    bg_R, bg_t = fus.background_pose()
    cell, bin = kw.get("cell", 2.0 * vs), kw.get("bin", 2.0 * vs)
    up = kw.get("up", -bg_R[:, 1].astype(np.float64))
    ref = kw.get("reference", fus.pose(0)[1].astype(np.float64))
    band = kw.get("band", (-1.5, 0.5))
    assert got["cell"] == cell and got["bin"] == bin and got["band"] == tuple(float(v) for v in band)
    args = (got["box"][0], got["box"][1], (BG, BG, BG), VOX, bg_R, bg_t, up, cell, bin, ref, band)
    G, W, H, B, pose = rf.frame(*args)
    theirs = pipeline.ground_frame(*args)
    assert theirs[0].tobytes() == G.tobytes() and theirs[1:4] == (W, H, B) and theirs[4].tobytes() == pose.tobytes()
    assert got["frame"][0].dtype == np.float32 and got["frame"][0].tobytes() == G.tobytes() and got["frame"][1:] == (W, H, B)
    assert got["ground_pose"].dtype == np.float64 and got["ground_pose"].tobytes() == pose.tobytes()
    robot, step = pipeline.ground_bins(kw.get("robot_height", 0.3), kw.get("max_step", 0.05), bin)
    assert (got["robot_bins"], got["max_step_bins"]) == (robot, step)
    occ, fre, cells, classes2d = rf.ground_map(classes, G, W, H, B, robot, step)
    assert got["cells"].dtype == rf.CELL_DTYPE and got["cells"].tobytes() == cells.tobytes()
    assert got["classes"].dtype == np.uint8 and got["classes"].shape == (H, W) and got["classes"].tobytes() == classes2d.tobytes()
    for key in ("floor", "top", "clear", "levels"):
        assert got[key].dtype == np.int16 and got[key].tobytes() == np.ascontiguousarray(cells[key]).tobytes()
    has = cells["floor"] >= 0
    want_h = np.where(has, np.float64(band[0]) + (cells["floor"].astype(np.float64) + 1.0) * np.float64(bin), np.nan).astype(np.float32)
    assert got["height_m"].dtype == np.float32 and got["height_m"].tobytes() == want_h.tobytes()
    # the world points: the numpy frame, exactly
    v, u = np.nonzero(np.ones((H, W), bool))
    ch = np.where(has[v, u], (cells["floor"][v, u].astype(np.float64) + 1.0) * np.float64(bin), np.nan)
    want = rf.ground_point(pose, (u + 0.5) * np.float64(cell), (v + 0.5) * np.float64(cell), ch).astype(np.float32)
    pts = got["cell_world"](u, v)
    assert pts.dtype == np.float32 and pts.shape == (H * W, 3) and pts.tobytes() == want.tobytes()
    assert np.isnan(got["cell_world"]([-1, W], [0, 0])).all()
    return classes, (G, W, H, B, pose), cells, classes2d


def test_ground_map_equals_the_restatement(session):
    fus, oid = session
    before = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    got = fus.ground_map(**WALL)
    assert got["box"] == ((0, 0, 0), (BG, BG, BG))
    classes, frame, cells, classes2d = check_map(fus, got, **WALL)
    # the wall is a floor one can drive on, and the object stands on it as an obstacle
    assert (classes2d == rf.FREE).sum() > 300 and (classes2d == rf.OCCUPIED).sum() > 50 and (cells["levels"] > 1).any()
    # with the object excluded the map differs, and equals the restatement again
    bare = fus.ground_map(exclude=[oid], **WALL)
    check_map(fus, bare, exclude=[oid], **WALL)
    assert bare["cells"].tobytes() != got["cells"].tobytes() and (bare["top"] <= got["top"]).all()
    # the defaults (up = minus the background's y axis, the camera as the reference), a tilted up, a camera box
    check_map(fus, fus.ground_map())
    check_map(fus, fus.ground_map(**TILTED), **TILTED)
    boxed = fus.ground_map(box="camera", size=(40, 24, 48), **TILTED)
    assert boxed["box"] == fus.camera_box((40, 24, 48))
    check_map(fus, boxed, **TILTED)
    other = dict(WALL, cell=0.1, bin=0.09, reference=(0.1, 0.0, 0.3))
    check_map(fus, fus.ground_map(**other), **other)
    # nothing of the session changed, and a second call gives the same
    after = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    for a, b in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) if isinstance(a, tuple) else a.tobytes() == b.tobytes()
    again = fus.ground_map(**WALL)
    assert again["cells"].tobytes() == got["cells"].tobytes() and again["classes"].tobytes() == got["classes"].tobytes()


def test_slots_below_two_voxels_need_an_up_along_a_box_axis(session):
    from emfusion_amd import pipeline
    fus, _ = session
    one = dict(WALL, cell=VOX, bin=VOX)
    check_map(fus, fus.ground_map(**one), **one)  # along -z: one voxel is fine
    for kw in (dict(TILTED, cell=VOX), dict(TILTED, bin=1.9 * VOX)):
        with pytest.raises(ValueError, match="below two voxels"):
            fus.ground_map(**kw)
    with pytest.raises(ValueError):
        fus.ground_map(up=(0, 0, 0))
    with pytest.raises(ValueError):
        fus.ground_map(band=(0.5, 0.5))
    with pytest.raises(ValueError):
        fus.ground_map(**dict(WALL, band=(-30.0, 0.2)))  # more than 256 bins
    with pytest.raises(pipeline.FusionError) as err:
        fus.ground_map(box=((40, 0, 0), (25, 8, 8)), **WALL)
    assert err.value.code == -4
    with pytest.raises(ValueError):
        fus.ground_map(box="camera")


def check_plan(got, robot_radius=0.0, through_unknown=False, min_cells=8, frontiers=True):
    """got = fus.ground_plan(...) against the frontier and plan restatements on the 2-D classes it returns."""
    gm = got["ground"]
    classes = gm["classes"][None]
    H, W = gm["classes"].shape
    radius = int(np.ceil(np.float32(robot_radius) / np.float32(gm["cell"]))) if robot_radius > 0 else 0
    assert got["clearance_voxels"] == radius and got["start_radius_voxels"] == max(radius, 1)
    d2 = dr.distance_transform(classes, 1 << dr.OCCUPIED, radius) if radius else None
    if frontiers:
        _, kept, counts = fr.frontiers(classes, d2, radius * radius, min_cells)
        want = fr.session_order(kept)
        assert (got["frontiers"]["kept"], got["frontiers"]["n_clusters"], got["frontiers"]["n_voxels"]) == counts
        assert got["frontiers"]["records"].tobytes() == want.tobytes()
        assert sorted(g["voxel"] for g in got["goals"]) == sorted(tuple(r["rep"].tolist()) for r in want)
        assert got["clusters"] is got["goals"]
        keys = [(not g["reachable"], g["cost"] if g["reachable"] else 0) for g in got["goals"]]
        assert keys == sorted(keys)
    cost, (finite, used) = pl.cost_field(classes, got["start_voxels"], d2=d2, min_d2=radius * radius,
                                         mask=5 if through_unknown else 1, radius=got["start_radius_voxels"], max_cost=0)
    assert got["converged"] and (got["n_finite"], got["n_starts"]) == (finite, used)
    goals = [g["voxel"] for g in got["goals"]]
    if goals:
        _, lengths, goal_cost = pl.paths(cost, goals, 0)
        paths, _, _ = pl.paths(cost, goals, int(lengths.max(initial=0)))
    for k, g in enumerate(got["goals"]):
        assert g["reachable"] == bool(lengths[k] > 0) and g["cost"] == int(goal_cost[k])
        lin = paths[k, :lengths[k]].astype(np.int64)
        vox = np.stack([lin % W, lin // W, np.zeros_like(lin)], axis=1).astype(np.int32)
        assert g["path_vox"].dtype == np.int32 and g["path_vox"].tobytes() == vox.tobytes()
        f, e, c = pl.step_counts(lin, cost.shape) if len(lin) else (0, 0, 0)
        assert g["steps"] == (f, e, 0) and c == 0 and 3 * f + 4 * e == (g["cost"] if g["reachable"] else 0)
        assert g["length_m"] == (f + np.sqrt(2.0) * e) * np.float64(gm["cell"])
        # the path in the world: every cell's centre at its floor height, through the numpy frame, exactly
        floor = gm["floor"][vox[:, 1], vox[:, 0]].astype(np.float64)
        ch = np.where(floor >= 0, (floor + 1.0) * np.float64(gm["bin"]), np.nan)
        want_w = rf.ground_point(gm["ground_pose"], (vox[:, 0] + 0.5) * np.float64(gm["cell"]),
                                 (vox[:, 1] + 0.5) * np.float64(gm["cell"]), ch).astype(np.float32).reshape(-1, 3)
        assert g["path_world"].dtype == np.float32 and g["path_world"].tobytes() == want_w.tobytes()
        if g["reachable"]:
            assert tuple(vox[0]) == g["voxel"] and cost[0, vox[-1][1], vox[-1][0]] == 0
            if not through_unknown:
                assert not np.isnan(g["path_world"][1:]).any()  # a path through free cells stays on floors
    return cost


def test_ground_plan_equals_the_restatements(session):
    fus, oid = session
    got = fus.ground_plan(**WALL)
    check_map(fus, got["ground"], **WALL)
    check_plan(got)
    assert len(got["goals"]) >= 2 and any(g["reachable"] for g in got["goals"]) and got["n_starts"] == 1
    # the start is the cell under the camera
    gm = got["ground"]
    cam = fus.pose(0)[1].astype(np.float64)
    pose = gm["ground_pose"]
    d = cam - pose[9:]
    uv = [int(np.floor(((d[0] * pose[k] + d[1] * pose[3 + k]) + d[2] * pose[6 + k]) / np.float64(gm["cell"]))) for k in range(2)]
    assert got["start_voxels"].tolist() == [[uv[0], uv[1], 0]]
    # a robot radius, smaller clusters, the object excluded; a tilted up through unknown cells
    got = fus.ground_plan(robot_radius=0.1, min_cells=2, exclude=[oid], **WALL)
    check_map(fus, got["ground"], exclude=[oid], **WALL)
    check_plan(got, robot_radius=0.1, min_cells=2)
    plain = fus.ground_plan(min_cells=1, **TILTED)
    check_plan(plain, min_cells=1)
    got = fus.ground_plan(through_unknown=True, min_cells=1, **TILTED)
    check_plan(got, through_unknown=True, min_cells=1)
    assert got["n_finite"] > plain["n_finite"]
    # explicit goals and starts as world points: taken to the cells they lie over, never moved
    free = np.argwhere(gm["classes"] == rf.FREE)
    pts = gm["cell_world"](free[[3, -3], 1], free[[3, -3], 0])
    got = fus.ground_plan(goals=np.concatenate([pts, [[50.0, 0.0, 0.0]]]), start=pts[:1], **WALL)
    assert [g["voxel"] for g in got["goals"]][:2] == [(int(free[3, 1]), int(free[3, 0]), 0), (int(free[-3, 1]), int(free[-3, 0]), 0)]
    assert got["goals"][0]["cost"] == 0 and not got["goals"][2]["reachable"] and "clusters" not in got
    check_plan(got, frontiers=False)
    with pytest.raises(ValueError):
        fus.ground_plan(goals="nearest", **WALL)


def test_earlier_queries_are_unchanged_after_a_ground_map(session):
    fus, _ = session
    from emfusion_amd.pipeline import _check, load
    df = fus.distance_field()
    plan = fus.plan(field=True)
    fus.ground_plan(robot_radius=0.1, **WALL)
    d2, classes = np.empty_like(df["d2"]), np.empty_like(df["classes"])
    _check("emf_fusion_copy_distance_field", load().emf_fusion_copy_distance_field(fus._h, classes.ctypes.data, d2.ctypes.data, None))
    assert d2.tobytes() == df["d2"].tobytes() and classes.tobytes() == df["classes"].tobytes()
    assert fus.plan(field=True)["cost"].tobytes() == plan["cost"].tobytes()


def digest(root):
    return {k: hashlib.sha256(v).hexdigest() if isinstance(v, bytes) else v for k, v in listing(root).items()}


def test_write_results_writes_the_files_only_with_the_switch(dev, tmp_path):
    out = {}
    for on in (False, True):
        fus, _ = new_session()
        if on:
            fus.setup_output(False, False, exp_ground_map=True, ground_up=WALL["up"], ground_band=WALL["band"],
                             ground_robot_height=WALL["robot_height"], ground_max_step=WALL["max_step"])
        else:
            fus.setup_output(False, False)
        fus.write_results(tmp_path / str(on), volumes=False)
        if on:
            got = fus.ground_map(**WALL)
        fus.close()
        out[on] = digest(tmp_path / str(on))
    assert set(out[True]) - set(out[False]) == {"ground.bin", "ground.txt"} and set(out[False]) <= set(out[True])
    assert all(out[True][k] == v for k, v in out[False].items()) and len(out[False]) >= 3
    G, W, H, B = got["frame"]
    raw = (tmp_path / "True" / "ground.bin").read_bytes()
    assert len(raw) == W * H * 9
    assert raw[:W * H] == got["classes"].tobytes() and raw[W * H:] == got["cells"].tobytes()
    lines = (tmp_path / "True" / "ground.txt").read_text().splitlines()
    assert lines[0].startswith("#") and lines[1] == f"map {W} {H}"
    assert lines[2] == f"bins {B} robot {got['robot_bins']} step {got['max_step_bins']}"
    assert np.abs(np.array([float(v) for v in lines[3].split()[1::2]]) - [got["cell"], got["bin"]]).max() < 1e-9  # %.9g
    rows = np.array([[np.float32(v) for v in line.split()[1:]] for line in lines[4:7]], np.float32)
    assert rows.tobytes() == G.tobytes()  # %.9g round-trips a float32
    pose = np.array([[float(v) for v in line.split()[1:]] for line in lines[7:11]], np.float64).reshape(-1)
    assert np.abs(pose - got["ground_pose"]).max() < 1e-8 and len(lines) == 11


def test_a_checkpoint_after_the_calls_equals_one_without_them(dev, tmp_path):
    files = []
    for ask in (False, True):
        fus, oid = new_session()
        if ask:
            fus.ground_map(**WALL)
            fus.ground_plan(robot_radius=0.1, **TILTED)
        fus.save_checkpoint(tmp_path / f"{ask}.ckpt")
        fus.close()
        files.append((tmp_path / f"{ask}.ckpt").read_bytes())
    assert files[0] == files[1] and len(files[0]) > 1000


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.ground_map(**WALL), lambda: fus.ground_plan(box=((0, 0, 0), (8, 8, 8)), **WALL)):
            with pytest.raises(pipeline.FusionError, match="the ground map is not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4, -4], [-4, -4]]


def test_the_app_writes_the_files_and_nothing_else_changes(dev, tmp_path):
    """apps/emfusion_synth on its synthetic stream: with --ground-map the results gain ground.bin and ground.txt, whose
    sizes agree, and no other byte changes; the parameters alone, or a malformed list, are a usage error."""
    import subprocess
    from tests.test_gpu_frontier_pipeline import APP, ROOT
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = [str(APP), "--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    ground = ["--ground-map", "--ground-up", "0,0,-1", "--ground-band", "-3.0,0.2", "--ground-robot-height", "0.2", "--ground-max-step", "0.1"]
    outs = {}
    for name, extra in (("plain", []), ("ground", ground)):
        p = subprocess.run([*small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = digest(tmp_path / name)
    assert set(outs["ground"]) - set(outs["plain"]) == {"ground.bin", "ground.txt"}
    assert all(outs["ground"][k] == v for k, v in outs["plain"].items()) and len(outs["plain"]) > 3
    lines = (tmp_path / "ground" / "ground.txt").read_text().splitlines()
    W, H = (int(v) for v in lines[1].split()[1:])
    raw = (tmp_path / "ground" / "ground.bin").read_bytes()
    assert len(raw) == 9 * W * H and len(lines) == 11
    classes = np.frombuffer(raw[:W * H], np.uint8)
    cells = np.frombuffer(raw[W * H:], rf.CELL_DTYPE)
    assert set(np.unique(classes)) <= {0, 1, 2} and (classes == rf.FREE).sum() > 50
    assert ((cells["floor"] >= 0) == (classes == rf.FREE) | ((classes == rf.OCCUPIED) & (cells["floor"] >= 0))).all()
    assert ((classes == rf.UNKNOWN) == ((cells["floor"] < 0) & (cells["top"] < 0))).all()
    for bad in (["--ground-cell", "0.1"], ["--ground-map", "--ground-up", "0,1"]):
        p = subprocess.run([*small, "--out", str(tmp_path / "bad"), *bad], cwd=ROOT, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--ground-map" in p.stderr
