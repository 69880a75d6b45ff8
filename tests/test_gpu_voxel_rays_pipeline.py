"""Fusion.cast_rays, Fusion.view_gain and Fusion.plan(shortcut=W) on a live session: the 64^3 background
with one object the frontier pipeline test uses.  Every record equals tests/rays_reference.py applied to the classes
Fusion.distance_field() reports for the same box and exclude list, byte for byte; the view targets equal the numpy
float64 restatement; the waypoints equal the greedy on the reference visibility; the outputs of write_results and of both
apps gain their waypoints lines only with the switch; the refusal on a sharded session; the session stays untouched."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import rays_reference as rr
from tests.test_gpu_frontier_pipeline import APP, BG, H, ROOT, VOX, W, listing, new_session, params
from tests.test_gpu_plan_pipeline import voxels_of, world_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def snapshot(fus, oid):
    return [fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.volume("weights", oid), *fus.pose(0),
            *fus.pose(oid), *fus.background_pose()]


def reference_classes(fus, box, exclude=(), clearance=0.0):
    """(classes, d2 or None, min_d2) of the box as Fusion.distance_field() reports them, and the clearance transform."""
    classes = fus.distance_field(box=box, exclude=exclude, metres=False)["classes"]
    cv = voxels_of(clearance)
    return classes, (dr.distance_transform(classes, 1 << dr.OCCUPIED, cv) if cv else None), cv * cv


def check_rays(fus, got, a, b, clearance=0.0, through_unknown=False, count=("unknown",), exclude=(), group=0):
    """got = cast_rays(world_of(a), world_of(b), ...) against the restatement; returns its records."""
    lo, size = got["box"]
    classes, d2, min_d2 = reference_classes(fus, got["box"], exclude, clearance)
    count_mask = sum({"free": 1, "occupied": 2, "unknown": 4}[c] for c in count)
    want = rr.cast(classes, a, b, d2, min_d2, 5 if through_unknown else 1, count_mask)
    assert got["clearance_voxels"] == voxels_of(clearance) and got["voxel_size"] == float(np.float32(VOX))
    assert got["from_voxel"].dtype == np.int32 and got["from_voxel"].tobytes() == np.asarray(a, np.int32).tobytes()
    assert got["to_voxel"].tobytes() == np.asarray(b, np.int32).tobytes()
    for key, field in (("status", "status"), ("steps", "steps"), ("counted", "counted"), ("weighted", "weighted")):
        assert got[key].dtype == want[field].dtype and got[key].tobytes() == want[field].tobytes(), key
    assert (got["visible"] == (want["status"] == rr.REACHED)).all() and got["visible"].dtype == bool
    has = want["stop"] >= 0
    lin = np.where(has, want["stop"], 0).astype(np.int64)
    site = np.stack([lin % size[0], lin // size[0] % size[1], lin // (size[0] * size[1])], axis=1)
    stop = np.where(has[:, None], site, -1).astype(np.int32)
    assert got["stop_voxel"].dtype == np.int32 and got["stop_voxel"].tobytes() == stop.tobytes()
    world = np.where(has[:, None], world_of(fus, lo, site), np.nan).astype(np.float32)
    assert got["stop_world"].dtype == np.float32 and got["stop_world"].tobytes() == world.tobytes()
    if group:
        assert got["groups"].dtype == rr.GROUP and got["groups"].tobytes() == rr.group_records(want, group).tobytes()
    else:
        assert "groups" not in got
    return want


def random_ends(size, n, seed):
    rng = np.random.default_rng(seed)
    size = np.array(size)
    a = rng.integers(0, size, (n, 3))
    b = np.where((rng.random(n) < 0.5)[:, None], a + rng.integers(-12, 13, (n, 3)), rng.integers(-3, size + 3, (n, 3)))
    a[:4] = [(-1, 5, 5), (5, 5, size[2]), (0, 0, 0), (3, 3, 3)]  # origins outside, a zero-length ray
    b[2:4] = [(0, 0, 0), (3, 3 + 4096, 3)]                       # ... and an invalid one
    a[4], b[4] = (3, 3, 0), (3, 3, -5)                           # leaves the box at its first step
    return a.astype(np.int32), b.astype(np.int32)


def test_cast_rays_equal_the_reference(session):
    fus, oid = session
    before = snapshot(fus, oid)
    a, b = random_ends((BG, BG, BG), 300, 1)
    pa, pb = world_of(fus, (0, 0, 0), a), world_of(fus, (0, 0, 0), b)
    got = fus.cast_rays(pa + np.float32(0.3 * VOX), pb - np.float32(0.2 * VOX))  # off the centres: rounded, never moved
    assert got["box"] == ((0, 0, 0), (BG, BG, BG))
    want = check_rays(fus, got, a, b)
    assert set(want["status"].tolist()) == {rr.REACHED, rr.BLOCKED, rr.LEFT, rr.OUTSIDE, rr.INVALID}
    plain_reached = int(got["visible"].sum())
    got = fus.cast_rays(pa, pb, through_unknown=True, count=("unknown", "free"), group=7)
    want = check_rays(fus, got, a, b, through_unknown=True, count=("unknown", "free"), group=7)
    assert int(got["visible"].sum()) > plain_reached and want["counted"].max() > 0
    got = fus.cast_rays(pa, pb, clearance=0.07, through_unknown=True, group=64)
    gated = check_rays(fus, got, a, b, clearance=0.07, through_unknown=True, group=64)
    assert (gated["steps"] <= want["steps"]).all() and (gated["steps"] < want["steps"]).any()  # the gate does stop rays
    # a box of its own: box coordinates throughout
    box = ((8, 4, 2), (40, 50, 30))
    a2, b2 = random_ends(box[1], 200, 2)
    got = fus.cast_rays(world_of(fus, box[0], a2), world_of(fus, box[0], b2), box=box, clearance=0.04, count=("free",), group=1)
    assert got["box"] == box
    check_rays(fus, got, a2, b2, clearance=0.04, count=("free",), group=1)
    got = fus.cast_rays(pa[:0], pb[:0], group=3)
    assert len(got["status"]) == 0 and len(got["groups"]) == 0
    from emfusion_amd import pipeline
    with pytest.raises(pipeline.FusionError) as err:
        fus.cast_rays(pa, pb, box=((40, 0, 0), (25, 8, 8)))
    assert err.value.code == -4
    with pytest.raises(ValueError):
        fus.cast_rays(pa, pb[:5])
    with pytest.raises(ValueError):
        fus.cast_rays(pa, pb, count=("wall",))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, snapshot(fus, oid)))  # nothing of the session changed


def test_an_excluded_object_no_longer_blocks(session):
    fus, oid = session
    whole = ((0, 0, 0), (BG, BG, BG))
    with_obj, _, _ = reference_classes(fus, whole)
    without, _, _ = reference_classes(fus, whole, exclude=[oid])
    stamped = np.argwhere(with_obj != without)[:, ::-1]  # the voxels only the object occupies
    assert len(stamped) >= 8 and (with_obj[without != with_obj] == dr.OCCUPIED).all()
    targets = stamped[:: max(len(stamped) // 40, 1)][:40].astype(np.int32)
    cam = np.array(fus.camera_box(1)[0], np.int32)
    origins = np.repeat(cam[None], len(targets), axis=0)
    pa, pb = world_of(fus, (0, 0, 0), origins), world_of(fus, (0, 0, 0), targets)
    got = fus.cast_rays(pa, pb, through_unknown=True)
    want = check_rays(fus, got, origins, targets, through_unknown=True)
    assert (want["status"] == rr.BLOCKED).all()  # the target itself is occupied
    freed = fus.cast_rays(pa, pb, through_unknown=True, exclude=[oid])
    check_rays(fus, freed, origins, targets, through_unknown=True, exclude=[oid])
    assert (freed["steps"] >= got["steps"]).all() and (freed["steps"] > got["steps"]).any()  # rays go on through it
    hit = {tuple(v) for v in stamped.tolist()}
    assert all(tuple(v) in hit for v in got["stop_voxel"].tolist() if tuple(v) not in
               {tuple(w) for w in freed["stop_voxel"].tolist()})  # what no longer stops a ray is the object
    assert not any(tuple(v) in hit for v in freed["stop_voxel"].tolist())


def side_views(fus):
    """Candidate views at the camera's place: the camera's own (it faces the observed wall), and the same turned a quarter
    about its y axis to either side (they face space no frame has seen)."""
    R, t = fus.pose(0)
    R, t = R.astype(np.float64), t.astype(np.float64)
    quarter = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    return [(R, t), (R @ quarter, t), (R @ quarter.T, t)]


def check_gain(fus, got, views, grid, range_m, K4, exclude=()):
    lo, size = got["box"]
    bg_R, bg_t = fus.background_pose()
    classes, _, _ = reference_classes(fus, got["box"], exclude)
    per = grid[0] * grid[1]
    assert got["targets"].shape == (len(views), grid[1], grid[0], 3) and got["targets"].dtype == np.int32
    origins = np.zeros((len(views), 3), np.int32)
    for v, (R, t) in enumerate(views):
        origin, targets, scaled = rr.view_targets(R, t, K4, grid, range_m, bg_R, bg_t, (BG, BG, BG), np.float32(VOX), lo)
        assert np.abs(scaled - np.floor(scaled) - 0.5).min() > 1e-6  # no tie decides a target
        origins[v] = origin
        assert got["targets"][v].tobytes() == targets.tobytes(), v
    assert got["origin_voxel"].dtype == np.int32 and got["origin_voxel"].tobytes() == origins.tobytes()
    a = np.repeat(origins, per, axis=0)
    want = rr.cast(classes, a, got["targets"].reshape(-1, 3), None, 0, 5, 4)  # on its own returned targets
    groups = rr.group_records(want, per)
    assert got["records"].dtype == rr.RESULT and got["records"].tobytes() == want.tobytes()
    assert got["groups"].tobytes() == groups.tobytes()
    for key, field in (("unknown", "counted"), ("weighted", "weighted"), ("reached", "reached"), ("blocked", "blocked"), ("left", "left")):
        assert got[key].tobytes() == groups[field].tobytes(), key
    assert (got["rays"]["status"] == want["status"]).all() and got["rays"]["weighted"].tobytes() == want["weighted"].tobytes()
    inside = ((origins >= 0) & (origins < np.array(size))).all(axis=1)
    assert (got["inside"] == inside).all()
    order = sorted(range(len(views)), key=lambda v: (-int(groups["weighted"][v]), v))
    assert got["order"].tolist() == order
    return groups


def test_view_gain_equals_the_reference_and_ranks_the_unknown_first(session):
    fus, oid = session
    before = snapshot(fus, oid)
    views = side_views(fus)
    grid, range_m = (32, 24), 1.0
    got = fus.view_gain(views, range_m=range_m, rays=True)
    prm = params()
    K = np.array(prm.K, np.float32).reshape(3, 3)
    sx, sy = np.float32(grid[0] / W), np.float32(grid[1] / H)
    K4 = np.array([K[0, 0] * sx, K[1, 1] * sy, K[0, 2] * sx, K[1, 2] * sy], np.float64)  # as default_3d_view scales them
    assert got["K"].tobytes() == K4.tobytes() and got["box"] == ((0, 0, 0), (BG, BG, BG))
    groups = check_gain(fus, got, views, grid, range_m, K4)
    assert got["inside"].all() and (groups["invalid"] == 0).all()
    # the views that face unseen space outrank the one that faces the observed wall
    assert got["order"][-1] == 0 and got["weighted"][1] > got["weighted"][0] and got["weighted"][2] > got["weighted"][0]
    assert got["unknown"][1] > got["unknown"][0]
    # without the rays: the same group records, no per-ray entries
    lean = fus.view_gain(views, range_m=range_m)
    assert lean["groups"].tobytes() == got["groups"].tobytes() and "rays" not in lean and "targets" not in lean
    assert lean["order"].tolist() == got["order"].tolist()
    # an explicit K, another grid, a box of its own and the object excluded; a camera outside the box
    Kx = np.array([[9.0, 0, 3.5], [0, 9.5, 2.5], [0, 0, 1]])
    box = ((4, 6, 0), (56, 50, 40))
    R0, t0 = views[0]
    outside = (R0, t0 - 0.5 * R0[:, 2])  # half a metre behind the camera: behind the background's near face
    some = views + [outside]
    got = fus.view_gain(some, grid=(8, 6), K=Kx, range_m=1.3, box=box, exclude=[oid], rays=True)
    assert got["box"] == box
    groups = check_gain(fus, got, some, (8, 6), 1.3, (9.0, 9.5, 3.5, 2.5), exclude=[oid])
    assert got["inside"].tolist() == [True, True, True, False]
    assert got["unknown"][3] == 0 and got["weighted"][3] == 0 and got["reached"][3] == got["blocked"][3] == got["left"][3] == 0
    assert groups["invalid"][3] == 48 and (got["records"]["status"][3 * 48:] == rr.OUTSIDE).all()
    assert len(fus.view_gain([], rays=True)["order"]) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, snapshot(fus, oid)))


def check_shortcut(fus, got, window, clearance=0.0, through_unknown=False, exclude=()):
    classes, d2, min_d2 = reference_classes(fus, got["box"], exclude, clearance)
    vs = np.float64(np.float32(VOX))
    jumps = 0
    for g in got["goals"]:
        path = g["path_vox"]
        k = len(path) - 1
        vis = rr.path_visibility(classes, path, window, d2, min_d2, 5 if through_unknown else 1)
        want = rr.shortcut_greedy(k, window, lambda i, j: vis[(i, j)])
        way = g["waypoints"]
        assert way.dtype == np.int32 and way.tolist() == want, (g["voxel"], way.tolist(), want)
        if not g["reachable"]:
            assert len(way) == 0 and g["waypoints_length_m"] == 0 and g["waypoints_vox"].shape == (0, 3)
            continue
        assert way[0] == 0 and way[-1] == k and (np.diff(way) >= 1).all() and (np.diff(way) <= max(window, 1)).all()
        for i, j in zip(way[:-1], way[1:]):
            assert j == i + 1 or vis[(int(i), int(j))]  # every chosen jump has a REACHED reference ray
            jumps += j > i + 1
        assert g["waypoints_vox"].dtype == np.int32 and g["waypoints_vox"].tobytes() == path[way].tobytes()
        assert g["waypoints_world"].tobytes() == g["path_world"][way].tobytes()
        hops = np.diff(path[way].astype(np.float64), axis=0)
        length = np.sqrt((hops * hops).sum(axis=1)).sum() * vs
        assert g["waypoints_length_m"] == length and length <= g["length_m"] * (1 + 1e-12)
    return jumps


def plain(v):
    """A result of plan() as comparable values: arrays as (dtype, shape, bytes), the shortcut's entries left out."""
    skip = ("waypoints", "waypoints_vox", "waypoints_world", "waypoints_length_m")
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items() if k not in skip}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def plan_key(got):
    return plain(got)


def test_plan_shortcut_equals_the_greedy_on_the_reference(session):
    fus, oid = session
    before = snapshot(fus, oid)
    first = fus.plan(field=True, min_voxels=3)
    assert all("waypoints" not in g for g in first["goals"])
    got = fus.plan(field=True, min_voxels=3, shortcut=8)
    assert plan_key(got) == plan_key(first) and sorted(got) == sorted(first)  # the plan itself: the same keys and bytes
    assert all(set(g) - set(p) == {"waypoints", "waypoints_vox", "waypoints_world", "waypoints_length_m"}
               for g, p in zip(got["goals"], first["goals"]))
    assert any(g["reachable"] and len(g["path_vox"]) > 10 for g in got["goals"])
    jumps = check_shortcut(fus, got, 8)
    assert jumps > 0 and any(g["reachable"] and len(g["waypoints"]) < len(g["path_vox"]) for g in got["goals"])
    again = fus.plan(field=True, min_voxels=3)
    assert plan_key(again) == plan_key(first) and again["cost"].tobytes() == first["cost"].tobytes()
    # the plan's own gate and mask; another query uses the shared clearance scratch in between
    got = fus.plan(min_voxels=1, clearance=0.07, through_unknown=True, shortcut=64)
    check_shortcut(fus, got, 64, clearance=0.07, through_unknown=True)
    got = fus.plan(min_voxels=1, clearance=0.07, shortcut=5, exclude=[oid], box="camera", size=48)
    check_shortcut(fus, got, 5, clearance=0.07, exclude=[oid])
    # explicit goals, one of them without a path; a window of 1 casts nothing and keeps the path
    cost = first["cost"]
    reachable = np.argwhere((cost < 0xfffffffe) & (cost > 60))[0][::-1]
    blocked = np.argwhere(cost == 0xfffffffe)[0][::-1]
    got = fus.plan(goals=world_of(fus, (0, 0, 0), np.array([reachable, blocked])), shortcut=1)
    check_shortcut(fus, got, 1)
    assert got["goals"][0]["waypoints"].tolist() == list(range(len(got["goals"][0]["path_vox"]))) and not got["goals"][1]["reachable"]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, snapshot(fus, oid)))


def test_the_gate_of_a_plan_survives_other_queries(session):
    """plan(), then another query that refills the shared clearance scratch, then the shortcut entry on that plan: the
    gate is the plan's own again."""
    import ctypes as C
    from emfusion_amd.pipeline import _check, load
    fus, _ = session
    got = fus.plan(min_voxels=1, clearance=0.07, through_unknown=True, shortcut=6)
    fus.frontiers(min_voxels=1, clearance=0.03)  # another transform into the scratch
    n = len(got["goals"])
    counts, most = np.zeros(max(n, 1), np.int32), C.c_int32(0)
    _check("emf_fusion_plan_shortcut", load().emf_fusion_plan_shortcut(fus._h, 6, counts.ctypes.data, C.byref(most)))
    ways = np.full((max(n, 1), max(most.value, 1)), -1, np.int32)
    _check("emf_fusion_copy_plan_shortcut", load().emf_fusion_copy_plan_shortcut(fus._h, ways.ctypes.data, ways.shape[1]))
    # the goals of got are sorted for the caller: match them by their voxel
    fresh = {}
    raw = fus.plan(min_voxels=1, clearance=0.07, through_unknown=True, shortcut=6)
    assert [g["voxel"] for g in raw["goals"]] == [g["voxel"] for g in got["goals"]]
    for g, h in zip(got["goals"], raw["goals"]):
        assert g["waypoints"].tolist() == h["waypoints"].tolist()
        fresh[g["voxel"]] = g["waypoints"].tolist()
    assert sorted(ways[k, :counts[k]].tolist() for k in range(n)) == sorted(fresh.values())


def read_plan_with_waypoints(path):
    """(the text without its waypoints lines, [(n_path, waypoints or None)] per goal) of a plan.txt."""
    lines = Path(path).read_text().splitlines(keepends=True)
    kept, goals, k = [lines[0]], [], 1
    while k < len(lines):
        r = lines[k].split()
        assert len(r) == 8, lines[k]
        n = int(r[7])
        kept += lines[k:k + 1 + n]
        k += 1 + n
        way = None
        if k < len(lines) and lines[k].startswith("waypoints "):
            w = lines[k].split()
            way = [int(v) for v in w[2:]]
            assert int(w[1]) == len(way)
            k += 1
        goals.append((int(r[1]), n, way))
    return "".join(kept), goals


def check_waypoint_lines(goals, window):
    assert any(reachable for reachable, _, _ in goals)
    for reachable, n, way in goals:
        assert (way is not None) == bool(reachable)
        if way is not None:
            assert way[0] == 0 and way[-1] == n - 1 and all(1 <= b - a <= window for a, b in zip(way, way[1:]))


def test_write_results_writes_the_waypoints_only_with_the_switch(dev, tmp_path):
    out = {}
    for window in (0, 8):
        fus, _ = new_session()
        fus.setup_output(False, False, frontier_min_voxels=3, exp_plan=True, plan_clearance=0.07, exp_plan_shortcut=window)
        fus.write_results(tmp_path / str(window), volumes=False)
        if window:
            got = fus.plan(min_voxels=3, clearance=0.07, shortcut=window)
            order = [c["label"] for c in fus.frontiers(min_voxels=3, clearance=0.07)["clusters"]]
        fus.close()
        out[window] = listing(tmp_path / str(window))
    assert set(out[0]) == set(out[8]) and all(out[8][k] == v for k, v in out[0].items() if k != "plan.txt")
    text, goals = read_plan_with_waypoints(tmp_path / "8" / "plan.txt")
    assert text.encode() == out[0]["plan.txt"] and b"waypoints" not in out[0]["plan.txt"]  # without the switch: byte for byte
    check_waypoint_lines(goals, 8)
    by_label = {g["label"]: g for g in got["goals"]}
    assert len(goals) == len(order)
    for (reachable, n, way), label in zip(goals, order):  # the file keeps the order of frontiers.txt
        g = by_label[label]
        assert bool(reachable) == g["reachable"] and n == len(g["path_vox"])
        assert way == (g["waypoints"].tolist() if g["reachable"] else None)
    fus, _ = new_session()
    try:
        with pytest.raises(ValueError):  # the waypoints go into plan.txt: refused without exp_plan
            fus.setup_output(False, False, exp_plan_shortcut=4)
    finally:
        fus.close()


def test_the_apps_write_the_waypoints_only_with_the_switch(dev, tmp_path):
    from tests import tum_staging as T
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    seq, masks, _ = T.stage(tmp_path)
    plan = ["--frontiers", "--frontier-min-voxels", "4", "--frontier-clearance", "0.05", "--plan", "--plan-clearance", "0.05"]
    small = ["--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    apps = {"synth": [str(APP), *small],
            "sequence": [str(APP), "--sequence", seq, "--masks", str(masks), *T.SMALL],
            "tum": [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]}
    for app, cmd in apps.items():
        # refused with a usage message without --plan, before any device is touched
        p = subprocess.run([*cmd, "--out", str(tmp_path / app / "refused"), "--plan-shortcut", "8"], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 2 and "usage" in p.stderr and "--plan" in p.stderr, (app, p.returncode, p.stderr[-500:])
        outs = {}
        for name, extra in (("plan", plan), ("shortcut", plan + ["--plan-shortcut", "8"])):
            p = subprocess.run([*cmd, "--out", str(tmp_path / app / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            outs[name] = listing(tmp_path / app / name)
        assert set(outs["plan"]) == set(outs["shortcut"]) and len(outs["plan"]) > 3, app
        assert all(outs["shortcut"][k] == v for k, v in outs["plan"].items() if k != "plan.txt"), app
        text, goals = read_plan_with_waypoints(tmp_path / app / "shortcut" / "plan.txt")
        assert text.encode() == outs["plan"]["plan.txt"] and b"waypoints" not in outs["plan"]["plan.txt"], app
        check_waypoint_lines(goals, 8)


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        one = np.zeros((1, 3), np.float32)
        for call in (lambda: fus.cast_rays(one, one), lambda: fus.cast_rays(one, one, box=((0, 0, 0), (8, 8, 8)), group=1),
                     lambda: fus.view_gain([(np.eye(3), np.zeros(3))]), lambda: fus.plan(goals=one, shortcut=4)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 4, [-4] * 4]


def test_the_next_frame_is_that_of_a_session_that_never_asked(dev):
    from tests.test_gpu_frontier_pipeline import feed, open_session
    out = []
    for ask in (False, True):
        fus, oid, synth = open_session()
        if ask:
            one = np.zeros((4, 3), np.float32)
            fus.cast_rays(one, one + np.float32(0.7), clearance=0.07, group=2)
            fus.view_gain(side_views(fus), range_m=1.0)
            fus.plan(clearance=0.07, shortcut=8)
        feed(fus, synth, oid, 3)
        synth.close()
        out.append(snapshot(fus, oid))
        fus.close()
    assert len(out[0]) == len(out[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*out))
