"""Scene queries over the world extent (Fusion.set_query_extent("world")): the distance field, point
queries, frontiers and plans of a box that covers the current background AND the tiles the background store holds,
against the numpy restatements on tests/world_queries_reference.classes_of_tiles of the restated store plus the session's
own volumes.  The stream is test_gpu_background_store's out-and-back walk (96^3, 160 x 120, 15 frames, rolls at frames
6 and 12), driven as test_gpu_world_mesh's `walk` drives it.  Bytes against numpy, no tolerance."""
import hashlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import frontier_reference as fr
from tests import nearest_reference as nr
from tests import plan_reference as pl
from tests import roll_reference as rr
from tests import store_reference as sr
from tests import world_queries_reference as wq
from tests.test_gpu_background_store import bits, frames, new_session, volumes
from tests.test_gpu_world_mesh import digest, listing, world_tiles

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
RES = (rr.BG,) * 3
VS = np.float64(np.float32(rr.VOX))


def world_of(pose, lo, vox):
    """Box voxels (of the box at `lo`, volume voxels, possibly negative) in the world frame, float64: the formula of
    the background's own boxes with the REAL resolution.  pose: Fusion.background_pose() or the session itself."""
    R, t = pose.background_pose() if hasattr(pose, "background_pose") else pose
    p = (np.asarray(vox, np.float64) + np.asarray(lo, np.float64) - (rr.BG - 1) / 2.0) * VS
    return p @ R.astype(np.float64).T + t.astype(np.float64)


def reference_extent(store, origin):
    """The bounding box of the background and the restated store's tiles, in volume voxels."""
    lo, hi = np.zeros(3, np.int64), np.array(RES, np.int64)
    for key in store.tiles:
        first = np.array(key, np.int64) * np.array(sr.TILE) - np.array(origin, np.int64)
        lo, hi = np.minimum(lo, first), np.maximum(hi, first + np.array(sr.TILE))
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)


def reference_classes(fus, store, box):
    """classes_of_tiles over the box (volume voxels) of the session's volumes plus the restated store."""
    t, w, _ = volumes(fus, False)
    origin = fus.background_origin()
    tiles, stored, _ = world_tiles(t, w, None, origin, store)
    return wq.classes_of_tiles(tiles, RES, (wq.lattice_of(box[0], origin), box[1])), tiles, stored


def check_frontiers(got, classes, min_voxels):
    labels, kept, counts = fr.frontiers(classes, None, 0, min_voxels)
    want = fr.session_order(kept)
    assert (got["kept"], got["n_clusters"], got["n_voxels"]) == counts
    assert got["records"].tobytes() == want.tobytes()
    assert got["labels"].dtype == np.int32 and got["labels"].tobytes() == labels.tobytes()
    return want


def check_plan(pose, got, classes):
    seeds = got["start_voxels"]
    cost, (finite, used) = pl.cost_field(classes, seeds, d2=None, min_d2=0, mask=1, radius=got["start_radius_voxels"], max_cost=0)
    assert got["converged"] and (got["n_finite"], got["n_starts"]) == (finite, used)
    assert got["cost"].dtype == np.uint32 and got["cost"].tobytes() == cost.tobytes()
    goals = [g["voxel"] for g in got["goals"]]
    nz, ny, nx = cost.shape
    _, lengths, goal_cost = pl.paths(cost, goals, 0)
    paths, _, _ = pl.paths(cost, goals, int(lengths.max(initial=0)))
    out = []
    for k, g in enumerate(got["goals"]):
        assert g["reachable"] == bool(lengths[k] > 0) and g["cost"] == int(goal_cost[k])
        lin = paths[k, :lengths[k]].astype(np.int64)
        vox = np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1).astype(np.int32)
        assert g["path_vox"].tobytes() == vox.tobytes()
        assert g["path_world"].tobytes() == world_of(pose, got["box"][0], vox).astype(np.float32).tobytes()
        out.append(vox)
    return cost, out


def ask_after_the_roll_out(fus, extent, classes):
    """What the queries return right after the roll out, with the points, start and goals that the tests' conditions
    need -- all chosen on the reference classes."""
    lo, size = extent
    pose = fus.background_pose()
    got = dict(pose=pose, inner=fus.distance_field(box=((0, 0, 0), RES)), df=fus.distance_field(box="world", nearest=True))
    # 50 points, half of them at a volume x below 0, off the voxel centres by less than half a voxel
    rng = np.random.default_rng(528)
    vox = np.concatenate([rng.integers((0, 0, 0), (32, 96, 96), (25, 3)), rng.integers((32, 0, 0), size, (25, 3))]).astype(np.int64)
    got.update(vox=vox, q=fus.query_distance(world_of(pose, lo, vox + rng.uniform(-0.45, 0.45, vox.shape))))
    got["frontiers"] = fus.frontiers(box="world", min_voxels=4, labels=True)
    # the start: the free voxel of the stored slab (volume x below 0) farthest from an occupied voxel, the first such
    d2 = dr.distance_transform(classes, 1 << dr.OCCUPIED, 0).astype(np.int64)
    slab = np.where(classes[:, :, :32] == dr.FREE, d2[:, :, :32], -1)
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(slab)), slab.shape))
    # the goals: the frontier representatives, and the free voxel of the current volume with the largest x
    free = np.argwhere(classes[:, :, 40:] == dr.FREE)
    far = free[np.argmax(free[:, 2])]
    goals = np.array([c["rep"] for c in got["frontiers"]["clusters"]] + [[int(far[2]) + 40, int(far[1]), int(far[0])]], np.int64)
    start = world_of(pose, lo, [[x, y, z]])
    got.update(start_voxel=(x, y, z), slab_clearance=int(slab.max()), goals=goals,
               plan=fus.plan(goals=world_of(pose, lo, goals), start=start, box="world", field=True),
               inner_plan=fus.plan(goals=world_of(pose, lo, goals), start=start, box=((0, 0, 0), RES)),
               auto_plan=fus.plan(box="world", min_voxels=4, field=True))
    return got


def ask_after_the_return(fus):
    got = dict(df=fus.distance_field(box="world", nearest=True), inner=fus.distance_field(box=((0, 0, 0), RES)),
               volumes=volumes(fus, False), world=fus.frontiers(box=((0, 0, 0), RES), min_voxels=1, labels=True))
    fus.set_query_extent("background")
    got["background"] = fus.frontiers(box=((0, 0, 0), RES), min_voxels=1, labels=True)
    fus.set_query_extent("world")
    return got


@pytest.fixture(scope="module")
def walk(dev):
    """Store on, extent world, the policy's rolls by hand; the store restated from the volumes just before each roll.
    After each roll: the extent, the reference classes over it and what the queries return at that moment."""
    fus = new_session()
    fus.set_query_extent("world")
    store, origin, out, at = sr.DictStore(), np.zeros(3, np.int64), {}, 0
    for f, shift in sorted(sr.ROLLS.items()):
        log = frames(fus, at, f + 1, explicit={f: shift})
        pre = log[-1]["pre"]
        sr.roll_with_store(store, pre[0], pre[1], None, tuple(int(v) for v in origin), shift)
        origin += shift
        at = f + 1
        assert fus.background_store_info() == store.info()
        ext = fus.world_extent()
        classes, tiles, stored = reference_classes(fus, store, ext)
        out[f] = dict(extent=ext, want_extent=reference_extent(store, origin), classes=classes, stored=stored,
                      held=len(store.tiles))
        out[f].update(ask_after_the_roll_out(fus, ext, classes) if f == 6 else ask_after_the_return(fus))
    fus.close()
    return out


def test_after_the_roll_out_the_distance_field_covers_the_stored_slab(walk):
    r = walk[6]
    assert r["extent"] == r["want_extent"] == ((-32, 0, 0), (128, 96, 96))
    classes = r["classes"]
    # condition 1, on the reference: the stored tiles hold occupied and free voxels at a volume x below 0
    assert r["stored"].sum() == r["held"] > 0
    slab = classes[:, :, :32]
    assert (slab == dr.OCCUPIED).any() and (slab == dr.FREE).any()
    df = r["df"]
    assert df["box"] == r["extent"] and df["classes"].shape == (96, 96, 128)
    assert df["classes"].tobytes() == classes.tobytes()
    d2 = dr.distance_transform(classes, 1 << dr.OCCUPIED, 0)
    assert df["d2"].tobytes() == d2.tobytes()
    assert df["metres"].tobytes() == dr.metres_of(d2, df["voxel_size"]).tobytes()
    _, near = nr.nearest_separable(dr.sites_of(classes, 1 << dr.OCCUPIED), 0)
    assert df["nearest"].tobytes() == near.tobytes()
    # a clearance next to the old cube face sees the wall that rolled out behind it: the background form does not
    inner = r["inner"]
    assert inner["box"] == ((0, 0, 0), RES) and inner["classes"].tobytes() == classes[:, :, 32:].tobytes()
    cube = dr.distance_transform(classes[:, :, 32:], 1 << dr.OCCUPIED, 0)
    assert (cube >= d2[:, :, 32:]).all() and (cube > d2[:, :, 32:]).any()         # on the reference
    assert inner["d2"].tobytes() == cube.tobytes()
    # the pose of the box's voxel (0, 0, 0)
    assert np.abs(df["pose"][1] - world_of(r["pose"], r["extent"][0], [0, 0, 0])).max() < 1e-5


def test_query_distance_of_world_points_equals_the_field(walk):
    r = walk[6]
    df, q, vox = r["df"], r["q"], r["vox"]
    lo, size = r["extent"]
    assert ((vox[:, 0] + lo[0]) < 0).sum() == 25                          # half of them at a volume x below 0
    assert q["voxel"].tobytes() == vox.astype(np.int32).tobytes() and q["inside"].all()
    at = (vox[:, 2], vox[:, 1], vox[:, 0])
    assert q["class"].tobytes() == df["classes"][at].tobytes()
    assert q["d2"].tobytes() == df["d2"][at].tobytes()
    near = df["nearest"][at].astype(np.int64)
    want = np.where((near >= 0)[:, None], np.stack([near % size[0], near // size[0] % size[1], near // (size[0] * size[1])], 1), -1)
    assert q["nearest_voxel"].tobytes() == want.astype(np.int32).tobytes()
    assert len(np.unique(q["class"])) >= 2


def test_frontiers_and_a_plan_through_the_stored_slab(walk):
    r = walk[6]
    classes, got, goals = r["classes"], r["frontiers"], r["goals"]
    assert got["box"] == r["extent"]
    want = check_frontiers(got, classes, 4)
    assert len(want) >= 1 and r["slab_clearance"] > 0
    plan = r["plan"]
    assert plan["box"] == r["extent"] and tuple(int(v) for v in plan["start_voxels"][0]) == r["start_voxel"]
    assert [g["voxel"] for g in plan["goals"]] == [tuple(int(v) for v in g) for g in goals]
    cost, paths = check_plan(r["pose"], plan, classes)
    # condition 2, on the reference: a plan to at least one goal in the current volume passes through the slab.  The
    # stream's own camera never stands in the slab after the roll, so the START is the chosen one: the free voxel of
    # the slab with the largest clearance
    through = [p for g, p in zip(goals, paths) if len(p) and g[0] >= 32 and (p[:, 0] < 32).any()]
    assert len(through) >= 1
    # the background form cannot start there: the start lies outside its box and is ignored
    inner = r["inner_plan"]
    assert inner["n_starts"] == 0 and not any(g["reachable"] for g in inner["goals"])
    # "frontiers" as goals, from the camera, over the world box
    auto = r["auto_plan"]
    assert auto["frontiers"]["records"].tobytes() == got["records"].tobytes()
    check_plan(r["pose"], auto, classes)


def test_after_the_return_world_equals_the_background_where_they_overlap(walk):
    r = walk[12]
    assert r["extent"] == r["want_extent"]
    (lo, size) = r["extent"]
    assert lo == (0, 0, 0) and size[0] > rr.BG and r["held"] > 0               # what left on the other side is held now
    assert r["df"]["classes"].tobytes() == r["classes"].tobytes()
    inner = r["inner"]
    assert inner["classes"].tobytes() == r["df"]["classes"][:, :, :rr.BG].tobytes()
    t, w, _ = r["volumes"]
    assert inner["classes"].tobytes() == dr.classes_of(t, w).tobytes()
    fw, fb = r["world"], r["background"]
    assert fw["labels"].tobytes() == fb["labels"].tobytes() and fw["records"].tobytes() == fb["records"].tobytes()


def arrays_of(value, prefix=""):
    """Every numpy array of a query's result, by path."""
    out = {}
    if isinstance(value, np.ndarray):
        out[prefix] = value.tobytes()
    elif isinstance(value, dict):
        for k, v in value.items():
            out.update(arrays_of(v, f"{prefix}/{k}"))
    elif isinstance(value, (list, tuple)):
        for k, v in enumerate(value):
            out.update(arrays_of(v, f"{prefix}/{k}"))
    else:
        out[prefix] = repr(value).encode()
    return out


def test_never_rolled_every_query_is_byte_identical_in_both_extents(dev):
    fus = new_session()
    frames(fus, 0, 3, camera=rr.camera_t, render=rr.render)
    assert fus.world_extent() == ((0, 0, 0), RES) and fus.query_extent() == "background"
    box = ((5, 8, 3), (70, 61, 50))
    cam = fus.pose(0)[1].astype(np.float64)
    pts = world_of(fus, box[0], [[10, 10, 10], [60, 50, 40], [30, 30, 5], [1, 59, 48]])
    views = [(np.eye(3), cam), (np.eye(3), cam + np.array([0.1, 0.0, 0.2]))]
    calls = dict(distance_field=lambda: fus.distance_field(box=box, nearest=True, signed=True),
                 frontiers=lambda: fus.frontiers(box=box, min_voxels=1, clearance=0.05, labels=True),
                 plan=lambda: fus.plan(box=box, min_voxels=1, field=True, shortcut=4),
                 cast_rays=lambda: fus.cast_rays(pts[:2], pts[2:], box=box, through_unknown=True, count=("unknown", "free")),
                 view_gain=lambda: fus.view_gain(views, grid=(16, 12), box=box, rays=True),
                 ground_map=lambda: fus.ground_map(box=box))
    got = {}
    for extent in ("background", "world", "background"):
        fus.set_query_extent(extent)
        got.setdefault(extent, []).append({name: arrays_of(call()) for name, call in calls.items()})
    first, again = got["background"]
    world, = got["world"]
    for name in calls:
        assert len(first[name]) >= 3, name
        assert first[name] == again[name], name
        assert world[name] == first[name], (name, [k for k in first[name] if world[name].get(k) != first[name][k]])
    # over the whole extent, which is the background here
    fus.set_query_extent("world")
    a = fus.distance_field(box="world")
    fus.set_query_extent("background")
    b = fus.distance_field()
    assert arrays_of(a) == arrays_of(b)
    fus.close()


def test_world_queries_change_nothing(dev, tmp_path):
    """A session that switches the extent to world and back before the first frame and asks distance_field(box="world")
    after every frame ends where one that never does ends."""
    got = []
    for ask in (False, True):
        fus = new_session(follow=True)
        if ask:
            fus.set_query_extent("world")
            fus.set_query_extent("background")
            fus.set_query_extent("world")
        log = []
        for f in range(sr.FRAMES):
            log += frames(fus, f, f + 1)
            if ask:
                fus.distance_field(box="world")
        path = tmp_path / f"ck{int(ask)}"
        fus.save_checkpoint(str(path))
        got.append((digest(fus, log), hashlib.sha256(path.read_bytes()).hexdigest()))
        fus.close()
    assert got[0] == got[1]


def test_refusals_leave_the_session_untouched(dev):
    from emfusion_amd.pipeline import FusionError
    fus = new_session()
    frames(fus, 0, 3, camera=rr.camera_t, render=rr.render)
    before = volumes(fus, False)
    out_of_cube = ((-8, 0, 0), (24, 16, 16))
    with pytest.raises(ValueError, match="world"):
        fus.distance_field(box="world")                                     # while the extent is the background
    with pytest.raises(ValueError):
        fus.set_query_extent("everything")
    with pytest.raises(FusionError, match="leaves the background") as e:
        fus.distance_field(box=out_of_cube)                                 # off: today's refusal
    assert e.value.code == -4
    fus.set_query_extent("world")
    assert fus.distance_field(box=out_of_cube)["classes"].shape == (16, 16, 24)
    with pytest.raises(FusionError, match="axis of 2049") as e:
        fus.frontiers(box=((-1000, 0, 0), (2049, 8, 8)))
    assert e.value.code == -5
    with pytest.raises(FusionError, match=r"2\^31 - 1") as e:
        fus.plan(box=((-1000, -1000, -100), (2048, 2048, 512)))
    assert e.value.code == -5
    with pytest.raises(FusionError, match="leaves the background") as e:
        fus.planes(box=out_of_cube)                                         # tsdf values: the volume only
    assert e.value.code == -4
    # off the tile: every world query is refused, as world_mesh() is
    fus.set_background_store(False)
    fus.roll_background((4, 0, 0))
    mid = volumes(fus, False)
    for call in (lambda: fus.distance_field(box=out_of_cube), lambda: fus.ground_map(box=((8, 8, 8), (32, 32, 32))),
                 lambda: fus.cast_rays(np.zeros((1, 3)), np.ones((1, 3)), box=out_of_cube)):
        with pytest.raises(FusionError, match="multiples of the tile") as e:
            call()
        assert e.value.code == -4
    after = volumes(fus, False)
    assert bits(mid[0]) == bits(after[0]) and bits(mid[1]) == bits(after[1])
    fus.set_query_extent("background")
    assert fus.distance_field(box=((8, 8, 8), (32, 32, 32)))["classes"].shape == (32, 32, 32)   # off: as before
    del before
    fus.close()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(rr.params(), comm)
        fus.set_query_extent("world")
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.distance_field(box=((-8, 0, 0), (24, 16, 16)))
        code = err.value.code
        ready.wait(timeout=JOIN_S)
        fus.close()
        return code

    assert list(run_ranks(2, body)) == [-4, -4]


def header_box(text):
    """(lo, size) of the "# world extent" comment line of frontiers.txt / plan.txt, or None without one."""
    for line in text.decode().splitlines():
        if line.startswith("# world extent:"):
            v = [int(s) for s in line.replace("# world extent: lo", "").replace("size", "").split()]
            return tuple(v[:3]), tuple(v[3:])
        if not line.startswith("#"):
            break
    return None


def test_write_results_covers_the_world_extent_only_with_the_switch(dev, tmp_path):
    out = {}
    for world in (False, True):
        fus = new_session()
        if world:
            fus.set_query_extent("world")
        fus.setup_output(False, False, exp_distance_field=True, exp_frontiers=True, frontier_min_voxels=4, exp_plan=True)
        frames(fus, 0, 7, explicit={6: sr.ROLLS[6]})
        d = tmp_path / f"out{int(world)}"
        fus.write_results(str(d), volumes=False)
        out[world] = listing(d)
        if world:
            extent = fus.world_extent()
            found = fus.frontiers(box="world", min_voxels=4)
        fus.close()
    assert set(out[True]) == set(out[False]) and {"frontiers.txt", "plan.txt", "distance.bin"} <= set(out[True])
    assert extent == ((-32, 0, 0), (128, 96, 96))
    for name in ("frontiers.txt", "plan.txt"):
        assert header_box(out[False][name]) is None and header_box(out[True][name]) == extent, name
    rows = [l.split() for l in out[True]["frontiers.txt"].decode().splitlines() if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == [c["count"] for c in found["clusters"]] and len(rows) >= 1
    # the cluster boxes are in voxels of the current background: lo + the cluster's own
    assert [tuple(int(v) for v in r[7:10]) for r in rows] == [tuple(a + b for a, b in zip(extent[0], c["lo"])) for c in found["clusters"]]
    assert len(out[True]["distance.bin"]) > len(out[False]["distance.bin"])


def test_the_apps(dev, tmp_path):
    """--world-queries alone is refused before a device is opened; with --follow-camera --follow-store the result files
    are the same set, frontiers.txt and plan.txt over the world extent by their headers."""
    synth = str(ROOT / "apps" / "emfusion_synth")
    for cmd in ([sys.executable, str(ROOT / "apps" / "run_tum.py"), "no-such-sequence", "--world-queries"],
                [sys.executable, str(ROOT / "apps" / "run_tum.py"), "no-such-sequence", "--world-queries", "--follow-camera"],
                [synth, "--world-queries"], [synth, "--world-queries", "--follow-camera"]):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (cmd, p.stderr)
        assert "--world-queries needs --follow-camera --follow-store" in p.stderr, (cmd, p.stderr)
    base = [synth, "--frames", "3", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width", "160", "--height", "120",
            "--follow-camera", "--follow-store", "--frontiers", "--plan"]
    got = {}
    for flag in ((), ("--world-queries",)):
        d = tmp_path / f"synth{len(flag)}"
        r = subprocess.run(base + ["--out", str(d)] + list(flag), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got[len(flag)] = listing(d)
    assert set(got[1]) == set(got[0]) and {"frontiers.txt", "plan.txt"} <= set(got[1])
    for name in ("frontiers.txt", "plan.txt"):
        assert header_box(got[0][name]) is None, name
        lo, size = header_box(got[1][name])
        assert all(a <= 0 for a in lo) and all(a + s >= 128 for a, s in zip(lo, size)), name   # it holds the background
    assert got[1]["mesh_bg.ply"] == got[0]["mesh_bg.ply"]
