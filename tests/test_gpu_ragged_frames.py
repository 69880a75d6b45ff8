"""The per-frame image kernels at image sizes that do not fill their tiles.

The other parity tests run at 160 x 120 and 640 x 480: multiples of the raycast's 16 x 16 tiles and 8 x 8 cells, and (160 x
120) of the tracker's 256-pixel workgroups.  Here the same scenes (tests/frame_scenes.py), the same references and the
same bounds at sizes chosen for the size-dependent branches of k_raycast_batched (cells that hang over the edge, the
ring / no-ring block-to-tile maps, footprints clamped to a one-pixel tile) and of k_track_step (an image shorter than a
row of 1024 + 192 pixels, one that ends among the second pixels of the first three waves, a short last row, pitched
points, rows grouped into passes), and one ragged frame sequence through the host classes."""
import numpy as np
import pytest

from tests import test_gpu_parity as parity
from tests import test_gpu_pipeline as pipeline_tests
from tests.frame_scenes import DeviceTracker, batched_scene, oracle_track, ramped, start_pose, tracking_world
from tests.parity_util import assert_parity, dev_full, to_dev, to_np
from tests.test_gpu_tracking import LEGACY, _fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


def size_id(size):
    return f"{size[0]}x{size[1]}"


def differing(a, b):
    """Names of the state fields in which two LM states differ."""
    fa, fb = _fields(a), _fields(b)
    return [n for n in LEGACY if fa[n] != fb[n]]


# ---- 1. batched raycast ---------------------------------------------------------------------------
# width x height -> tiles; what the size reaches
RAYCAST_SIZES = [(161, 77),   # 11 x 5: last tile column one pixel wide (its second cell column empty), last tile row 13 high
                 (150, 107),  # 10 x 7: 6 valid columns in the last column's first cell, 3 valid rows in the last row's second
                 (47, 33),    # 3 x 3: a ring with exactly one interior tile; last tile row one pixel high
                 (24, 20),    # 2 x 2: no ring
                 (17, 130),   # 2 x 9: no ring although tilesY > 2; second tile column one pixel wide
                 (5, 3)]      # one tile, one partly valid cell
NAMES = ["ray", "vert", "normal", "mask"]


@pytest.fixture(params=RAYCAST_SIZES, ids=size_id)
def scene(request, ops, oracle, dev):
    return batched_scene(ops, oracle, dev, request.param)


def check_images(sc, which, what):
    for k in which:
        for got, want, name in zip(sc.models[k].images, sc.want[k], NAMES):
            assert_parity(to_np(got), want, f"{size_id(sc.size)} {what}: {name} model {k}", exact=True)


def test_scene_is_not_degenerate(scene):
    """The oracle alone: the background is hit in at least half the pixels at every size, every object at least once from
    24 x 20 upward (5 x 3 sees the background only)."""
    w, h = scene.size
    hits = [scene.hits(k) for k in range(3)]
    print(f"{size_id(scene.size)}: oracle hits background {hits[0]}, objects {hits[1:]}")
    assert 2 * hits[0] >= w * h, hits
    if w * h >= 24 * 20:
        assert all(n >= 1 for n in hits[1:]), hits


@pytest.mark.parametrize("lanes,use_flags", [(1, False), (2, False), (4, False), (1, True)],
                         ids=["one_lane", "two_lanes", "four_lanes", "brick_flags"])
@pytest.mark.parametrize("footprints", [False, True], ids=["whole_image", "footprints"])
def test_raycast_batched(ops, scene, footprints, lanes, use_flags):
    """Every pixel of every model's images is written, bit for bit the oracle's, and the samples taken are the oracle's:
    one, two and four lanes per background ray, the flag-aware march (MODE 0), objects with and without footprints."""
    sc = scene
    w, h = sc.size
    table = ops.upload_models([m.table_entry() for m in sc.models])
    for m in sc.models:
        m.poison()
    st = dev_full((4,), 0, np.uint64)
    ops.raycast_batched(table, sc.poses, [m.res for m in sc.models], w, h, sc.K, stats=st, use_brick_flags=use_flags,
                        voxel_sizes=[m.vox for m in sc.models] if footprints else None, lanes=lanes)
    check_images(sc, range(3), "batched")
    assert int(to_np(st)[0]) == sc.samples(range(3))


@pytest.mark.parametrize("footprints", [False, True], ids=["whole_image", "footprints"])
def test_raycast_of_an_objects_only_table(ops, scene, footprints):
    sc = scene
    w, h = sc.size
    objs = sc.models[1:]
    table = ops.upload_models([m.table_entry() for m in objs])
    for m in objs:
        m.poison()
    st = dev_full((4,), 0, np.uint64)
    ops.raycast_batched(table, sc.poses[1:], [m.res for m in objs], w, h, sc.K, stats=st, objects_only=True,
                        voxel_sizes=[m.vox for m in objs] if footprints else None)
    check_images(sc, (1, 2), "objects only")
    assert int(to_np(st)[0]) == sc.samples((1, 2))


def test_raycast_far_bounds(ops, scene):
    """emf_hip_raycastFarBounds where cells hang over the image's edge: an array of 2 x 2 cells per tile, finite and
    non-negative, the same from scanned sign maps and from relevant-tile lists; marches cut at it leave the oracle's
    images, with one, two and four lanes per background ray."""
    sc = scene
    w, h = sc.size
    res = [m.res for m in sc.models]
    try:
        for m in sc.models:
            m.d_sign = dev_full((ops.sign_map_bytes(m.res),), 7, np.uint8)
            ops.rebuild_sign_maps(m.d_tsdf, m.d_sign)
        table = ops.upload_models([m.table_entry() for m in sc.models])
        scanned = ops.raycast_far_bounds(table, sc.poses, res, w, h, sc.K)
        for m in sc.models:
            m.d_rel = dev_full((ops.relevant_tile_words(m.res),), 0xdead, np.uint32)
        table = ops.upload_models([m.table_entry() for m in sc.models])
        ops.update_relevant_tiles(table, res)
        listed = ops.raycast_far_bounds(table, sc.poses, res, w, h, sc.K, scan_mask=0)
        b = to_np(scanned)
        assert b.shape == (3, 2 * ((h + 15) // 16), 2 * ((w + 15) // 16))
        assert np.isfinite(b).all() and (b >= 0).all()
        assert np.array_equal(to_np(listed), b)
        for bounds, what in ((scanned, "scanned bounds"), (listed, "listed bounds")):
            for lanes in (1, 2, 4):
                for m in sc.models:
                    m.poison()
                ops.raycast_batched(table, sc.poses, res, w, h, sc.K, far_bounds=bounds, voxel_sizes=[m.vox for m in sc.models],
                                    lanes=lanes)
                check_images(sc, range(3), f"{what}, {lanes} lanes")
    finally:
        for m in sc.models:
            m.d_sign = m.d_rel = None


def test_raycast_per_volume(ops, scene):
    """k_raycast, the per-volume launch, against the same oracle images.  Its ray lengths are an input and it writes hits
    only (the reference's contract): it starts from cleared images, like the oracle."""
    sc = scene
    for k, (m, (R, t)) in enumerate(zip(sc.models, sc.poses)):
        m.clear()
        ops.raycast_tsdf(m.d_tsdf, None, m.d_wts, m.d_vmask if m.is_obj else None, m.d_ray, m.d_vert, m.d_nrm, m.d_hit, R, t,
                         sc.K, m.vox, m.trunc)
        check_images(sc, (k,), "per volume")


def test_composite_and_visibility_with_a_row_tail(oracle, ops, dev):
    """The composite / visibility pair and the occlusion mask at 161 x 77: their 64 x 4 pixel tiles get a tail in y."""
    parity.check_composite_and_visibility(oracle, ops, dev, 2, W=161, H=77)
    parity.check_occluded_mask(oracle, ops, dev, W=161, H=77)


# ---- 2. tracker -------------------------------------------------------------------------------------
# rows of 1024 + 192 pixels: lanes 0..1023 take one pixel each, the lanes of waves 0..2 a second one
TRACK_SIZES = [(37, 23),   # 851 pixels: fewer than a workgroup has lanes
               (40, 28),   # 1120: ends among the second pixels of row 0 (wave 0's are all there, wave 1's half, wave 2's none)
               (47, 33),   # 1551: two rows, the second of 335 pixels
               (161, 77),  # 12397: 11 rows, the last of 237 pixels; odd width
               (8, 8)]     # 64: one wave holds the image
PITCHED_SIZES = [(161, 77), (40, 28)]


@pytest.mark.parametrize("which", [[0], [1], [0, 1]], ids=["background", "object", "both"])
@pytest.mark.parametrize("size", TRACK_SIZES, ids=size_id)
def test_tracker_first_iteration_and_twelve(oracle, ops, dev, size, which):
    """One iteration within the bounds of test_first_iteration_matches_oracle, twelve within those of
    test_speculation_miss_stays_in_parity (tests/test_gpu_tracking.py), for each model alone and both in lockstep."""
    world = tracking_world(oracle, size)
    first = DeviceTracker(ops, world, which).iterate(1)
    final = DeviceTracker(ops, world, which).iterate(12)
    for st, st12, k in zip(first, final, which):
        snaps = oracle_track(oracle, world, k, 12)
        o1, h = snaps[1], snaps[1]["history"][0]
        A, b = np.array(st.A, np.float32).reshape(6, 6), np.array(st.b, np.float32)
        assert np.abs(h["A"]).max() > 1.0
        assert np.abs(A - h["A"]).max() <= 2e-5 * np.abs(h["A"]).max(), "Hessian"
        assert np.abs(b - h["b"]).max() <= 2e-5 * max(np.abs(h["b"]).max(), 1e-3), "gradient"
        assert abs(st.err - h["err"]) <= 1e-5 * h["err"], "error at the current pose"
        x = np.array(st.x, np.float32)
        assert np.abs(x - h["x"]).max() <= 1e-4 * np.abs(h["x"]).max(), "LM step"
        assert abs(st.errNew - h["err_new"]) <= 1e-5 * h["err_new"], "error at the trial pose"
        assert (st.rho > 0) == (h["rho"] > 0) and abs(st.rho - h["rho"]) <= 1e-2 * abs(h["rho"]) + 1e-3
        assert st.iterations == 1 and st.accepted == o1["accepted"]
        assert np.allclose(np.array(st.R, np.float32).reshape(3, 3), o1["R"], atol=1e-6)
        assert np.allclose(np.array(st.t, np.float32), o1["t"], atol=1e-6)
        assert abs(st.mu - o1["mu"]) <= 1e-4 * o1["mu"]
        o12 = snaps[12]
        print(f"{size_id(size)} model {k}: {o12['accepted']} of 12 steps accepted")
        assert st12.iterations == 12 and st12.accepted == o12["accepted"] and o12["accepted"] >= 3
        assert np.abs(np.array(st12.R, np.float32).reshape(3, 3) - o12["R"]).max() < 1e-5
        assert np.abs(np.array(st12.t, np.float32) - o12["t"]).max() < 1e-5


@pytest.mark.parametrize("which", [[0], [1], [0, 1]], ids=["background", "object", "both"])
@pytest.mark.parametrize("size", PITCHED_SIZES, ids=size_id)
def test_tracker_with_pitched_points(oracle, ops, dev, size, which):
    """Points with padded rows (k_track_step's per-pixel y / x addressing): the states of the dense run bit for bit, and the
    weight images of the finished stage bit for bit the oracle's chain at its final pose."""
    w, h = size
    world = tracking_world(oracle, size)
    dense = DeviceTracker(ops, world, which).iterate(12)
    dt = DeviceTracker(ops, world, which, pad_cols=5)
    assert dt.points.padded
    pitched = dt.iterate(12)
    for a, b, k in zip(dense, pitched, which):
        assert a.iterations == 12 and not differing(a, b), (k, differing(a, b))
    if len(which) > 1:
        return
    k, st = which[0], pitched[0]
    huber, track = dev_full((1, h, w), -1.0), dev_full((1, h, w), -1.0)
    ops.track_weight_images(dt.table, dt.states, 1, dt.points, dt.params, dt.scratch, dt.per_model, huber, track)
    v = world["vols"][k]
    R, t = np.array(st.R, np.float32), np.array(st.t, np.float32)
    vals = oracle.get_volume_vals(v["tsdf"], world["points"], R, t, v["vox"])
    raw = oracle.get_volume_vals(v["wts"], world["points"], R, t, v["vox"])
    tw, comb = oracle.tracking_weights(vals, raw, world["assoc"][k], 0.2, 64.0)
    assert (tw.reshape(-1) > 0).any() and (comb.reshape(-1) > 0).any()
    assert to_np(huber).shape == to_np(track).shape == (1, h, w)
    assert_parity(to_np(huber)[0], tw.reshape(h, w), "Huber weights", exact=True)
    assert_parity(to_np(track)[0], comb.reshape(h, w), "combined tracking weights", exact=True)


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "pitched"])
@pytest.mark.parametrize("size", PITCHED_SIZES, ids=size_id)
def test_pose_gradients(oracle, ops, dev, size, pad):
    """k_pose_gradients with a partial last workgroup."""
    w, h = size
    world = tracking_world(oracle, size)
    v = world["vols"][0]
    R, t = start_pose(world, 0)
    want = oracle.compute_pose_gradients(v["tsdf"], None, world["points"], R, t, v["vox"])
    out = dev_full((h * w, 6), 9.0)
    ops.compute_pose_gradients(to_dev(v["tsdf"]), None, to_dev(world["points"], pad_cols=pad), R, t,
                               float(np.float32(v["vox"])), out)
    assert (np.abs(want).sum(1) > 0).sum() > w * h // 4
    assert_parity(to_np(out), want, "pose gradients", exact=True)


def test_weight_maximum_launch_at_a_ragged_size(oracle, ops, dev, monkeypatch):
    """EMF_TRACK_RESCALE=0 (k_track_maxw, with a partial last workgroup) on the ramped weights at 161 x 77: the poses stay
    with the oracle as in test_speculation_miss_stays_in_parity."""
    monkeypatch.setenv("EMF_TRACK_RESCALE", "0")
    w2 = ramped(tracking_world(oracle, (161, 77)))
    iters = 12
    dt = DeviceTracker(ops, w2, [0])
    st = dt.iterate(iters)[0]
    calls = 1
    assert 0 < st.iterations < iters  # every accepted step costs a launch more than the call provides for
    while st.iterations < iters and not st.converged:
        st = dt.iterate(iters - st.iterations)[0]
        calls += 1
        assert calls < 40
    assert st.iterations == iters and st.haveTrial == 0
    ot = oracle_track(oracle, w2, 0, iters)[iters]
    assert st.accepted == ot["accepted"] and ot["accepted"] >= 3
    assert np.abs(np.array(st.R, np.float32).reshape(3, 3) - ot["R"]).max() < 1e-5
    assert np.abs(np.array(st.t, np.float32) - ot["t"]).max() < 1e-5
    assert abs(st.mu - ot["mu"]) <= 1e-3 * ot["mu"]


GROUPED = (251, 157)  # 39407 pixels: 33 rows


@pytest.mark.parametrize("copies", [12, 32])
@pytest.mark.parametrize("k", [0, 1], ids=["background", "object"])
def test_rows_grouped_into_passes_give_the_same_sums(oracle, ops, dev, k, copies):
    """A table that lists one model `copies` times leaves each copy 1 / copies of the launch's workgroups: with 32 copies
    on a 256-CU device 8 workgroups for 33 rows (some take 5: two passes of up to kMaxRows), with 12 an uneven single pass
    of two rows.  The sums depend neither on the grid nor on the grouping: every copy's state is the state of the model
    run alone (a row per workgroup), bit for bit -- and that one agrees with the oracle within the bounds of
    test_large_image_many_blocks."""
    world = tracking_world(oracle, GROUPED)
    one = DeviceTracker(ops, world, [k]).iterate(3)[0]
    ot = oracle_track(oracle, world, k, 3)[3]
    h = ot["history"][-1]
    assert one.iterations == 3 and one.accepted == ot["accepted"]
    A = np.array(one.A, np.float32).reshape(6, 6)
    assert np.abs(A - h["A"]).max() <= 2e-5 * np.abs(h["A"]).max(), "Hessian of the third iteration"
    assert abs(one.errNew - h["err_new"]) <= 2e-5 * h["err_new"]
    assert np.allclose(np.array(one.R, np.float32).reshape(3, 3), ot["R"], atol=2e-6)
    assert np.allclose(np.array(one.t, np.float32), ot["t"], atol=2e-6)
    for i, st in enumerate(DeviceTracker(ops, world, [k] * copies).iterate(3)):
        assert not differing(st, one), (i, differing(st, one))


# ---- 3. the host classes ----------------------------------------------------------------------------
# the scenario, the assertions, tolerances and budgets of tests/test_gpu_pipeline.py at 150 x 107 (the sharded paths'
# band and slot alignment at such sizes is not settled: they stay at 160 x 120)

@pytest.fixture(scope="module", params=["batched", "per_volume"])
def run(request, oracle, dev):
    yield from pipeline_tests.run_scenario(request.param, oracle, W=150, H=107)


from tests.test_gpu_pipeline import (test_association_weights, test_background_volume, test_frames_were_processed,  # noqa: E402,F401
                                     test_march_sample_count_close_to_oracle, test_object_volumes_and_foreground,
                                     test_raycast_and_segmentation, test_visible_sets_match_every_frame)
