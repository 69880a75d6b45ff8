"""The restatement of the voxel rays (tests/rays_reference.py) checked without a device: the two
statements of the walk agree; every visited voxel is touched by the centre-to-centre segment (exact rational slab
test); a walk has d_x + d_y + d_z face steps and ends at b; the fixture rays produce every status; the host-only entry
emf_fusion_view_ray_targets equals the numpy float64 targets exactly; the shortcut greedy on hand-made visibility
tables; and the new entries are declared, bound and exported."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import rays_reference as rr

ROOT = Path(__file__).resolve().parent.parent


def valid(f, t, shape):
    nz, ny, nx = shape
    f, t = np.asarray(f, np.int64), np.asarray(t, np.int64)
    return (f >= 0).all() and (f < (nx, ny, nz)).all() and (np.abs(t - f) <= rr.MAX_DELTA).all()


def check_walk(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    v, w = rr.walk_steps(a, b), rr.walk_sorted(a, b)
    assert v.shape == w.shape == (int(np.abs(b - a).sum()), 3) and (v == w).all()
    if len(v):
        assert (v[-1] == b).all()
        hops = np.abs(np.diff(np.concatenate([a[None], v]), axis=0))
        assert (hops.sum(axis=1) == 1).all() and hops.max() == 1  # face steps only
    return v


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_the_two_walks_agree_on_the_fixture_rays(shape):
    classes = rr.class_field(shape, "sparse")
    f, t = rr.ray_list(shape, classes)
    assert len(f) >= max(rr.COUNTS)
    walked = 0
    for a, b in zip(f, t):
        if valid(a, b, shape):
            check_walk(a, b)
            walked += 1
    assert walked >= 200


def test_the_two_walks_agree_on_random_rays_and_ties():
    rng = np.random.default_rng(0x51)
    for _ in range(400):
        a = rng.integers(-50, 50, 3)
        check_walk(a, a + rng.integers(-40, 41, 3))
    for _ in range(60):  # many exact ties: small common factors
        a = rng.integers(-5, 5, 3)
        check_walk(a, a + rng.integers(1, 4, 3) * rng.integers(-6, 7))
    check_walk((0, 0, 0), (4095, 4095, 4095))
    check_walk((7, 7, 7), (7 - 4095, 7 + 4094, 7 - 1))
    # the tie rule itself: x before y before z
    assert rr.walk_steps((0, 0, 0), (1, 1, 1)).tolist() == [[1, 0, 0], [1, 1, 0], [1, 1, 1]]
    assert rr.walk_steps((0, 0, 0), (-1, 0, 1)).tolist() == [[-1, 0, 0], [-1, 0, 1]]
    assert rr.walk_steps((0, 0, 0), (0, 2, 2)).tolist() == [[0, 1, 0], [0, 1, 1], [0, 2, 1], [0, 2, 2]]


def test_the_walk_is_not_symmetric():
    rng = np.random.default_rng(0x52)
    differ = 0
    for _ in range(300):
        a = rng.integers(0, 12, 3)
        b = a + rng.integers(-8, 9, 3)
        fwd = {tuple(v) for v in rr.walk_sorted(a, b)} | {tuple(a)}
        back = {tuple(v) for v in rr.walk_sorted(b, a)} | {tuple(b)}
        differ += fwd != back
    assert differ > 100  # about 70 % of random short rays


def touches(a, b, v):
    """The closed segment from the centre of a to the centre of b meets the closed cube of voxel v: exact."""
    lo, hi = Fraction(0), Fraction(1)
    for k in range(3):
        p, d = Fraction(int(a[k])), int(b[k]) - int(a[k])
        near, far = Fraction(int(v[k])) - Fraction(1, 2), Fraction(int(v[k])) + Fraction(1, 2)
        if d == 0:
            if not near <= p <= far:
                return False
            continue
        t0, t1 = (near - p) / d, (far - p) / d
        lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
    return lo <= hi


def test_every_visited_voxel_is_touched_by_the_segment():
    rng = np.random.default_rng(0x53)
    for _ in range(250):
        a = rng.integers(-6, 7, 3)
        b = a + rng.integers(-7, 8, 3)
        for v in rr.walk_sorted(a, b):
            assert touches(a, b, v), (a, b, v)


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_the_fixture_rays_produce_every_status(shape):
    """A condition on the fixtures: over the contents, every status the shape can host and a ray that counts; on the
    sparse content alone wherever the box has the room for it."""
    seen, counted = {}, {}
    for content in rr.CONTENTS:
        classes = rr.class_field(shape, content)
        f, t = rr.ray_list(shape, classes)
        rec = rr.cast(classes, f, t, pass_mask=1, count_mask=1)
        seen[content] = set(int(s) for s in rec["status"])
        counted[content] = int(rec["counted"].max())
        assert (rec["steps"] >= rec["counted"]).all()
        groups = rr.group_records(rec, 100)
        assert int(groups["reached"].sum() + groups["blocked"].sum() + groups["left"].sum() + groups["invalid"].sum()) == len(f)
    every = {rr.REACHED, rr.BLOCKED, rr.LEFT, rr.OUTSIDE, rr.INVALID}
    host = every - ({rr.BLOCKED} if np.prod(shape) == 1 else set())  # one voxel: the origin, which is never tested
    assert set().union(*seen.values()) == host
    if np.prod(shape) > 1:
        assert max(counted.values()) > 0
    if np.prod(shape) >= 65:
        assert seen["sparse"] == every and counted["sparse"] > 0


def test_a_group_of_full_rows_exceeds_32_bits():
    shape = (1, 2, 2048)
    classes = rr.class_field(shape, "all_free")
    f, t = rr.ray_list(shape, classes)
    rec = rr.cast(classes, f[:3], t[:3], pass_mask=1, count_mask=1)
    assert rec["steps"][0] == rec["steps"][1] == 2047 and rec["weighted"][0] == 2047 * 2048 * 4095 // 6 > 2.8e9
    assert rr.group_records(rec, 3)["weighted"][0] > 2 ** 32


def test_the_counts_and_groups_hold_every_run_edge():
    """What steers the run scan of the group sums (csrc/wave_ops.hpp): ray i sits in lane i % 64 of wave i // 64 and its
    run is group i // group.  Over COUNTS x GROUPS: a run that ends at lane 63 with the next wave going on in another
    group, a run that is a whole wave, a group split across two waves, every lane a run of its own, and a last wave
    with a single live lane."""
    seen = set()
    for n in rr.COUNTS:
        for group in rr.GROUPS:
            i = np.arange(n)
            g, wave = i // group, i // 64
            for w in range(-(-n // 64)):
                runs = g[wave == w]
                if len(runs) == 64 and runs[0] == runs[-1] and (g == runs[0]).sum() == 64:
                    seen.add("whole wave")
                if len(runs) == 64 and 64 * (w + 1) < n and g[64 * (w + 1)] != runs[-1]:
                    seen.add("ends at lane 63")
                if 64 * (w + 1) < n and g[64 * (w + 1)] == runs[-1]:
                    seen.add("split across two waves")
                if len(runs) == 64 and len(set(runs)) == 64:
                    seen.add("every lane a run")
                if len(runs) == 1 and w == 2:
                    seen.add("one live lane")
    assert seen == {"whole wave", "ends at lane 63", "split across two waves", "every lane a run", "one live lane"}
    assert 129 in rr.COUNTS and {1, 64} <= set(rr.GROUPS)


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    return np.array(m[axis], np.float64)


def view_cases():
    from emfusion_amd import pipeline
    eye3 = np.eye(3)
    bg_t = np.array([0.0, 0.0, 1.26], np.float32)
    rolled = (rot("z", 0.3) @ rot("x", -0.2)).astype(np.float32)
    k = (20.5, 21.25, 15.5, 11.5)
    return [
        # (R, t), K, grid, range, bg_R, bg_t, res, voxel, lo
        ((eye3, np.zeros(3)), k, (32, 24), 3.0, eye3, bg_t, (64, 64, 64), 0.04, (0, 0, 0)),
        (pipeline.look_at((0.3, -0.2, 0.1), (0.0, 0.1, 1.5)), k, (32, 24), 2.0, eye3, bg_t, (64, 64, 64), 0.04, (0, 0, 0)),
        (pipeline.look_at((-0.4, 0.25, 2.2), (0.2, 0.0, 0.7)), (9.0, 9.5, 3.5, 2.5), (8, 6), 1.3, eye3, bg_t, (64, 48, 80), 0.04,
         (3, 0, 7)),
        (pipeline.look_at((0.11, 0.07, 0.3), (1.0, -1.0, 2.0)), k, (32, 24), 3.0, rolled, bg_t, (64, 64, 64), 0.04, (0, 0, 0)),
        (pipeline.look_at((0.5, 0.5, 0.5), (0.0, 0.0, 3.0)), (3.1, 2.9, 2.0, 1.0), (5, 3), 5.11, rolled,
         np.array([0.1, -0.3, 2.56], np.float32), (512, 512, 512), 0.01, (100, 37, 250)),
    ]


def test_view_ray_targets_equal_the_numpy_targets():
    from emfusion_amd import pipeline
    for (R, t), K, grid, rng_m, bg_R, bg_t, res, voxel, lo in view_cases():
        origin, targets, scaled = rr.view_targets(R, t, K, grid, rng_m, bg_R, bg_t, res, voxel, lo)
        # no component within 1e-6 of a half-integer: the equality below cannot hinge on a tie
        frac = np.abs(scaled - np.floor(scaled) - 0.5)
        assert frac.min() > 1e-6, frac.min()
        got_origin, got = pipeline.view_ray_targets(R, t, K, grid, rng_m, bg_R, bg_t, res, voxel, lo)
        assert got.dtype == np.int32 and got.shape == (grid[1], grid[0], 3)
        assert got_origin.tobytes() == origin.tobytes() and got.tobytes() == targets.tobytes()
        assert np.abs(targets - origin).max() <= np.ceil(rng_m / float(np.float32(voxel)))
        # the central ray looks along the camera's z axis
        centre = np.asarray(bg_R, np.float64).T @ np.asarray(R, np.float64)[:, 2]
        mid = (targets[grid[1] // 2, grid[0] // 2] - origin) / (rng_m / float(np.float32(voxel)))
        assert np.abs(mid - centre).max() < 0.12


def test_view_ray_targets_refuses_a_range_above_the_limit():
    from emfusion_amd import pipeline
    with pytest.raises(pipeline.FusionError) as err:
        pipeline.view_ray_targets(np.eye(3), np.zeros(3), (10, 10, 1.5, 1.5), (4, 4), 41.0, np.eye(3), np.zeros(3), (64, 64, 64), 0.01)
    assert err.value.code == -4
    origin, targets = pipeline.view_ray_targets(np.eye(3), np.zeros(3), (10, 10, 1.5, 1.5), (4, 4), 40.9, np.eye(3), np.zeros(3),
                                                (64, 64, 64), 0.01)
    assert np.abs(targets - origin).max() <= rr.MAX_DELTA


def test_the_shortcut_greedy_on_hand_made_tables():
    def table(pairs):
        return lambda i, j: (i, j) in pairs

    assert rr.shortcut_greedy(-1, 4, table(set())) == []
    assert rr.shortcut_greedy(0, 4, table(set())) == [0]
    assert rr.shortcut_greedy(1, 4, table(set())) == [0, 1]
    assert rr.shortcut_greedy(5, 4, table(set())) == [0, 1, 2, 3, 4, 5]  # nothing visible: the path itself
    everything = {(i, j) for i in range(10) for j in range(10)}
    assert rr.shortcut_greedy(9, 4, table(everything)) == [0, 4, 8, 9]    # the window limits a jump
    assert rr.shortcut_greedy(9, 64, table(everything)) == [0, 9]
    assert rr.shortcut_greedy(9, 1, table(everything)) == list(range(10))  # a window of 1 has no ray
    # the largest visible j wins even where a nearer one is hidden; a hidden far one falls back
    assert rr.shortcut_greedy(6, 6, table({(0, 3), (0, 5), (5, 6), (3, 6)})) == [0, 5, 6]
    assert rr.shortcut_greedy(6, 6, table({(0, 2), (2, 4), (2, 5), (5, 6)})) == [0, 2, 5, 6]
    # not symmetric: (j, i) says nothing about (i, j)
    assert rr.shortcut_greedy(3, 3, table({(3, 0), (2, 0)})) == [0, 1, 2, 3]


def test_path_visibility_feeds_the_greedy():
    classes = np.zeros((1, 5, 7), np.uint8)
    classes[0, 0:4, 3] = rr.OCCUPIED  # a wall with a gap at y = 4
    path = [(0, 0, 0), (1, 1, 0), (2, 2, 0), (2, 3, 0), (3, 4, 0), (4, 3, 0), (5, 2, 0), (6, 1, 0)]
    vis = rr.path_visibility(classes, path, 8)
    assert not vis[(0, 7)] and vis[(0, 2)] and not vis[(2, 6)]
    way = rr.shortcut_greedy(len(path) - 1, 8, lambda i, j: vis[(i, j)])
    assert way[0] == 0 and way[-1] == 7 and way == sorted(set(way)) and 4 in way and len(way) < len(path)
    for i, j in zip(way, way[1:]):
        assert j == i + 1 or vis[(i, j)]


def test_the_new_entries_are_declared_bound_and_exported():
    from emfusion_amd import _lib, pipeline
    hip_h = (ROOT / "include" / "emf_hip.h").read_text()
    fusion_h = (ROOT / "include" / "emf_fusion.h").read_text()
    assert int(re.search(r"#define\s+EMF_HIP_ABI_VERSION\s+(\d+)", hip_h).group(1)) == 8
    assert "emf_hip_castVoxelRays" in _lib.declared_symbols() and "emf_hip_castVoxelRays" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["emf_hip_castVoxelRays"]) == 13
    for name, value in (("EMF_RAY_MAX_DELTA", 4095), ("EMF_RAY_REACHED", 0), ("EMF_RAY_BLOCKED", 1), ("EMF_RAY_LEFT", 2),
                        ("EMF_RAY_OUTSIDE", 3), ("EMF_RAY_INVALID", 4)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hip_h).group(1)) == value
    assert (_lib.RAY_MAX_DELTA, _lib.RAY_REACHED, _lib.RAY_BLOCKED, _lib.RAY_LEFT, _lib.RAY_OUTSIDE, _lib.RAY_INVALID) == \
        (rr.MAX_DELTA, rr.REACHED, rr.BLOCKED, rr.LEFT, rr.OUTSIDE, rr.INVALID)
    assert np.dtype(_lib.RAY_RESULT_DTYPE) == rr.RESULT and np.dtype(_lib.RAY_GROUP_DTYPE) == rr.GROUP
    assert rr.RESULT.itemsize == 24 and rr.GROUP.itemsize == 32
    lib, fus = _lib.load(), pipeline.load()
    assert lib.emf_hip_abi_version() == 8
    getattr(lib, "emf_hip_castVoxelRays")
    declared = pipeline.declared_symbols()
    for name in ("emf_fusion_cast_rays", "emf_fusion_view_gain", "emf_fusion_view_ray_targets", "emf_fusion_plan_shortcut",
                 "emf_fusion_copy_plan_shortcut", "emf_fusion_set_plan_shortcut_output"):
        assert name in declared and name in fusion_h and name in fus._emf_sigs
        getattr(fus, name)
    assert "not symmetric" in hip_h.lower() or "NOT symmetric" in hip_h
