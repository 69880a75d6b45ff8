"""The planning kernels (include/emf_hip.h "Planning"; ops.plan_cost, ops.plan_paths) against
tests/plan_reference.py.  Every comparison is tobytes() equality: the cost field, the counters and the paths are
integer functions of the class bytes.  The shapes are the smallest at which a tiled kernel can go wrong for any tile
side up to 32 x 8 x 8 -- one voxel, one tile exactly, one voxel less and one more on each axis, three ragged tiles per
axis, the longest row -- not the workload's."""
import ctypes as C

import numpy as np
import pytest

from tests import plan_reference as pl
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0x5EEDBEE5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
_expected = {}


def expected(shape, content, n_seeds=1, seeds=None, d2=False, **kw):
    """(classes, d2, seeds, cost, (finite, used)) of the restatement, computed once and shared."""
    key = (shape, content, n_seeds, None if seeds is None else tuple(map(tuple, seeds)), d2, tuple(sorted(kw.items())))
    if key not in _expected:
        classes = pl.class_field(shape, content)
        field = pl.d2_field(shape) if d2 else None
        seeds = pl.seeds_of(shape, content, n_seeds) if seeds is None else seeds
        cost, counts = pl.cost_field(classes, seeds, d2=field, **kw)
        for a in (classes, cost) + ((field,) if d2 else ()):
            a.setflags(write=False)
        _expected[key] = (classes, field, seeds, cost, counts)
    return _expected[key]


def run_cost(classes, seeds, d2=None, min_d2=0, mask=1, radius=0, max_cost=0, **kw):
    from emfusion_amd import ops
    return ops.plan_cost(to_dev(classes) if isinstance(classes, np.ndarray) else classes, seeds,
                         d2=to_dev(d2) if isinstance(d2, np.ndarray) else d2, min_d2=min_d2, traverse_mask=mask,
                         seed_radius=radius, max_cost=max_cost, **kw)


def assert_cost(got, want, counts, what):
    host = got.numpy()
    assert host.dtype == np.uint32 and host.shape == want.shape
    assert host.tobytes() == want.tobytes(), (what, int((host != want).sum()), np.argwhere(host != want)[:4].tolist())
    counters = got.counters.numpy().tolist()
    assert counters[pl.CONVERGED] == 1 and counters[pl.ROUNDS] >= 1 and counters[2:] == list(counts), (what, counters)


def goals_of(cost, seeds):
    """A few goals of every kind: finite ones (the first, the last, the dearest, some at random), a seed itself, a
    blocked voxel, an unreached one, and three that are no voxel of the box."""
    nz, ny, nx = cost.shape
    finite = np.argwhere(cost < pl.BLOCKED)
    goals = [(-1, 0, 0), (0, ny, 0), (nx, ny, nz), tuple(seeds[0])]
    if len(finite):
        rng = np.random.default_rng(3)
        dearest = np.unravel_index(np.argmax(np.where(cost < pl.BLOCKED, cost, 0)), cost.shape)
        for z, y, x in [finite[0], finite[-1], dearest, *finite[rng.choice(len(finite), 4)]]:
            goals.append((int(x), int(y), int(z)))
    for value in (pl.BLOCKED, pl.UNREACHED):
        where = np.argwhere(cost == value)
        if len(where):
            goals.append(tuple(int(v) for v in where[len(where) // 2][::-1]))
    return goals


def assert_paths(d_cost, cost, goals):
    """The paths at the capacities 0, 1, the longest path less one, the longest and one more: what is written is the
    restatement's, what is not written stays as it was."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray, DeviceView
    n = len(goals)
    _, full_lengths, _ = pl.paths(cost, goals, 0)
    longest = int(full_lengths.max(initial=0))
    for capacity in sorted({0, 1, max(longest - 1, 0), longest, longest + 1}):
        want, lengths, goal_cost = pl.paths(cost, goals, capacity, poison=np.int32(POISON))
        sink = DeviceArray.from_numpy(np.full(n * capacity + 8, POISON, np.int32))  # 8 more: untouched beyond
        d_lengths = DeviceArray.from_numpy(np.full(n, POISON, np.int32))
        d_goal_cost = DeviceArray.from_numpy(np.full(n, POISON, np.uint32))
        view = DeviceView(sink.ptr, (n, capacity), np.int32) if capacity else None
        ops.plan_paths(d_cost, goals, capacity=capacity, paths=view, lengths=d_lengths, goal_cost=d_goal_cost)
        got = sink.numpy()
        assert d_lengths.numpy().tobytes() == lengths.tobytes(), (capacity, d_lengths.numpy().tolist(), lengths.tolist())
        assert d_goal_cost.numpy().tobytes() == goal_cost.tobytes(), capacity
        assert got[:n * capacity].tobytes() == want.tobytes(), capacity
        assert (got[n * capacity:] == POISON).all()
    host, lengths, goal_cost = ops.plan_paths(d_cost, goals)  # capacity None: the longest path
    want, want_lengths, want_cost = pl.paths(cost, goals, longest, poison=0)
    assert host.shape == (n, longest) and lengths.tobytes() == want_lengths.tobytes() and goal_cost.tobytes() == want_cost.tobytes()
    for g in range(n):
        assert host[g, :lengths[g]].tobytes() == want[g, :lengths[g]].tobytes()


@pytest.mark.parametrize("content", pl.CONTENTS)
@pytest.mark.parametrize("shape", pl.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_cost_and_paths_are_exact(dev, shape, content):
    for n_seeds in (1, 3):
        classes, _, seeds, want, counts = expected(shape, content, n_seeds)
        d_classes = to_dev(classes)
        cost = run_cost(d_classes, seeds)
        assert_cost(cost, want, counts, (shape, content, n_seeds))
        again = run_cost(d_classes, seeds, out=cost)  # a second run into the same buffers gives the same bytes
        assert again is cost
        assert_cost(cost, want, counts, (shape, content, n_seeds, "again"))
        assert d_classes.numpy().tobytes() == classes.tobytes()  # only read
        if n_seeds == 3 or shape == (19, 21, 70):
            assert_paths(cost, want, goals_of(want, seeds))


# every value of every parameter, and the pairs that meet in the code: the bubble with the clearance gate and with
# the mask, the cap with several seeds
PARAMETERS = [dict(radius=1), dict(radius=3), dict(d2=True, min_d2=1), dict(d2=True, min_d2=4, radius=3),
              dict(d2=True, min_d2=0), dict(mask=5), dict(mask=5, d2=True, min_d2=4, n_seeds=3), dict(mask=4, radius=1),
              dict(max_cost=7, n_seeds=3), dict(max_cost=7, radius=3, mask=5), dict(radius=3, n_seeds=3, d2=True, min_d2=1)]


@pytest.mark.parametrize("content", ["random30", "unknown_shell", "pockets", "serpentine"])
@pytest.mark.parametrize("shape", [(9, 17, 65), (19, 21, 70)], ids=lambda s: "x".join(str(v) for v in s))
def test_every_parameter(dev, shape, content):
    largest = None
    for p in PARAMETERS + [dict(max_cost="half", radius=3)]:
        p = dict(p)
        if p.get("max_cost") == "half":  # half the largest finite cost
            full = expected(shape, content, radius=3)[3]
            largest = int(full[full < pl.BLOCKED].max())
            p["max_cost"] = largest // 2
        n_seeds, d2 = p.pop("n_seeds", 1), p.pop("d2", False)
        classes, field, seeds, want, counts = expected(shape, content, n_seeds, d2=d2, **p)
        d_field = to_dev(field) if d2 else None
        cost = run_cost(classes, seeds, d2=d_field, **p)
        assert_cost(cost, want, counts, (shape, content, p))
        if d2:
            assert d_field.numpy().tobytes() == field.tobytes()  # only read
        if "max_cost" in p:  # where the truncated field is finite it is the full field, and the paths are its paths
            full = expected(shape, content, n_seeds, d2=d2, **{k: v for k, v in p.items() if k != "max_cost"})[3]
            assert (want[want < pl.BLOCKED] == full[want < pl.BLOCKED]).all() and (want[want < pl.BLOCKED] <= p["max_cost"]).all()
            assert_paths(cost, want, goals_of(want, seeds)[:8])
    assert largest is not None and largest > 14


def test_ignored_seeds(dev):
    """A seed on an occupied voxel and one outside the box are ignored: the field is the one of the others."""
    shape = (9, 17, 65)
    classes = pl.class_field(shape, "random30")
    occupied = tuple(int(v) for v in np.argwhere(classes == pl.OCCUPIED)[7][::-1])
    good = pl.seeds_of(shape, "random30", 1)
    for seeds, used in (([occupied, good[0], (65, 0, 0)], 1), ([occupied, (0, -1, 0)], 0), ([good[0], good[0]], 2)):
        want, counts = pl.cost_field(classes, seeds, radius=1)
        assert counts[1] == used
        assert_cost(run_cost(classes, seeds, radius=1), want, counts, seeds)
    assert pl.cost_field(classes, [occupied], radius=3)[0].tobytes() == pl.cost_field(classes, [(-5, 0, 0)])[0].tobytes()


def test_a_run_that_is_cut_off_holds_upper_bounds(dev):
    """max_rounds = 1 on the corridor through (19, 21, 70): not converged, no cost below the true one, the seed at 0.
    Only these are asserted -- what a cut-off run holds depends on scheduling.  An unlimited call into the same buffer
    then gives the exact bytes."""
    shape = (19, 21, 70)
    classes, _, seeds, want, counts = expected(shape, "serpentine")
    d_classes = to_dev(classes)
    cost = run_cost(d_classes, seeds, max_rounds=1)
    host, counters = cost.numpy(), cost.counters.numpy().tolist()
    assert counters[pl.CONVERGED] == 0 and counters[pl.ROUNDS] == 1 and counters[pl.SEEDS] == 1
    assert (host >= want).all() and (host == want).sum() < host.size
    assert ((host == pl.BLOCKED) == (want == pl.BLOCKED)).all()
    for x, y, z in seeds:
        assert host[z, y, x] == 0
    assert_cost(run_cost(d_classes, seeds, out=cost), want, counts, "after the cut")


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    from emfusion_amd.devmem import DeviceArray
    lib = _lib.load()
    i3 = lambda *v: (C.c_int32 * 3)(*v)  # noqa: E731

    def cost_rc(size, classes=None, seeds=None, cost=None, scratch=None, counters=None, n_seeds=1, radius=0):
        p = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
        return lib.emf_hip_planCost(p(classes), size, None, 0, 1, p(seeds), n_seeds, radius, 0, 0, p(cost), p(scratch),
                                    p(counters), None)

    # the limits come from the sizes alone, before any buffer is looked at and before any launch
    for size, rc in ((i3(0, 4, 4), E_ARG), (i3(4, -1, 4), E_ARG), (i3(2049, 1, 1), E_LIMIT),
                     (i3(4, 4, 2049), E_LIMIT), (i3(1024, 1024, 513), E_LIMIT),
                     (i3(2048, 2048, 2048), E_LIMIT)):
        assert cost_rc(size) == rc, list(size)
        assert lib.emf_hip_planPaths(None, size, None, 1, 0, None, None, None, None) == rc
        assert lib.emf_hip_planScratchBytes(size) == 0
    assert cost_rc(i3(1024, 1024, 512)) == E_ARG  # 2^29 voxels pass the limit: the NULL buffers are refused
    assert lib.emf_hip_planScratchBytes(i3(1024, 1024, 512)) > 0
    shape = (3, 5, 2)
    classes = to_dev(pl.class_field(shape, "all_free"))
    seeds = DeviceArray.from_numpy(np.zeros(3, np.int32))
    cost = DeviceArray.from_numpy(np.full(shape, 0x11111111, np.uint32))
    counters = DeviceArray.from_numpy(np.full(4, 0x22222222, np.uint32))
    scratch = DeviceArray((lib.emf_hip_planScratchBytes(i3(2, 5, 3)),), np.uint8)
    size = i3(2, 5, 3)
    ok = dict(classes=classes, seeds=seeds, cost=cost, scratch=scratch, counters=counters)
    for bad in (dict(n_seeds=0), dict(n_seeds=-2), dict(radius=-1), dict(classes=None), dict(seeds=None), dict(cost=None),
                dict(scratch=None), dict(counters=None)):
        assert cost_rc(size, **{**ok, **bad}) == E_ARG, bad
    assert (cost.numpy() == 0x11111111).all() and (counters.numpy() == 0x22222222).all()  # nothing was enqueued
    assert cost_rc(size, **ok) == 0 and cost.numpy()[0, 0, 0] == 0
    lengths, goal_cost = DeviceArray.from_numpy(np.full(1, 7, np.int32)), DeviceArray.from_numpy(np.full(1, 7, np.uint32))
    p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
    for n_goals, capacity, paths in ((-1, 0, None), (1, -1, None), (1, 2, None)):
        assert lib.emf_hip_planPaths(p(cost), size, p(seeds), n_goals, capacity, paths, p(lengths), p(goal_cost), None) == E_ARG
    assert lib.emf_hip_planPaths(p(cost), size, None, 1, 0, None, p(lengths), p(goal_cost), None) == E_ARG
    assert lengths.numpy()[0] == 7 and goal_cost.numpy()[0] == 7
    with pytest.raises(Exception):
        ops.plan_cost(classes, [(0, 0, 0)], seed_radius=-1)


def test_chained_with_the_distance_transform_and_the_frontiers(dev):
    """ops.plan on the transform's own d2 towards the representatives ops.frontiers returns for the same gate: every
    kept representative is in T, and its path is the restatement's."""
    from emfusion_amd import ops
    from tests import distance_reference as dr
    from tests import frontier_reference as fr
    classes = np.random.default_rng(0xF7).choice(np.array([0, 0, 0, 0, 0, 0, 1, 2, 2], np.uint8), (12, 20, 70))
    d_classes = to_dev(classes)
    d2 = ops.distance_transform(d_classes, site_mask=2, cap=2)
    want_d2 = dr.distance_transform(classes, 2, 2)
    assert d2.numpy().tobytes() == want_d2.tobytes()
    _, records, counts = ops.frontiers(d_classes, d2=d2, min_d2=4, min_voxels=5)
    _, want_records, want_counts = fr.frontiers(classes, want_d2, 4, 5)
    assert records.tobytes() == want_records.tobytes() and counts == want_counts and counts[0] >= 2
    goals = [tuple(int(v) for v in r["rep"]) for r in records]
    free = np.argwhere((classes == pl.FREE) & (want_d2 >= 4))
    seeds = [tuple(int(v) for v in free[len(free) // 2][::-1])]
    cost, paths, lengths, goal_cost = ops.plan(d_classes, seeds, goals, d2=d2, min_d2=4, seed_radius=1)
    want, want_counts = pl.cost_field(classes, seeds, d2=want_d2, min_d2=4, radius=1)
    assert_cost(cost, want, want_counts, "chained")
    assert all(want[z, y, x] != pl.BLOCKED for x, y, z in goals)  # a representative passed the same gate: it is in T
    want_paths, want_lengths, want_goal_cost = pl.paths(want, goals, int(lengths.max()))
    assert lengths.tobytes() == want_lengths.tobytes() and goal_cost.tobytes() == want_goal_cost.tobytes()
    assert (lengths > 0).any()
    for g in range(len(goals)):
        assert paths[g, :lengths[g]].tobytes() == want_paths[g, :lengths[g]].tobytes()
