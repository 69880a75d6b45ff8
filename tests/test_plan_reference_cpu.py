"""The yardstick of the planning tests (tests/plan_reference.py; include/emf_hip.h "Planning") checked
on its own, without a GPU: the heap Dijkstra against scipy's on the same graph, the closed form of open space, the
properties of the paths, the truncation rule, and what the named contents hold."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

from tests import plan_reference as pl

SHAPE = (9, 17, 65)


def scipy_cost(classes, seeds, **kw):
    """The same field through scipy.sparse.csgraph.dijkstra (min_only): integer weights are exact in float64."""
    t = pl.traversable(classes, kw.get("d2"), kw.get("min_d2", 0), kw.get("mask", 1), seeds, kw.get("radius", 0))
    nz, ny, nx = classes.shape
    idx = np.arange(classes.size).reshape(classes.shape)
    rows, cols, wts = [], [], []
    for (dz, dy, dx), w in zip(pl.MOVES, pl.WEIGHTS):
        src = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
        dst = (slice(max(0, dz), nz - max(0, -dz)), slice(max(0, dy), ny - max(0, -dy)), slice(max(0, dx), nx - max(0, -dx)))
        both = t[src] & t[dst]
        rows.append(idx[src][both])
        cols.append(idx[dst][both])
        wts.append(np.full(int(both.sum()), w, np.float64))
    graph = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(classes.size,) * 2).tocsr()
    used = [(z * ny + y) * nx + x for x, y, z in pl.used_seeds(classes, seeds)]
    cost = np.full(classes.size, pl.BLOCKED, np.uint32)
    cost[t.reshape(-1)] = pl.UNREACHED
    if used:
        d = dijkstra(graph, directed=True, indices=used, min_only=True)
        reached = np.isfinite(d) & t.reshape(-1)
        cost[reached] = d[reached].astype(np.uint32)
    return cost.reshape(classes.shape)


@pytest.mark.parametrize("content", pl.CONTENTS)
def test_the_heap_dijkstra_is_scipys(content):
    for shape in ((3, 5, 2), (9, 17, 65)):
        classes, d2 = pl.class_field(shape, content), pl.d2_field(shape)
        for kw in (dict(), dict(radius=3), dict(mask=5, d2=d2, min_d2=1), dict(radius=1, d2=d2, min_d2=4)):
            for n in (1, 3):
                seeds = pl.seeds_of(shape, content, n)
                got, (finite, used) = pl.cost_field(classes, seeds, **kw)
                want = scipy_cost(classes, seeds, **kw)
                assert got.tobytes() == want.tobytes(), (shape, content, kw, n)
                assert finite == int((want < pl.BLOCKED).sum()) and used == len(pl.used_seeds(classes, seeds))


def test_open_space_has_the_closed_form():
    """With sorted |dx|, |dy|, |dz| = hi >= mid >= lo: lo corner moves, mid - lo edge moves, hi - mid face moves."""
    classes = pl.class_field(SHAPE, "all_free")
    for seed in ((0, 0, 0), pl.centre(SHAPE), (64, 3, 8)):
        cost, (finite, used) = pl.cost_field(classes, [seed])
        z, y, x = np.meshgrid(*(np.arange(n) for n in SHAPE), indexing="ij")
        d = np.sort(np.stack([abs(x - seed[0]), abs(y - seed[1]), abs(z - seed[2])]), axis=0)
        want = 3 * (d[2] - d[1]) + 4 * (d[1] - d[0]) + 5 * d[0]
        assert cost.tobytes() == want.astype(np.uint32).tobytes()
        assert finite == classes.size and used == 1


@pytest.mark.parametrize("content", ["random30", "serpentine", "unknown_shell", "pockets"])
def test_paths_walk_through_T_down_to_a_seed(content):
    classes = pl.class_field(SHAPE, content)
    seeds = pl.seeds_of(SHAPE, content, 3)
    radius = 3 if content == "unknown_shell" else 0
    cost, _ = pl.cost_field(classes, seeds, radius=radius)
    t = pl.traversable(classes, None, 0, 1, seeds, radius)
    nz, ny, nx = SHAPE
    finite = np.argwhere(cost < pl.BLOCKED)
    pick = finite[np.random.default_rng(5).choice(len(finite), 40)]
    goals = pick[:, ::-1]
    longest = 4 * (nx + ny + nz) * 4
    walks, lengths, goal_cost = pl.paths(cost, goals, longest)
    used = {(z * ny + y) * nx + x for x, y, z in pl.used_seeds(classes, seeds)}
    for g, (z, y, x) in enumerate(pick):
        assert goal_cost[g] == cost[z, y, x] and 1 <= lengths[g] <= longest
        p = walks[g, :lengths[g]].astype(np.int64)
        assert p[0] == (z * ny + y) * nx + x and int(p[-1]) in used
        xyz = np.stack([p % nx, p // nx % ny, p // (nx * ny)], axis=1)
        assert t[xyz[:, 2], xyz[:, 1], xyz[:, 0]].all()
        step = np.abs(np.diff(xyz, axis=0))
        assert (step.max(axis=1, initial=0) <= 1).all() and (step.sum(axis=1) >= 1).all()  # 26-neighbours
        assert int((2 + (step ** 2).sum(axis=1)).sum()) == goal_cost[g]  # the weights sum to the cost
        f, e, c = pl.step_counts(p, SHAPE)
        assert 3 * f + 4 * e + 5 * c == goal_cost[g] and f + e + c == lengths[g] - 1
    # goals that are no voxel of the box, blocked or unreached have no path
    blocked = np.argwhere(cost == pl.BLOCKED)
    odd = [(-1, 0, 0), (nx, 0, 0), (0, 0, nz)] + ([tuple(blocked[0][::-1])] if len(blocked) else [])
    walks, lengths, goal_cost = pl.paths(cost, odd, 4)
    assert (walks == -1).all() and (lengths == 0).all() and (goal_cost == pl.BLOCKED).all()


@pytest.mark.parametrize("content", ["all_free", "random30", "serpentine"])
def test_the_truncated_field_is_the_full_field_where_finite(content):
    classes = pl.class_field(SHAPE, content)
    seeds = pl.seeds_of(SHAPE, content, 1)
    full, _ = pl.cost_field(classes, seeds)
    largest = int(full[full < pl.BLOCKED].max())
    for cap in (7, largest // 2):
        cut, (finite, _) = pl.cost_field(classes, seeds, max_cost=cap)
        want = np.where((full < pl.BLOCKED) & (full > cap), pl.UNREACHED, full).astype(np.uint32)
        assert cut.tobytes() == want.tobytes()
        assert finite == int((full <= cap).sum())


def test_the_contents_are_what_they_claim():
    def field(content, n=1, **kw):
        classes = pl.class_field(SHAPE, content)
        return classes, pl.cost_field(classes, pl.seeds_of(SHAPE, content, n), **kw)

    voxels = 9 * 17 * 65
    classes, (cost, (finite, used)) = field("all_free")
    assert finite == voxels and used == 1 and cost.max() == 3 * (32 - 8) + 4 * (8 - 4) + 5 * 4
    classes, (cost, (finite, used)) = field("all_blocked")
    assert finite == 0 and used == 0 and (cost == pl.BLOCKED).all()  # the seed is occupied: ignored
    classes, (cost, (finite, used)) = field("random30", 3)
    assert used == 3 and finite == int((classes == pl.FREE).sum()) == 6925  # 26 moves reach every free voxel
    assert abs((classes != pl.FREE).mean() - 0.3) < 0.01
    classes, (cost, (finite, used)) = field("serpentine")
    corridor = int((classes == pl.FREE).sum())
    assert finite == corridor == 2969 > voxels // 5  # a walk through the whole box ...
    assert cost[cost < pl.BLOCKED].max() == 8728 > 0.98 * 3 * (corridor - 1)  # ... nearly all of it in face moves
    classes, (cost, (finite, used)) = field("pockets")
    assert (cost == pl.UNREACHED).sum() == 9 * 17 * 32 and finite == 9 * 17 * 32  # behind the wall: no seed reaches
    classes, (cost, (finite, used)) = field("corner_only")
    assert finite == 2 and sorted(cost[cost < pl.BLOCKED].tolist()) == [0, 5]
    classes, (cost, (finite, used)) = field("row_ends")
    # neighbours in linear index are none in space: the seed at the end of row 0 does not reach the start of row 1
    # (an odd ny makes equal row ends of adjacent slices edge neighbours, so half of them are reached)
    assert (classes == pl.FREE).sum() == 9 * 17 and finite == 77 and cost[0, 1, 0] == pl.UNREACHED
    narrow = pl.class_field((4, 5, 2), "row_ends")
    assert pl.cost_field(narrow, [(1, 0, 0)])[1][0] == 20  # ... unless the box is two voxels wide
    for radius, reached in ((0, 1), (1, 7), (3, voxels - 8)):
        classes, (cost, (finite, used)) = field("unknown_shell", radius=radius)
        assert used == 1 and classes[pl.centre(SHAPE)[::-1]] == pl.UNKNOWN
        assert finite == reached, (radius, finite)  # only the bubble of radius 3 opens the way out; the block's 8 corners stay blocked
