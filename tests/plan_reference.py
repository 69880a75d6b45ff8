"""Restatement of include/emf_hip.h "Planning"  for the tests.

The query runs over a box of class bytes in (z, y, x) order; what lies outside the box does not exist.

Traversable set T.  A voxel v is in T if either holds:
  gate    (1 << class[v]) & traverse_mask is non-zero (a class byte above 2 is in no mask) and, where a d2 array is
          passed with min_d2 > 0, d2[v] >= min_d2 (FAR passes);
  bubble  class[v] != OCCUPIED and v lies within seed_radius voxels of a used seed (integer |v - s|^2 <= radius^2).
Seeds: (x, y, z) voxels; one outside the box or on an OCCUPIED voxel is ignored, the others are "used".
Moves: 26-connected between two voxels of T, weights 3 (face), 4 (edge), 5 (corner).
Cost field (u32): 0 at a used seed, else the least total weight from any used seed; UNREACHED for a voxel of T no seed
reaches or whose cost exceeds max_cost (> 0); BLOCKED outside T.
Paths: from a goal with a finite cost, step to the neighbour n with cost[n] + w == cost[here], ties to the smallest
linear index (z * ny + y) * nx + x, until the cost is 0.

cost_field is a binary-heap Dijkstra in plain Python over a padded flat array; everything is an integer, so the tests
compare bytes."""
import heapq

import numpy as np

from tests.frontier_reference import serpentine_path

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
FAR = 0x7fffffff
UNREACHED, BLOCKED = 0xffffffff, 0xfffffffe
CONVERGED, ROUNDS, FINITE, SEEDS = 0, 1, 2, 3

# (nz, ny, nx): the smallest at which a tiled kernel can go wrong for any tile side up to 32 x 8 x 8
SHAPES = [(1, 1, 1), (1, 1, 65), (3, 5, 2), (8, 8, 32), (7, 8, 32), (9, 8, 32), (8, 7, 32), (8, 9, 32), (8, 8, 31),
          (8, 8, 33), (9, 17, 65), (19, 21, 70), (1, 2, 2048)]
CONTENTS = ["all_free", "all_blocked", "random30", "serpentine", "pockets", "corner_only", "row_ends", "unknown_shell"]

# (dz, dy, dx) in ascending linear-index order, and the weight of each move
MOVES = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
WEIGHTS = [2 + dz * dz + dy * dy + dx * dx for dz, dy, dx in MOVES]


def centre(shape):
    nz, ny, nx = shape
    return (nx // 2, ny // 2, nz // 2)


def class_field(shape, content):
    """u8 (nz, ny, nx) classes of a named content."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = np.full(shape, OCCUPIED, np.uint8)
    if content == "all_free":
        c[:] = FREE
    elif content == "all_blocked":
        pass
    elif content == "random30":  # 30 % of the voxels are no free space; 3 is no class
        c = np.random.default_rng([0x9A, nz, ny, nx]).choice(
            np.array([FREE] * 14 + [OCCUPIED] * 4 + [UNKNOWN, 3], np.uint8), shape)
        for sx, sy, sz in seeds_of(shape, content, 3):
            c[sz, sy, sx] = FREE
    elif content == "serpentine":
        # a one voxel wide corridor through the whole box between walls: it leaves a tile along x and comes back into
        # it a row later at a lower cost than a neighbour tile offered before, so tiles re-activate
        c[tuple(np.array(serpentine_path(shape)).T)] = FREE
    elif content == "pockets":
        # free space cut in two by a wall across the longest axis: the far half is a region the first seed, which lies
        # before the wall, does not reach
        c[:] = FREE
        axis = int(np.argmax(shape))
        cut = [slice(None)] * 3
        cut[axis] = shape[axis] // 2
        if shape[axis] >= 3:
            c[tuple(cut)] = OCCUPIED
    elif content == "corner_only":  # two free voxels that touch at a corner only (where the box has the room)
        c[0, 0, 0] = FREE
        c[min(1, nz - 1), min(1, ny - 1), min(1, nx - 1)] = FREE
    elif content == "row_ends":
        # free at the last voxel of every even row and the first of every odd row (rows counted through the slices):
        # neighbours in linear index, neighbours in space only where the box is two voxels wide
        row = z * ny + y
        c[(row % 2 == 0) & (x == nx - 1)] = FREE
        c[(row % 2 == 1) & (x == 0)] = FREE
    elif content == "unknown_shell":
        # free space with a block of unknown voxels (Chebyshev radius 2) around the centre, where the seed is: the
        # near field no sensor sees.  The seed reaches the free space only through a bubble of radius 3.
        cx, cy, cz = centre(shape)
        c[:] = FREE
        c[(abs(x - cx) <= 2) & (abs(y - cy) <= 2) & (abs(z - cz) <= 2)] = UNKNOWN
    else:
        raise AssertionError(content)
    return c


def seeds_of(shape, content, n=1):
    """The first n of three seeds (x, y, z) that suit the content."""
    nz, ny, nx = shape
    if content in ("serpentine", "corner_only", "all_blocked"):
        first = (0, 0, 0)
    elif content == "row_ends":
        first = (nx - 1, 0, 0)
    elif content == "pockets":
        first = (0, 0, 0)
    else:
        first = centre(shape)
    return [first, (nx - 1, ny - 1, nz - 1), (nx // 3, ny // 2, 0)][:n]


def d2_field(shape, seed=11):
    """A random i32 "d2" with values around the gates the tests use, FAR among them."""
    rng = np.random.default_rng([seed, *shape])
    d2 = rng.integers(0, 7, shape).astype(np.int32)
    d2[rng.random(shape) < 0.1] = FAR
    return d2


def used_seeds(classes, seeds):
    nz, ny, nx = classes.shape
    return [(int(x), int(y), int(z)) for x, y, z in np.asarray(seeds, np.int64).reshape(-1, 3)
            if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and classes[z, y, x] != OCCUPIED]


def traversable(classes, d2=None, min_d2=0, mask=1, seeds=(), radius=0):
    """bool (nz, ny, nx): T."""
    nz, ny, nx = classes.shape
    t = np.zeros(classes.shape, bool)
    for k in range(3):
        if mask & (1 << k):
            t |= classes == k
    if d2 is not None and min_d2 > 0:
        t &= d2.astype(np.int64) >= min_d2
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for sx, sy, sz in used_seeds(classes, seeds):
        t |= (classes != OCCUPIED) & ((x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2 <= radius * radius)
    return t


def cost_field(classes, seeds, d2=None, min_d2=0, mask=1, radius=0, max_cost=0):
    """(cost u32 (nz, ny, nx), (voxels with a finite cost, seeds used)) by a binary-heap Dijkstra."""
    nz, ny, nx = classes.shape
    t = traversable(classes, d2, min_d2, mask, seeds, radius)
    used = used_seeds(classes, seeds)
    py, pz = nx + 2, (nx + 2) * (ny + 2)  # strides of the array padded by one blocked voxel on every side
    open_ = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    open_[1:-1, 1:-1, 1:-1] = t
    open_ = open_.reshape(-1).tolist()
    offsets = [dz * pz + dy * py + dx for dz, dy, dx in MOVES]
    steps = list(zip(offsets, WEIGHTS))
    inf = 1 << 62
    dist = [inf] * len(open_)
    heap = []
    for sx, sy, sz in used:
        i = (sz + 1) * pz + (sy + 1) * py + sx + 1
        if dist[i]:
            dist[i] = 0
            heap.append((0, i))
    heapq.heapify(heap)
    while heap:
        d, i = heapq.heappop(heap)
        if d != dist[i]:
            continue
        for o, w in steps:
            j = i + o
            if open_[j]:
                e = d + w
                if e < dist[j] and (max_cost <= 0 or e <= max_cost):
                    dist[j] = e
                    heapq.heappush(heap, (e, j))
    d = np.array(dist, np.int64).reshape(nz + 2, ny + 2, nx + 2)[1:-1, 1:-1, 1:-1]
    cost = np.where(t, np.where(d < inf, d, UNREACHED), BLOCKED).astype(np.uint32)
    return cost, (int((cost < BLOCKED).sum()), len(used))


def paths(cost, goals, capacity, poison=-1):
    """(paths i32 (n, capacity) with `poison` where nothing is written, lengths i32 (n,), goal_cost u32 (n,))."""
    nz, ny, nx = cost.shape
    goals = np.asarray(goals, np.int64).reshape(-1, 3)
    out = np.full((len(goals), capacity), poison, np.int32)
    lengths = np.zeros(len(goals), np.int32)
    goal_cost = np.full(len(goals), BLOCKED, np.uint32)
    flat = cost.reshape(-1).tolist()
    for g, (x, y, z) in enumerate(goals.tolist()):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            continue
        c = flat[(z * ny + y) * nx + x]
        goal_cost[g] = c
        if c >= BLOCKED:
            continue
        walk = [(z * ny + y) * nx + x]
        while c != 0:
            for (dz, dy, dx), w in zip(MOVES, WEIGHTS):  # ascending linear index: the first hit is the smallest
                qx, qy, qz = x + dx, y + dy, z + dz
                if 0 <= qx < nx and 0 <= qy < ny and 0 <= qz < nz and flat[(qz * ny + qy) * nx + qx] + w == c:
                    x, y, z, c = qx, qy, qz, c - w
                    break
            else:
                raise AssertionError("no neighbour the cost came from: the field is no fixed point")
            walk.append((z * ny + y) * nx + x)
        lengths[g] = len(walk)
        out[g, :min(len(walk), capacity)] = walk[:capacity]
    return out, lengths, goal_cost


def step_counts(path, shape):
    """(faces, edges, corners) of a path of linear indices."""
    nz, ny, nx = shape
    p = np.asarray(path, np.int64)
    xyz = np.stack([p % nx, p // nx % ny, p // (nx * ny)], axis=1)
    kind = np.abs(np.diff(xyz, axis=0)).sum(axis=1)
    return int((kind == 1).sum()), int((kind == 2).sum()), int((kind == 3).sum())
