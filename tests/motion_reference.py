"""numpy / scipy restatement of the motion masks (include/emf_hip.h "Motion masks"): the five stages of
emf_hip_motionMasks, written for clarity.  Test infrastructure: the GPU tests compare the kernels with it byte for byte.

Every float operation is one float32 operation on both sides (a product, a sum, a square root, a difference, a
comparison), so the results are equal, not close.  The test-pattern builders at the end make inputs whose candidates
and ray lengths are known by construction."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

DEFAULTS = dict(band=0.08, continuity=0.05, erode=1, min_pixels=200, max_masks=8)
INFO_KEYS = ("label", "area", "x0", "y0", "x1", "y1")


def ray_lengths(points: np.ndarray) -> np.ndarray:
    """m = sqrtf(x * x + y * y + z * z), summed left to right, every operation rounded to float32."""
    p = np.asarray(points, np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        return np.sqrt((x * x + y * y) + z * z, dtype=np.float32)


def candidates(points: np.ndarray, bg: np.ndarray, band: float) -> np.ndarray:
    """Stage 1.  NaN fails every comparison; a missed background ray (0) is unknown, never novel."""
    m = ray_lengths(points)
    b = np.asarray(bg, np.float32)
    with np.errstate(all="ignore"):
        return (np.asarray(points, np.float32)[..., 2] > 0) & (b > 0) & ((b - m) > np.float32(band))


def erode_candidates(cand: np.ndarray, passes: int) -> np.ndarray:
    """Stage 2: 3 x 3 binary erosion, the border counting as not-candidate."""
    out = np.asarray(cand, bool)
    for _ in range(int(passes)):
        out = ndimage.binary_erosion(out, structure=np.ones((3, 3), bool), border_value=0)
    return out


def label_min_index(cand: np.ndarray, m: np.ndarray, continuity: float) -> np.ndarray:
    """Stage 3: for every candidate pixel the smallest linear index of its component (-1 elsewhere).  Explicit
    union-find over the two neighbour relations (right, down), a pair joined only if |m_a - m_b| <= continuity."""
    h, w = cand.shape
    n = h * w
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    with np.errstate(all="ignore"):
        right = cand[:, :-1] & cand[:, 1:] & (np.abs(m[:, :-1] - m[:, 1:]) <= np.float32(continuity))
        down = cand[:-1, :] & cand[1:, :] & (np.abs(m[:-1, :] - m[1:, :]) <= np.float32(continuity))
    ys, xs = np.nonzero(right)
    pairs = [(y * w + x, y * w + x + 1) for y, x in zip(ys.tolist(), xs.tolist())]
    ys, xs = np.nonzero(down)
    pairs += [(y * w + x, (y + 1) * w + x) for y, x in zip(ys.tolist(), xs.tolist())]
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            lo, hi = (ra, rb) if ra < rb else (rb, ra)
            parent[hi] = lo  # the smaller index stays the root: a root is its tree's minimum
    labels = np.full(n, -1, np.int64)
    for i in np.nonzero(cand.reshape(-1))[0].tolist():
        labels[i] = find(i)
    return labels.reshape(h, w)


def motion_masks(points, bg, band=DEFAULTS["band"], continuity=DEFAULTS["continuity"], erode=DEFAULTS["erode"],
                 min_pixels=DEFAULTS["min_pixels"], max_masks=DEFAULTS["max_masks"]):
    """Stages 1-5.  Returns dict(labels (H, W) i32 ranks, masks (max_masks, H, W) u8, info (max_masks, 6) i32,
    count, components: the min-index label image of stage 3)."""
    points = np.asarray(points, np.float32)
    bg = np.asarray(bg, np.float32)
    h, w = bg.shape
    m = ray_lengths(points)
    cand = erode_candidates(candidates(points, bg, band), erode)
    comp = label_min_index(cand, m, continuity)
    # stage 4: areas, threshold, order by area descending then label ascending, truncate
    roots, areas = np.unique(comp[comp >= 0], return_counts=True)
    kept = [(int(a), int(r)) for r, a in zip(roots, areas) if a >= min_pixels]
    kept.sort(key=lambda t: (-t[0], t[1]))
    kept = kept[:max_masks]
    # stage 5
    labels = np.full((h, w), -1, np.int32)
    masks = np.zeros((max_masks, h, w), np.uint8)
    info = np.zeros((max_masks, 6), np.int32)
    for rank, (area, root) in enumerate(kept):
        inside = comp == root
        labels[inside] = rank
        masks[rank][inside] = 1
        ys, xs = np.nonzero(inside)
        info[rank] = (root, area, xs.min(), ys.min(), xs.max(), ys.max())
    return dict(labels=labels, masks=masks, info=info, count=len(kept), components=comp)


def proposals(result) -> list:
    return [dict(zip(INFO_KEYS, (int(v) for v in row))) for row in result["info"][:result["count"]]]


# ---- test patterns --------------------------------------------------------------------------------------------------

def scene(cand: np.ndarray, m=None, bg_gap=0.5):
    """(points, bg) whose stage-1 candidates are exactly `cand`: every pixel looks down its own z axis (x = y = 0, so
    the ray length IS z, exactly), candidates lie bg_gap in front of the background, the others on it.  `m`: the
    ray lengths (default 1.0), multiples of 2^-6 so that sums and differences are exact."""
    cand = np.asarray(cand, bool)
    z = np.full(cand.shape, 1.0, np.float32) if m is None else np.asarray(m, np.float32)
    points = np.zeros(cand.shape + (3,), np.float32)
    points[..., 2] = z
    bg = np.where(cand, z + np.float32(bg_gap), z).astype(np.float32)
    return points, bg


def serpentine(h: int, w: int) -> np.ndarray:
    """A one-pixel-wide path that covers the image: every second row is full, joined alternately at the right and the
    left end -- one component, and the deepest trees a union-find can be asked to flatten."""
    c = np.zeros((h, w), bool)
    c[0::2, :] = True
    for k, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            c[y, w - 1 if k % 2 == 0 else 0] = True
    return c


def checkerboard(h: int, w: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


def random_field(h: int, w: int, density: float, seed: int):
    """Random candidates at the given density with random ray lengths quantised to multiples of 2^-6."""
    rng = np.random.default_rng(seed)
    cand = rng.random((h, w)) < density
    m = (1.0 + rng.integers(0, 16, (h, w)) / 64.0).astype(np.float32)
    return cand, m


# ---- hand-made cases, scaled to the image so that every size gets every one of them ----------------------------------

def two_blobs_with_bridge(h: int, w: int) -> np.ndarray:
    """Two blocks side by side, three columns apart, joined by a one-pixel-high bridge."""
    c = np.zeros((h, w), bool)
    mid = w // 2
    c[1:h - 1, 1:max(mid - 1, 1)] = True
    c[1:h - 1, mid + 2:max(w - 1, mid + 2)] = True
    c[h // 2, max(mid - 1, 0):mid + 2] = True
    return c


def overlapping_blobs(h: int, w: int):
    """One block whose left and right halves lie 0.25 m apart in ray length: two things, one silhouette."""
    c = np.zeros((h, w), bool)
    c[1:max(h - 1, 2), 1:max(w - 1, 2)] = True
    m = np.full((h, w), 1.0, np.float32)
    m[:, w // 2:] = 1.25
    return c, m


def blob_grid(h: int, w: int, size: int = 5, pitch: int = 8) -> np.ndarray:
    """size x size blobs every `pitch` pixels: equal areas (ties), and more of them than any max_masks."""
    c = np.zeros((h, w), bool)
    for y in range(1, h - size + 1, pitch):
        for x in range(1, w - size + 1, pitch):
            c[y:y + size, x:x + size] = True
    return c


def big_and_small(h: int, w: int) -> np.ndarray:
    """A block over the left two thirds and a 2 x 3 blob in the lower right corner."""
    c = np.zeros((h, w), bool)
    c[0:h, 0:(2 * w) // 3] = True
    c[max(h - 3, 0):h - 1, max(w - 4, 0):w - 1] = True
    if (2 * w) // 3 < w:
        c[:, (2 * w) // 3] = False
    return c


def cases(h: int, w: int, seed: int = 7):
    """(name, points, bg, params) for one image size: the hand-made cases, a serpentine, a checkerboard, random fields
    at three densities, non-finite inputs, and max_masks at both ends of its range."""
    out = []

    def add(name, cand, m=None, **params):
        p, b = scene(cand, m)
        out.append((name, p, b, params))

    add("bridge", two_blobs_with_bridge(h, w), min_pixels=1)
    c, m = overlapping_blobs(h, w)
    add("overlap", c, m, min_pixels=1)
    add("small-dropped", big_and_small(h, w), min_pixels=7)
    add("ties", blob_grid(h, w), min_pixels=1, max_masks=8)
    add("one-mask", blob_grid(h, w), min_pixels=1, max_masks=1)
    add("sixteen-masks", blob_grid(h, w, 7, 9), min_pixels=1, max_masks=16)
    p, b = scene(np.ones((h, w), bool))
    out.append(("all-miss", p, np.zeros((h, w), np.float32), dict(min_pixels=1)))
    add("serpentine", serpentine(h, w), min_pixels=1)
    add("checkerboard", checkerboard(h, w), min_pixels=1, max_masks=16)
    for k, density in enumerate((0.3, 0.6, 0.9)):
        c, m = random_field(h, w, density, seed + k)
        add(f"random-{density}", c, m, min_pixels=2, max_masks=16)
    # non-finite points and ray lengths sprinkled over a dense random field
    rng = np.random.default_rng(seed + 100)
    c, m = random_field(h, w, 0.8, seed + 3)
    p, b = scene(c, m)
    bad = (np.nan, np.inf, -np.inf)
    for arr in (p[..., 0], p[..., 1], p[..., 2], b):
        hit = rng.random((h, w)) < 0.05
        arr[hit] = rng.choice(bad, size=int(hit.sum()))
    out.append(("non-finite", p, b, dict(min_pixels=2, max_masks=16)))
    return out
