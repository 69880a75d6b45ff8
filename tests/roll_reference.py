"""Shared by the background-roll tests: the numpy restatement of a roll, and a small synthetic stream
whose wide-angle camera translates in front of a tilted wall so that the follow policy fires twice within a dozen
frames -- once along x only, once along y and z together -- and the wall crosses every slab that leaves."""
import numpy as np

TILE = (32, 8, 8)


def rolled(src, shift):
    """emf_hip_rollVolume: dst(v) = src(v + shift) inside the volume, 0 elsewhere; arrays are (z, y, x[, c]),
    shift = (x, y, z)."""
    dst = np.zeros_like(src)
    nz, ny, nx = src.shape[:3]
    lo = [max(0, -s) for s in shift]                          # first dst index with a source
    hi = [min(n, n - s) for s, n in zip(shift, (nx, ny, nz))]  # one past the last
    if all(h > l for l, h in zip(lo, hi)):
        dst[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = \
            src[lo[2] + shift[2]:hi[2] + shift[2], lo[1] + shift[1]:hi[1] + shift[1], lo[0] + shift[0]:hi[0] + shift[0]]
    return dst


def rolled_pose_t(R, t, shift, vox):
    """ObjTSDF::resize's pose update in float32: t + R * (float(k_i) * voxelSize), row dots summed left to right."""
    f32 = np.float32
    d = [f32(f32(k) * f32(vox)) for k in shift]
    R = np.asarray(R, f32).reshape(3, 3)
    return np.array([f32(f32(f32(f32(R[i, 0] * d[0]) + f32(R[i, 1] * d[1])) + f32(R[i, 2] * d[2])) + f32(t[i]))
                     for i in range(3)], f32)


def retired_boxes(res, shift):
    """The sub-boxes (lo (x, y, z), size (x, y, z)) that retiring cuts for a roll by `shift`: x first over all y, z, then
    y over the x that stays, then z over the x, y that stay; each one voxel layer thicker on the staying side."""
    lo, hi, out = [0, 0, 0], list(res), []
    for a in range(3):
        k, n = shift[a], res[a]
        if k == 0:
            continue
        if abs(k) >= n:
            b0, b1 = 0, n
        elif k > 0:
            b0, b1 = 0, k + 1
        else:
            b0, b1 = n + k - 1, n
        blo, bsz = list(lo), [h - l for l, h in zip(lo, hi)]
        blo[a], bsz[a] = b0, b1 - b0
        if min(bsz) >= 2:
            out.append((tuple(blo), tuple(bsz)))
        if abs(k) >= n:
            hi[a] = lo[a]
        elif k > 0:
            lo[a] = k
        else:
            hi[a] = n + k
        if hi[a] - lo[a] < 2:
            break
    return out


# ---- the stream --------------------------------------------------------------------------------------------------
W, H, BG, VOX, FRAMES = 160, 120, 96, 0.02, 12
STEP = (32, 8, 8)                       # cells of 0.64, 0.16 and 0.16 m
LOOK = float(np.float32(BG * VOX / 2))  # the followed point starts at the volume's centre
ROLLS = {6: (32, 0, 0), 9: (0, 8, -8)}  # frame -> what the policy decides at its end
FOCAL = 80.0                            # pixels: a half field of view of 45 x 37 degrees, so that the volume's rim is seen
EYE = np.eye(3, dtype=np.float32).reshape(-1)


def params():
    from emfusion_amd import pipeline
    p = pipeline.make_params(W, H, BG, VOX, 32, visibility_thresh=100, boundary=5)
    p.K[:] = [FOCAL, 0, W / 2 - 0.5, 0, FOCAL, H / 2 - 0.5, 0, 0, 1]
    return p


def camera_t(f):
    """0.11 m per frame along x for six frames (0.66 m > one x cell at frame 6), then 0.06 m per frame along +y and -z
    (0.18 m > one cell at frame 9)."""
    yz = 0.06 * max(0, f - 6)
    return np.array([0.11 * min(f, 6), yz, -yz], np.float32)


def render(f):
    """Depth (H, W) f32 of the wall z = 1.5 + 0.4 x + 0.05 y (world) from the frame's camera (no rotation): it runs
    from z = 1.1 to the far face of the volume, through the low-x, low-y and high-z slabs that the rolls retire."""
    K = np.array(params().K, np.float64).reshape(3, 3)
    c = camera_t(f).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    t = (1.5 + 0.4 * c[0] + 0.05 * c[1] - c[2]) / (1.0 - 0.4 * dx - 0.05 * dy)
    return t.astype(np.float32)


def color_image(f):
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([(xs * 3 + f) % 256, (ys * 2 + 5 * f) % 256, (xs + ys) % 256], axis=2).astype(np.uint8)
