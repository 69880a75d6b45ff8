"""numpy restatement of updateTSDF (oracle/emf_oracle.c orc_updateTSDF, reference TSDF.cu:327-401) and of the
colour rule defined in include/emf_hip.h (emf_hip_integrateColorBatched), op for op in float32.

The reference has no colour kernel, so the colour update is pinned to this restatement -- and the restatement's
pixel, depth gate and signed distance, which the colour rule reuses, are pinned to the oracle: its tsdf / weight
volumes must be bit-identical to orc_updateTSDF's (tests/test_color_reference.py).

Volumes are (Nz, Ny, Nx) float32, colour volumes (Nz, Ny, Nx, 4) uint16 = R, G, B, Wc in 8.8 fixed point.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def _dot3(r, x, y, z):
    """(r0 * x + r1 * y) + r2 * z  (common.cuh:92-94)"""
    return r[0] * x + r[1] * y + r[2] * z


def update(depth, assoc, tsdf, weights, R_OC, t_OC, K, voxel_size, truncdist, max_weight, rgb=None, color=None):
    """One frame into (tsdf, weights) -- and, if rgb and color are given, into color -- IN PLACE.
    Returns the number of voxels coloured."""
    depth = np.ascontiguousarray(depth, F)
    assoc = np.ascontiguousarray(assoc, F)
    R = np.asarray(R_OC, F).reshape(3, 3)
    t = np.asarray(t_OC, F).reshape(3)
    Km = np.asarray(K, F).reshape(3, 3)
    h, w = depth.shape
    nz, ny, nx = tsdf.shape
    vs, T, mw = F(voxel_size), F(truncdist), F(max_weight)
    two = F(2)
    xs = (np.arange(nx, dtype=F) - F(nx - 1) / two) * vs
    ys = (np.arange(ny, dtype=F) - F(ny - 1) / two) * vs
    X, Y = np.meshgrid(xs, ys)  # (Ny, Nx)
    coloured = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for z in range(nz):
            Z = np.full_like(X, (F(z) - F(nz - 1) / two) * vs)
            cx = _dot3(R[0], X, Y, Z) + t[0]
            cy = _dot3(R[1], X, Y, Z) + t[1]
            cz = _dot3(R[2], X, Y, Z) + t[2]
            tv, wv = tsdf[z], weights[z]
            behind = cz <= 0
            sel = behind & (wv == 0)  # TSDF.cu:351-356
            tv[sel] = 0
            px_ = _dot3(Km[0], cx, cy, cz)
            py_ = _dot3(Km[1], cx, cy, cz)
            pz_ = _dot3(Km[2], cx, cy, cz)
            qx = np.rint(px_ / pz_)  # __float2int_rn
            qy = np.rint(py_ / pz_)
            inimg = ~behind & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            px = np.where(inimg, qx, 0).astype(np.int64)
            py = np.where(inimg, qy, 0).astype(np.int64)
            d = depth[py, px]
            hole = inimg & (d <= 0)  # TSDF.cu:367-372
            sel = hole & (wv == 0)
            tv[sel] = 0
            visited = inimg & ~(d <= 0)
            lx = (px.astype(F) - Km[0, 2]) / Km[0, 0]
            ly = (py.astype(F) - Km[1, 2]) / Km[1, 1]
            lam = np.sqrt(lx * lx + ly * ly + F(1) * F(1))
            sdf = d - (F(1) / lam) * np.sqrt(cx * cx + cy * cy + cz * cz)
            apix = assoc[py, px]
            fuse = visited & (sdf >= -T)
            samp = np.copysign(np.minimum(F(1), np.abs(sdf / T)), sdf)
            aw = np.where(sdf < T, apix, F(1)).astype(F)
            go = fuse & (wv + aw > 0)
            nt = (wv * tv + aw * samp) / (wv + aw)
            nw = np.minimum(wv + aw, mw)
            neg = visited & ~(sdf >= -T) & (wv == 0)  # TSDF.cu:398-400 (on the weight before this frame)
            tv[neg] = -1
            tv[go] = nt[go]
            wv[go] = nw[go]
            if rgb is None or color is None:
                continue
            # ---- the colour rule: visited, |sdf| < truncdist, association weight of the pixel > 0
            col = visited & (np.abs(sdf) < T) & (apix > 0)
            if not col.any():
                continue
            cq = color[z]
            a = apix[col]
            W = cq[..., 3][col].astype(F) / F(256)
            c_new = rgb[py[col], px[col]].astype(F)  # (n, 3)
            for k in range(3):
                c_old = cq[..., k][col].astype(F) / F(256)
                v = ((W * c_old + a * c_new[:, k]) / (W + a)) * F(256)
                ch = cq[..., k]
                ch[col] = np.rint(v).astype(np.uint16)
            wq = cq[..., 3]
            wq[col] = np.rint(np.minimum(W + a, mw) * F(256)).astype(np.uint16)
            coloured += int(col.sum())
    return coloured
