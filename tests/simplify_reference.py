"""Simplified meshes restated in numpy (include/emf_hip.h "Simplified meshes"): vertex clustering by cubic cell.  Cells in
float64 with a true division, clusters in order of first occurrence (np.unique's first indices), integer sums in int64,
kept triangles in input order, the referenced clusters in cluster order.  Plain numpy: no mesh library."""
import numpy as np

E_LIMIT, E_ARG = -5, -4


class Refused(Exception):
    """The definition's refusal; .code is the EMF_E_* the device reports, .partial the output the device still writes
    (EMF_E_ARG only: the mesh without the offending triangles)."""

    def __init__(self, code, what, partial=None):
        super().__init__(what)
        self.code, self.partial = code, partial


def cells_of(v, cell, origin=(0.0, 0.0, 0.0)):
    """(nv, 3) int64 cell coordinates: floor(((double)p - (double)origin) / (double)cell) per axis."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    if not np.all(np.abs(v) < 1024.0):                       # NaN and infinities fail the comparison too
        raise Refused(E_LIMIT, "a coordinate is not finite or 2^10 m or more from zero")
    c = np.floor((v.astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)) /
                 np.float64(np.float32(cell)))
    if not np.all((c >= -32768.0) & (c < 32768.0)):
        raise Refused(E_LIMIT, "a cell coordinate is outside [-2^15, 2^15)")
    return c.astype(np.int64)


def cluster_keys(v, cell, origin=(0.0, 0.0, 0.0), slot=0):
    c = cells_of(v, cell, origin) + 32768
    return (np.int64(slot) << 48) | (c[:, 2] << 32) | (c[:, 1] << 16) | c[:, 0]


def q20(x):
    return np.rint(np.ldexp(x.astype(np.float64), 20)).astype(np.int64)


def simplify(v, n, t, c=None, cell=0.0, origin=(0.0, 0.0, 0.0), slot=0, stats=False):
    """Simplified (vertices, normals, triangles[, colours]) of one mesh; with stats also dict(vertices_in,
    triangles_in, vertices_out, triangles_out, clusters, and for the property tests kept: the input triangles' kept
    flags, cells: the cell of every output vertex or None for a pass-through).  Raises Refused."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(t, np.int32).reshape(-1, 4)
    nv = len(v)
    inr = np.all((t[:, 1:] >= 0) & (t[:, 1:] < nv), axis=1)    # a triangle outside the vertices is dropped and reported
    tin = t[inr]
    if not np.float32(cell) > 0:                               # pass-through
        cluster = np.arange(nv, dtype=np.int64)
        first = cluster.copy()
        keep_t = np.ones(len(tin), bool)
        used = np.ones(nv, bool)
        cell_of = None
    else:
        keys = cluster_keys(v, cell, origin, slot)
        _, first_of_key, inv = np.unique(keys, return_index=True, return_inverse=True)
        order = np.argsort(first_of_key, kind="stable")        # clusters by their smallest member index
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        cluster = rank[inv.reshape(-1)]
        first = first_of_key[order]
        cell_of = cells_of(v[first], cell, origin)
        ct = cluster[tin[:, 1:]]
        keep_t = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
        used = np.zeros(len(first), bool)
        used[ct[keep_t].reshape(-1)] = True
    nc = len(first)
    count = np.bincount(cluster, minlength=nc).astype(np.int64)
    cv, cn = v[first].copy(), n[first].copy()                  # one member: its own bits
    cc = None if c is None else np.ascontiguousarray(c, np.uint8).reshape(-1, 3)[first].copy()
    many = count > 1
    if many.any():
        den = count[many].astype(np.float64)[:, None]
        nq = np.where(np.abs(n) < 1024.0, n, np.float32(0))    # NaN, infinities and |n| >= 2^10 count as 0
        for src, dst in ((v, cv), (nq, cn)):
            q = q20(src)
            s = np.zeros((nc, 3), np.int64)
            np.add.at(s, cluster, q)
            dst[many] = ((s[many].astype(np.float64) / den) * 2.0 ** -20).astype(np.float32)
        if cc is not None:
            s = np.zeros((nc, 3), np.int64)
            np.add.at(s, cluster, np.asarray(c, np.uint8).reshape(-1, 3).astype(np.int64))
            cnt = count[many][:, None]
            cc[many] = ((2 * s[many] + cnt) // (2 * cnt)).astype(np.uint8)
    newidx = np.cumsum(used) - 1
    kt = tin[keep_t].copy()
    if len(kt):
        kt[:, 1:] = newidx[cluster[kt[:, 1:]]].astype(np.int32)
        kt[:, 0] = 3
    out = (cv[used], cn[used], kt.reshape(-1, 4)) + (() if cc is None else (cc[used],))
    kept = inr.copy()
    kept[inr] = keep_t
    st = dict(vertices_in=nv, triangles_in=len(t), vertices_out=int(used.sum()), triangles_out=len(kt), clusters=nc,
              kept=kept, cells=None if cell_of is None else cell_of[used])
    if not inr.all():
        raise Refused(E_ARG, "a triangle index lies outside the vertices", (out, st) if stats else out)
    return (out, st) if stats else out


def simplify_table(v, n, t, c=None, cells=0.0, origin=(0.0, 0.0, 0.0), tri_bases=None, vertex_bases=None):
    """A table of meshes: the list of simplify() of each slice, cells a scalar or one per model."""
    nm = len(tri_bases) - 1
    cells = np.broadcast_to(np.asarray(cells, np.float32), (nm,))
    out = []
    for k in range(nm):
        vs, ts = slice(int(vertex_bases[k]), int(vertex_bases[k + 1])), slice(int(tri_bases[k]), int(tri_bases[k + 1]))
        out.append(simplify(v[vs], n[vs], t[ts], None if c is None else c[vs], cells[k], origin, slot=k))
    return out
