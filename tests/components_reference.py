"""Mesh components restated in numpy (include/emf_hip.h "Mesh components"): connectivity by index, labels = the smallest
index of the component, sizes = its triangles, and the filter that keeps components by size.  Plain Python and numpy:
the labels come from a sequential union-find over the triangles' edges, no graph library."""
import numpy as np


def components(tri, nv):
    """(labels (nv,) i32, sizes (nv,) u32) of the mesh whose (m, 4) records (3, i0, i1, i2) index nv vertices."""
    tri = np.asarray(tri).reshape(-1, 4)
    parent = list(range(nv))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, c in tri[:, 1:].tolist():
        for other in (b, c):
            ra, rb = find(a), find(other)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)   # the smaller index stays the root: a root is its tree's minimum
    labels = np.array([find(x) for x in range(nv)], np.int64).reshape(nv)
    per_label = np.bincount(labels[tri[:, 1]], minlength=nv) if len(tri) else np.zeros(nv, np.int64)
    return labels.astype(np.int32), per_label[labels].astype(np.uint32)


def kept_labels(labels, sizes, min_triangles=0, largest_only=False):
    """The labels of the components the filter keeps, ascending."""
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    size = sizes[roots].astype(np.int64)
    keep = np.ones(len(roots), bool) if min_triangles <= 1 else size >= min_triangles
    if largest_only and len(roots):
        best = roots[size == size.max()].min()   # the largest by triangles, a tie to the smaller label
        keep &= roots == best
    return roots[keep]


def filter_mesh(v, n, t, c=None, min_triangles=0, largest_only=False, comps=None):
    """Filtered (vertices, normals, triangles[, colours]): kept vertices in order, bits unchanged; kept triangles in
    order, re-indexed to the compacted vertices.  comps: components(t, len(v)) where the caller has it already (the
    sequential union-find takes seconds on a mesh of millions of triangles)."""
    labels, sizes = components(t, len(v)) if comps is None else comps
    keepv = np.isin(labels, kept_labels(labels, sizes, min_triangles, largest_only))
    rank = np.cumsum(keepv) - 1
    t = np.asarray(t).reshape(-1, 4)
    kt = t[keepv[t[:, 1]]].copy() if len(t) else t.copy()
    if len(kt):
        kt[:, 1:] = rank[kt[:, 1:]].astype(t.dtype)
    return (v[keepv], n[keepv], kt) + (() if c is None else (c[keepv],))


_cases = {}


def welded_case(oracle, name):
    """(tsdf, weights, fg or None, voxel size, the oracle's soup welded by the restatement) of a welded-mesh test volume
    (tests/weld_volumes.py; "fused" is fused(oracle, (40, 36, 32), 0.016)) -- computed once."""
    from tests import weld_volumes as WV
    from tests.weld_reference import edge_keys, weld
    if name not in _cases:
        if name == "fused":
            tsdf, wts, fg, vox = WV.fused(oracle, (40, 36, 32), 0.016)
        elif name == "fused_masked":
            tsdf, wts, fg, vox = WV.fused_masked(oracle)
        else:
            tsdf, wts, fg, vox = getattr(WV, name)()
        soup = oracle.marching_cubes(tsdf, wts, vox, fg=fg) if fg is not None else oracle.marching_cubes(tsdf, wts, vox)
        _cases[name] = (tsdf, wts, fg, vox, weld(*soup, edge_keys(tsdf, wts, fg)))
    return _cases[name]


def summary(tri, nv, min_triangles=8):
    """What the issue's table lists: (components, sizes descending, the largest's (vertices, triangles), the
    (vertices, triangles, components) left by min_triangles)."""
    labels, sizes = components(tri, nv)
    roots = np.flatnonzero(labels == np.arange(nv))
    big = kept_labels(labels, sizes, 0, True)
    lv = int((labels == big[0]).sum()) if len(big) else 0
    lt = int(sizes[big[0]]) if len(big) else 0
    kept = kept_labels(labels, sizes, min_triangles)
    return (len(roots), sorted(sizes[roots].tolist(), reverse=True), (lv, lt),
            (int(np.isin(labels, kept).sum()), int(sizes[kept].sum()), len(kept)))
