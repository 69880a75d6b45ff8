"""tests/absorb_reference.py against itself (include/emf_hip.h "Absorbing a volume"): the vectorised
statement and the loop agree byte for byte on the cases the GPU test runs (the loop over at most 12 x 6 x 5 voxels of each
case's box); the count identity; an absorption between
equal lattices under the identity carries the source's bits; a sphere band absorbed into an empty volume reads as an
occupied shell to the distance field's classes; the pose helper in numpy and in Python floats."""
import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import contacts_reference as cr
from tests import shape_reference as sr

f32 = np.float32
OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = 0, 1, 2  # include/emf_hip.h


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def loop_box(box, limit=(12, 6, 5)):
    """The box of a case cut down to what the loop walks in a blink: the same corner, at most `limit` voxels per axis."""
    lo, size = box
    return lo, tuple(min(s, m) for s, m in zip(size, limit))


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_agree(shape, content):
    fused = outside = 0
    for name, dst, src, pose, box in ar.cases(shape, content):
        box = loop_box(box)
        a, b = ar.absorb(dst, src, pose, box), ar.absorb_loop(dst, src, pose, box)
        assert same(a, b), (name, a[2], b[2])
        ar.check_identities(a[2])
        fused, outside = fused + int(a[2]["fused"]), outside + int(a[2]["outside"])
        # outside the box nothing changes; inside it only fused voxels can
        lo, size = box
        keep = np.ones(dst["tsdf"].shape, bool)
        keep[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = False
        for got, was in ((a[0], dst["tsdf"]), (a[1], dst["weights"])):
            assert got.view(np.uint32)[keep].tobytes() == was.view(np.uint32)[keep].tobytes(), name
            assert int((got.view(np.uint32) != was.view(np.uint32)).sum()) <= int(a[2]["fused"]), name
    assert fused > 0 and outside > 0  # the sweep reaches the fusion and the outside rule


def test_the_planted_corners():
    dst, src, poses = ar.planted_case()
    box = ((6, 2, 1), (18, 9, 6))
    for pose in poses:
        a, b = ar.absorb(dst, src, pose, box), ar.absorb_loop(dst, src, pose, box)
        assert same(a, b)
        ar.check_identities(a[2])
        assert a[2]["unknown"] > 0 and a[2]["saturated"] > 0 and a[2]["fresh"] > 0 and a[2]["fused"] > a[2]["fresh"]


def test_identity_between_equal_lattices_copies_the_band():
    """Identity pose, equal lattices, equal truncation, unobserved destination: every fused voxel holds the source's tsdf
    bits and min(w, maxWeight) of the cell's eight weights (here: a constant weight); nothing else changes."""
    shape = (33, 17, 9)
    st, sw, _ = sr.volume(shape, "half_shell")
    sw = np.where(sw > 0, f32(100.0), f32(0)).astype(f32)
    dt, dw, _ = sr.volume(shape, "unobserved")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, 64.0), ar.src_vol(st, sw, None, 0.01, 0.04)
    tsdf, weights, rec = ar.absorb(dst, src, ar.pose_of())
    ar.check_identities(rec)
    changed = weights.view(np.uint32) != dw.view(np.uint32)
    assert rec["fused"] == rec["fresh"] == changed.sum() > 50
    assert tsdf[changed].tobytes() == st[changed].tobytes() and (weights[changed] == 64.0).all()
    assert tsdf[~changed].tobytes() == dt[~changed].tobytes()
    # a fused voxel: all eight corners of its own cell observed and |tsdf| < 1
    z, y, x = np.nonzero(changed)
    assert (np.abs(st[changed]) < 1).all() and (sw[z + 1, y + 1, x + 1] > 0).all() and (sw[z, y, x] > 0).all()
    # the same with the source's weights below the cap
    src["weights"] = np.where(sw > 0, f32(2.5), f32(0)).astype(f32)
    again = ar.absorb(dst, src, ar.pose_of())
    assert again[0].tobytes() == tsdf.tobytes() and (again[1][changed] == 2.5).all()


def test_a_sphere_band_reads_as_an_occupied_shell():
    """A sphere band absorbed through a rotation onto a coarser lattice with another truncation distance: the destination's
    classes are OCCUPIED on the shell (inside the sphere, within the band) and nowhere else."""
    radius, strunc, dtrunc = 0.07, 0.03, 0.04
    st, sw, _ = ar.sphere_band((32, 32, 32), 0.008, radius, strunc)
    shape, voxel = (28, 24, 26), 0.01
    dst = ar.dst_vol(np.zeros(shape[::-1], f32), np.zeros(shape[::-1], f32), voxel, dtrunc, 64.0)
    src = ar.src_vol(st, sw, None, 0.008, strunc)
    offset = np.array([0.012, -0.007, 0.004])  # the sphere's centre in the destination's frame
    R = cr.rot_z(20.0)
    pose = ar.pose_of(R, -(R.astype(np.float64) @ offset))
    tsdf, weights, rec = ar.absorb(dst, src, pose)
    ar.check_identities(rec)
    classes = np.where(weights > 0, np.where(tsdf > 0, OCC_FREE, OCC_OCCUPIED), OCC_UNKNOWN)
    nz, ny, nx = tsdf.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt(((x - (nx - 1) / 2) * voxel - offset[0]) ** 2 + ((y - (ny - 1) / 2) * voxel - offset[1]) ** 2 +
                ((z - (nz - 1) / 2) * voxel - offset[2]) ** 2) - radius
    occupied = classes == OCC_OCCUPIED
    assert occupied.sum() > 500 and rec["solid"] == occupied.sum() and rec["fused"] == rec["fresh"] == (weights > 0).sum()
    slack = 0.008  # the trilinear blend of a curved distance over one source cell
    # a saturated corner (d <= -strunc) blends with its cell's other corners to |s| < 1: up to one source cell's diagonal deeper
    assert (d[occupied] < slack / 4).all() and (d[occupied] > -strunc - 0.008 * 1.75).all()
    shell = (d < -slack / 4) & (d > -strunc + 2 * slack)  # safely inside the band, on every side of the sphere
    assert shell.sum() > 400 and occupied[shell].all()
    # in metres, through the ratio 0.75: where no clipped corner takes part (a cell's diagonal, 0.014, inside the band) only
    # the curvature of the distance over one cell is left, diagonal^2 / (8 radius) = 0.35 mm
    near = (weights > 0) & (np.abs(d) < strunc - 0.015)
    assert near.sum() > 1000 and np.abs(tsdf[near] * dtrunc - d[near]).max() < 0.001
    lo, hi = rec["lo"], rec["hi"]
    assert (lo >= 0).all() and (hi < shape).all() and (lo > 0).any()


def test_the_pose_helper_in_numpy_and_in_python_floats():
    """... and in C (emf_fusion_absorb_pose needs no device): bit for bit, a NaN and an infinity included."""
    from emfusion_amd import pipeline
    rng = np.random.default_rng(17)
    for k in range(50):
        Rd, Rs = (np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(f32) for _ in range(2))
        td, ts = (rng.normal(size=3) * 10.0 ** rng.integers(-3, 3)).astype(f32), rng.normal(size=3).astype(f32)
        if k == 7:
            td[1] = np.nan
        if k == 8:
            Rs[0, 0] = np.inf
        a, b = ar.absorb_pose_np(Rd, td, Rs, ts), ar.absorb_pose_py(Rd, td, Rs, ts)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), k
        c = pipeline.absorb_pose((Rd, td), (Rs, ts))
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes(), k
        c = cr.contact_pose_np(Rd, td, Rs, ts)  # the same rule with the roles named a = destination, b = source
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    R, t = ar.absorb_pose_np(np.eye(3), (1, 2, 3), cr.rot_z(90.0), (1, 1, 3))
    assert np.allclose(R.reshape(3, 3), cr.rot_z(90.0).T, atol=1e-7) and np.allclose(t, (1, 0, 0), atol=1e-6)
