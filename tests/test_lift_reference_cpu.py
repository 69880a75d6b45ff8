"""tests/lift_reference.py against itself (include/emf_hip.h "Lifting a volume"): the vectorised statements
and the loops agree byte for byte on the cases the GPU test runs (the loops over at most 12 x 6 x 5 voxels of each case's
box), with the count identities; a seed between equal lattices under the identity copies the source's in-band bits; an
observed destination is KEPT; a release with a NULL claim zeroes exactly the band; seed then release moves a sphere band
from one volume into another; pipeline.lifted_line round-trips an event."""
import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import contacts_reference as cr
from tests import lift_reference as lr
from tests import shape_reference as sr

f32 = np.float32


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def loop_box(box, limit=(12, 6, 5)):
    lo, size = box
    return lo, tuple(min(s, m) for s, m in zip(size, limit))


def unchanged_outside(got, dst, box, moved, name):
    """Outside the box nothing changes; inside it at most `moved` voxels can."""
    lo, size = box
    keep = np.ones(dst["tsdf"].shape, bool)
    keep[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = False
    for new, was in ((got[0], dst["tsdf"]), (got[1], dst["weights"])):
        assert new.view(np.uint32)[keep].tobytes() == was.view(np.uint32)[keep].tobytes(), name
        assert int((new.view(np.uint32) != was.view(np.uint32)).sum()) <= int(moved), name


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_of_the_seed_agree(shape, content):
    total = np.zeros((), lr.SEED)
    for name, dst, src, pose, box in lr.seed_cases(shape, content):
        box = loop_box(box)
        a, b = lr.seed(dst, src, pose, box), lr.seed_loop(dst, src, pose, box)
        assert same(a, b), (name, a[2], b[2])
        lr.check_identities(a[2])
        unchanged_outside(a, dst, box, a[2]["seeded"], name)
        with np.errstate(invalid="ignore"):
            had = dst["weights"] > 0
        assert a[0][had].tobytes() == dst["tsdf"][had].tobytes() and a[1][had].tobytes() == dst["weights"][had].tobytes(), name
        assert not (np.abs(a[0][a[1].view(np.uint32) != dst["weights"].view(np.uint32)]) >= 1).any(), name  # no clamped +-1
        for k in lr.SEED_COUNTS:
            total[k] += a[2][k]
    assert total["kept"] > 0 and total["outside"] > 0
    if content in ("all_solid", "gated_block", "random", "half_shell") and min(shape) >= 8:  # the sweep reaches both band rules
        assert total["seeded"] > 0 and total["saturated"] > 0


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_of_the_release_agree(shape, content):
    total = np.zeros((), lr.RELEASE)
    for name, dst, claim, pose, box in lr.release_cases(shape, content):
        box = loop_box(box)
        a, b = lr.release(dst, claim, pose, box), lr.release_loop(dst, claim, pose, box)
        assert same(a, b), (name, a[2], b[2])
        lr.check_identities(a[2])
        unchanged_outside(a, dst, box, a[2]["released"], name)
        changed = a[1].view(np.uint32) != dst["weights"].view(np.uint32)
        assert changed.sum() == a[2]["released"] and not a[0].view(np.uint32)[changed].any() and not a[1].view(np.uint32)[changed].any()
        if name.endswith("-zero"):
            assert a[2]["released"] == 0
        for k in lr.RELEASE_COUNTS:
            total[k] += a[2][k]
    assert total["empty"] > 0
    if shape != (1, 1, 1):
        assert total["released"] > 0 and total["free_space"] > 0 and total["outside"] > 0 and total["unclaimed"] > 0


def test_the_planted_corners_and_both_band_rules():
    """Ratio 0.5: s saturated where u = s / 2 is not; ratio 2: u saturated where s is not."""
    sat = {}
    box = ((6, 2, 1), (18, 9, 6))
    for name, ratio, dst, src, pose in lr.planted_cases():
        a, b = lr.seed(dst, src, pose, box), lr.seed_loop(dst, src, pose, box)
        assert same(a, b), name
        full = lr.seed(dst, src, pose)
        lr.check_identities(full[2])
        assert full[2]["unknown"] > 0 and full[2]["kept"] > 0 and full[2]["seeded"] > 0 and full[2]["saturated"] > 0, name
        sat[name[-5:], ratio] = int(full[2]["saturated"])
    for p in ("pose0", "pose1"):
        assert 0 < sat[p, 0.5] == sat[p, 1.0] < sat[p, 2.0]


def test_a_seed_between_equal_lattices_copies_the_band():
    """Identity pose, equal lattices, equal truncation, unobserved destination: every seeded voxel holds the source's tsdf
    bits and min(w, maxWeight); nothing else changes."""
    shape = (33, 17, 9)
    st, sw, _ = sr.volume(shape, "half_shell")
    sw = np.where(sw > 0, f32(100.0), f32(0)).astype(f32)
    dt, dw, _ = sr.volume(shape, "unobserved")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, 64.0), ar.src_vol(st, sw, None, 0.01, 0.04)
    tsdf, weights, rec = lr.seed(dst, src, ar.pose_of())
    lr.check_identities(rec)
    changed = weights.view(np.uint32) != dw.view(np.uint32)
    assert rec["seeded"] == changed.sum() > 50 and rec["kept"] == 0
    assert tsdf[changed].tobytes() == st[changed].tobytes() and (weights[changed] == 64.0).all()
    assert tsdf[~changed].tobytes() == dt[~changed].tobytes() and weights[~changed].tobytes() == dw[~changed].tobytes()
    z, y, x = np.nonzero(changed)
    assert (np.abs(st[changed]) < 1).all() and (sw[z + 1, y + 1, x + 1] > 0).all() and (sw[z, y, x] > 0).all()
    # an absorption into the same destination fuses the same voxels and the saturated ones of the band's rim never
    fused = ar.absorb(dst, src, ar.pose_of())
    assert fused[0].tobytes() == tsdf.tobytes() and fused[1].tobytes() == weights.tobytes()
    src["weights"] = np.where(sw > 0, f32(2.5), f32(0)).astype(f32)
    again = lr.seed(dst, src, ar.pose_of())
    assert again[0].tobytes() == tsdf.tobytes() and (again[1][changed] == 2.5).all()
    # ... and a second seed on top finds them KEPT
    twice = lr.seed(dict(dst, tsdf=tsdf, weights=weights), src, ar.pose_of())
    assert twice[0].tobytes() == tsdf.tobytes() and twice[1].tobytes() == weights.tobytes()
    assert twice[2]["kept"] == rec["seeded"] and twice[2]["seeded"] == 0


def test_an_observed_destination_is_kept():
    shape = (33, 17, 9)
    st, sw, sf = sr.volume(shape, "all_solid")
    dt, dw, _ = sr.volume(shape, "all_solid")
    dt = np.full_like(dt, 0.25)
    for fg in (None, sf):
        tsdf, weights, rec = lr.seed(ar.dst_vol(dt, dw), ar.src_vol(st, sw, fg), ar.pose_of())
        assert tsdf.tobytes() == dt.tobytes() and weights.tobytes() == dw.tobytes()
        assert rec["kept"] == rec["visited"] == dt.size and rec["seeded"] == 0 and (rec["hi"] == -1).all()


def test_a_release_without_a_claim_zeroes_the_band():
    """NULL claim, identity pose, equal lattices: exactly the voxels with pw > 0 and |pt| < 1 that lie inside the cube by
    the pad-1 rule (all but the last plane of each axis) become +0.0."""
    shape = (33, 17, 9)
    dt, dw, _ = sr.volume(shape, "random")
    dst = ar.dst_vol(dt, dw)
    tsdf, weights, rec = lr.release(dst, lr.claim_of(None, shape, 0.01), ar.pose_of())
    lr.check_identities(rec)
    with np.errstate(invalid="ignore"):
        band = (dw > 0) & (np.abs(dt) < 1)
    inner = np.zeros(band.shape, bool)
    inner[:-1, :-1, :-1] = True
    want = band & inner
    assert rec["released"] == want.sum() > 500 and rec["outside"] == (band & ~inner).sum() > 0
    assert not tsdf.view(np.uint32)[want].any() and not weights.view(np.uint32)[want].any()
    assert tsdf[~want].tobytes() == dt[~want].tobytes() and weights[~want].tobytes() == dw[~want].tobytes()
    with np.errstate(invalid="ignore"):
        assert rec["empty"] == (~(dw > 0)).sum() and rec["free_space"] == ((dw > 0) & ~(np.abs(dt) < 1)).sum()
    again = lr.release(dict(dst, tsdf=tsdf, weights=weights), lr.claim_of(None, shape, 0.01), ar.pose_of())
    assert again[0].tobytes() == tsdf.tobytes() and again[2]["released"] == 0
    assert again[2]["empty"] == rec["empty"] + rec["released"]


def test_seed_then_release_moves_a_sphere_band():
    """The analytic sphere of the absorption's test (radius 0.07 m) held by a 10 mm volume as a TSDF holds a surface --
    observed from one truncation distance behind it outwards -- is lifted into an empty 32^3 volume at 8 mm through the 20
    degree rotation: afterwards the destination holds the shell and the source classifies no voxel as occupied."""
    radius, strunc, dtrunc, svoxel, dvoxel = 0.07, 0.03, 0.04, 0.01, 0.008
    sshape = (28, 24, 26)
    offset = np.array([0.012, -0.007, 0.004])  # the sphere's centre in the source's frame
    nz, ny, nx = sshape[::-1]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt(((x - (nx - 1) / 2) * svoxel - offset[0]) ** 2 + ((y - (ny - 1) / 2) * svoxel - offset[1]) ** 2 +
                ((z - (nz - 1) / 2) * svoxel - offset[2]) ** 2) - radius
    st = np.clip(d / strunc, -1, 1).astype(f32)
    sw = ((d > -strunc) & (np.abs(st) < 1) | (d >= strunc) & (d <= 2 * strunc)).astype(f32) * f32(5)
    src = ar.src_vol(st, sw, None, svoxel, strunc)
    occupied_before = (sw > 0) & ~(st > 0)
    assert occupied_before.sum() > 300
    dst = ar.dst_vol(np.zeros((32, 32, 32), f32), np.zeros((32, 32, 32), f32), dvoxel, dtrunc, 64.0)
    R = cr.rot_z(20.0)  # source frame <- destination frame: p_s = R p_d + offset
    tsdf, weights, rec = lr.seed(dst, src, ar.pose_of(R, offset))
    lr.check_identities(rec)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    dd = np.sqrt(((xx - 15.5) * dvoxel) ** 2 + ((yy - 15.5) * dvoxel) ** 2 + ((zz - 15.5) * dvoxel) ** 2) - radius
    occupied = (weights > 0) & ~(tsdf > 0)
    assert rec["kept"] == 0 and rec["seeded"] == (weights > 0).sum() and rec["solid"] == occupied.sum() > 500
    assert (np.abs(tsdf[weights > 0]) < 1).all() and (weights[weights > 0] == 5.0).all()
    slack = svoxel  # the trilinear blend of a curved distance over one source cell
    assert (dd[occupied] < slack / 4).all() and (dd[occupied] > -strunc).all()
    shell = (dd < -slack / 4) & (dd > -strunc + 2 * slack)  # inside the band with every corner of the cell observed
    assert shell.sum() > 300 and occupied[shell].all()
    near = (weights > 0) & (np.abs(dd) < strunc - 2 * slack)
    assert near.sum() > 1000 and np.abs(tsdf[near] * dtrunc - dd[near]).max() < 0.001
    # the release: claimant frame <- source frame is the inverse pose; the whole cube claims
    Rt = R.astype(np.float64).T
    back = ar.pose_of(Rt.astype(f32), -(Rt @ offset))
    claim = lr.claim_of(None, (32, 32, 32), dvoxel)
    stsdf, sweights, rel = lr.release(ar.dst_vol(st, sw, svoxel, strunc), claim, back)
    lr.check_identities(rel)
    assert rel["released"] == ((sw > 0) & (np.abs(st) < 1)).sum() and rel["outside"] == 0 and rel["solid"] == occupied_before.sum()
    assert not ((sweights > 0) & ~(stsdf > 0)).any()  # no voxel of the source is occupied any more
    free = (sw > 0) & ~(np.abs(st) < 1)
    assert rel["free_space"] == free.sum() > 0 and sweights[free].tobytes() == sw[free].tobytes()


def test_lifted_line_round_trips_an_event():
    from emfusion_amd import pipeline
    seed, rel = np.zeros((), lr.SEED), np.zeros((), lr.RELEASE)
    for k, name in enumerate(lr.SEED_COUNTS):
        seed[name] = 1000 + k
    for k, name in enumerate(lr.RELEASE_COUNTS):
        rel[name] = 2 ** 33 + k
    seed["lo"], seed["hi"], rel["lo"], rel["hi"] = (1, 2, 3), (30, 29, 28), (64, 65, 66), (-1, -1, -1)
    R, t = cr.rot_z(20.0).reshape(9), np.array([0.1, -1e-9, 3.0000002], f32)
    event = dict(id=7, frame=12, clipped=True, seed_R=R, seed_t=t, release_R=R.reshape(3, 3).T.reshape(9).copy(), release_t=-t,
                 lo=(60, 61, 62), size=(40, 41, 42), seed=seed, release=rel)
    line = pipeline.lifted_line(event)
    v = line.split()
    assert len(v) == 3 + 6 + 8 + 6 + 7 + 6 + 24
    assert [int(s) for s in v[:9]] == [7, 12, 1, 60, 61, 62, 40, 41, 42]
    assert [int(s) for s in v[9:17]] == [int(seed[k]) for k in lr.SEED_COUNTS]
    assert [int(s) for s in v[17:23]] == [1, 2, 3, 30, 29, 28]
    assert [int(s) for s in v[23:30]] == [int(rel[k]) for k in lr.RELEASE_COUNTS]
    assert [int(s) for s in v[30:36]] == [64, 65, 66, -1, -1, -1]
    poses = np.array([float(s) for s in v[36:]], f32)  # %.9g: the float32 bits come back
    assert poses.tobytes() == np.concatenate([event["seed_R"], event["seed_t"], event["release_R"], event["release_t"]]).astype(f32).tobytes()
