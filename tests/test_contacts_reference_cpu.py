"""Object contacts without a GPU: the two statements of the device stage agree, the host stage agrees
bit for bit in C, numpy float64 and Python floats, and the restatement reads two analytic spheres as physics says."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import contacts_reference as cr
from tests import shape_reference as sr

f32 = np.float32
SMALL = [(1, 1, 1), (5, 3, 2), (7, 9, 11), (16, 16, 16)]  # the loop statement walks every voxel in Python


def small_volume(shape, content, masked, voxel):
    tsdf, weights, fg = sr.volume(shape, content)
    return cr.vol(tsdf, weights, fg if masked else None, voxel)


def poses_for(shape_a, shape_b, voxel_b):
    """Identity, a fractional translation, the 20 degree rotation, everything outside, a NaN in t."""
    return [(None, (0, 0, 0)), (None, (0.37 * voxel_b, -0.21 * voxel_b, 0.5 * voxel_b)), (cr.rot_z(20.0), (0.3 * voxel_b, 0, -voxel_b)),
            (None, (100.0, 0, 0)), (None, (0, np.nan, 0))]


@pytest.mark.parametrize("content", sr.CONTENTS)
def test_the_two_statements_agree_on_the_fixtures(content):
    for shape_a in SMALL:
        for shape_b, ratio in ((shape_a, 1.0), (SMALL[2], 0.8), (SMALL[1], 2.0)):
            for masked in (True, False):
                va = small_volume(shape_a, content, masked, 0.01)
                vb = small_volume(shape_b, "random" if content == "unobserved" else content, masked, 0.01 * ratio)
                for k, (R, t) in enumerate(poses_for(shape_a, shape_b, 0.01 * ratio)):
                    pr = cr.pair(0, 1, R, t, (-1.0, -0.0, 0.0, 0.25, 1.0, np.inf)[(k + len(content)) % 6])
                    a, b = cr.probe(va, vb, pr), cr.probe_loop(va, vb, pr)
                    assert a.tobytes() == b.tobytes(), (shape_a, shape_b, masked, k, a, b)
                    cr.check_identities(a)


def test_the_two_statements_agree_on_random_volumes():
    rng = np.random.default_rng(0xC7)
    seen = dict.fromkeys(cr.COUNTS, 0)
    for trial in range(24):
        shapes = [tuple(int(v) for v in rng.integers(2, 10, 3)) for _ in range(2)]
        vols = []
        for nx, ny, nz in shapes:
            dims = (nz, ny, nx)
            tsdf = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 1.0, np.nan], f32), dims, p=[.2, .2, .05, .05, .2, .25, .05])
            weights = rng.choice(np.array([0.0, -1.0, np.nan, 1.0, 8.0], f32), dims, p=[.1, .03, .02, .45, .4])
            fg = rng.choice(np.array([0, 1, 255], np.uint8), dims, p=[.2, .5, .3]) if trial % 2 else None
            vols.append(cr.vol(tsdf, weights, fg, float(rng.choice([0.01, 0.008, 0.02]))))
        t = rng.uniform(-0.02, 0.02, 3)
        pr = cr.pair(0, 1, cr.rot_z(float(rng.uniform(-40, 40))), t, float(rng.choice([-1.0, 0.0, 0.25, 1.0, np.inf])))
        a, b = cr.probe(vols[0], vols[1], pr), cr.probe_loop(vols[0], vols[1], pr)
        assert a.tobytes() == b.tobytes(), (trial, a, b)
        cr.check_identities(a)
        for k in cr.COUNTS:
            seen[k] += int(a[k])
    assert all(seen.values()), seen  # every class and sub-class occurred


def test_identity_between_equal_lattices_reads_the_fields_own_bits():
    """At q on the lattice f is 0, so s is the field's tsdf at the voxel, bit for bit: min_s is the smallest of them."""
    tsdf, weights, _ = sr.volume((16, 16, 16), "half_shell")
    va = cr.vol(tsdf, weights, None, 0.01)
    other = np.where(np.arange(tsdf.size).reshape(tsdf.shape) % 3 == 0, f32(-0.625), f32(0.375))
    vb = cr.vol(other, np.ones_like(weights), None, 0.01)
    rec = cr.probe(va, vb, cr.pair(0, 1, None, (0, 0, 0), 0.0))
    z, y, x = np.nonzero(cr.surface_mask(tsdf, weights))
    inner = (x < 15) & (y < 15) & (z < 15)  # q + 1 >= N is outside
    assert rec["sampled"] == inner.sum() > 0 and rec["outside"] == (~inner).sum()
    vals = other[z[inner], y[inner], x[inner]]
    assert rec["inside"] == (vals < 0).sum() and rec["min_s"] == vals.min()


# ---- the host stage ----------------------------------------------------------------------------------------------------

def random_pose(rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-3, 3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return R.astype(f32), rng.uniform(-2, 2, 3).astype(f32)


def random_record(rng, res, touching=True, normals=True):
    r = np.zeros((), cr.CONTACT)
    sampled = int(rng.integers(1, 5000))
    r["sampled"], r["surface"] = sampled, sampled
    r["min_s"] = f32(rng.choice([1.0, 0.5371, -0.4412, -0.0, 0.25]))
    if touching:
        n = int(rng.integers(1, sampled + 1))
        r["touching"], r["inside"] = n, int(rng.integers(0, n + 1)) if r["min_s"] < 0 else 0
        lo = [int(rng.integers(0, res[j])) for j in range(3)]
        hi = [int(rng.integers(lo[j], res[j])) for j in range(3)]
        r["lo"], r["hi"] = lo, hi
        r["sum"] = [int(rng.integers(lo[j] * n, hi[j] * n + 1)) for j in range(3)]
        if normals:
            r["normals"] = int(rng.integers(1, n + 1))
            r["gsum"] = [int(v) for v in rng.integers(-8192 * int(r["normals"]), 8192 * int(r["normals"]) + 1, 3)]
    else:
        r["lo"], r["hi"] = res, (-1, -1, -1)
    return r


def test_the_host_stage_agrees_bit_for_bit_in_c_numpy_and_python_floats():
    from emfusion_amd import pipeline
    rng = np.random.default_rng(0x5EED)
    for trial in range(40):
        pa, pb = random_pose(rng), random_pose(rng)
        want = cr.contact_pose_np(*pa, *pb)
        for got in (cr.contact_pose_py(*pa, *pb), pipeline.contact_pose(pa, pb)):
            assert np.asarray(got[0], f32).tobytes() == want[0].tobytes() and np.asarray(got[1], f32).tobytes() == want[1].tobytes()
        touch_m, trunc = float(rng.choice([0.0, 0.01, 0.0125, 0.3, -0.02, np.inf])), f32(rng.choice([0.04, 0.05, 0.1, 1e-3]))
        want_t = cr.contact_touch_np(touch_m, trunc)
        assert cr.contact_touch_py(touch_m, trunc).tobytes() == want_t.tobytes() == pipeline.contact_touch(touch_m, trunc).tobytes()
        res_a, res_b = [int(v) for v in rng.integers(1, 200, 3)], [int(v) for v in rng.integers(1, 200, 3)]
        sa, sb = cr.side(res_a, 0.01, 0.04, *pa), cr.side(res_b, 0.0125, 0.05, *pb)
        ab = random_record(rng, res_a, touching=trial % 4 != 0, normals=trial % 3 != 0)
        ba = None if trial % 5 == 0 else random_record(rng, res_b, touching=trial % 2 == 0, normals=trial % 3 != 1)
        want_s = cr.contact_summary_np(ab, ba, sa, sb)
        for got in (cr.contact_summary_py(ab, ba, sa, sb), pipeline.contact_summary(ab, ba, sa, sb)):
            assert got.tobytes() == want_s.tobytes(), (trial, got, want_s)


def test_the_summary_states_and_the_empty_records():
    from emfusion_amd import pipeline
    sa, sb = cr.side((8, 8, 8), 0.01, 0.04), cr.side((8, 8, 8), 0.01, 0.05)
    empty = np.zeros((), cr.CONTACT)
    empty["lo"], empty["hi"], empty["min_s"] = (8, 8, 8), (-1, -1, -1), np.inf
    for fn in (cr.contact_summary_np, cr.contact_summary_py, pipeline.contact_summary):
        s = fn(empty, empty, sa, sb)
        assert s["state"] == cr.UNSEEN and s["direction"] == -1 and np.isinf(s["distance_m"]) and not s["saturated"]
        apart = empty.copy()
        apart["sampled"], apart["min_s"] = 3, 1.0
        s = fn(empty, apart, sa, sb)
        assert s["state"] == cr.APART and s["saturated"] == 1 and s["distance_m"] == float(f32(0.04))  # b -> a reads a's volume
        touch = apart.copy()
        touch["touching"], touch["min_s"], touch["sum"], touch["lo"], touch["hi"] = 2, 0.125, (7, 7, 7), (3, 3, 3), (4, 4, 4)
        s = fn(touch, touch, sa, sb)
        assert s["state"] == cr.TOUCHING and s["direction"] == 0 and not s["has_normal"] and not s["normal"].any()
        assert np.array_equal(s["point"], [0.0, 0.0, 0.0])  # 3.5 is the centre of 8 voxels
        deep = touch.copy()
        deep["inside"], deep["min_s"], deep["touching"] = 1, -0.5, 3
        s = fn(touch, deep, sa, sb)
        assert s["state"] == cr.PENETRATING and s["direction"] == 1 and s["distance_m"] == -0.5 * float(f32(0.04))


# ---- the physics of the restatement: two analytic sphere bands -----------------------------------------------------------

@pytest.fixture(scope="module")
def spheres():
    va, vb = cr.sphere_band(*cr.SPHERE_PROBE), cr.sphere_band(*cr.SPHERE_FIELD)
    return va, vb, [cr.probe(va, vb, cr.sphere_pair(dx)) for dx in cr.SPHERE_DX]


def test_two_spheres_read_as_physics_says(spheres):
    """The restatement alone.  Radius 0.07 m, truncation 0.04 m, probe 24^3 at 0.01 m, field 32 x 20 x 24 at 0.0125 m,
    20 degrees about z plus (dx, 0.01, -0.005), touch 0.25.  Observed (456 surface voxels): dx 0.60 all outside; 0.19:
    238 sampled, min_s 1; 0.16: min_s 0.537 = 21.5 mm against a gap of 20.4 mm; 0.14: 9 touching, none inside; 0.12: 30
    inside, min_s -0.441 = -17.6 mm against -19.5 mm; 0.06: 42 unknown, 89 inside."""
    va, vb, recs = spheres
    sa = cr.side(cr.SPHERE_PROBE[0], cr.SPHERE_PROBE[1], cr.SPHERE_TRUNC)
    sb = cr.side(cr.SPHERE_FIELD[0], cr.SPHERE_FIELD[1], cr.SPHERE_TRUNC)
    bound = cr.SPHERE_PROBE[1] * math.sqrt(3.0) + cr.SPHERE_FIELD[1]  # one probe-voxel diagonal plus one field voxel
    total = dict.fromkeys(cr.COUNTS, 0)
    for dx, want, rec in zip(cr.SPHERE_DX, cr.SPHERE_STATES, recs):
        cr.check_identities(rec)
        s = cr.contact_summary_py(rec, None, sa, sb)
        print(dx, {k: int(rec[k]) for k in cr.COUNTS}, float(rec["min_s"]), float(s["distance_m"]), cr.sphere_gap(dx))
        assert s["state"] == want, (dx, rec)
        assert rec["surface"] == recs[0]["surface"] > 0  # the probe's surface does not depend on the pose
        for k in cr.COUNTS:
            total[k] += int(rec[k])
        if dx in (0.16, 0.14, 0.12):
            assert not s["saturated"] and abs(s["distance_m"] - cr.sphere_gap(dx)) < bound, (dx, s["distance_m"], cr.sphere_gap(dx))
        if want >= cr.TOUCHING:  # the contact lies between the centres, the normal points from a's centre to b's
            to_b = np.array([dx, 0.01, -0.005])  # b's centre in a's frame is R^T (0 - t); a's frame is the world here
            Rt = cr.rot_z(20.0).astype(np.float64).T
            to_b = -(Rt @ to_b)
            assert s["has_normal"] and np.dot(s["normal"], to_b / np.linalg.norm(to_b)) > 0.9, (dx, s["normal"], to_b)
    assert recs[0]["outside"] == recs[0]["surface"] and recs[1]["min_s"] == 1.0 and recs[1]["sampled"] > 0
    assert recs[3]["touching"] > 0 and recs[3]["inside"] == 0 and recs[5]["unknown"] > 0 and recs[5]["inside"] > 0
    assert all(total[k] for k in cr.COUNTS if k != "masked"), total
    half = np.ones(vb["tsdf"].shape, np.uint8)
    half[:, :, vb["tsdf"].shape[2] // 2:] = 0  # a gate over the field's high-x half, where the probe arrives
    gated = cr.probe(va, dict(vb, fg=half), cr.sphere_pair(0.14))
    cr.check_identities(gated)
    assert gated["masked"] > 0 and gated["masked"] + gated["sampled"] == recs[3]["sampled"]
