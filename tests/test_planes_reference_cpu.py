"""tests/planes_reference.py, the host restatement of the plane finder (include/emf_hip.h "Planes"):
every device stage stated twice agrees with itself; on the analytic 48^3 room it finds the three planes and not the
sphere, each within the bounds that follow from the definitions; the records of a box are the whole volume's records
cropped and re-indexed; kinds and the floor choice on hand-made plane lists."""
import math

import numpy as np
import pytest

from tests import planes_reference as pr

SMALL = [((1, 1, 1), "random"), ((3, 3, 3), "random"), ((33, 9, 9), "random"), ((31, 7, 7), "tilted"), ((33, 9, 9), "axis"),
         ((12, 10, 9), "infinite"), ((13, 5, 5), "zero_gradient"), ((9, 9, 9), "unseen")]


@pytest.mark.parametrize("shape,content", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_the_stages_stated_twice_agree(shape, content):
    tsdf, weights = pr.volume(shape, content)
    rec, counts = pr.records(tsdf, weights)
    rec2, counts2 = pr.records_loop(tsdf, weights)
    assert counts == counts2 and rec.tobytes() == rec2.tobytes()
    for K in (1, 2, 15, 16, 31):
        assert pr.direction_bins(rec, K).tobytes() == pr.direction_bins_loop(rec, K).tobytes()
        assert int(pr.direction_bins(rec, K).sum()) == len(rec)
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(5, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    shift = rng.uniform(0, 20, 5).astype(np.float32)
    args = (rec, shape, dirs, shift, 0.5, 0.7, 40)
    assert pr.offset_hist(*args).tobytes() == pr.offset_hist_loop(*args).tobytes()
    planes = np.concatenate([dirs, rng.uniform(-3, 12, (5, 1)).astype(np.float32)], 1)
    a, b = pr.assign(rec, shape, planes, 0.3, 2.5), pr.assign_loop(rec, shape, planes, 0.3, 2.5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_fixtures_hold_what_their_names_say():
    assert pr.records(*pr.volume((1, 1, 1), "random"))[1][1] == 0                # a single voxel has no normal
    assert pr.records(*pr.volume((9, 9, 9), "unseen"))[1] == (0, 0)
    surface, normals = pr.records(*pr.volume((13, 5, 5), "zero_gradient"))[1]
    assert surface == 3 * 25 and normals == 0                                    # three slabs, every difference 0
    tsdf, weights = pr.volume((12, 10, 9), "infinite")
    surface, normals = pr.records(tsdf, weights)[1]
    assert surface > normals > 0
    tsdf, weights = pr.volume((33, 9, 9), "random")
    assert np.isnan(tsdf).any() and np.isnan(weights).any() and (weights < 0).any() and np.signbit(tsdf[tsdf == 0]).any()
    assert pr.records(tsdf, weights)[1][1] > 50


def test_the_carry_case_has_records_on_both_sides_of_the_carry():
    """The case of tests/test_gpu_planes.py with more than 1024 tiles: the one workgroup that scans the tiles' counts
    takes them 1024 at a time, and a tile behind the first 1024 holds a record whose rank needs what came before."""
    from tests.test_gpu_planes import CASES
    shape, box, content = CASES[-1]
    assert box is None and content == "random"
    ntx, nty, ntz = (-(-shape[k] // pr.TILE[k]) for k in range(3))
    assert ntx * nty * ntz > 1024
    rec, counts = pr.records(*pr.volume(shape, content))
    x, y, z = pr.voxel_of(rec["index"], shape)
    tile = ((z // pr.TILE[2]) * nty + y // pr.TILE[1]) * ntx + x // pr.TILE[0]
    assert (np.diff(tile) >= 0).all()  # records are in tile order
    assert (tile >= 1024).sum() >= 1 and (tile < 1024).sum() >= 1


def test_the_recurring_labels_recur():
    rec, size, planes, cos2, band = pr.recurring_labels()
    labels, mom = pr.assign(rec, size, planes, cos2, band)
    assert labels.tolist() == pr.RECURRING * 8  # A, B, A within one wave of 64 records, and lanes without a label
    assert mom[0]["count"] == 32 and mom[1]["count"] == 24
    a, b = pr.assign_loop(rec, size, planes, cos2, band)
    assert a.tobytes() == labels.tobytes() and b.tobytes() == mom.tobytes()


def truth(k):
    n, d = pr.ROOM_PLANES[k]
    return np.asarray(n) / np.linalg.norm(n), d


@pytest.mark.parametrize("noise", [0.0, 0.02])
def test_the_room_has_three_planes_and_no_sphere(noise):
    """Centroids lie within (-1, 0] voxels of the true plane along its normal: a solid voxel with a free face neighbour is
    less than one voxel behind the zero crossing.  A refined normal is no farther from the truth than the seed's own
    bound atan(sqrt(2) / K), the half-diagonal of a cube-map cell.  Figures of this restatement without noise:
    0.00, 0.01 and 0.26 degrees, offsets 0.00, -0.47 and -0.51; with noise 0.03 to 0.33 degrees, -0.54 to -0.48."""
    K = 15
    tsdf, weights = pr.room(noise)
    planes, rec, labels = pr.find_planes(tsdf, weights, K=K)
    assert len(planes) == 3
    bound = math.degrees(math.atan(math.sqrt(2.0) / K))
    matched = set()
    for p in planes:
        angles = [math.degrees(math.acos(min(1.0, float(np.dot(truth(k)[0], p["n"]))))) for k in range(3)]
        k = int(np.argmin(angles))
        matched.add(k)
        offset = float(np.dot(truth(k)[0], p["centroid"])) - truth(k)[1]
        print(f"noise {noise}: plane {k}: {p['count']} voxels, {angles[k]:.3f} degrees, offset {offset:.3f}, thickness {p['thickness']:.3f}")
        assert angles[k] <= bound
        assert -1.0 < offset <= 1e-9
        assert p["thickness"] < 1.0
    assert matched == {0, 1, 2}
    # the sphere's shell is in the records; a plane can only take the cap whose normals lie within 20 degrees of its
    # own, (1 - cos 20) / 2 = 3 % of a sphere, so three planes take less than a tenth
    x, y, z = pr.voxel_of(rec["index"], (48, 48, 48))
    c, r = pr.ROOM_SPHERE
    on_sphere = np.abs(np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r) < 1.5
    assert on_sphere.sum() > 300 and (labels[on_sphere] >= 0).mean() < 0.1


def test_a_box_is_a_crop_of_the_volume():
    tsdf, weights = pr.volume((40, 24, 20), "random")
    whole, _ = pr.records(tsdf, weights)
    lo, size = (5, 3, 2), (33, 17, 9)
    x, y, z = pr.voxel_of(whole["index"], (40, 24, 20))
    inside = ((x >= lo[0]) & (x < lo[0] + size[0]) & (y >= lo[1]) & (y < lo[1] + size[1]) & (z >= lo[2]) & (z < lo[2] + size[2]))
    bx, by, bz = x[inside] - lo[0], y[inside] - lo[1], z[inside] - lo[2]
    want = whole[inside][pr.tile_order(bx, by, bz, size)]
    want["index"] = ((bz * size[1] + by) * size[0] + bx)[pr.tile_order(bx, by, bz, size)]
    got, counts = pr.records(tsdf, weights, (lo, size))
    assert counts[1] == len(want) > 100 and got.tobytes() == want.tobytes()
    assert got.tobytes() == pr.records_loop(tsdf, weights, (lo, size))[0].tobytes()


def rot(deg):
    a = math.radians(deg)
    return [math.sin(a), math.cos(a), 0.0]  # tilted from +y towards +x


def test_kinds_and_the_floor_choice():
    up = [0.0, 2.0, 0.0]
    # at floor_angle and just beyond
    assert pr.kinds([rot(30.0 - 1e-9)], [0.0], up)[0] == 0 and pr.kinds([rot(30.0 + 1e-6)], [0.0], up)[0] is None
    # the lowest candidate wins, ties to the lowest index
    assert pr.kinds([rot(0), rot(5), rot(1)], [2.0, 1.0, 1.5], up)[0] == 1
    assert pr.kinds([rot(0), rot(5), rot(1)], [1.0, 1.0, 1.0], up)[0] == 0
    # kinds relative to the floor's normal, at kind_angle and just beyond
    normals = [rot(0), rot(10.0 - 1e-9), rot(10.0 + 1e-6), rot(180), rot(90), rot(80.0 + 1e-9), rot(80.0 - 1e-6), rot(45)]
    floor, names = pr.kinds(normals, [0.0] + [1.0] * 7, up)
    assert floor == 0 and names == ["floor", "level", "slope", "ceiling", "wall", "wall", "slope", "slope"]
    # no candidate: kinds relative to up itself
    floor, names = pr.kinds([rot(90), rot(180), rot(40)], [0.0, 0.0, 0.0], up)
    assert floor is None and names == ["wall", "ceiling", "slope"]


def host_fixtures():
    yield "room", pr.room(0.0), (48, 48, 48)
    yield "noisy room", pr.room(0.02), (48, 48, 48)
    yield "random", pr.volume((33, 17, 9), "random"), (33, 17, 9)
    yield "tilted", pr.volume((40, 24, 20), "tilted"), (40, 24, 20)


class c_entries:
    """The C statement: emf_fusion_plane_directions / _offsets / _fit called directly (no device, no handle), with the
    return values of their numpy twins in emfusion_amd.pipeline."""

    @staticmethod
    def plane_directions(bins, k, min_votes, separation):
        import ctypes as C
        from emfusion_amd import pipeline
        b = np.ascontiguousarray(np.asarray(bins, np.uint32).reshape(-1))
        dirs, which, votes, n = np.zeros((16, 3)), np.zeros(16, np.int32), np.zeros(16, np.uint32), C.c_int32(0)
        assert pipeline.load().emf_fusion_plane_directions(b.ctypes.data, int(k), int(min_votes), float(separation), dirs.ctypes.data,
                                                           which.ctypes.data, votes.ctypes.data, C.byref(n)) == 0
        return dirs[:n.value].copy(), which[:n.value].copy(), votes[:n.value].copy()

    @staticmethod
    def plane_offsets(n, size, bin, row, min_votes, peak_gap):
        import ctypes as C
        from emfusion_amd import pipeline
        n = np.ascontiguousarray(np.asarray(n, np.float64).reshape(3))
        r = np.ascontiguousarray(np.asarray(row, np.uint32).reshape(-1))
        lo, slots, inv_bin, shift, count = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_int32(0)
        ps, pv = np.zeros(max(r.size, 1), np.int32), np.zeros(max(r.size, 1), np.uint32)
        assert pipeline.load().emf_fusion_plane_offsets(n.ctypes.data, (C.c_int32 * 3)(*size), float(bin), C.byref(lo), C.byref(slots),
                                                        C.byref(inv_bin), C.byref(shift), r.ctypes.data, int(min_votes), int(peak_gap),
                                                        ps.ctypes.data, pv.ctypes.data, r.size, C.byref(count)) == 0
        return lo.value, slots.value, inv_bin.value, shift.value, [(int(ps[i]), int(pv[i])) for i in range(count.value)]

    @staticmethod
    def plane_fit(moments, seed_n, seed_d):
        from emfusion_amd import pipeline
        m = np.ascontiguousarray(np.asarray(moments, pr.MOMENTS).reshape(()))
        seed = np.ascontiguousarray(np.asarray(seed_n, np.float64).reshape(3))
        out = np.zeros((), pipeline.PLANE_DTYPE)
        assert pipeline.load().emf_fusion_plane_fit(m.ctypes.data, seed.ctypes.data, float(seed_d), out.ctypes.data) == 0
        return out


def statements():
    from emfusion_amd import pipeline
    return (("C", c_entries), ("numpy", pipeline))


@pytest.mark.parametrize("stmt", [0, 1], ids=["C", "numpy"])
def test_the_host_steps_in_c_numpy_and_python_floats_agree_bit_for_bit(stmt):
    """The three statements of the host steps: emf_fusion_plane_directions / _offsets / _fit in C, their numpy twins in
    emfusion_amd.pipeline and the Python floats of tests/planes_reference.py.  Each of the first two equals the third in
    directions, offset frames, peaks and fits as float64 bits on every fixture, so all three agree."""
    name_, pipeline = statements()[stmt]
    checked = 0
    for name, (tsdf, weights), size in host_fixtures():
        rec, _ = pr.records(tsdf, weights)
        for K, min_votes, sep in ((15, 20, 20.0), (16, 1, 5.0), (31, 3, 45.0), (1, 1, 20.0)):
            bins = pr.direction_bins(rec, K)
            want = pr.directions(bins, K, min_votes, sep)
            dirs, which, votes = pipeline.plane_directions(bins, K, min_votes, sep)
            assert which.tolist() == [d[0] for d in want] and votes.tolist() == [d[1] for d in want], (name, K)
            assert dirs.tobytes() == np.array([d[2] for d in want], np.float64).reshape(-1, 3).tobytes(), (name, K)
        c = math.cos(math.radians(20.0))
        few = 20 if "random" not in name else 2  # a random volume has no strong direction
        dirs = pr.directions(pr.direction_bins(rec, 15), 15, few, 20.0)
        assert dirs
        for bin_vox in (1.0, 0.7, 2.5):
            frames = [pr.offset_frame(d[2], size, bin_vox) for d in dirs]
            S = max(f[1] for f in frames)
            hist = pr.offset_hist(rec, size, [d[2] for d in dirs], [f[3] for f in frames], c * c, frames[0][2], S)
            for d, f, row in zip(dirs, frames, hist):
                for gap in (0, 2):
                    lo, slots, inv_bin, shift, peaks = pipeline.plane_offsets(d[2], size, bin_vox, row[:f[1]], few // 2, gap)
                    assert np.array([lo, inv_bin, shift]).tobytes() == np.array([f[0], f[2], f[3]]).tobytes() and slots == f[1]
                    assert peaks == pr.offset_peaks(row[:f[1]], few // 2, gap)
        planes, rec, labels = pr.find_planes(tsdf, weights, min_votes=few, refine=0)
        seeds = [(p["n"], p["d"]) for p in planes]
        labels, mom = pr.assign(rec, size, [list(n) + [d] for n, d in seeds], c * c, 2.0)
        for k, (n, d) in enumerate(seeds):
            for flip in (1.0, -1.0):
                seed = [flip * v for v in n]
                want = pr.fit(mom[k], seed, d)
                got = pipeline.plane_fit(mom[k], seed, d)
                assert int(got["fitted"]) == int(want["fitted"]) and int(got["count"]) == int(mom[k]["count"])
                assert got.tobytes() == statements()[1 - stmt][1].plane_fit(mom[k], seed, d).tobytes(), (name, k)  # whole records
                assert got["n"].tobytes() == np.array(want["n"]).tobytes() and float(got["d"]) == want["d"], (name, k)
                if want["fitted"]:
                    assert got["centroid"].tobytes() == np.array(want["centroid"]).tobytes()
                    assert float(got["thickness"]) == want["thickness"]
                    assert got["axes"].tobytes() == np.array(want["axes"]).tobytes()
                    assert got["eigenvalues"].tobytes() == np.array(want["eigenvalues"]).tobytes()
                    checked += 1
        pair = np.zeros((), pr.MOMENTS)
        pair["count"], pair["sum"] = 2, (3, 4, 5)
        got = pipeline.plane_fit(pair, [0.0, 0.6, 0.8], 1.25)
        assert int(got["fitted"]) == 0 and got["n"].tolist() == [0.0, 0.6, 0.8] and float(got["d"]) == 1.25
    assert checked >= 8


def test_kinds_agree_between_the_pipeline_and_the_restatement():
    from emfusion_amd import pipeline
    rng = np.random.default_rng(5)
    for _ in range(20):
        normals = rng.normal(size=(6, 3))
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
        normals[0] = (0.05, 0.99, 0.02) / np.linalg.norm((0.05, 0.99, 0.02))
        heights = rng.uniform(-1, 1, 6).tolist()
        up = rng.normal(size=3) * 0.1 + (0, 1, 0)
        assert pipeline.plane_kinds(normals, heights, up) == pr.kinds([list(n) for n in normals], heights, list(up))
