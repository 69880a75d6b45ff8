"""tests/patches_reference.py against itself and against the host steps of the library, without a
device: the two statements of the device stage agree on every fixture and on random volumes; the rectangle and the
support test agree bit for bit between emf_fusion_plane_patch_rect / emf_fusion_plane_support, pipeline's numpy float64
and the restatement's Python floats; two slabs whose tops lie on one level are one plane and two patches, with and
without noise and tilt, each rectangle holding its own slab and not the other; a noisy side face falls apart at a reach
of one voxel and is whole at two; plane_support on analytic boxes."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import patches_reference as qr
from tests import planes_reference as pr

SIZE = (48, 48, 48)
_found = {}


def slabs(noise, tilt):
    """(planes, records, labels) of planes_reference.find_planes on two_slabs: computed once, read-only."""
    if (noise, tilt) not in _found:
        planes, rec, labels = pr.find_planes(*qr.two_slabs(noise, tilt))
        rec.setflags(write=False)
        labels.setflags(write=False)
        _found[noise, tilt] = (planes, rec, labels)
    return _found[noise, tilt]


def level_of(planes):
    """The plane of the slabs' tops: the one facing up that is not the lowest."""
    up = [p for p in planes if p["n"][1] > 0.9]
    assert len(up) == 2, [(p["n"], p["d"], p["count"]) for p in planes]
    return max(up, key=lambda p: p["d"])


def patches_of(planes, rec, labels, reach):
    P = max(p["label"] for p in planes) + 1
    axes = np.zeros((P, 6), np.float32)
    for p in planes:
        axes[p["label"]] = np.array(p["axes"], np.float64).reshape(6).astype(np.float32)
    patch = qr.patch_ids(rec, labels, SIZE, reach)
    return patch, qr.patch_records(rec, labels, patch, SIZE, axes), axes


def test_the_half_neighbourhood():
    for reach, count in ((1, 13), (2, 62)):
        half = qr.half_offsets(reach)
        assert len(half) == count == ((2 * reach + 1) ** 3 - 1) // 2
        assert len({tuple(o) for o in half} | {(-a, -b, -c) for a, b, c in half}) == 2 * count  # every pair once


@pytest.mark.parametrize("fixture", ["doorway", "recurring", "slabs", "noisy_slabs"])
def test_the_two_statements_agree_on_the_fixtures(fixture):
    if fixture in ("doorway", "recurring"):
        rec, labels, size = getattr(qr, fixture)()
        P = int(labels.max()) + 1
    else:
        planes, rec, labels = slabs(0.02 if fixture == "noisy_slabs" else 0.0, 0.0)
        size, P = SIZE, max(p["label"] for p in planes) + 1
    axes = np.random.default_rng(3).normal(size=(P, 6)).astype(np.float32)
    for reach in (1, 2):
        patch = qr.patch_ids(rec, labels, size, reach)
        assert patch.tobytes() == qr.patch_ids_loop(rec, labels, size, reach).tobytes()
        assert qr.patch_records(rec, labels, patch, size, axes).tobytes() == qr.patch_records_loop(rec, labels, patch, size, axes).tobytes()
        if reach == 1:
            assert patch.tobytes() == qr.patch_ids_label(rec, labels, size).tobytes()
        assert ((patch >= 0) == (labels >= 0)).all() and (patch <= np.arange(len(rec))).all()
        roots = patch[patch >= 0]
        assert (patch[roots] == roots).all()  # an id is a member of its own patch


@pytest.mark.parametrize("shape", [(33, 9, 9), (31, 7, 7), (40, 24, 20), (2048, 2, 2)])
def test_the_two_statements_agree_on_random_volumes(shape):
    tsdf, weights = pr.random_volume(shape, 5)
    rec, _ = pr.records(tsdf, weights)
    if shape == (2048, 2, 2):  # no voxel of this box has six neighbours: records by hand
        rng = np.random.default_rng(2)
        vox = [(int(x), int(y), int(z)) for x, y, z in zip(rng.integers(0, 2048, 600), rng.integers(0, 2, 600), rng.integers(0, 2, 600))]
        rec = qr.records_of(sorted(set(vox)), shape)
    labels = np.random.default_rng(1).integers(-1, 3, len(rec)).astype(np.int16)
    axes = np.random.default_rng(4).normal(size=(3, 6)).astype(np.float32)
    assert len(rec) > 50
    for reach in (1, 2):
        patch = qr.patch_ids(rec, labels, shape, reach)
        assert patch.tobytes() == qr.patch_ids_loop(rec, labels, shape, reach).tobytes()
        assert qr.patch_records(rec, labels, patch, shape, axes).tobytes() == qr.patch_records_loop(rec, labels, patch, shape, axes).tobytes()
        assert len(np.unique(patch[patch >= 0])) > 3


def test_what_the_fixtures_hold():
    rec, labels, size = qr.doorway()
    for reach in (1, 2):
        assert np.unique(qr.patch_ids(rec, labels, size, reach), return_counts=True)[1].tolist() == [96, 96]
    rec, labels, size = qr.recurring()
    assert len(rec) == 64
    order = qr.patch_ids(rec, labels, size, 1).tolist()
    runs = [p for k, p in enumerate(order) if k == 0 or order[k - 1] != p]
    assert len(runs) == 6 and runs[1] == runs[3] == runs[5] and len(set(runs)) == 4  # p, r, q, r, s, r
    assert labels[runs[0]] == labels[runs[4]] == labels[runs[1]] != labels[runs[2]]   # A, A, B, A, A, A


@pytest.mark.parametrize("noise,tilt", [(0.0, 0.0), (0.02, 0.0), (0.0, 3.0), (0.02, 3.0)])
def test_two_slabs_of_one_height_are_one_plane_and_two_patches(noise, tilt):
    planes, rec, labels = slabs(noise, tilt)
    level = level_of(planes)
    patch, records, axes = patches_of(planes, rec, labels, 1)
    mine = records[records["plane"] == level["label"]]
    print(noise, tilt, level["count"], mine["count"].tolist())
    assert len(mine) == 2 and int(mine["count"].sum()) == level["count"] and mine["count"].min() > 100
    # each rectangle holds the footprint of its own slab's top and not the other's: in the plane's own coordinates
    u, v = (np.array(a) for a in level["axes"])
    x, y, z = pr.voxel_of(rec["index"], SIZE)
    pts = np.stack([x, y, z], 1).astype(np.float64)
    rects = [qr.rect(level, m) for m in mine]
    for k, (m, r) in enumerate(zip(mine, rects)):
        assert 0.2 < r["fill"] < 1.05, r["fill"]  # the axes are the PLANE's, fitted to both slabs: a turned rectangle is larger
        cu, cv = float(np.dot(r["center"], u)), float(np.dot(r["center"], v))
        for j, other in enumerate(mine):
            p = pts[patch == other["id"]]
            inside = (np.abs(p @ u - cu) <= r["half"][0]) & (np.abs(p @ v - cv) <= r["half"][1])
            assert inside.all() if j == k else not inside.any(), (k, j)
        for c in r["corners"]:
            assert abs(float(np.dot(level["n"], c)) - level["d"]) < 1e-9
        assert r["fit"]["fitted"] and float(np.dot(r["fit"]["n"], level["n"])) > 0.999


def test_a_noisy_side_face_needs_a_reach_of_two():
    """Gaussian noise 0.05 on the tsdf: the face x = 19 of the long slab loses a voxel's neighbours at a reach of one and
    is one piece at two.  So the reach has to be a parameter."""
    planes, rec, labels = slabs(0.05, 0.0)
    face = [p for p in planes if p["n"][0] > 0.9 and abs(p["d"] - 19.0) < 0.5]
    assert len(face) == 1 and face[0]["count"] > 300
    counts = {}
    for reach in (1, 2):
        patch = qr.patch_ids(rec, labels, SIZE, reach)
        counts[reach] = sorted(np.unique(patch[labels == face[0]["label"]], return_counts=True)[1].tolist(), reverse=True)
    print(counts)
    assert len(counts[1]) > 1 and len(counts[2]) == 1 and counts[2][0] == face[0]["count"] == sum(counts[1])


# ---- the host steps: C, numpy float64 and Python floats ------------------------------------------------------------

def test_the_rectangle_agrees_bit_for_bit():
    from emfusion_amd import pipeline
    from emfusion_amd._lib import PLANE_PATCH_DTYPE
    lib = pipeline.load()
    checked = 0
    for noise, tilt in ((0.0, 0.0), (0.02, 3.0)):
        planes, rec, labels = slabs(noise, tilt)
        patch, records, axes = patches_of(planes, rec, labels, 1)
        assert records.dtype == np.dtype(PLANE_PATCH_DTYPE)
        for p in planes:
            raw = np.zeros((), pipeline.PLANE_DTYPE)
            raw["n"], raw["d"], raw["axes"], raw["label"] = p["n"], p["d"], np.array(p["axes"]).reshape(6), p["label"]
            for m in records[records["plane"] == p["label"]]:
                want = qr.rect(p, m)
                got_np = pipeline.plane_patch_rect(raw, m)
                got_c = np.zeros((), pipeline.PLANE_PATCH_RECT_DTYPE)
                one = np.ascontiguousarray(m).reshape(1)
                assert lib.emf_fusion_plane_patch_rect(raw.ctypes.data, one.ctypes.data, got_c.ctypes.data) == 0
                assert got_c.tobytes() == got_np.tobytes(), (p["label"], m["id"])
                assert got_np["center"].tobytes() == np.array(want["center"]).tobytes()
                assert got_np["half"].tobytes() == np.array(want["half"]).tobytes()
                assert got_np["corners"].tobytes() == np.array(want["corners"]).tobytes()
                assert float(got_np["fill"]) == want["fill"]
                fit = want["fit"]
                assert got_np["fit"]["n"].tobytes() == np.array(fit["n"]).tobytes() and float(got_np["fit"]["d"]) == fit["d"]
                assert bool(got_np["fit"]["fitted"]) == fit["fitted"] and int(got_np["fit"]["count"]) == int(m["count"])
                if fit["fitted"]:
                    assert got_np["fit"]["centroid"].tobytes() == np.array(fit["centroid"]).tobytes()
                    assert float(got_np["fit"]["thickness"]) == fit["thickness"]
                checked += 1
    assert checked > 20
    null = lib.emf_fusion_plane_patch_rect(None, one.ctypes.data, got_c.ctypes.data)
    assert null != 0


def support_all(n, d, center, axes, half, box):
    """(s, over) by the C entry, by numpy float64 and by Python floats: equal as bits."""
    from emfusion_amd import pipeline
    lib = pipeline.load()
    arrays = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (n, center, axes, half, box["center"], box["axes"], box["half"])]
    outs = []
    for margin in (0.0, 0.25):
        s, over = C.c_double(0.0), C.c_int32(-1)
        assert lib.emf_fusion_plane_support(arrays[0].ctypes.data, float(d), arrays[1].ctypes.data, arrays[2].ctypes.data,
                                            arrays[3].ctypes.data, arrays[4].ctypes.data, arrays[5].ctypes.data,
                                            arrays[6].ctypes.data, margin, C.byref(s), C.byref(over)) == 0
        got_np = pipeline.plane_support_of(n, d, center, axes, half, box["center"], box["axes"], box["half"], margin)
        want = qr.support([float(v) for v in n], float(d), [float(v) for v in center], [[float(v) for v in a] for a in axes],
                          [float(v) for v in half], [float(v) for v in box["center"]], [[float(v) for v in a] for a in box["axes"]],
                          [float(v) for v in box["half"]], margin)
        assert np.float64(s.value).tobytes() == np.float64(got_np[0]).tobytes() == np.float64(want[0]).tobytes()
        assert bool(over.value) == got_np[1] == want[1]
        outs.append(want)
    return outs


def test_the_support_agrees_bit_for_bit():
    rng = np.random.default_rng(8)
    flips = 0
    for _ in range(200):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        b, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        center = rng.normal(size=3)
        box = dict(center=center + q[0] * rng.uniform(-1.5, 1.5) + q[1] * rng.uniform(-1.5, 1.5) + q[2] * rng.uniform(0, 0.5), axes=b,
                   half=rng.uniform(0.05, 0.4, 3))
        outs = support_all(q[2], float(np.dot(q[2], center)), center, q[:2], rng.uniform(0.5, 1.3, 2), box)
        flips += outs[0][1] != outs[1][1]
    assert flips > 3  # the margin decides some of them


def slab_patch(kind="level"):
    """A patch in the world: a 1.0 x 0.6 m rectangle at height y = 0.7, normal +y."""
    return dict(kind=kind, normal=[0.0, 1.0, 0.0], d=0.7, rect=dict(center=[0.2, 0.7, 1.0], axes=[[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]],
                                                                     half_m=[0.5, 0.3]))


def box_at(x, z, bottom, half=(0.1, 0.15, 0.1), turn=0.0):
    c, s = math.cos(turn), math.sin(turn)
    return dict(center=[x, bottom + half[1], z], axes=[[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], half=list(half))


def test_plane_support_on_analytic_boxes():
    from emfusion_amd import pipeline
    slab, floor = slab_patch(), dict(slab_patch("floor"), d=0.0)
    floor["rect"] = dict(center=[0.0, 0.0, 1.0], axes=slab["rect"]["axes"], half_m=[3.0, 3.0])
    wall = dict(kind="wall", normal=[1.0, 0.0, 0.0], d=-0.3, rect=dict(center=[-0.3, 0.7, 1.0], axes=[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
                                                                       half_m=[0.7, 3.0]))
    patches = [floor, wall, slab]
    boxes = [box_at(0.3, 1.1, 0.7),              # on the slab
             box_at(0.3, 1.1, 0.7, turn=0.6),    # ... turned about up: the same height
             box_at(0.9, 1.1, 0.7),              # beside it, at its height: over the floor only, 0.7 above it
             box_at(0.3, 1.1, 0.7 + 0.051),      # hovering just above the gap
             box_at(0.3, 1.1, 0.7 + 0.049),      # ... and just inside it
             box_at(0.9, 1.1, 0.0),              # on the floor beside the slab
             box_at(-0.2, 1.0, 0.35, half=(0.1, 0.1, 0.1)),  # touching the wall, on nothing
             None]
    got = pipeline.plane_support(patches, boxes)
    assert [None if g is None else g[0] for g in got] == [2, 2, None, None, 2, 0, None, None]
    assert abs(got[0][1]) < 1e-12 and abs(got[1][1]) < 1e-12 and abs(got[4][1] - 0.049) < 1e-12 and got[5][1] == 0.0
    for box, g in zip(boxes[:-1], got):
        assert qr.rests_on(patches, box) == g
    # over a wall: the wrong kind, however close
    s, over = pipeline.plane_support_of(wall["normal"], wall["d"], wall["rect"]["center"], wall["rect"]["axes"], wall["rect"]["half_m"],
                                        boxes[6]["center"], boxes[6]["axes"], boxes[6]["half"])
    assert over and abs(s) < 1e-12
    assert pipeline.plane_support([wall], [boxes[6]]) == [None] and pipeline.plane_support([dict(wall, kind="level")], [boxes[6]])[0][0] == 0
    # equal |s| to two patches: the earlier one
    twin = dict(slab_patch(), rect=dict(slab["rect"], center=[0.25, 0.7, 1.05]))
    assert pipeline.plane_support([slab, twin], [boxes[0]])[0][0] == 0 and pipeline.plane_support([twin, slab], [boxes[0]])[0][0] == 0
    above, below = dict(slab_patch(), d=0.68), dict(slab_patch(), d=0.72)  # |s| = 0.02 on either side
    assert [g[0] for g in pipeline.plane_support([above, below], [boxes[0]])] == [0]
    assert qr.rests_on([above, below], boxes[0])[0] == 0
    # the margin widens the rectangle
    edge = box_at(0.2 + 0.5 + 0.02, 1.0, 0.7)
    assert pipeline.plane_support([slab], [edge]) == [None] and pipeline.plane_support([slab], [edge], margin=0.05)[0][0] == 0


def test_the_gpu_cases_hold_what_they_claim():
    from tests import test_gpu_plane_patches as cases
    cases.test_what_the_cases_hold()
