"""emf_hip_planePatchLabel and emf_hip_planePatches (include/emf_hip.h "Planes", stage 4) against
tests/patches_reference.py, byte for byte: the volume / box / content cases of the plane finder rebuilt from
tests/planes_reference.py, and record lists built by hand -- none, one, no member, one patch of everything, every record
its own patch, counts across the wave and the scan's carry, a patch that comes back within a wave, links that exist only
across a tile face, edge and corner, links at a distance of exactly two, neighbours outside the box and a 2048 x 2 x 2
box; min_count, capacity_patches and n_patches at their ends; outputs poisoned beforehand, a second call into the dirty
buffers, the library built with contraction on, every refusal, and a shuffled list that only has to come back."""
import ctypes as C

import numpy as np
import pytest

from tests import patches_reference as qr
from tests import planes_reference as pr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 5                # elements of room behind every output

# (volume shape, box or None, content), shapes (nx, ny, nz): the cases of the plane finder's own test
VOLUMES = [
    ((1, 1, 1), None, "random"),
    ((3, 3, 3), None, "random"),
    ((32, 8, 8), None, "random"),
    ((33, 9, 9), None, "random"),
    ((31, 7, 7), None, "random"),
    ((33, 9, 9), None, "tilted"),
    ((33, 9, 9), None, "axis"),
    ((96, 40, 40), ((5, 3, 7), (64, 16, 16)), "random"),
    ((96, 40, 40), ((5, 3, 7), (64, 16, 16)), "tilted"),
    ((96, 40, 40), ((17, 9, 13), (64, 16, 16)), "axis"),
    ((40, 24, 20), None, "tilted"),
    ((40, 24, 20), ((7, 8, 4), (33, 16, 16)), "random"),
    ((40, 24, 20), ((0, 0, 0), (33, 9, 9)), "random"),
    ((2048, 2, 2), None, "random"),
    ((2048, 4, 4), ((0, 1, 1), (2048, 2, 2)), "random"),
    ((12, 10, 9), None, "infinite"),
    ((13, 5, 5), None, "zero_gradient"),
    ((40, 24, 20), None, "unseen"),
]
P_CASE = 6  # planes of a volume case: the six axis directions through the middle of the box


def volume_id(c):
    box = "" if c[1] is None else "-" + "x".join(map(str, c[1][1])) + "at" + "x".join(map(str, c[1][0]))
    return "x".join(map(str, c[0])) + box + "-" + c[2]


def volume_case(case):
    """(records, labels, size) of a volume case: stage 1's records and stage 3's labels for the six axis planes through
    the middle of the box with a gate of 60 degrees and a band of 3 voxels, so that planes share voxels' neighbourhoods
    and some records stay without a label."""
    shape, box, content = case
    tsdf, weights = pr.volume(shape, content)
    rec, _ = pr.records(tsdf, weights, box)
    size = shape if box is None else box[1]
    planes = []
    for j in range(3):
        for sign in (1.0, -1.0):
            n = [0.0, 0.0, 0.0]
            n[j] = sign
            planes.append(n + [sign * (size[j] - 1) / 2.0])
    labels, _ = pr.assign(rec, size, np.array(planes, np.float32), np.float32(0.25), 3.0)
    return rec, labels, tuple(size)


def first_records(n, every=7):
    """The first n voxels of a 64 x 8 x 8 box in stage 1's order, label 0 but every `every`-th without one."""
    size = (64, 8, 8)
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(64), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    order = pr.tile_order(x, y, z, size)[:n]
    rec = qr.records_of(np.stack([x[order], y[order], z[order]], 1), size)
    labels = np.zeros(n, np.int16)
    labels[every - 1::every] = -1
    return rec, labels, size


def by_hand(name):
    """(records, labels, size) of a hand-built case, labels in the records' order."""
    if name == "none":
        return np.zeros(0, pr.VOXEL), np.zeros(0, np.int16), (8, 8, 8)
    if name == "one":
        return qr.records_of([(3, 2, 1)], (8, 8, 8)), np.zeros(1, np.int16), (8, 8, 8)
    if name == "no_member":
        rec, labels, size = first_records(100)
        return rec, np.full(100, -1, np.int16), size
    if name == "one_patch":
        rec, labels, size = first_records(512, every=10 ** 6)
        return rec, labels, size
    if name in ("checkerboard", "carry"):  # no two voxels within one step of each other share a label: every record its
        size = (12, 10, 9) if name == "checkerboard" else (128, 64, 40)  # own patch; carry: 1280 workgroups of each
        z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
        vox = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        order = pr.tile_order(vox[:, 0], vox[:, 1], vox[:, 2], size)
        vox = vox[order]
        return qr.records_of(vox, size), (vox[:, 0] % 2 + 2 * (vox[:, 1] % 2) + 4 * (vox[:, 2] % 2)).astype(np.int16), size
    if name.startswith("first"):
        return first_records(int(name[5:]))
    if name == "recurring":
        return qr.recurring()
    if name == "across_tiles":  # a pair across a tile face, one across a tile edge, one across a tile corner
        size = (64, 16, 16)
        vox = [(31, 3, 3), (32, 3, 3), (31, 7, 3), (32, 8, 3), (31, 7, 7), (32, 8, 8), (31, 15, 15), (32, 15, 15)]
        return qr.records_of(vox, size), np.zeros(len(vox), np.int16), size
    if name == "distance_two":  # pairs exactly two apart along (2, 0, 0), (0, 2, 1), (2, 2, 2), (-2, 1, 2) and (1, -2, -2)
        size = (40, 16, 16)
        vox = []
        for k, d in enumerate([(2, 0, 0), (0, 2, 1), (2, 2, 2), (-2, 1, 2), (1, -2, -2)]):
            a = (4 + 7 * k, 6, 6)
            vox += [a, (a[0] + d[0], a[1] + d[1], a[2] + d[2])]
        return qr.records_of(vox, size), np.zeros(len(vox), np.int16), size
    if name == "box_faces":  # three columns on the faces of a small box: most neighbours fall outside it, and (4, 2, z) and
        size = (5, 4, 3)     # (0, 3, z) are neighbours in the linear index but four voxels apart
        vox = [(x, y, z) for z in range(size[2]) for x, y in ((0, 0), (4, 2), (0, 3))]
        return qr.records_of(vox, size), np.zeros(len(vox), np.int16), size
    if name == "long_box":
        size = (2048, 2, 2)
        rng = np.random.default_rng(11)
        z, y, x = np.meshgrid(np.arange(2), np.arange(2), np.arange(2048), indexing="ij")
        vox = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)[rng.uniform(size=8192) < 0.45]
        order = pr.tile_order(vox[:, 0], vox[:, 1], vox[:, 2], size)
        return qr.records_of(vox, size), rng.integers(-1, 2, len(vox)).astype(np.int16)[order], size
    raise ValueError(name)


HAND = ["none", "one", "no_member", "one_patch", "checkerboard", "first63", "first64", "first65", "first1024", "first1025",
        "recurring", "across_tiles", "distance_two", "box_faces", "long_box"]
_expected = {}


def axes_of(P, seed=5):
    """Tilted in-plane axes, P x 6 f32: what the device takes them for is the restatement's matter, not geometry's."""
    a = np.random.default_rng(seed).normal(size=(P, 6))
    return (a / np.linalg.norm(a.reshape(P, 2, 3), axis=2).repeat(3, 1)).astype(np.float32)


def expected(key):
    """(records, labels, size, axes, {reach: (patch, all patch records)}) of the restatement: computed once, shared and
    read-only."""
    if key not in _expected:
        rec, labels, size = by_hand(key) if isinstance(key, str) else volume_case(key)
        P = max(int(labels.max()) + 1 if len(labels) else 1, P_CASE)
        axes = axes_of(P)
        per_reach = {}
        for reach in ((1,) if key == "carry" else (1, 2)):
            patch = qr.patch_ids(rec, labels, size, reach)
            per_reach[reach] = (patch, qr.patch_records(rec, labels, patch, size, axes))
            for a in per_reach[reach]:
                a.setflags(write=False)
        for a in (rec, labels, axes):
            a.setflags(write=False)
        _expected[key] = (rec, labels, size, axes, per_reach)
    return _expected[key]


def i3(v):
    return (C.c_int32 * 3)(*[int(c) for c in v])


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def poisoned(n, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray((n,), dtype).fill_bytes_(POISON)


def ptr(a, offset=0):
    return None if a is None else C.c_void_p(a.ptr + offset)


def is_poison(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


class Inputs:
    """The records, labels and stage 1 counters of a case on the device; capacity = records + EXTRA, the room poisoned."""

    def __init__(self, rec, labels):
        n = len(rec)
        self.n, self.capacity = n, n + EXTRA
        host = np.zeros(self.capacity, pr.VOXEL)
        host[:n] = rec
        host[n:].view(np.uint8)[:] = POISON
        lab = np.full(self.capacity, 0x2525, np.int16)  # a label >= 0 behind the end: it must not be read as a member
        lab[:n] = labels
        self.rec, self.labels = to_dev(host), to_dev(lab)
        self.counters = to_dev(np.array([0, n, n, 0], np.uint32))


def run_label(lib, inp, size, reach, want_patch, want_counters):
    """The labelling into poisoned outputs, twice; returns (patch, patch counters) on the device."""
    d_patch, d_pc = poisoned(inp.capacity + EXTRA, np.int32), poisoned(3 + EXTRA, np.uint32)
    for again in (False, True):
        rc = lib.emf_hip_planePatchLabel(ptr(inp.rec), ptr(inp.labels), ptr(inp.counters), inp.capacity, i3(size), reach,
                                         ptr(d_patch), ptr(d_pc), None)
        assert rc == 0, lib.emf_hip_last_error_string()
        got, got_pc = d_patch.numpy(), d_pc.numpy()
        assert got[:inp.n].tobytes() == want_patch.tobytes(), (reach, again, got[:inp.n], want_patch)
        assert is_poison(got[inp.n:]), "written beyond the records"
        assert got_pc[:3].tolist() == [0, want_counters[1], want_counters[2]], (reach, again, got_pc[:3], want_counters)
        assert is_poison(got_pc[3:])
    return d_patch, d_pc


def run_patches(lib, inp, size, axes, d_patch, d_pc, all_records, min_count, n_patches, capacity_patches, labels, patch):
    want, kept = qr.emitted(all_records, min_count, n_patches, capacity_patches)
    want_pc = qr.counters(labels, patch, kept)
    scratch_bytes = lib.emf_hip_planePatchScratchBytes(inp.capacity, n_patches)
    assert scratch_bytes % 16 == 0 and scratch_bytes >= 132 * min(n_patches, inp.capacity)
    d_scratch = poisoned(scratch_bytes + 16, np.uint8)
    d_out = poisoned(capacity_patches + EXTRA, qr.PATCH)
    for again in (False, True):
        rc = lib.emf_hip_planePatches(ptr(inp.rec), ptr(inp.labels), ptr(d_patch), ptr(inp.counters), inp.capacity, i3(size),
                                      fp(axes), len(axes), min_count, n_patches, ptr(d_scratch), ptr(d_out), capacity_patches,
                                      ptr(d_pc), None)
        assert rc == 0, lib.emf_hip_last_error_string()
        got, got_pc = d_out.numpy(), d_pc.numpy()
        what = (min_count, n_patches, capacity_patches, again)
        assert got_pc[:3].tobytes() == want_pc.tobytes(), (what, got_pc[:3], want_pc)
        assert got[:len(want)].tobytes() == want.tobytes(), (what, got[:len(want)], want)
        assert is_poison(got[len(want):]), ("written beyond the patches", what)
        assert is_poison(d_scratch.numpy()[scratch_bytes:]) and is_poison(got_pc[3:])


def run_case(lib, key, reaches=(1, 2), full=True):
    rec, labels, size, axes, per_reach = expected(key)
    inp = Inputs(rec, labels)
    before = (inp.rec.numpy().tobytes(), inp.labels.numpy().tobytes(), inp.counters.numpy().tobytes())
    for reach in reaches:
        patch, all_records = per_reach[reach]
        total = len(all_records)
        d_patch, d_pc = run_label(lib, inp, size, reach, patch, qr.counters(labels, patch, 0))
        largest = int(all_records["count"].max()) if total else 0
        for min_count in ((1, 2, largest + 1) if full else (1,)):
            for n_patches in sorted({total, max(total - 1, 0), total + 3} if full else {total}):
                kept = qr.emitted(all_records, min_count, n_patches, 1 << 30)[1]
                for capacity_patches in sorted({0, max(kept - 1, 0), kept} if full else {kept}):
                    run_patches(lib, inp, size, axes, d_patch, d_pc, all_records, min_count, n_patches, capacity_patches,
                                labels, patch)
        assert d_patch.numpy()[:inp.n].tobytes() == patch.tobytes()  # the patches are only read
    assert (inp.rec.numpy().tobytes(), inp.labels.numpy().tobytes(), inp.counters.numpy().tobytes()) == before


def lib_():
    from emfusion_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", VOLUMES, ids=volume_id)
def test_the_plane_finders_cases_are_exact(dev, case):
    run_case(lib_(), case)


@pytest.mark.parametrize("name", HAND)
def test_the_cases_built_by_hand_are_exact(dev, name):
    run_case(lib_(), name)


def test_the_scans_cross_their_carry(dev):
    """327680 records, each a patch of its own: 1280 sums of roots and 1280 of kept patches, above the 1024 that the one
    workgroup scans at a time."""
    run_case(lib_(), "carry", reaches=(1,), full=False)
    assert len(expected("carry")[4][1][1]) == 128 * 64 * 40 > 256 * 1024


def test_what_the_cases_hold():
    """So that their exactness means something.  No device."""
    patches = {name: {r: expected(name)[4][r] for r in (1, 2)} for name in HAND}
    assert len(patches["none"][1][1]) == 0 and len(patches["no_member"][1][1]) == 0
    assert patches["one_patch"][1][1]["count"].tolist() == [512]
    n = len(expected("checkerboard")[0])
    assert len(patches["checkerboard"][1][1]) == n == 12 * 10 * 9 and len(patches["checkerboard"][2][1]) == 8
    assert patches["across_tiles"][1][1]["count"].tolist() == [2, 2, 2, 2]
    assert patches["distance_two"][1][1]["count"].tolist() == [1] * 10 and patches["distance_two"][2][1]["count"].tolist() == [2] * 5
    assert len(patches["box_faces"][1][1]) == 3
    order = patches["recurring"][1][0].tolist()
    runs = [p for k, p in enumerate(order) if k == 0 or order[k - 1] != p]
    assert len(runs) == 6 and len(set(runs)) == 4 and len(order) == 64  # p, r, q, r, s, r
    for key in (VOLUMES[7], VOLUMES[11], VOLUMES[14], "long_box"):
        rec, labels, size, axes, per_reach = expected(key)
        counts = per_reach[1][1]["count"]
        assert len(counts) > 3 and counts.max() > 1 and (labels < 0).any() and len(np.unique(labels[labels >= 0])) > 1, key
        assert len(per_reach[2][1]) < len(per_reach[1][1]), key
    rec, labels, size, axes, per_reach = expected(VOLUMES[7])
    x, y, z = pr.voxel_of(rec["index"], size)
    tile = (x // 32, y // 8, z // 8)
    for p in per_reach[1][1][:50]:  # patches that span tiles
        sel = per_reach[1][0] == p["id"]
        if len({(a, b, c) for a, b, c in zip(tile[0][sel], tile[1][sel], tile[2][sel])}) > 1:
            break
    else:
        raise AssertionError("no patch spans two tiles")


def test_the_contraction_build_gives_the_same_bytes(dev):
    from emfusion_amd import _lib
    fma = _lib.load_variant("_fma")
    for key in (VOLUMES[3], VOLUMES[8], VOLUMES[9], "recurring", "long_box"):
        run_case(fma, key, full=False)


def test_the_wrappers(dev):
    from emfusion_amd import ops
    rec, labels, size, axes, per_reach = expected(VOLUMES[8])
    assert ops.PLANE_PATCH_DTYPE == qr.PATCH and ops.PLANE_MAX_REACH == qr.MAX_REACH
    inp = Inputs(rec, labels)
    for reach in (1, 2):
        patch, all_records = per_reach[reach]
        d_patch, d_pc = ops.plane_patch_label(inp.rec, inp.labels, inp.counters, size, reach)
        assert d_patch.numpy()[:inp.n].tobytes() == patch.tobytes()
        out = ops.plane_patches(inp.rec, inp.labels, d_patch, inp.counters, size, axes, d_pc, min_count=2)
        want, kept = qr.emitted(all_records, 2, len(all_records), len(all_records))
        assert d_pc.numpy().tobytes() == qr.counters(labels, patch, kept).tobytes()
        assert out.numpy()[:kept].tobytes() == want.tobytes()


def test_a_shuffled_list_comes_back(dev):
    """Records that are not in stage 1's order give unspecified patches; the calls return, and the counters are in range."""
    lib = lib_()
    rec, labels, size, axes, per_reach = expected(VOLUMES[7])
    order = np.random.default_rng(1).permutation(len(rec))
    wild = rec[order].copy()
    wild["index"][::17] = -5
    wild["index"][5::17] = size[0] * size[1] * size[2] + 3
    inp = Inputs(wild, labels[order])
    for reach in (1, 2):
        d_patch, d_pc = poisoned(inp.capacity, np.int32), poisoned(3, np.uint32)
        assert lib.emf_hip_planePatchLabel(ptr(inp.rec), ptr(inp.labels), ptr(inp.counters), inp.capacity, i3(size), reach,
                                           ptr(d_patch), ptr(d_pc), None) == 0
        pc = d_pc.numpy()
        assert 0 < pc[qr.PATCHES] <= pc[qr.MEMBERS] == (labels >= 0).sum() <= inp.n
        n_patches = int(pc[qr.PATCHES])
        d_scratch = poisoned(lib.emf_hip_planePatchScratchBytes(inp.capacity, n_patches), np.uint8)
        d_out = poisoned(n_patches, qr.PATCH)
        assert lib.emf_hip_planePatches(ptr(inp.rec), ptr(inp.labels), ptr(d_patch), ptr(inp.counters), inp.capacity, i3(size),
                                        fp(axes), len(axes), 1, n_patches, ptr(d_scratch), ptr(d_out), n_patches, ptr(d_pc),
                                        None) == 0
        pc = d_pc.numpy()
        assert pc[qr.KEPT] <= pc[qr.PATCHES] <= pc[qr.MEMBERS] <= inp.n


def test_the_refusals(dev):
    """EMF_E_ARG / EMF_E_LIMIT with nothing enqueued: the poisoned outputs keep every byte."""
    lib = lib_()
    rec, labels, size, axes, per_reach = expected(VOLUMES[3])
    inp = Inputs(rec, labels)
    total = len(per_reach[1][1])
    assert total > 2
    d_patch, d_pc = poisoned(inp.capacity, np.int32), poisoned(3, np.uint32)
    d_scratch, d_out = poisoned(lib.emf_hip_planePatchScratchBytes(inp.capacity, total), np.uint8), poisoned(total, qr.PATCH)

    def label(code, records=inp.rec, labels=inp.labels, counters=inp.counters, capacity=inp.capacity, size=size, reach=1,
              patch=d_patch, pc=d_pc, offsets=(0, 0, 0)):
        rc = lib.emf_hip_planePatchLabel(ptr(records, offsets[0]), ptr(labels, offsets[1]), ptr(counters), capacity, i3(size),
                                         reach, ptr(patch, offsets[2]), ptr(pc), None)
        assert rc == code, (rc, lib.emf_hip_last_error_string())

    label(E_ARG, records=None)
    label(E_ARG, labels=None)
    label(E_ARG, counters=None)
    label(E_ARG, patch=None)
    label(E_ARG, pc=None)
    label(E_ARG, capacity=0)
    label(E_LIMIT, capacity=0x80000000)
    label(E_ARG, size=(0, 9, 9))
    label(E_LIMIT, size=(2049, 1, 1))
    label(E_ARG, reach=0)
    label(E_ARG, reach=-1)
    label(E_LIMIT, reach=3)
    label(E_ARG, offsets=(8, 0, 0))
    label(E_ARG, offsets=(0, 1, 0))
    label(E_ARG, offsets=(0, 0, 2))

    def patches(code, records=inp.rec, labels=inp.labels, patch=d_patch, counters=inp.counters, capacity=inp.capacity, size=size,
                axes=fp(axes), P=len(axes), min_count=1, n_patches=total, scratch=d_scratch, out=d_out, capacity_patches=total,
                pc=d_pc, offsets=(0, 0, 0)):
        rc = lib.emf_hip_planePatches(ptr(records), ptr(labels), ptr(patch, offsets[0]), ptr(counters), capacity, i3(size), axes, P,
                                      min_count, n_patches, ptr(scratch, offsets[1]), ptr(out, offsets[2]), capacity_patches,
                                      ptr(pc), None)
        assert rc == code, (rc, lib.emf_hip_last_error_string())

    patches(E_ARG, records=None)
    patches(E_ARG, labels=None)
    patches(E_ARG, patch=None)
    patches(E_ARG, counters=None)
    patches(E_ARG, axes=None)
    patches(E_ARG, scratch=None)
    patches(E_ARG, out=None)
    patches(E_ARG, pc=None)
    patches(E_ARG, capacity=0)
    patches(E_ARG, size=(33, -1, 9))
    patches(E_ARG, P=0)
    patches(E_LIMIT, P=65)
    patches(E_ARG, min_count=0)
    patches(E_ARG, min_count=-3)
    patches(E_ARG, capacity_patches=-1)
    patches(E_ARG, offsets=(2, 0, 0))
    patches(E_ARG, offsets=(0, 8, 0))
    patches(E_ARG, offsets=(0, 0, 4))
    assert lib.emf_hip_planePatchScratchBytes(0, 4) == 0 and lib.emf_hip_planePatchScratchBytes(0x80000000, 4) == 0
    dev.synchronize()
    for o in (d_patch, d_pc, d_scratch, d_out):
        assert is_poison(o.numpy()), "a refused call wrote something"
