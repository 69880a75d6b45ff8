"""emf_hip_contactProbe (include/emf_hip.h "Object contacts") against tests/contacts_reference.py, byte for
byte, in the default library and in the one built with a*b+c contraction on: probes and fields of the restatement's
shapes and contents with and without masks and unseen-tile maps; identity between equal lattices, fractional
translations, a rotation, sample points exactly on the field's first and last cells, everything outside, a NaN in the
pose; voxel-size ratios 1, 0.8 and 2; NaN and -0.0 tsdf, zero, negative and NaN weights at a cell's corner; every touch
value; pair lists of one pair, a shared probe, both directions and 33 pairs in an ungrouped order; outputs poisoned
beforehand and untouched beyond the records; a second call; every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import contacts_reference as cr
from tests import shape_reference as sr
from tests.parity_util import to_dev
from tests.resample_util import POISON, lib_for, upload_src

pytestmark = pytest.mark.gpu

f32 = np.float32
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3  # records of room behind the ones a call writes
SHAPES = [(1, 1, 1), (5, 3, 2), (33, 17, 9), (64, 8, 8), (40, 24, 20)]
CONTENTS = ["unobserved", "all_solid", "half_shell", "random", "gated_block"]
TOUCHES = (-1.0, -0.0, 0.0, 0.25, 1.0, np.inf)


def host_volume(shape, content, masked, voxel):
    tsdf, weights, fg = sr.volume(shape, content)
    return cr.vol(tsdf, weights, fg if masked else None, voxel)


def poisoned(n, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray((n,), dtype).fill_bytes_(POISON)


def upload(volumes, maps=False):
    return [upload_src(v, maps) for v in volumes]


def run(volumes, pairs, variants=("", "_fma"), maps=(False,), want=None):
    """The pair list over the volumes in every asked library, into poisoned records, twice; returns the expected records."""
    from emfusion_amd import ops
    pairs = np.array(pairs, cr.PAIR)
    want = cr.expected(volumes, pairs) if want is None else want
    cr.check_identities(want)
    n = len(pairs)
    for with_maps in maps:
        dev_volumes = upload(volumes, with_maps)
        for variant in variants:
            d_rec = poisoned(n + EXTRA, cr.CONTACT)
            for again in (False, True):
                assert ops.contact_probe(dev_volumes, pairs, out=d_rec, lib=lib_for(variant)) is d_rec
                got = d_rec.numpy()
                assert got[:n].tobytes() == want.tobytes(), (variant, with_maps, again, [(k, got[k], want[k]) for k in range(n)
                                                                                         if got[k] != want[k]][:2])
                assert (got[n:].view(np.uint8) == POISON).all(), "written beyond the records"
        for d, v in zip(dev_volumes, volumes):  # inputs are only read
            assert d["tsdf"].numpy().tobytes() == v["tsdf"].tobytes() and d["weights"].numpy().tobytes() == v["weights"].tobytes()
    return want


def poses(voxel_b):
    """Identity, two fractional translations, the 20 degree rotation, everything outside, a NaN in t."""
    return [(None, (0, 0, 0)), (None, (0.37 * voxel_b, -0.21 * voxel_b, 0.5 * voxel_b)), (None, (-1.5 * voxel_b, 2.25 * voxel_b, 0)),
            (cr.rot_z(20.0), (0.3 * voxel_b, 0, -voxel_b)), (None, (100.0, 0, 0)), (None, (0, np.nan, 0))]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_probe_against_three_fields(dev, shape, content):
    """The probe against a field of its own lattice, a finer one (ratio 0.8) and a coarser one (ratio 2), each under six
    poses, with and without masks, the touch values in turn; with and without the probe's unseen-tile map."""
    total = 0
    for masked in (True, False):
        volumes = [host_volume(shape, content, masked, 0.01),
                   host_volume(shape, "half_shell" if content in ("unobserved", "all_solid") else content, masked, 0.01),
                   host_volume((40, 24, 20), "random" if content == "random" else "half_shell", masked, 0.008),
                   host_volume((33, 17, 9), "gated_block", masked, 0.02)]
        pairs = []
        for b in (1, 2, 3):
            for k, (R, t) in enumerate(poses(float(volumes[b]["voxel_size"]))):
                pairs.append(cr.pair(0, b, R, t, TOUCHES[(k + b + len(content)) % 6]))
        want = run(volumes, pairs, maps=(False, True))
        total += int(want["surface"].sum())
    assert (total > 0) == (content in ("half_shell", "random", "gated_block") and shape != (1, 1, 1))


def test_equal_lattices_read_the_fields_own_bits_and_the_edge_cells(dev):
    """Voxel size 0.25 and whole-voxel shifts make q exact: q = v + shift.  s is then the field's tsdf at a voxel, bit for
    bit, and q is exactly 0, exactly N - 2 (the last inside cell) and exactly N - 1 (outside) for some surface voxels."""
    shape = (33, 17, 9)
    va = host_volume(shape, "gated_block", False, 0.25)
    rng = np.random.default_rng(5)
    other = rng.uniform(-1, 1, va["tsdf"].shape).astype(f32)
    vb = cr.vol(other, np.ones_like(other), None, 0.25)
    z, y, x = np.nonzero(cr.surface_mask(va["tsdf"], va["weights"]))
    pairs, hits = [], set()
    for shift in ((0, 0, 0), (-int(x.min()), 0, 0), (shape[0] - 2 - int(x.max()), 0, 0), (shape[0] - 1 - int(x.max()), 0, 0),
                  (0, -int(y.min()), shape[2] - 2 - int(z.max()))):
        pairs.append(cr.pair(0, 1, None, [0.25 * s for s in shift], np.inf))
        q = cr.sample_points((x, y, z), shape, va["voxel_size"], pairs[-1]["R"], pairs[-1]["t"], shape, vb["voxel_size"])
        for j in range(3):
            assert (q[j] == (x, y, z)[j] + shift[j]).all()
            hits |= {("first", j) for v in q[j] if v == 0} | {("last", j) for v in q[j] if v == shape[j] - 2}
            hits |= {("past", j) for v in q[j] if v == shape[j] - 1}
    assert {("first", 0), ("last", 0), ("past", 0), ("first", 1), ("last", 2)} <= hits
    want = run([va, vb], pairs)
    inner = (x < shape[0] - 1) & (y < shape[1] - 1) & (z < shape[2] - 1)
    assert want[0]["sampled"] == inner.sum() and want[0]["min_s"] == other[z[inner], y[inner], x[inner]].min()
    assert want[3]["outside"] > want[2]["outside"] > 0


def test_field_values_at_a_cells_corner(dev):
    """NaN and -0.0 tsdf and a zero, a negative and a NaN weight at single corners of cells that surface voxels sample."""
    shape = (33, 17, 9)
    va = host_volume(shape, "gated_block", False, 0.01)
    nz, ny, nx = va["tsdf"].shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    tsdf = np.clip((x - 14.3) / 6.0, -1, 1).astype(f32)  # a wall through the probe's block
    weights = np.ones_like(tsdf)
    sz, sy, sx = np.nonzero(cr.surface_mask(va["tsdf"], va["weights"]))
    pick = np.linspace(0, len(sx) - 1, 12).astype(int)
    for k, i in enumerate(pick):  # the voxel itself is corner (0, 0, 0) of the cell a shift below one voxel samples
        at = (sz[i], sy[i], sx[i])
        if k % 4 == 0:
            tsdf[at] = (np.nan, -0.0, 0.0)[k // 4]
        else:
            weights[at] = (0.0, -1.0, np.nan)[k % 4 - 1]
    vb = cr.vol(tsdf, weights, None, 0.01)
    pairs = [cr.pair(0, 1, None, (0.0031, 0.0047, 0.0013), touch) for touch in TOUCHES] + [cr.pair(0, 1, None, (0, 0, 0), 0.0)]
    want = run([va, vb], pairs)
    clean = cr.expected([va, cr.vol(np.clip((x - 14.3) / 6.0, -1, 1), np.ones_like(tsdf), None, 0.01)], pairs)
    assert (want["unknown"] > clean["unknown"]).all() and (want["sampled"] > 0).all()
    assert [int(v) for v in want["touching"][:6]] == sorted(int(v) for v in want["touching"][:6])  # touch ascends
    assert want["touching"][0] == 0 and want["touching"][5] == want["sampled"][5] and want["touching"][1] == want["touching"][2]


def test_pair_lists(dev):
    """One pair; two pairs that share a probe; both directions of a pair; a surface voxel on the volume's border."""
    a = host_volume((40, 24, 20), "half_shell", False, 0.01)
    b = host_volume((33, 17, 9), "gated_block", True, 0.0125)
    c = host_volume((64, 8, 8), "gated_block", False, 0.01)
    R, t = cr.rot_z(20.0), (0.02, -0.01, 0.005)
    Rb, tb = cr.contact_pose_np(np.eye(3, dtype=f32), np.zeros(3, f32), R, np.asarray(t, f32))  # the way back
    one = run([a, b], [cr.pair(0, 1, R, t, 0.25)])
    two = run([a, b, c], [cr.pair(0, 1, R, t, 0.25), cr.pair(0, 2, None, (0.1, 0, 0), np.inf)])
    both = run([a, b], [cr.pair(0, 1, R, t, 0.25), cr.pair(1, 0, Rb, tb, 0.25)], maps=(False, True))
    assert one[0].tobytes() == two[0].tobytes() == both[0].tobytes() and one[0]["sampled"] > 0 and both[1]["sampled"] > 0
    border = run([c, a], [cr.pair(0, 1, None, (0, 0, 0), np.inf)])[0]  # the block of c reaches its volume's far faces
    assert border["touching"] == border["sampled"] > border["normals"] > 0


def test_thirty_three_pairs_in_an_ungrouped_order(dev):
    """EMF_MAX_BATCH + 1 pairs over seven volumes, the probes interleaved: the kernel walks each probe's span of the list
    and skips the pairs of other probes.  Small fields cut through the tiles of the large probes."""
    shapes = [(33, 17, 9), (64, 8, 8), (40, 24, 20), (5, 3, 2), (33, 17, 9), (40, 24, 20), (64, 8, 8)]
    contents = ["gated_block", "half_shell", "gated_block", "gated_block", "random", "half_shell", "gated_block"]
    volumes = [host_volume(shapes[k], contents[k], k in (0, 5), (0.01, 0.008, 0.02)[k % 3]) for k in range(7)]
    ps = poses(0.01)
    pairs = []
    for k in range(33):
        a = (2, 4, 3, 1, 5, 6, 0)[k % 7]
        b = (a + 1 + k // 7) % 7
        R, t = ps[k % 4]
        pairs.append(cr.pair(a, b, R, t, TOUCHES[k % 6]))
    want = run(volumes, pairs, maps=(False, True))
    assert (want["sampled"] > 0).sum() > 8 and (want["touching"] > 0).sum() > 4 and (want["outside"] > 0).sum() > 8


def test_the_plain_return_value(dev):
    from emfusion_amd import ops
    volumes = [host_volume((33, 17, 9), "half_shell", True, 0.01), host_volume((40, 24, 20), "half_shell", False, 0.01)]
    pairs = [(0, 1, np.eye(3), (0.004, 0, 0), 0.25), (1, 0, np.eye(3), (-0.004, 0, 0), 0.25)]
    got = ops.contact_probe(upload(volumes), pairs)
    want = cr.expected(volumes, [cr.pair(*p) for p in pairs])
    assert got.dtype == cr.CONTACT == ops.CONTACT_DTYPE and got.shape == (2,) and got.tobytes() == want.tobytes()
    assert cr.PAIR == ops.CONTACT_PAIR_DTYPE


def test_the_refusals(dev):
    from emfusion_amd import ops
    lib = lib_for("")
    p = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
    volumes = [host_volume((5, 3, 2), "gated_block", False, 0.01), host_volume((5, 3, 2), "half_shell", False, 0.01)]
    dev_volumes = upload(volumes)  # alive to the end: the table holds their addresses
    table, res = ops.contact_table(dev_volumes)
    good = np.array([cr.pair(0, 1, None, (0, 0, 0), 0.25), cr.pair(1, 0, None, (0, 0, 0), 0.25)], cr.PAIR)
    d_pairs, rec = to_dev(good), poisoned(2 + EXTRA, cr.CONTACT)

    def i3n(*v):
        return (C.c_int32 * len(v))(*v)

    def call(table=table, res=res, n_models=2, pairs=d_pairs, host=good, n_pairs=2, rec=rec, offsets=(0, 0)):
        host_ptr = None if host is None else C.c_void_p(host.ctypes.data)
        dp = None if pairs is None else C.c_void_p(pairs.ptr + offsets[0])
        dr = None if rec is None else C.c_void_p(rec.ptr + offsets[1])
        return lib.emf_hip_contactProbe(p(table), res, n_models, dp, host_ptr, n_pairs, dr, None)

    def named(a, b):
        bad = good.copy()
        bad[1]["a"], bad[1]["b"] = a, b
        return bad

    for bad in (dict(table=None), dict(res=None), dict(pairs=None), dict(host=None), dict(rec=None), dict(n_pairs=0), dict(n_pairs=-1),
                dict(n_models=0), dict(n_models=257), dict(host=named(1, 1)), dict(host=named(2, 0)), dict(host=named(0, -1)),
                dict(host=named(0, 2)), dict(n_models=1), dict(res=i3n(5, 3, 2, 0, 3, 2)), dict(res=i3n(5, -1, 2, 5, 3, 2)),
                dict(offsets=(2, 0)), dict(offsets=(0, 4))):
        assert call(**bad) == E_ARG, bad
    for bad in (dict(n_pairs=65536), dict(res=i3n(5, 3, 2, 2049, 1, 1)), dict(res=i3n(5, 3, 2049, 5, 3, 2)),
                dict(res=i3n(2048, 2048, 512, 5, 3, 2))):
        assert call(**bad) == E_LIMIT, bad
    ring = np.array([cr.pair(k, (k + 1) % 17) for k in range(17)], cr.PAIR)  # 17 probes of 2^20 tiles each: above 2^24 - 1
    assert call(res=i3n(*[2048, 2048, 511] * 17), n_models=17, host=ring, n_pairs=17) == E_LIMIT
    dev.synchronize()
    assert (rec.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert call() == 0
    got = rec.numpy()
    assert got[:2].tobytes() == cr.expected(volumes, good).tobytes() and (got[2:].view(np.uint8) == POISON).all()
    with pytest.raises(Exception):
        ops.contact_probe(upload(volumes), [(0, 0, np.eye(3), (0, 0, 0), 0.0)])
