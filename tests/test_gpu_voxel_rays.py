"""emf_hip_castVoxelRays (include/emf_hip.h "Voxel rays") against tests/rays_reference.py, byte for
byte: every shape x content x ray count x group of the restatement's fixtures, with and without a d2 gate and for two
mask pairs; outputs poisoned beforehand and untouched beyond n and n_groups; inputs only read; a second run into the
same buffers; every rejected argument."""
import ctypes as C

import numpy as np
import pytest

from tests import plan_reference as pl
from tests import rays_reference as rr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
MASKS = [(1, 1), (5, 4)]  # (pass_mask, count_mask): free space counting itself; through unknown space counting it
MIN_D2 = 1
_expected = {}


def expected(shape, content, gate, masks):
    """(classes, d2 or None, from, to, records of the whole list) of the restatement, computed once and shared."""
    key = (shape, content, gate, masks)
    if key not in _expected:
        classes = rr.class_field(shape, content)
        d2 = pl.d2_field(shape) if gate else None
        f, t = rr.ray_list(shape, classes, pass_mask=masks[0])
        rec = rr.cast(classes, f, t, d2, MIN_D2 if gate else 0, *masks)
        for a in (classes, f, t, rec) + ((d2,) if gate else ()):
            a.setflags(write=False)
        _expected[key] = (classes, d2, f, t, rec)
    return _expected[key]


def poisoned(n, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray((n,), dtype).fill_bytes_(POISON)


def run(d_classes, d_from, d_to, n, d_d2, gate, masks, group, out=None, extra=(5, 3)):
    """One call on the first n rays into poisoned buffers with `extra` records of room: (results, groups) as numpy."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceView
    n_groups = -(-n // group) if group else 0
    if out is None:
        out = (poisoned(n + extra[0], rr.RESULT), poisoned(n_groups + extra[1], rr.GROUP) if group else None)
    got = ops.cast_voxel_rays(d_classes, DeviceView(d_from.ptr, (n, 3), np.int32), DeviceView(d_to.ptr, (n, 3), np.int32),
                              d2=d_d2, min_d2=MIN_D2 if gate else 0, pass_mask=masks[0], count_mask=masks[1], group=group, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return out


def assert_records(out, want, n, group, what):
    res = out[0].numpy()
    assert res[:n].tobytes() == want[:n].tobytes(), (what, np.flatnonzero(res[:n] != want[:n])[:4].tolist())
    assert (res[n:].view(np.uint8) == POISON).all(), what  # untouched beyond n
    if group:
        groups, want_groups = out[1].numpy(), rr.group_records(want[:n], group)
        k = len(want_groups)
        assert groups[:k].tobytes() == want_groups.tobytes(), (what, groups[:k][:3], want_groups[:3])
        assert (groups[k:].view(np.uint8) == POISON).all(), what


@pytest.mark.parametrize("content", rr.CONTENTS)
@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_rays_are_exact(dev, shape, content):
    from emfusion_amd.devmem import DeviceArray
    for gate in (False, True):
        for masks in MASKS:
            classes, d2, f, t, want = expected(shape, content, gate, masks)
            assert len(f) >= max(rr.COUNTS)
            d_classes, d_d2 = to_dev(classes), to_dev(d2) if gate else None
            d_from, d_to = DeviceArray.from_numpy(f.reshape(-1)), DeviceArray.from_numpy(t.reshape(-1))
            for n in rr.COUNTS + [len(f)]:
                for group in [0] + rr.GROUPS:
                    what = (shape, content, gate, masks, n, group)
                    out = run(d_classes, d_from, d_to, n, d_d2, gate, masks, group)
                    assert_records(out, want, n, group, what)
                    if (n, group) in ((65, 3), (len(f), 100)):  # a second run into the same buffers: the same bytes
                        run(d_classes, d_from, d_to, n, d_d2, gate, masks, group, out=out)
                        assert_records(out, want, n, group, what + ("again",))
            # inputs only read
            assert d_classes.numpy().tobytes() == classes.tobytes() and d_from.numpy().tobytes() == f.tobytes()
            assert d_to.numpy().tobytes() == t.tobytes() and (d2 is None or d_d2.numpy().tobytes() == d2.tobytes())


def test_only_the_groups_and_numpy_ends(dev):
    """results = NULL with groups: the same group records; rays given as numpy lists; the plain return values."""
    from emfusion_amd import ops
    shape, masks = (9, 17, 65), (5, 4)
    classes, _, f, t, want = expected(shape, "sparse", False, masks)
    d_classes = to_dev(classes)
    groups = poisoned(-(-len(f) // 64) + 2, rr.GROUP)
    got = ops.cast_voxel_rays(d_classes, f, t, pass_mask=5, count_mask=4, group=64, out=(None, groups))
    assert got[0] is None
    host, want_groups = groups.numpy(), rr.group_records(want, 64)
    assert host[:len(want_groups)].tobytes() == want_groups.tobytes() and (host[len(want_groups):].view(np.uint8) == POISON).all()
    res, grp = ops.cast_voxel_rays(d_classes, f, t, pass_mask=5, count_mask=4, group=64)
    assert res.dtype == rr.RESULT and grp.dtype == rr.GROUP and res.tobytes() == want.tobytes() and grp.tobytes() == want_groups.tobytes()
    res = ops.cast_voxel_rays(d_classes, f[:7], t[:7], pass_mask=5, count_mask=4)
    assert res.tobytes() == want[:7].tobytes()
    assert len(ops.cast_voxel_rays(d_classes, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))) == 0
    # pass_mask 0: every ray that takes a step is blocked at its first voxel or leaves there
    res = ops.cast_voxel_rays(d_classes, f, t, pass_mask=0, count_mask=7)
    assert res.tobytes() == rr.cast(classes, f, t, pass_mask=0, count_mask=7).tobytes() and res["steps"].max() == 0


def test_a_group_of_full_rows_sums_beyond_32_bits(dev):
    shape = (1, 2, 2048)
    classes, _, f, t, want = expected(shape, "all_free", False, (1, 1))
    d_classes = to_dev(classes)
    from emfusion_amd import ops
    res, grp = ops.cast_voxel_rays(d_classes, f[:65], t[:65], pass_mask=1, count_mask=1, group=64)
    assert res.tobytes() == want[:65].tobytes() and grp.tobytes() == rr.group_records(want[:65], 64).tobytes()
    assert res["weighted"][0] == res["weighted"][1] == 2047 * 2048 * 4095 // 6 and int(grp["weighted"][0]) > 2 ** 32


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    from emfusion_amd.devmem import DeviceArray
    lib = _lib.load()
    i3 = lambda *v: (C.c_int32 * 3)(*v)  # noqa: E731
    p = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
    shape, n = (3, 5, 2), 4
    classes = to_dev(rr.class_field(shape, "all_free"))
    ends = DeviceArray.from_numpy(np.zeros(3 * n, np.int32))
    results, groups = poisoned(n, rr.RESULT), poisoned(n, rr.GROUP)
    d2 = DeviceArray.from_numpy(np.zeros(shape, np.int32))

    def rc(size=None, classes=classes, d2=None, pass_mask=1, count_mask=0, src=ends, dst=ends, n=n, results=results, group=0,
           groups=None):
        return lib.emf_hip_castVoxelRays(p(classes), size if size is not None else i3(2, 5, 3), p(d2), 1, pass_mask, count_mask,
                                         p(src), p(dst), n, p(results), group, p(groups), None)

    # the limits of the distance field, from the sizes alone
    for size, code in ((i3(0, 4, 4), E_ARG), (i3(4, -1, 4), E_ARG), (i3(2049, 1, 1), E_LIMIT), (i3(4, 4, 2049), E_LIMIT),
                       (i3(2048, 2048, 512), E_LIMIT), (i3(2048, 2048, 2048), E_LIMIT)):
        assert rc(size=size) == code, list(size)
    assert lib.emf_hip_castVoxelRays(p(classes), None, None, 0, 1, 0, p(ends), p(ends), n, p(results), 0, None, None) == E_ARG
    for bad in (dict(classes=None), dict(src=None), dict(dst=None), dict(pass_mask=8), dict(count_mask=8), dict(count_mask=0xffffffff),
                dict(n=-1), dict(group=-1), dict(results=None), dict(results=None, group=2), dict(group=2), dict(groups=groups),
                dict(group=-3, groups=groups)):
        assert rc(**bad) == E_ARG, bad
    assert (results.numpy().view(np.uint8) == POISON).all() and (groups.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert rc(n=0) == 0 and rc(n=0, group=2, groups=groups) == 0  # n == 0 enqueues nothing
    assert (results.numpy().view(np.uint8) == POISON).all() and (groups.numpy().view(np.uint8) == POISON).all()
    assert rc(d2=d2, group=3, groups=groups) == 0
    res, grp = results.numpy(), groups.numpy()
    assert (res["status"] == rr.REACHED).all() and (res["steps"] == 0).all() and (res["stop"] == rr.NONE).all()
    assert grp["reached"][:2].tolist() == [3, 1] and (grp[2:].view(np.uint8) == POISON).all()
    with pytest.raises(Exception):
        ops.cast_voxel_rays(classes, np.zeros((2, 3), np.int32), np.zeros((3, 3), np.int32))
    with pytest.raises(Exception):
        ops.cast_voxel_rays(classes, np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32), pass_mask=9)
