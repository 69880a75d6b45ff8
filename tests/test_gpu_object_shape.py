"""emf_hip_shapeMoments and emf_hip_shapeExtents (include/emf_hip.h "Object shapes") against
tests/shape_reference.py, byte for byte: every shape x content of the restatement's fixtures with and without the
foreground mask, tables of one, two and EMF_MAX_BATCH + 1 models (the last with first > 0), a 128^3 volume whose sums
pass 2^32, and volumes with an unseen-tile map; outputs poisoned beforehand and untouched beyond n records; inputs only
read; a second run into the same buffers; every rejected argument."""
import ctypes as C

import numpy as np
import pytest

from tests import shape_reference as sr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3  # records of room behind the n a call writes
_expected = {}


def expected(shape, content, masked):
    """(tsdf, weights, fg or None, moments, [axes], [extents]) of the restatement, computed once and shared."""
    key = (shape, content, masked)
    if key not in _expected:
        tsdf, weights, fg = sr.volume(shape, content)
        fg = fg if masked else None
        mom = sr.moments(tsdf, weights, fg)
        axes = [sr.axes_for(mom, shape), sr.skew_axes(shape)]
        ext = [sr.extents(tsdf, weights, fg, a) for a in axes]
        for a in (tsdf, weights, mom) + ((fg,) if masked else ()):
            a.setflags(write=False)
        _expected[key] = (tsdf, weights, fg, mom, axes, ext)
    return _expected[key]


def poisoned(n, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray((n,), dtype).fill_bytes_(POISON)


def upload(case):
    tsdf, weights, fg = case[:3]
    return dict(tsdf=to_dev(tsdf), weights=to_dev(weights), fg_mask=to_dev(fg) if fg is not None else None)


def assert_inputs_unchanged(volumes, cases):
    for v, case in zip(volumes, cases):
        assert v["tsdf"].numpy().tobytes() == case[0].tobytes() and v["weights"].numpy().tobytes() == case[1].tobytes()
        assert case[2] is None or v["fg_mask"].numpy().tobytes() == case[2].tobytes()


def check_table(cases, first, what):
    """Moments and both extents of a table of cases at slots [first, first + n): poisoned outputs, a second run."""
    from emfusion_amd import ops
    n = len(cases)
    volumes = [upload(c) for c in cases]
    want_mom = np.array([c[3] for c in cases], sr.MOMENTS)
    d_mom = poisoned(n + EXTRA, sr.MOMENTS)
    for again in (False, True):
        assert ops.shape_moments(volumes, first=first, out=d_mom) is d_mom
        got = d_mom.numpy()
        assert got[:n].tobytes() == want_mom.tobytes(), (what, again, [(k, got[k], want_mom[k]) for k in range(n)
                                                                       if got[k] != want_mom[k]][:2])
        assert (got[n:].view(np.uint8) == POISON).all(), what  # untouched beyond n
    for which in (0, 1):
        frames = np.array([c[4][which] for c in cases], sr.AXES)
        want_ext = np.array([c[5][which] for c in cases], sr.EXTENTS)
        d_frames, d_ext = to_dev(frames), poisoned(n + EXTRA, sr.EXTENTS)
        for again in (False, True):
            assert ops.shape_extents(volumes, d_frames, first=first, out=d_ext) is d_ext
            got = d_ext.numpy()
            assert got[:n].tobytes() == want_ext.tobytes(), (what, which, again, got[:n][:3], want_ext[:3])
            assert (got[n:].view(np.uint8) == POISON).all(), what
        assert d_frames.numpy().tobytes() == frames.tobytes()
    assert_inputs_unchanged(volumes, cases)
    return volumes


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_model_is_exact(dev, shape, content):
    for masked in (True, False):
        check_table([expected(shape, content, masked)], 0, (shape, content, masked))


def test_the_plain_return_values(dev):
    from emfusion_amd import ops
    case = expected((33, 17, 9), "random", True)
    volumes = [upload(case)]
    mom = ops.shape_moments(volumes)
    assert mom.dtype == sr.MOMENTS and mom.shape == (1,) and mom[0].tobytes() == case[3].tobytes()
    ext = ops.shape_extents(volumes, np.array([case[4][0]], sr.AXES))
    assert ext.dtype == sr.EXTENTS and ext.shape == (1,) and ext[0].tobytes() == case[5][0].tobytes()


def test_two_models_of_different_shapes(dev):
    cases = [expected((33, 17, 9), "half_shell", False), expected((7, 9, 11), "gated_block", True)]
    check_table(cases, 0, "two models")
    check_table(cases[::-1], 1, "two models, swapped, first = 1")


def test_more_models_than_a_batch_with_first_above_zero(dev):
    """EMF_MAX_BATCH + 1 = 33 small models of mixed shapes and contents in one call at the slots 5 .. 37."""
    small = sr.SHAPES[:5] + [sr.SHAPES[5]]
    cases = [expected(small[k % len(small)], sr.CONTENTS[(k // 2) % len(sr.CONTENTS)], k % 3 != 0) for k in range(33)]
    assert len({c[0].shape for c in cases}) == len(small) and sum(int(c[3]["solid"]) > 0 for c in cases) > 16
    check_table(cases, 5, "33 models")
    check_table(cases, 256 - 33, "33 models at the end of the table")


def test_sums_beyond_32_bits(dev):
    """One 128^3 all-solid volume: sum xx = 1.13e10; the record is known in closed form."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    n = 128
    tsdf = DeviceArray((n, n, n), np.float32).fill_bytes_(0x80)  # -1.18e-38: not above 0
    weights = to_dev(np.ones((n, n, n), np.float32))
    mom = ops.shape_moments([dict(tsdf=tsdf, weights=weights)])[0]
    s1, s2 = sum(range(n)), sum(i * i for i in range(n))
    want = np.zeros((), sr.MOMENTS)
    want["solid"] = want["observed"] = n ** 3
    want["sum"], want["sum2"] = [s1 * n * n] * 3, [s2 * n * n] * 3 + [s1 * s1 * n] * 3
    want["lo"], want["hi"] = 0, n - 1
    assert mom.tobytes() == want.tobytes(), (mom, want)
    assert int(mom["sum2"][0]) == 11319377920 > 2 ** 32
    axes = sr.frame(want)["f32"]
    ext = ops.shape_extents([dict(tsdf=tsdf, weights=weights)], np.array([axes], sr.AXES))[0]
    assert ext["lo"].tolist() == [-63.5] * 3 and ext["hi"].tolist() == [63.5] * 3  # identity axes about the centre


@pytest.mark.parametrize("shape", [(64, 8, 8), (40, 24, 20), (33, 17, 9)], ids=lambda s: "x".join(str(v) for v in s))
def test_an_unseen_tile_map_changes_nothing(dev, shape):
    """A model with an unseen-tile map skips the workgroups of its unseen tiles: the same bytes as without the map."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    cases = [expected(shape, content, masked) for content in ("half_shell", "corner", "unobserved") for masked in (True, False)]
    volumes = [upload(c) for c in cases]
    skipped = 0
    for v in volumes:
        tiles = DeviceArray((ops.unseen_tile_bytes(shape),), np.uint8).fill_bytes_(POISON)
        ops.rebuild_unseen_tiles(v["tsdf"], v["weights"], tiles)
        v["unseen_tiles"] = tiles
        skipped += int((tiles.numpy() != 0).sum())
    assert skipped >= 2  # the "unobserved" volumes at the least
    mom = ops.shape_moments(volumes)
    assert mom.tobytes() == np.array([c[3] for c in cases], sr.MOMENTS).tobytes()
    for which in (0, 1):
        ext = ops.shape_extents(volumes, np.array([c[4][which] for c in cases], sr.AXES))
        assert ext.tobytes() == np.array([c[5][which] for c in cases], sr.EXTENTS).tobytes()


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    lib = _lib.load()
    p = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
    case = expected((5, 3, 2), "all_solid", False)
    volumes = [upload(case), upload(case)]
    table, res = ops.shape_table(volumes, first=0)
    mom, ext = poisoned(4, sr.MOMENTS), poisoned(4, sr.EXTENTS)
    frames = to_dev(np.array([case[4][0]] * 2, sr.AXES))

    def i3n(*v):
        return (C.c_int32 * len(v))(*v)

    def both(res=res, table=table, first=0, n=2, mom=mom, frames=frames, ext=ext):
        return (lib.emf_hip_shapeMoments(p(table), res, first, n, p(mom), None),
                lib.emf_hip_shapeExtents(p(table), res, first, n, p(frames), p(ext), None))

    for bad in (dict(table=None), dict(res=None), dict(n=0), dict(n=-1), dict(first=-1), dict(first=255), dict(first=256, n=1),
                dict(first=0, n=257), dict(first=2 ** 31 - 1, n=2), dict(res=i3n(5, 3, 2, 0, 3, 2)), dict(res=i3n(5, 3, 2, 5, -1, 2))):
        assert both(**bad) == (E_ARG, E_ARG), bad
    for bad in (dict(res=i3n(5, 3, 2, 2049, 1, 1)), dict(res=i3n(5, 3, 2049, 5, 3, 2)), dict(res=i3n(5, 3, 2, 2048, 2048, 512))):
        assert both(**bad) == (E_LIMIT, E_LIMIT), bad
    assert lib.emf_hip_shapeMoments(p(table), res, 0, 2, None, None) == E_ARG
    assert lib.emf_hip_shapeExtents(p(table), res, 0, 2, None, p(ext), None) == E_ARG
    assert lib.emf_hip_shapeExtents(p(table), res, 0, 2, p(frames), None, None) == E_ARG
    assert (mom.numpy().view(np.uint8) == POISON).all() and (ext.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert both() == (0, 0)
    got_mom, got_ext = mom.numpy(), ext.numpy()
    assert got_mom[0].tobytes() == got_mom[1].tobytes() == case[3].tobytes()
    assert got_ext[0].tobytes() == got_ext[1].tobytes() == case[5][0].tobytes()
    assert (got_mom[2:].view(np.uint8) == POISON).all() and (got_ext[2:].view(np.uint8) == POISON).all()
    with pytest.raises(Exception):
        ops.shape_moments(volumes, first=255)
    with pytest.raises(Exception):
        ops.shape_extents(volumes, np.zeros(1, sr.AXES))  # fewer frames than volumes
