"""emf_hip_spillTiles / emf_hip_fillTiles (ops.spill_tiles / ops.fill_tiles; include/emf_hip.h "Storing and restoring
tiles") against the numpy restatement in tests/store_reference.py, compared as bytes: classes, words, literal
offsets, totals and every arena byte of a spill; the listed tiles, the untouched rest, a guard behind the arrays and
the written map entries of a fill; a roll out and back through spill and fill; and every refusal."""
import numpy as np
import pytest

from tests import store_reference as sr
from tests.parity_util import to_dev
from tests.test_gpu_volume_roll import contents as roll_contents
from tests.test_gpu_volume_roll import rebuilt_maps

pytestmark = pytest.mark.gpu

RES = [(64, 16, 16), (96, 24, 16)]  # 2 x 2 x 2 and 3 x 3 x 2 tiles


def contents(res, seed):
    """test_gpu_volume_roll's recipe -- a random-literal tile at (0, 0, 0), tsdf -1 under weight 0 at (0, 1, 0), all
    zero at (0, 0, 1), a scattering of -0.0 -- plus: all -0.0 at (1, 1, 0), weights all 64.0 over a literal tsdf at
    (1, 0, 1), one colour voxel repeated at (1, 1, 1).  The kinds are written after the scattering, so they hold."""
    tsdf, wts, color = roll_contents(res, seed)
    z0, z1, y0, y1, x0, x1 = slice(0, 8), slice(8, 16), slice(0, 8), slice(8, 16), slice(0, 32), slice(32, 64)
    tsdf[z0, y1, x0], wts[z0, y1, x0] = -1.0, 0.0
    tsdf[z1, y0, x0], wts[z1, y0, x0], color[z1, y0, x0] = 0.0, 0.0, 0
    tsdf[z0, y1, x1] = -0.0
    wts[z1, y0, x1] = 64.0
    color[z1, y1, x1] = (1, 2, 3, 0xfffe)
    return tsdf, wts, color


def boxes(res):
    nt = sr.tiles_of(res)
    return [((0, 0, 0), nt), ((nt[0] - 1, 0, 0), (1, nt[1], nt[2])), ((1, 1, 0), (1, 1, 1)), ((1, 0, 1), (0, nt[1], 1))]


CASES = [(res, color, b) for res in RES for color in (False, True) for b in range(4)]


def case_id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def volumes():
    """The host contents and the restated whole-volume spill per (res, with_color): computed once, never changed."""
    out = {}
    for res in RES:
        tsdf, wts, color = contents(res, 0x5707 + sum(res))
        for with_color in (False, True):
            c = color if with_color else None
            out[res, with_color] = (tsdf, wts, c, sr.spill(tsdf, wts, c, (0, 0, 0), sr.tiles_of(res)))
    return out


def test_the_contents_hold_every_tile_kind(volumes):
    classes, words, _, _, _ = volumes[(64, 16, 16), True][3]
    k = {(x, y, z): tuple(classes[(z * 2 + y) * 2 + x]) for z in range(2) for y in range(2) for x in range(2)}
    assert k[0, 0, 0] == (2, 2, 2)                                   # random literal
    assert k[0, 1, 0][:2] == (1, 0) and words[2][0] == 0xbf800000    # tsdf -1 under weight 0
    assert k[0, 0, 1] == (0, 0, 0)                                   # all zero
    assert k[1, 1, 0][0] == 1 and words[3][0] == 0x80000000          # all -0.0: class 1, not class 0
    assert k[1, 0, 1][:2] == (2, 1) and words[5][1] == 0x42800000    # weights all 64.0, tsdf literal
    assert k[1, 1, 1][2] == 1 and tuple(words[7][2:]) == (0x00020001, 0xfffe0003)  # one colour voxel repeated


@pytest.mark.parametrize("res,with_color,box", CASES, ids=case_id)
def test_spill_equals_the_restatement(dev, volumes, res, with_color, box):
    from emfusion_amd import ops
    tsdf, wts, color, _ = volumes[res, with_color]
    lo, size = boxes(res)[box]
    d_t, d_w = to_dev(tsdf), to_dev(wts)
    d_c = to_dev(color) if with_color else None
    want = sr.spill(tsdf, wts, color, lo, size)
    got = ops.spill_tiles(d_t, d_w, lo, size, color=d_c)
    again = ops.spill_tiles(d_t, d_w, lo, size, color=d_c)
    for g in (got, again):
        assert g["classes"].tobytes() == want[0].tobytes()
        assert g["words"].tobytes() == want[1].tobytes()
        assert g["lits"].tobytes() == want[2].tobytes()
        assert g["units"] == want[3]
        assert g["arena"].numpy()[:want[3]].tobytes() == want[4].tobytes()
    if box == 3:
        assert got["units"] == 0 and got["classes"].size == 0
    counted = ops.spill_tiles(d_t, d_w, lo, size, color=d_c, count_only=True)
    assert counted["arena"] is None and counted["units"] == want[3] and counted["lits"].tobytes() == want[2].tobytes()
    # the source is untouched
    assert d_t.numpy().view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes()
    assert d_w.numpy().view(np.uint32).tobytes() == wts.view(np.uint32).tobytes()
    if with_color:
        assert d_c.numpy().tobytes() == color.tobytes()


def poisoned(shape, dtype, guard):
    """A 0xFF-filled allocation whose front is a volume of `shape` and whose last `guard` bytes lie behind it."""
    from emfusion_amd.devmem import DeviceArray, DeviceView
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    whole = DeviceArray((n + guard,), np.uint8)
    whole.fill_bytes_(0xFF)
    return whole, DeviceView(whole.ptr, shape, dtype)


GUARD = 4096


@pytest.mark.parametrize("dst_color", [False, True], ids=["to-plain", "to-color"])
@pytest.mark.parametrize("res,with_color", [(r, c) for r in RES for c in (False, True)], ids=case_id)
def test_fill_writes_the_listed_tiles_and_nothing_else(dev, volumes, res, with_color, dst_color):
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    tsdf, wts, color, (classes, words, lits, units, arena) = volumes[res, with_color]
    nt = sr.tiles_of(res)
    every = [(x, y, z) for z in range(nt[2]) for y in range(nt[1]) for x in range(nt[0])]
    listed = [i for i in range(len(every)) if i % 5 != 1]  # every kind of the 2 x 2 x 2 corner but (1, 0, 0) and (0, 1, 1)
    coords = [every[i] for i in listed]
    shape = tsdf.shape
    w_t, d_t = poisoned(shape, np.float32, GUARD)
    w_w, d_w = poisoned(shape, np.float32, GUARD)
    w_c, d_c = poisoned(shape + (4,), np.uint16, GUARD) if dst_color else (None, None)
    tiles = nt[0] * nt[1] * nt[2]
    w_s, d_s = poisoned((2 * tiles,), np.uint8, GUARD)
    w_u, d_u = poisoned((tiles,), np.uint8, GUARD)
    d_arena = to_dev(arena) if units else None
    ops.fill_tiles(d_t, d_w, coords, classes[listed], words[listed], lits[listed], arena=d_arena, color=d_c, sign_maps=d_s,
                   unseen_tiles=d_u)
    got_t, got_w = d_t.numpy().view(np.uint32), d_w.numpy().view(np.uint32)
    got_c = d_c.numpy() if dst_color else None
    want_c = color if with_color else np.zeros(shape + (4,), np.uint16)  # a tile stored without colour gets zero colour
    for i, t in enumerate(every):
        sl = sr.tile_slices(t)
        if i in listed:
            assert got_t[sl].tobytes() == tsdf.view(np.uint32)[sl].tobytes(), t
            assert got_w[sl].tobytes() == wts.view(np.uint32)[sl].tobytes(), t
            if dst_color:
                assert got_c[sl].tobytes() == want_c[sl].tobytes(), t
        else:
            assert (got_t[sl] == 0xFFFFFFFF).all() and (got_w[sl] == 0xFFFFFFFF).all(), t
            if dst_color:
                assert (got_c[sl] == 0xFFFF).all(), t
    for whole, view in [(w_t, d_t), (w_w, d_w), (w_s, d_s), (w_u, d_u)] + ([(w_c, d_c)] if dst_color else []):
        assert (whole.numpy()[view.nbytes:] == 0xFF).all()  # the guard
    # the written entries are what the rebuild entries compute on a destination that was zeroed and then filled
    z_t, z_w = DeviceArray.zeros(shape, np.float32), DeviceArray.zeros(shape, np.float32)
    ops.fill_tiles(z_t, z_w, coords, classes[listed], words[listed], lits[listed], arena=d_arena)
    want_s, want_u = rebuilt_maps(ops, z_t, z_w, res)
    want_s, want_u, got_s, got_u = want_s.numpy(), want_u.numpy(), d_s.numpy(), d_u.numpy()
    host_s, host_u = sr.maps_of(z_t.numpy(), z_w.numpy())
    assert want_s.tobytes() == host_s.tobytes() and want_u.tobytes() == host_u.tobytes()
    for i in range(tiles):
        if i in listed:
            assert (got_s[i], got_s[tiles + i], got_u[i]) == (want_s[i], want_s[tiles + i], want_u[i]), every[i]
        else:
            assert (got_s[i], got_s[tiles + i], got_u[i]) == (0xFF, 0xFF, 0xFF), every[i]


@pytest.mark.parametrize("res,with_color", [(r, c) for r in RES for c in (False, True)], ids=case_id)
def test_roll_out_with_a_spill_and_back_with_a_fill_is_the_identity(dev, volumes, res, with_color):
    from emfusion_amd import ops
    tsdf, wts, color, _ = volumes[res, with_color]
    nt = sr.tiles_of(res)
    d_t, d_w = to_dev(tsdf), to_dev(wts)
    d_c = to_dev(color) if with_color else None
    sign, unseen = rebuilt_maps(ops, d_t, d_w, res)
    lo, size = sr.roll_boxes(nt, (1, 0, 0), False)[0]  # a roll by (32, 0, 0) moves the low-x slab out
    assert (lo, size) == ((0, 0, 0), (1, nt[1], nt[2]))
    s = ops.spill_tiles(d_t, d_w, lo, size, color=d_c)
    o_t, o_w, o_c, o_s, o_u = ops.roll_volume(d_t, d_w, (32, 0, 0), color=d_c, sign_maps=sign, unseen_tiles=unseen)
    b_t, b_w, b_c, b_s, b_u = ops.roll_volume(o_t, o_w, (-32, 0, 0), color=o_c, sign_maps=o_s, unseen_tiles=o_u)
    assert not b_t.numpy()[:, :, :32].view(np.uint32).any()  # the slab comes back as zeros ...
    coords = [(0, y, z) for z in range(nt[2]) for y in range(nt[1])]  # ... the entering box of the roll back
    assert sr.roll_boxes(nt, (-1, 0, 0), True) == [(lo, size)]
    ops.fill_tiles(b_t, b_w, coords, s["classes"], s["words"], s["lits"], arena=s["arena"], color=b_c, sign_maps=b_s, unseen_tiles=b_u)
    assert b_t.numpy().view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes()
    assert b_w.numpy().view(np.uint32).tobytes() == wts.view(np.uint32).tobytes()
    if with_color:
        assert b_c.numpy().tobytes() == color.tobytes()
    assert b_s.numpy().tobytes() == sign.numpy().tobytes() and b_u.numpy().tobytes() == unseen.numpy().tobytes()


def test_refusals(dev, volumes):
    from emfusion_amd import ops
    from emfusion_amd._lib import EmfHipError
    from emfusion_amd.devmem import DeviceArray, DeviceView
    res = (64, 16, 16)
    tsdf, wts, color, (classes, words, lits, units, arena) = volumes[res, True]
    d_t, d_w, d_c, d_a = to_dev(tsdf), to_dev(wts), to_dev(color), to_dev(arena)
    coords = [(x, y, z) for z in range(2) for y in range(2) for x in range(2)]
    tiles = 8
    sign, unseen = DeviceArray.zeros((2 * tiles,), np.uint8), DeviceArray.zeros((tiles,), np.uint8)

    def refused(code, call, *args, **kw):
        with pytest.raises(EmfHipError) as err:
            call(*args, **kw)
        assert err.value.code == code, err.value

    # spill: an arena below the box's worst case (EMF_E_LIMIT, before any launch); a box outside the volume
    refused(-5, ops.spill_tiles, d_t, d_w, (0, 0, 0), (2, 2, 2), color=d_c, arena_units=8 * 4 - 1)
    refused(-4, ops.spill_tiles, d_t, d_w, (1, 0, 0), (2, 1, 1))
    refused(-4, ops.spill_tiles, d_t, d_w, (0, 0, -1), (1, 1, 1))
    # fill: one map pointer only
    refused(-4, ops.fill_tiles, d_t, d_w, coords, classes, words, lits, arena=d_a, sign_maps=sign)
    refused(-4, ops.fill_tiles, d_t, d_w, coords, classes, words, lits, arena=d_a, unseen_tiles=unseen)
    # a resolution that is no tile multiple
    ragged = DeviceArray.zeros((16, 16, 40), np.float32)
    refused(-4, ops.fill_tiles, ragged, ragged, coords[:1], classes[:1], words[:1], lits[:1], arena=d_a)
    refused(-4, ops.spill_tiles, ragged, ragged, (0, 0, 0), (1, 1, 1))
    # a misaligned array
    off = DeviceView(d_t.ptr + 4, tsdf.shape, np.float32)  # (never dereferenced: the call is refused)
    refused(-4, ops.fill_tiles, off, d_w, coords, classes, words, lits, arena=d_a)
    refused(-4, ops.spill_tiles, off, d_w, (0, 0, 0), (1, 1, 1))
    # a class byte above 2
    bad = classes.copy()
    bad[3, 1] = 3
    refused(-4, ops.fill_tiles, d_t, d_w, coords, bad, words, lits, arena=d_a)
    # nothing was written by any of them
    assert d_t.numpy().view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes() and not sign.numpy().any()
    # a coordinate outside the volume and a literal outside the arena are skipped, the other tiles are written
    z_t, z_w = DeviceArray.zeros(tsdf.shape, np.float32), DeviceArray.zeros(tsdf.shape, np.float32)
    far = list(coords)
    far[0] = (2, 0, 0)
    ops.fill_tiles(z_t, z_w, far, classes, words, lits, arena=d_a, arena_units=units - 1)
    want_t, want_w = tsdf.copy(), wts.copy()
    want_t[sr.tile_slices((0, 0, 0))], want_w[sr.tile_slices((0, 0, 0))] = 0, 0  # the coordinate outside
    last = max(range(8), key=lambda i: int(lits[i].max()))  # the tile whose literal ends the arena
    want_t[sr.tile_slices(coords[last])], want_w[sr.tile_slices(coords[last])] = 0, 0
    assert z_t.numpy().view(np.uint32).tobytes() == want_t.view(np.uint32).tobytes()
    assert z_w.numpy().view(np.uint32).tobytes() == want_w.view(np.uint32).tobytes()
    # n == 0 launches nothing and is no error
    ops.fill_tiles(z_t, z_w, np.zeros((0, 3), np.int32), classes[:0], words[:0], lits[:0])
