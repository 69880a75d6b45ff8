"""emf_hip_rollVolume (ops.roll_volume; include/emf_hip.h "Rolling a volume") against numpy slicing, compared as
uint32 / uint16 so that -0.0 and every other bit pattern counts; the moved sign / unseen maps against the two rebuild
entries run on the result; and Fusion.roll_background on a live session: shifted volumes, the resize pose formula bit
for bit, and a next frame whose out-of-place integration equals the in-place one."""
import os

import numpy as np
import pytest

from tests import roll_reference as rr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

TILED_RES = (64, 16, 16)  # 2 x 2 x 2 tiles
TILED = [(32, 0, 0), (-32, 8, -8), (0, 0, 8), (64, 0, 0), (0, 0, 0)]
GENERAL_RES = (40, 12, 10)
GENERAL = [(3, -5, 2), (4, 0, 0)]


def contents(res, seed):
    """tsdf random in [-1, 1] with a few -0.0; where the volume has whole tiles: one all positive, one all negative, one
    with weight 0 but tsdf -1 (unseen, negative sign only), one all zero (unseen, no sign)."""
    nx, ny, nz = res
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    wts = np.where(rng.random((nz, ny, nx)) < 0.3, 0.0, rng.uniform(0.5, 64.0, (nz, ny, nx))).astype(np.float32)
    color = rng.integers(0, 65536, (nz, ny, nx, 4), dtype=np.uint16)
    if nx >= 64 and ny >= 16 and nz >= 16:
        tsdf[0:8, 0:8, 0:32] = np.abs(tsdf[0:8, 0:8, 0:32]) + np.float32(0.01)
        tsdf[0:8, 0:8, 32:64] = -np.abs(tsdf[0:8, 0:8, 32:64]) - np.float32(0.01)
        tsdf[0:8, 8:16, 0:32], wts[0:8, 8:16, 0:32] = -1.0, 0.0
        tsdf[8:16, 0:8, 0:32], wts[8:16, 0:8, 0:32], color[8:16, 0:8, 0:32] = 0.0, 0.0, 0
    for _ in range(7):
        z, y, x = (int(rng.integers(0, n)) for n in (nz, ny, nx))
        tsdf[z, y, x] = -0.0
    tsdf[-1, -1, -1] = -0.0
    assert np.signbit(tsdf[tsdf == 0]).any()
    return tsdf, wts, color


def rebuilt_maps(ops, tsdf_dev, wts_dev, res):
    from emfusion_amd.devmem import DeviceArray
    sign = DeviceArray.zeros((ops.sign_map_bytes(res),), np.uint8)
    unseen = DeviceArray.zeros((ops.unseen_tile_bytes(res),), np.uint8)
    ops.rebuild_sign_maps(tsdf_dev, sign)
    ops.rebuild_unseen_tiles(tsdf_dev, wts_dev, unseen)
    return sign, unseen


@pytest.mark.parametrize("with_color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("res,shift", [(TILED_RES, s) for s in TILED] + [(GENERAL_RES, s) for s in GENERAL],
                         ids=lambda v: "x".join(str(i) for i in v))
def test_roll_equals_numpy_slicing_bit_for_bit(dev, res, shift, with_color):
    from emfusion_amd import ops
    tsdf, wts, color = contents(res, 0x5011 + sum(res))
    d_t, d_w = to_dev(tsdf), to_dev(wts)
    d_c = to_dev(color) if with_color else None
    tiled = res == TILED_RES
    sign = unseen = None
    if tiled:
        sign, unseen = rebuilt_maps(ops, d_t, d_w, res)
        s, u = sign.numpy(), unseen.numpy()
        # the contents do hold the tile kinds the maps distinguish
        assert (s[0], s[8 + 0]) == (1, 0) and (s[1], s[8 + 1]) == (0, 1) and (s[2], s[8 + 2], u[2]) == (0, 1, 1)
        assert (s[4], s[8 + 4], u[4]) == (0, 0, 1) and u[0] == 0
    o_t, o_w, o_c, o_sign, o_unseen = ops.roll_volume(d_t, d_w, shift, color=d_c, sign_maps=sign, unseen_tiles=unseen)
    got_t, got_w = o_t.numpy(), o_w.numpy()
    assert got_t.view(np.uint32).tobytes() == rr.rolled(tsdf, shift).view(np.uint32).tobytes()
    assert got_w.view(np.uint32).tobytes() == rr.rolled(wts, shift).view(np.uint32).tobytes()
    if with_color:
        assert o_c.numpy().tobytes() == rr.rolled(color, shift).tobytes()
    else:
        assert o_c is None
    if shift == (64, 0, 0):
        assert not got_t.view(np.uint32).any() and not got_w.view(np.uint32).any()
    # the sources are untouched
    assert d_t.numpy().view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes() and np.array_equal(d_w.numpy(), wts)
    if tiled:  # the moved maps are what the rebuild entries compute from the result
        want_sign, want_unseen = rebuilt_maps(ops, o_t, o_w, res)
        assert o_sign.numpy().tobytes() == want_sign.numpy().tobytes()
        assert o_unseen.numpy().tobytes() == want_unseen.numpy().tobytes()
        if shift == (64, 0, 0):
            assert not o_sign.numpy().any() and o_unseen.numpy().all()
    else:
        assert o_sign is None and o_unseen is None


def test_tile_multiple_shift_on_a_ragged_volume_takes_the_general_path(dev):
    from emfusion_amd import ops
    res, shift = (40, 16, 16), (32, 8, 8)  # x is no multiple of 32
    tsdf, wts, _ = contents(res, 7)
    o_t, o_w, _, o_sign, _ = ops.roll_volume(to_dev(tsdf), to_dev(wts), shift)
    assert o_sign is None
    assert o_t.numpy().view(np.uint32).tobytes() == rr.rolled(tsdf, shift).view(np.uint32).tobytes()
    assert o_w.numpy().view(np.uint32).tobytes() == rr.rolled(wts, shift).view(np.uint32).tobytes()


def test_refusals(dev):
    from emfusion_amd import ops
    from emfusion_amd._lib import EmfHipError
    tsdf, wts, color = contents(TILED_RES, 1)
    d_t, d_w = to_dev(tsdf), to_dev(wts)
    with pytest.raises(EmfHipError) as err:  # in place
        ops.roll_volume(d_t, d_w, (32, 0, 0), out=(d_t, to_dev(wts)))
    assert err.value.code == -4
    with pytest.raises(EmfHipError):  # the two destinations are one array
        d_o = to_dev(wts)
        ops.roll_volume(d_t, d_w, (1, 0, 0), out=(d_o, d_o))
    assert np.array_equal(d_t.numpy().view(np.uint32), tsdf.view(np.uint32))


# ---- in a session ------------------------------------------------------------------------------------------------

def session(env, shifts):
    """Three frames, then for each shift: roll, check, one more frame.  Returns the volumes after every step.  `env`
    holds for the whole session: some switches are read again whenever a volume is described."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return run_session(shifts)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run_session(shifts):
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    fus = pipeline.Fusion(rr.params())
    keep, out, f = [], [], 0

    def frame():
        nonlocal f
        d = to_dev(rr.render(f))
        keep.append(d)
        fus.process_frame(image_view(d), rr.EYE, rr.camera_t(f), {}, {}, False)
        fus.synchronize()
        f += 1

    for _ in range(3):
        frame()
    origin = np.zeros(3, np.int64)
    for shift in shifts:
        before = fus.volume("tsdf", 0), fus.volume("weights", 0)
        assert (before[1] > 0).sum() > 1000
        R0, t0 = fus.background_pose()
        fus.roll_background(shift)
        after = fus.volume("tsdf", 0), fus.volume("weights", 0)
        assert after[0].view(np.uint32).tobytes() == rr.rolled(before[0], shift).view(np.uint32).tobytes()
        assert after[1].view(np.uint32).tobytes() == rr.rolled(before[1], shift).view(np.uint32).tobytes()
        R1, t1 = fus.background_pose()
        assert R1.tobytes() == R0.tobytes() and t1.tobytes() == rr.rolled_pose_t(R0, t0, shift, rr.VOX).tobytes()
        origin += shift
        assert fus.background_origin() == tuple(int(v) for v in origin)
        out.append(after)
        frame()
        out.append((fus.volume("tsdf", 0), fus.volume("weights", 0)))
        out.append((fus.image("bg_raylengths"), fus.image("bg_assoc")))
    fus.close()
    return out


SHIFTS = [(32, 8, -8), (3, -5, 2)]  # the tile-granular path, then the general one


@pytest.fixture(scope="module")
def overlapped(dev):
    return session({}, SHIFTS)  # background kept twice, integrated out of place, every accelerator on


def test_roll_background_in_a_session_and_the_next_frame_on_both_paths(dev, overlapped):
    shifts = SHIFTS
    in_place = session({"EMF_BG_OVERLAP": "0"}, shifts)  # one copy, the reference's sequence
    assert len(overlapped) == len(in_place) == 6
    for k, (a, b) in enumerate(zip(overlapped, in_place)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), k
    # the frame after a roll did integrate into the rolled volume and did hit it
    assert overlapped[1][1].sum() > overlapped[0][1].sum() and (overlapped[2][0] > 0).sum() > rr.W * rr.H // 8


def test_the_maps_a_roll_moved_serve_the_next_frame_like_no_maps_at_all(dev, overlapped):
    """TSDF::roll moves the sign and unseen-tile maps with the tiles (first shift) and leaves them to a rebuild (second
    shift).  Wrong entries would show in the frame that follows: a seen tile called unseen is integrated as a first
    sample, a tile that lost its sign drops out of the relevant-tile list and the far bounds stop rays in front of it.
    A session that uses neither the unseen maps nor the far bounds cannot see the maps, and the accelerators never
    change a byte: volumes, ray lengths and association weights must be equal after every step."""
    blind = session({"EMF_UNSEEN_TILES": "0", "EMF_FAR_BOUNDS": "0"}, SHIFTS)
    assert len(blind) == len(overlapped) == 6
    for k, (a, b) in enumerate(zip(overlapped, blind)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), k
    assert (overlapped[2][0] > 0).sum() > rr.W * rr.H // 8  # the rays of the frame after the tile-granular roll do hit
