"""The background store without a device: the numpy restatement that the GPU tests compare against is
itself checked -- spill then fill into a zeroed volume is the identity on volumes that hold every tile kind, and the
restated store evicts whole spills, the oldest first."""
import numpy as np
import pytest

from tests import roll_reference as rr
from tests import store_reference as sr


def volume(res, seed, with_color):
    """Random literals, with per tile kind one tile: all zero, all -0.0, tsdf -1 under weight 0, weights all 64.0, one
    colour voxel repeated."""
    nx, ny, nz = res
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    wts = rng.uniform(0.0, 64.0, (nz, ny, nx)).astype(np.float32)
    color = rng.integers(0, 65536, (nz, ny, nx, 4), dtype=np.uint16) if with_color else None
    t = sr.tile_slices
    tsdf[t((0, 0, 1))], wts[t((0, 0, 1))] = 0.0, 0.0
    tsdf[t((1, 1, 0))] = -0.0
    tsdf[t((0, 1, 0))], wts[t((0, 1, 0))] = -1.0, 0.0
    wts[t((1, 0, 1))] = 64.0
    if with_color:
        color[t((0, 0, 1))] = 0
        color[t((1, 1, 1))] = (1, 2, 3, 4)
    return tsdf, wts, color


@pytest.mark.parametrize("with_color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("res", [(64, 16, 16), (96, 24, 16)], ids=lambda r: "x".join(map(str, r)))
def test_spill_then_fill_into_zeros_is_the_identity(res, with_color):
    tsdf, wts, color = volume(res, 11 + sum(res), with_color)
    nt = sr.tiles_of(res)
    classes, words, lits, units, arena = sr.spill(tsdf, wts, color, (0, 0, 0), nt)
    kinds = {tuple(c) for c in classes}
    assert (0, 0, 0) in kinds and any(c[0] == 1 for c in kinds) and any(c[:2] == (2, 1) for c in kinds)
    assert classes[(0 * nt[1] + 1) * nt[0] + 1][0] == 1 and words[(0 * nt[1] + 1) * nt[0] + 1][0] == 0x80000000  # -0.0: class 1
    assert arena.shape == (units, sr.UNIT) and units == sum(sr.units_of(c) for c in classes)
    coords = [(x, y, z) for z in range(nt[2]) for y in range(nt[1]) for x in range(nt[0])]
    out_t, out_w = np.zeros_like(tsdf), np.zeros_like(wts)
    out_c = None if color is None else np.zeros_like(color)
    sr.fill(out_t, out_w, out_c, coords, classes, words, lits, arena)
    assert out_t.view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes()
    assert out_w.view(np.uint32).tobytes() == wts.view(np.uint32).tobytes()
    if with_color:
        assert out_c.tobytes() == color.tobytes()
    sign, unseen = sr.maps_of(tsdf, wts)
    n = nt[0] * nt[1] * nt[2]
    zero, minus = (1 * nt[1] + 0) * nt[0] + 0, (0 * nt[1] + 1) * nt[0] + 0
    assert (sign[zero], sign[n + zero], unseen[zero]) == (0, 0, 1) and (sign[minus], sign[n + minus], unseen[minus]) == (0, 1, 1)


def test_a_roll_out_and_back_through_the_restated_store_is_the_identity():
    res = (64, 16, 16)
    tsdf, wts, color = volume(res, 5, True)
    store = sr.DictStore()
    a = sr.roll_with_store(store, tsdf, wts, color, (0, 0, 0), (32, 8, -8))
    assert a[0].tobytes() == rr.rolled(tsdf, (32, 8, -8)).tobytes()  # nothing to restore yet
    held = store.info()
    assert held["tiles_spilled"] == held["tiles_held"] == 7 - 1  # 7 of 8 tiles leave, the all-zero one is not stored
    b = sr.roll_with_store(store, a[0], a[1], a[2], (32, 8, -8), (-32, -8, 8))
    assert b[0].view(np.uint32).tobytes() == tsdf.view(np.uint32).tobytes()
    assert b[1].view(np.uint32).tobytes() == wts.view(np.uint32).tobytes() and b[2].tobytes() == color.tobytes()
    info = store.info()
    # what left on the way back had entered as zeros: nothing is held, and nothing that belongs inside the volume
    assert info["tiles_restored"] == 6 and info["tiles_held"] == 0 and info["tiles_spilled"] == 6


def test_the_restated_store_evicts_whole_spills_oldest_first():
    lit = np.zeros(2 * sr.UNIT, np.uint8)
    cost = sr.RECORD_BYTES + lit.size
    store = sr.DictStore(budget=3 * cost)
    for spill, keys in enumerate([[(0, 0, 0), (1, 0, 0)], [(2, 0, 0)], [(3, 0, 0), (4, 0, 0)]]):
        store.begin_spill()
        for k in keys:
            store.insert(k, (2, 2, 0), (1, 2, 0, 0), lit)
        store.insert((9, 9, spill), (0, 0, 0), (0, 0, 0, 0), lit[:0])  # all zero: never stored
        store.end_spill()
        if spill < 2:
            assert store.info()["tiles_evicted"] == 0
    # five tiles exceed three: the first spill goes as a whole (two tiles), then it fits
    assert list(store.tiles) == [(2, 0, 0), (3, 0, 0), (4, 0, 0)]
    assert store.info() == dict(tiles_held=3, bytes_held=3 * cost, tiles_spilled=5, tiles_restored=0, tiles_evicted=2)
    assert store.take((0, 0, 0)) is None and store.take((3, 0, 0)) is not None
    # a spill larger than the budget on its own drops everything, itself included
    store.begin_spill()
    for x in range(10, 14):
        store.insert((x, 0, 0), (2, 2, 0), (1, 2, 0, 0), lit)
    store.end_spill()
    assert not store.tiles and store.info()["tiles_evicted"] == 2 + 2 + 4


# ---- checkpoint version 3, without a device ------------------------------------------------------------------------

def v3_file(tile=None, roll=True, version=3, tile_at=-1):
    from tests import checkpoint_format as CF
    from tests.test_checkpoint_roll_section_cpu import roll_payload
    from tests.test_pack_reference_cpu import BG, assembled
    parts, _ = assembled()
    parts[0] = CF.header(CF.params_block(bg_res=BG, bg_voxel=0.08, obj_res=(8, 8, 8)), version=version)
    if roll:
        parts.insert(len(parts) - 1, CF.section(b"ROLL", 0, 0, roll_payload()))
    if tile is not None:
        parts.insert(len(parts) + tile_at, CF.section(b"TILE", 0, 0, tile))
    return b"".join(parts)


def refused(tmp_path, data):
    from emfusion_amd import pipeline
    path = tmp_path / "bad.ckpt"
    path.write_bytes(data)
    with pytest.raises(pipeline.FusionError) as e:
        pipeline.checkpoint_info(path)
    assert e.value.code == -4  # EMF_E_ARG
    return str(e.value)


def test_checkpoint_info_reports_the_stored_tiles_of_a_version_3_file(tmp_path):
    from emfusion_amd import pipeline
    store = sr.small_store()
    path = tmp_path / "stored.ckpt"
    path.write_bytes(v3_file(sr.tile_payload(store)))
    d = pipeline.checkpoint_info(path)
    assert d["version"] == 3 and d["stored_tiles"] == 3 and d["stored_bytes"] == store.bytes_held == 3 * 40 + 5 * sr.UNIT
    assert d["background_origin"] == [32, 8, -8] and d["retired_slabs"] == 1 and d["file_bytes"] == path.stat().st_size
    # an empty store is a valid version 3 file
    path.write_bytes(v3_file(sr.tile_payload(sr.DictStore(budget=123))))
    d = pipeline.checkpoint_info(path)
    assert d["version"] == 3 and d["stored_tiles"] == 0 and d["stored_bytes"] == 0


def test_damaged_and_misplaced_tile_sections_are_refused(tmp_path):
    store = sr.small_store()
    good = v3_file(sr.tile_payload(store))
    assert "truncated" in refused(tmp_path, good[:-40])                       # the file ends inside the section
    assert "truncated" in refused(tmp_path, good[:len(good) // 2])
    payload = sr.tile_payload(store)
    assert "counts disagree" in refused(tmp_path, v3_file(payload + bytes(8)))      # an over-long section
    assert "shorter than its contents" in refused(tmp_path, v3_file(payload[:-sr.UNIT]))  # a literal cut short
    more = bytearray(payload)
    more[64:72] = (4).to_bytes(8, "little")                                   # claims a tile more than it holds
    assert "counts disagree" in refused(tmp_path, v3_file(bytes(more)))
    huge = bytearray(payload)
    huge[64:72] = (1 << 60).to_bytes(8, "little")
    huge[16:24] = (1 << 60).to_bytes(8, "little")
    assert "counts disagree" in refused(tmp_path, v3_file(bytes(huge)))
    bad = bytearray(payload)
    bad[72 + 20] = 3                                                          # the first tile's tsdf class
    assert "unknown class" in refused(tmp_path, v3_file(bytes(bad)))
    assert "format version 3 without its tile section" in refused(tmp_path, v3_file())
    assert "format version 3 without its roll section" in refused(tmp_path, v3_file(roll=False))
    assert "tile section out of place" in refused(tmp_path, v3_file(payload, version=2))
    assert "tile section out of place" in refused(tmp_path, v3_file(payload, tile_at=-2))   # in front of the roll section
    assert "tile section out of place" in refused(tmp_path, v3_file(payload, roll=False))
    two = v3_file(payload)
    from tests import checkpoint_format as CF
    tile = CF.section(b"TILE", 0, 0, payload)
    assert "tile section out of place" in refused(tmp_path, two[:-len(CF.END)] + tile + CF.END)
