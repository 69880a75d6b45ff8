"""CPU-side checks of the table-wide meshing entries: exported, typed, and bad arguments rejected before any
launch (no device is touched: every call below fails its argument checks)."""
import ctypes as C

from emfusion_amd import _lib

E_NULL, E_SHAPE, E_LIMIT = -1, -2, -5
FAKE = C.c_void_p(0x1000)  # never dereferenced: the calls fail before any launch


def _res(*vols):
    flat = [v for r in vols for v in r]
    return (C.c_int32 * max(len(flat), 3))(*flat)


def test_batched_mesh_entries_are_exported_and_typed():
    lib = _lib.load()
    for name in ("emf_hip_meshScratchBytesBatched", "emf_hip_meshCountBatched", "emf_hip_meshEmitBatched"):
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES
        getattr(lib, name)


def test_scratch_bytes_of_a_table():
    lib = _lib.load()
    one = _res((64, 48, 40))
    assert lib.emf_hip_meshScratchBytesBatched(one, 1) == lib.emf_hip_meshScratchBytes(one) > 0
    two = _res((64, 48, 40), (512, 512, 512))
    assert lib.emf_hip_meshScratchBytesBatched(two, 2) > lib.emf_hip_meshScratchBytes(_res((512, 512, 512)))
    assert lib.emf_hip_meshScratchBytesBatched(two, 0) == 0
    assert lib.emf_hip_meshScratchBytesBatched(_res((64, 1, 40)), 1) == 0
    assert lib.emf_hip_meshScratchBytesBatched(None, 1) == 0
    assert lib.emf_hip_meshScratchBytesBatched(_res(*[(8, 8, 8)] * 257), 257) == 0


def test_bad_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    res = _res((8, 8, 8), (8, 8, 8))
    assert lib.emf_hip_meshCountBatched(None, res, 2, FAKE, FAKE, None, None) == E_NULL
    assert b"models" in lib.emf_hip_last_error_string()
    assert lib.emf_hip_meshCountBatched(FAKE, None, 2, FAKE, FAKE, None, None) == E_NULL
    assert lib.emf_hip_meshCountBatched(FAKE, res, 0, FAKE, FAKE, None, None) == E_LIMIT
    assert lib.emf_hip_meshCountBatched(FAKE, res, -3, FAKE, FAKE, None, None) == E_LIMIT
    many = _res(*[(8, 8, 8)] * 257)
    assert lib.emf_hip_meshCountBatched(FAKE, many, 257, FAKE, FAKE, None, None) == E_LIMIT
    assert lib.emf_hip_meshCountBatched(FAKE, _res((8, 8, 8), (8, 1, 8)), 2, FAKE, FAKE, None, None) == E_SHAPE
    assert lib.emf_hip_meshCountBatched(FAKE, res, 2, None, FAKE, None, None) == E_NULL
    assert lib.emf_hip_meshCountBatched(FAKE, res, 2, FAKE, None, None, None) == E_NULL
    assert lib.emf_hip_meshEmitBatched(None, res, 2, FAKE, FAKE, FAKE, FAKE, None) == E_NULL
    assert lib.emf_hip_meshEmitBatched(FAKE, res, 257, FAKE, FAKE, FAKE, FAKE, None) == E_LIMIT
    assert lib.emf_hip_meshEmitBatched(FAKE, _res((0, 8, 8), (8, 8, 8)), 2, FAKE, FAKE, FAKE, FAKE, None) == E_SHAPE
    for k in range(3):
        outs = [FAKE, FAKE, FAKE]
        outs[k] = None
        assert lib.emf_hip_meshEmitBatched(FAKE, res, 2, FAKE, *outs, None) == E_NULL
