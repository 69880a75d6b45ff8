"""CPU-side checks of the batched clean-up entries (emf_hip_maskAssociationMassBatched and its scratch query):
declared in include/emf_hip.h, exported by libemf_hip.so, typed in _lib.py, and bad arguments rejected before any
launch (no device is touched: every call below fails its argument checks)."""
import ctypes as C
import re
from pathlib import Path

from emfusion_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("emf_hip_maskAssociationMassScratchBytes", "emf_hip_maskAssociationMassBatched")
E_NULL, E_SHAPE, E_ARG = -1, -2, -4
FAKE = C.c_void_p(0x1000)  # never dereferenced: the calls fail before any launch


def test_entries_are_declared_exported_and_typed():
    header = (ROOT / "include" / "emf_hip.h").read_text()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES
        getattr(lib, name)
    # the ABI only grew: the version is the one of the level-1 entry's last change
    assert "#define EMF_HIP_ABI_VERSION 8" in header


def test_scratch_bytes():
    lib = _lib.load()
    one = lib.emf_hip_maskAssociationMassScratchBytes(1)
    assert one > 0 and lib.emf_hip_maskAssociationMassBytes() == one + 16  # level 1: the answer + the partials
    assert lib.emf_hip_maskAssociationMassScratchBytes(40) == 40 * one
    assert lib.emf_hip_maskAssociationMassScratchBytes(0) == one
    assert lib.emf_hip_maskAssociationMassScratchBytes(-1) == 0
    assert lib.emf_hip_maskAssociationMassScratchBytes(257) == 0


def test_bad_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    f = lib.emf_hip_maskAssociationMassBatched
    pos = (C.c_int32 * 2)(0, 5)
    ok = dict(models=FAKE, first=1, n=2, w=16, h=8, masks=None, scratch=FAKE, out=FAKE, verdict=None, nall=0,
              pos=None, vis=None, ex=None, thr=0.2, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["models"], a["first"], a["n"], a["w"], a["h"], a["masks"], a["scratch"], a["out"], a["verdict"],
                 a["nall"], a["pos"], a["vis"], a["ex"], a["thr"], a["stream"])

    assert call(first=-1) == E_ARG
    assert call(first=200, n=60) == E_ARG
    assert call(n=-1) == E_ARG
    assert call(w=0) == E_SHAPE
    assert call(models=None) == E_NULL
    assert call(scratch=None) == E_NULL
    assert call(out=None) == E_NULL
    assert call(verdict=FAKE, nall=1) == E_ARG               # fewer objects in the job than in the call
    assert call(verdict=FAKE, nall=300) == E_ARG
    assert call(verdict=FAKE, nall=5, pos=None, vis=FAKE) == E_NULL
    assert call(verdict=FAKE, nall=5, pos=pos, vis=None) == E_NULL
    assert call(verdict=FAKE, nall=4, pos=pos, vis=FAKE) == E_ARG  # position 5 of 4
    bad = (_lib.EmfImage * 2)()
    bad[1] = _lib.EmfImage(0x2000, 16, 16, 9)  # 16 x 9, not 16 x 8
    assert call(masks=bad) == E_SHAPE
