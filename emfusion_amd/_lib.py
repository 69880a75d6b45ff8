"""ctypes binding of libemf_hip.so (the emf_hip_* C ABI declared in include/emf_hip.h).

Fails loudly when the library is missing or lacks a declared symbol -- there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
LIB_PATH = PKG_DIR / "libemf_hip.so"
HEADER_PATH = REPO_ROOT / "include" / "emf_hip.h"

EMF_OK = 0
EMF_E_NULL, EMF_E_SHAPE, EMF_E_PITCH, EMF_E_ARG, EMF_E_LIMIT = -1, -2, -3, -4, -5


class EmfImage(C.Structure):
    """Mirror of emf_image_t: device pointer + byte pitch + size."""

    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("width", C.c_int32),
                ("height", C.c_int32)]


MAX_PEERS = 8  # EMF_MAX_PEERS


class EmfPeer(C.Structure):
    """Mirror of emf_peer_t: what one rank of a direct peer-write exchange group knows about the group."""

    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("slots", C.c_void_p * MAX_PEERS),
                ("flags", C.c_void_p * MAX_PEERS), ("slotBytes", C.c_size_t), ("error", C.c_void_p),
                ("timeoutMs", C.c_uint32), ("waitInFront", C.c_uint32), ("systemFences", C.c_uint32)]


class EmfHipError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed with {code}: {msg}")
        self.code = code


_F9 = C.POINTER(C.c_float)
_I3 = C.POINTER(C.c_int32)
_IMG = C.POINTER(EmfImage)
_FP = C.c_void_p  # device float*/u8* passed as integers
_STREAM = C.c_void_p

# name -> argtypes; every entry returns int.  Must cover every function in include/emf_hip.h.
SIGNATURES = {
    "emf_hip_abi_version": [],
    "emf_hip_device_info": [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)],
    "emf_hip_computePoints": [_IMG, _IMG, _F9, _STREAM],
    "emf_hip_updateTSDF": [_IMG, _IMG, _FP, _FP, _FP, _F9, _F9, _F9, _I3, C.c_float, C.c_float,
                           C.c_float, _IMG, _STREAM],
    "emf_hip_computeInvLambda": [_F9, _IMG, _STREAM],
    "emf_hip_computeTSDFGrads": [_FP, _FP, _I3, _STREAM],
    "emf_hip_raycastTSDF": [_FP, _FP, _FP, _FP, _FP, _IMG, _IMG, _IMG, _IMG, _F9, _F9, _F9, _I3,
                            C.c_float, C.c_float, C.c_float, _FP, _STREAM],
    "emf_hip_getVolumeVals": [_FP, C.c_int, _IMG, _F9, _F9, _I3, C.c_float, _IMG, _STREAM],
    "emf_hip_updateFgBgProbs": [_IMG, _IMG, _FP, _FP, _FP, _F9, _F9, _F9, _I3, C.c_float, _STREAM],
    "emf_hip_computeFgProbs": [_FP, _FP, _FP, _I3, _STREAM],
    "emf_hip_maskRaycastWeights": [_FP, _FP, _FP, _I3, _STREAM],
    "emf_hip_computeAssociation": [_FP, _FP, _IMG, _F9, _F9, _I3, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_float, _IMG, _STREAM],
    "emf_hip_normalizeAssociation": [_IMG, C.c_int, C.c_int, _IMG, _IMG, _STREAM],
    "emf_hip_sumAssociation": [_IMG, C.c_int, _IMG, _STREAM],
    "emf_hip_compositeRaycast": [C.c_int, _I3, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG,
                                 _IMG, _IMG, _IMG, _IMG, _IMG, C.c_int, _FP, _STREAM],
    "emf_hip_compositeVisibility": [C.c_int, _I3, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG,
                                    _IMG, _IMG, _IMG, _IMG, _IMG, C.c_int, _FP, C.c_int, _FP, _FP, _STREAM],
    "emf_hip_occludedMask": [_IMG, _IMG, C.c_int, _IMG, _STREAM],
    "emf_hip_estepBatched": [_FP, _FP, C.c_int, _IMG, C.c_int, _IMG, _IMG, _STREAM],
    "emf_hip_estepBatchedFromDepth": [_FP, _FP, C.c_int, _IMG, _F9, _IMG, C.c_int, _IMG, _IMG, _STREAM],
    "emf_hip_raycastBatched": [_FP, _FP, _I3, C.c_int, C.c_int, C.c_int, _F9, C.c_int, C.c_int,
                               C.c_int, _FP, _FP, _FP, _STREAM],
    "emf_hip_renderView": [_FP, _FP, _I3, C.c_int, C.c_int, C.c_int, _F9, _F9, C.c_void_p, C.c_void_p, _IMG, _IMG,
                           _IMG, _IMG, _IMG, _FP, _STREAM],
    "emf_hip_normalizeAssociationTable": [_FP, C.c_int, C.c_int, C.c_int, _FP, _STREAM],
    "emf_hip_raycastBatchedLanes": [_FP, _FP, _I3, C.c_int, C.c_int, C.c_int, _F9, C.c_int, C.c_int,
                                    C.c_int, _FP, _FP, C.c_int, _FP, _STREAM],
    "emf_hip_raycastBatchedObjects": [_FP, _FP, _I3, C.c_int, C.c_int, C.c_int, _F9, C.c_int, _FP, _FP, _FP,
                                      _STREAM],
    "emf_hip_signMapBytes": [_I3],
    "emf_hip_rebuildSignMaps": [_FP, _I3, _FP, _STREAM],
    "emf_hip_unseenTileBytes": [_I3],
    "emf_hip_rebuildUnseenTiles": [_FP, _FP, _I3, _FP, _STREAM],
    "emf_hip_raycastFarBoundBytes": [C.c_int, C.c_int, C.c_int],
    "emf_hip_raycastFarBounds": [_FP, _FP, _I3, C.c_int, C.c_int, C.c_int, _F9, C.c_uint32, _FP, _STREAM],
    "emf_hip_relevantTileBytes": [_I3],
    "emf_hip_updateRelevantTiles": [_FP, _I3, C.c_int, _STREAM],
    "emf_hip_voxelReciprocal": [C.c_float, C.POINTER(C.c_float)],
    "emf_hip_voxelReciprocalCached": [C.c_float, C.POINTER(C.c_float)],
    "emf_hip_voxelReciprocalBegin": [C.c_float, C.c_void_p, _STREAM],
    "emf_hip_voxelReciprocalEnd": [C.c_float, C.c_ulonglong, C.POINTER(C.c_float)],
    "emf_hip_voxelReciprocalExhaustive": [C.c_float, C.POINTER(C.c_ulonglong)],
    "emf_hip_spinProbe": [C.c_void_p, C.c_uint32, _STREAM],
    "emf_hip_spinDelay": [C.c_uint32, _STREAM],
    "emf_hip_l1GatherProbe": [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, _STREAM],
    "emf_hip_peerBufferBytes": [C.c_int, C.c_size_t],
    "emf_hip_peerScatter": [C.c_void_p, _FP, C.c_size_t, C.c_size_t, C.c_uint32, _STREAM],
    "emf_hip_peerSignalWait": [C.c_void_p, C.c_uint32, C.c_uint32, _STREAM],
    "emf_hip_peerReduceSumF32": [C.c_void_p, C.c_uint32, C.c_size_t, _FP, _STREAM],
    "emf_hip_peerReduceMinU64": [C.c_void_p, C.c_uint32, C.c_size_t, _FP, _STREAM],
    "emf_hip_peerCopyFromSlot": [C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, _FP, C.c_size_t, _STREAM],
    "emf_hip_peerWaitReduceSumF32": [C.c_void_p, C.c_uint32, C.c_size_t, _FP, _STREAM],
    "emf_hip_peerWaitReduceMinU64": [C.c_void_p, C.c_uint32, C.c_size_t, _FP, _STREAM],
    "emf_hip_peerWaitCopyFromSlots": [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      _STREAM],
    "emf_hip_estepBatchedPeer": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, _STREAM],
    "emf_hip_peerNormalizeAssociation": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _STREAM],
    "emf_hip_peerRaycastSlotBytes": [C.c_int, C.c_int],
    "emf_hip_packHitKeysPeer": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                C.c_void_p, C.c_uint32, _STREAM],
    "emf_hip_compositeFromKeysPeer": [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
                                     + [C.c_void_p] * 13 + [C.c_int, C.c_void_p, _STREAM],
    "emf_hip_visibilityFlagsMirror": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _STREAM],
    "emf_hip_sweepFastPathPremises": [C.c_void_p, _STREAM],
    "emf_hip_debugPixelRounding": [_FP, _FP, C.c_int, _FP, _FP, _STREAM],
    "emf_hip_debugBandDecision": [_FP, _FP, _FP, C.c_int, C.c_float, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_streamCopy": [_FP, _FP, C.c_size_t, _STREAM],
    "emf_hip_preprocessDepth": [_IMG, _IMG, C.c_int, C.c_float, C.c_float, _STREAM],
    "emf_hip_pointStatsScratchBytes": [],
    "emf_hip_maskedPointStats": [_IMG, _IMG, _F9, _F9, _FP, _FP, _STREAM],
    "emf_hip_maskOverlap": [_IMG, _IMG, _FP, _STREAM],
    "emf_hip_maskAssociationMassBytes": [],
    "emf_hip_maskAssociationMass": [_IMG, _IMG, _IMG, _FP, _STREAM],
    "emf_hip_maskAssociationMassScratchBytes": [C.c_int],
    "emf_hip_maskAssociationMassBatched": [_FP, C.c_int, C.c_int, C.c_int, C.c_int, _IMG, _FP, _FP, _FP, C.c_int, _I3,
                                           _FP, C.POINTER(C.c_uint8), C.c_float, _STREAM],
    "emf_hip_carveMask": [_IMG, _IMG, C.c_int, _IMG, _FP, _STREAM],
    "emf_hip_objectExtentStats": [_IMG, _IMG, _F9, _F9, _FP, _FP, _FP, _I3, C.c_float, _FP, _FP, _STREAM],
    "emf_hip_copyValues": [_FP, _FP, C.c_int, _I3, _I3, _I3, _STREAM],
    "emf_hip_meshScratchBytes": [_I3],
    "emf_hip_hideLabel": [_IMG, C.c_int, _IMG, _IMG, _IMG, _IMG, _STREAM],
    "emf_hip_renderPhong": [_IMG, _IMG, _IMG, C.c_void_p, _F9, _IMG, _STREAM],
    "emf_hip_meshCount": [_FP, _FP, _FP, _I3, _FP, _FP, _STREAM],
    "emf_hip_meshEmit": [_FP, _FP, _FP, _FP, _I3, C.c_float, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshScratchBytesBatched": [_I3, C.c_int],
    "emf_hip_meshCountBatched": [_FP, _I3, C.c_int, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshEmitBatched": [_FP, _I3, C.c_int, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_trackScratchBytes": [C.c_int, C.c_int],
    "emf_hip_trackPrepare": [_FP, _FP, C.c_int, C.c_float, _STREAM],
    "emf_hip_trackIterate": [_FP, _FP, C.c_int, _IMG, C.c_void_p, _FP, C.c_size_t,
                             C.c_int, _STREAM],
    "emf_hip_trackStep": [_FP, _FP, C.c_int, _IMG, C.c_void_p, _FP, C.c_size_t,
                          C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, _STREAM],
    "emf_hip_trackWeightImages": [_FP, _FP, C.c_int, _IMG, C.c_void_p, _FP, C.c_size_t, _FP, _FP, _STREAM],
    "emf_hip_computePoseGradients": [_FP, _FP, _IMG, _F9, _F9, _I3, C.c_float, _FP, _STREAM],
    "emf_hip_integrateBatched": [_FP, _FP, _I3, C.c_int, _FP, _IMG, _IMG, _F9, C.c_int, _FP,
                                 _STREAM],
    "emf_hip_integrateCullScratchBytes": [_I3, C.c_int],
    "emf_hip_integrateBatchedCulled": [_FP, _FP, _I3, C.c_int, _FP, _IMG, _IMG, _F9, _FP, C.c_uint32, _FP, _FP,
                                       _STREAM],
    "emf_hip_integrateDirtyMapBytes": [_I3],
    "emf_hip_integrateBatchedCulledOut": [_FP, _FP, _I3, C.c_int, _FP, _IMG, _IMG, _F9, C.c_void_p, C.c_int, _FP,
                                          C.c_uint32, _FP, _FP, _STREAM],
    "emf_hip_integratePrepareOut": [C.c_void_p, _I3, C.c_int, _FP, _STREAM],
    "emf_hip_visibilityFlags": [_FP, C.c_int, C.c_int, _FP, _FP, _STREAM],
    "emf_hip_resetBrickFlags": [_FP, _I3, _STREAM],
    "emf_hip_packHitKeys": [C.c_int, _I3, _IMG, _IMG, _FP, C.c_int, C.c_int, _STREAM],
    "emf_hip_compositeFromKeys": [_FP, C.c_int, _I3, C.c_int, _I3, _IMG, _IMG, _IMG, _IMG, _IMG,
                                  _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, C.c_int, _FP,
                                  _STREAM],
    "emf_hip_visibilityFlagsIndexed": [_FP, C.c_int, _I3, C.c_int, _FP, _STREAM],
    "emf_hip_integrateColorBatched": [_FP, _FP, _FP, _I3, C.c_int, _FP, _IMG, _IMG, _IMG, _F9, _FP, _STREAM],
    "emf_hip_copyColorValues": [_FP, _FP, _I3, _I3, _I3, _STREAM],
    "emf_hip_sampleColor": [_FP, _FP, _FP, _I3, C.c_int, _IMG, _IMG, C.c_void_p, _IMG, _STREAM],
    "emf_hip_renderPhongColor": [_IMG, _IMG, _IMG, _F9, _IMG, _STREAM],
    "emf_hip_meshColors": [_FP, _FP, _FP, _FP, _I3, _FP, _FP, _STREAM],
    "emf_hip_meshColorsBatched": [_FP, _FP, _I3, C.c_int, _FP, _FP, _STREAM],
    "emf_hip_meshEdgeKeys": [_FP, _FP, _FP, _I3, _FP, _FP, _STREAM],
    "emf_hip_meshEdgeKeysBatched": [_FP, _I3, C.c_int, _FP, _FP, _STREAM],
    "emf_hip_meshWeldScratchBytes": [C.c_uint64],
    "emf_hip_meshWeldCount": [_FP, C.c_uint64, _FP, _FP, _STREAM],
    "emf_hip_meshWeldCountBatched": [_FP, C.c_uint64, _FP, C.c_int, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshWeldStatus": [_FP, C.c_uint64, _STREAM],
    "emf_hip_meshWeldEmit": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshWeldEmitBatched": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                    _FP, _STREAM],
    "emf_hip_meshComponentsScratchBytes": [C.c_uint64, C.c_uint64],
    "emf_hip_meshComponentsLabel": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshComponentsLabelBatched": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshComponentsFilterCount": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshComponentsFilterCountBatched": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _FP,
                                                 _FP, _FP, _FP, _STREAM],
    "emf_hip_meshComponentsStatus": [_FP, C.c_uint64, C.c_uint64, _STREAM],
    "emf_hip_meshComponentsEmit": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshComponentsEmitBatched": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP,
                                          _FP, _FP, _STREAM],
    "emf_hip_meshSimplifyScratchBytes": [C.c_uint64, C.c_uint64],
    "emf_hip_meshSimplifyCount": [_FP, _FP, _FP, _FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _FP,
                                  _FP, _FP, _STREAM],
    "emf_hip_meshSimplifyStatus": [_FP, C.c_uint64, C.c_uint64, _STREAM],
    "emf_hip_meshSimplifyEmit": [_FP, C.c_uint64, C.c_uint64, _FP, _FP, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                 _FP, _STREAM],
    "emf_hip_packScratchBytes": [C.c_uint64],
    "emf_hip_packClassify": [_FP, C.c_uint64, _FP, _FP, _STREAM],
    "emf_hip_packRank": [_FP, _FP, C.c_uint64, _FP, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_packGather": [_FP, C.c_uint64, _FP, C.c_uint32, C.c_uint32, _FP, _STREAM],
    "emf_hip_unpackFill": [_FP, C.c_uint64, _FP, _FP, _FP, C.c_uint32, _STREAM],
    "emf_hip_unpackLiterals": [_FP, C.c_uint64, _FP, C.c_uint32, C.c_uint32, _FP, _STREAM],
    "emf_hip_motionMasksScratchBytes": [C.c_int, C.c_int, C.c_int],
    "emf_hip_motionMasks": [_FP, _FP, C.c_int, C.c_int, C.c_void_p, _FP, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_rollVolumeIsTiled": [_I3, _I3],
    "emf_hip_rollVolume": [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _I3, _I3, _STREAM],
    "emf_hip_spillScratchBytes": [C.c_uint64],
    "emf_hip_spillTiles": [_FP, _FP, _FP, _I3, _I3, _I3, _FP, _FP, _FP, _FP, _FP, _FP, C.c_uint64, _STREAM],
    "emf_hip_fillTiles": [_FP, _FP, _FP, _FP, _FP, _I3, _FP, _FP, _FP, _FP, _FP, _FP, C.c_uint64, C.c_uint32, _STREAM],
    "emf_hip_meshTilesScratchBytes": [C.c_uint32],
    "emf_hip_meshTilesCount": [_FP, C.c_void_p, C.c_uint32, C.c_void_p, _FP, _FP, _STREAM],
    "emf_hip_meshTilesEmit": [_FP, C.c_uint32, C.c_void_p, _F9, C.c_float, _FP, _FP, _FP, _FP, _STREAM],
    "emf_hip_meshTilesColors": [_FP, C.c_uint32, C.c_void_p, _FP, _FP, _STREAM],
    "emf_hip_meshTilesEdgeKeys": [_FP, C.c_uint32, C.c_void_p, _FP, _FP, _STREAM],
    "emf_hip_occupancyClasses": [_FP, _FP, _I3, _I3, _I3, _FP, _STREAM],
    "emf_hip_occupancyObjectBox": [C.c_void_p, _I3, C.c_float],
    "emf_hip_occupancyTiles": [_FP, C.c_void_p, C.c_uint32, C.c_void_p, _I3, _I3, _FP, _STREAM],
    "emf_hip_occupancyStampObjects": [_FP, _I3, C.c_float, _I3, _I3, C.c_void_p, C.c_int32, _STREAM],
    "emf_hip_distanceTransform": [_FP, _I3, C.c_uint32, C.c_int32, _FP, _FP, C.c_float, _STREAM],
    "emf_hip_nearestSiteScratchBytes": [_I3],
    "emf_hip_distanceTransformNearest": [_FP, _I3, C.c_uint32, C.c_int32, _FP, _FP, _FP, _FP, C.c_float, _STREAM],
    "emf_hip_distanceQuery": [_FP, _FP, _FP, _I3, _FP, C.c_int32, _FP, _FP, _FP, _STREAM],
    "emf_hip_frontierLabel": [_FP, _I3, _FP, C.c_int32, _FP, _FP, _STREAM],
    "emf_hip_frontierScratchBytes": [_I3, C.c_uint32],
    "emf_hip_frontierClusters": [_FP, _I3, C.c_int32, C.c_uint32, _FP, _FP, C.c_int32, _FP, _STREAM],
    "emf_hip_planScratchBytes": [_I3],
    "emf_hip_planCost": [_FP, _I3, _FP, C.c_int32, C.c_uint32, _FP, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, _FP, _FP,
                         _FP, _STREAM],
    "emf_hip_planPaths": [_FP, _I3, _FP, C.c_int32, C.c_int32, _FP, _FP, _FP, _STREAM],
    "emf_hip_castVoxelRays": [_FP, _I3, _FP, C.c_int32, C.c_uint32, C.c_uint32, _FP, _FP, C.c_int32, _FP, C.c_int32, _FP,
                              _STREAM],
    "emf_hip_shapeMoments": [_FP, _I3, C.c_int32, C.c_int32, _FP, _STREAM],
    "emf_hip_shapeExtents": [_FP, _I3, C.c_int32, C.c_int32, _FP, _FP, _STREAM],
    "emf_hip_groundColumns": [_FP, _I3, None, _FP, _FP, _STREAM],  # [2]: EmfGroundFrame by value, set below its class
    "emf_hip_groundCells": [_FP, _FP, C.POINTER(C.c_int32), C.c_int32, C.c_int32, _FP, _STREAM],
    "emf_hip_groundClasses": [_FP, C.POINTER(C.c_int32), C.c_int32, _FP, _STREAM],
    "emf_hip_planeSurfaceScratchBytes": [_I3],
    "emf_hip_planeSurface": [_FP, _FP, _I3, _I3, _I3, _FP, _FP, C.c_uint32, _FP, _FP, _STREAM],
    "emf_hip_planeDirections": [_FP, _FP, C.c_uint32, C.c_int32, _FP, _STREAM],
    "emf_hip_planeOffsets": [_FP, _FP, C.c_uint32, _I3, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_float,
                             C.c_float, C.c_int32, _FP, _STREAM],
    "emf_hip_planeAssign": [_FP, _FP, C.c_uint32, _I3, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_float, _FP, _FP,
                            _STREAM],
    "emf_hip_planePatchLabel": [_FP, _FP, _FP, C.c_uint32, _I3, C.c_int32, _FP, _FP, _STREAM],
    "emf_hip_planePatchScratchBytes": [C.c_uint32, C.c_uint32],
    "emf_hip_planePatches": [_FP, _FP, _FP, _FP, C.c_uint32, _I3, C.POINTER(C.c_float), C.c_int32, C.c_int64, C.c_uint32, _FP,
                             _FP, C.c_int32, _FP, _STREAM],
    "emf_hip_contactProbe": [_FP, C.POINTER(C.c_int32), C.c_int32, _FP, C.c_void_p, C.c_int32, _FP, _STREAM],
    "emf_hip_absorbVolume": [_FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_float),
                             C.POINTER(C.c_float), _I3, _I3, _FP, _STREAM],
    "emf_hip_seedVolume": [_FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_float),
                           C.POINTER(C.c_float), _I3, _I3, _FP, _STREAM],
    "emf_hip_releaseVolume": [_FP, _FP, _I3, C.c_float, _FP, _I3, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), _I3,
                              _I3, _FP, _STREAM],
    # the colour variants: dst_color behind the destination's weights, src_color behind the source, the colour record
    # behind the record
    "emf_hip_absorbVolumeColor": [_FP, _FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, _FP, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), _I3, _I3, _FP, _FP, _STREAM],
    "emf_hip_seedVolumeColor": [_FP, _FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, _FP, C.POINTER(C.c_float),
                                C.POINTER(C.c_float), _I3, _I3, _FP, _FP, _STREAM],
    "emf_hip_releaseVolumeColor": [_FP, _FP, _FP, _I3, C.c_float, _FP, _I3, C.c_float, C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), _I3, _I3, _FP, _FP, _STREAM],
    # merging: dst_fgbg behind the destination's weights, src_fgbg behind the source, the count record behind the record;
    # with colour dst_color behind dst_fgbg, src_color behind src_fgbg and the colour record last
    "emf_hip_mergeVolume": [_FP, _FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, _FP, C.POINTER(C.c_float),
                            C.POINTER(C.c_float), _I3, _I3, _FP, _FP, _STREAM],
    "emf_hip_mergeVolumeColor": [_FP, _FP, _FP, _FP, _I3, C.c_float, C.c_float, C.c_float, C.c_void_p, _FP, _FP,
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), _I3, _I3, _FP, _FP, _FP, _STREAM],
}


class EmfVolumeOut(C.Structure):
    """Mirror of emf_volume_out_t (second copy of a double-buffered volume + its dirty maps)."""
    _fields_ = [("tsdf", C.c_void_p), ("weights", C.c_void_p), ("dirtyPrev", C.c_void_p), ("dirtyNext", C.c_void_p)]


class EmfModel(C.Structure):
    """Mirror of emf_model_t (device model table entry)."""

    _fields_ = [("tsdf", C.c_void_p), ("weights", C.c_void_p), ("grads", C.c_void_p),
                ("fgProbs", C.c_void_p), ("fgVolMask", C.c_void_p), ("brickFlags", C.c_void_p),
                ("assoc", C.c_void_p), ("raylengths", C.c_void_p), ("vertices", C.c_void_p),
                ("normals", C.c_void_p), ("hitMask", C.c_void_p), ("signMaps", C.c_void_p),
                ("relevantTiles", C.c_void_p), ("unseenTiles", C.c_void_p), ("res", C.c_int32 * 3),
                ("id", C.c_int32), ("voxelSize", C.c_float), ("truncdist", C.c_float),
                ("maxWeight", C.c_float), ("assocC1", C.c_float), ("assocC2", C.c_float),
                ("alpha", C.c_float), ("assocC3", C.c_float), ("reserved", C.c_int32),
                ("rcpVoxel", C.c_float), ("pad_", C.c_int32)]


class EmfMeshTile(C.Structure):
    """Mirror of emf_mesh_tile_t (include/emf_hip.h "Meshing a set of tiles"): 88 bytes."""

    _fields_ = [("coord", C.c_int32 * 3), ("cls", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("words", C.c_uint32 * 4),
                ("nbr", C.c_int32 * 7), ("reserved1", C.c_int32), ("at", C.c_uint64 * 3)]


class EmfMeshTilesSource(C.Structure):
    """Mirror of emf_mesh_tiles_source_t: the arena of the literals and the dense volume of the in-place tiles."""

    _fields_ = [("arena", C.c_void_p), ("arena_units", C.c_uint64), ("tsdf", C.c_void_p), ("weights", C.c_void_p),
                ("color", C.c_void_p), ("volume_elements", C.c_uint64), ("row_stride", C.c_uint64),
                ("plane_stride", C.c_uint64)]


class EmfShapeMoments(C.Structure):
    """Mirror of emf_shape_moments_t (include/emf_hip.h "Object shapes"): 128 bytes, integers only."""

    _fields_ = [("solid", C.c_uint64), ("observed", C.c_uint64), ("sum", C.c_uint64 * 3), ("sum2", C.c_uint64 * 6),
                ("faces_free", C.c_uint64), ("faces_unknown", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


class EmfShapeAxes(C.Structure):
    """Mirror of emf_shape_axes_t: three row vectors and a centre, f32, voxel coordinates (48 bytes)."""

    _fields_ = [("A", C.c_float * 9), ("c", C.c_float * 3)]


class EmfShapeExtents(C.Structure):
    """Mirror of emf_shape_extents_t: minimum and maximum along the three axes (24 bytes)."""

    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class EmfGroundFrame(C.Structure):
    """Mirror of emf_ground_frame_t (include/emf_hip.h "Ground map"): 60 bytes, passed by value."""

    _fields_ = [("G", C.c_float * 12), ("map", C.c_int32 * 2), ("bins", C.c_int32)]


SIGNATURES["emf_hip_groundColumns"][2] = EmfGroundFrame


class EmfOccObject(C.Structure):
    """Mirror of emf_occ_object_t (include/emf_hip.h "Distance field"): 112 bytes."""

    _fields_ = [("tsdf", C.c_void_p), ("weights", C.c_void_p), ("fgVolMask", C.c_void_p), ("res", C.c_int32 * 3),
                ("voxelSize", C.c_float), ("R", C.c_float * 9), ("t", C.c_float * 3), ("lo", C.c_int32 * 3),
                ("size", C.c_int32 * 3)]


class EmfAbsorbSource(C.Structure):
    """Mirror of emf_absorb_source_t (include/emf_hip.h "Absorbing a volume"): 56 bytes."""

    _fields_ = [("tsdf", C.c_void_p), ("weights", C.c_void_p), ("fgVolMask", C.c_void_p), ("unseenTiles", C.c_void_p),
                ("res", C.c_int32 * 3), ("voxelSize", C.c_float), ("truncdist", C.c_float), ("reserved", C.c_int32)]


OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = 0, 1, 2
DF_FAR = 0x7fffffff
DF_NONE = -1  # nearest site: none (exactly where d2 is DF_FAR)
DF_MAX_AXIS = 2048


class EmfFrontierCluster(C.Structure):
    """Mirror of emf_frontier_cluster_t (include/emf_hip.h "Frontiers"): 72 bytes."""

    _fields_ = [("label", C.c_int32), ("count", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("sum", C.c_uint64 * 3), ("rep", C.c_int32 * 3), ("reserved", C.c_int32)]


# the same record as a numpy structured dtype (what ops.frontier_clusters returns)
FRONTIER_CLUSTER_DTYPE = [("label", "<i4"), ("count", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum", "<u8", 3),
                          ("rep", "<i4", 3), ("reserved", "<i4")]
# include/emf_hip.h "Voxel rays": emf_ray_result_t (24 bytes) and emf_ray_group_t (32 bytes)
RAY_RESULT_DTYPE = [("stop", "<i4"), ("steps", "<i4"), ("counted", "<u4"), ("status", "<u4"), ("weighted", "<u8")]
RAY_GROUP_DTYPE = [("counted", "<u8"), ("weighted", "<u8"), ("reached", "<u4"), ("blocked", "<u4"), ("left", "<u4"),
                   ("invalid", "<u4")]
RAY_MAX_DELTA = 4095
# include/emf_hip.h "Object shapes": emf_shape_moments_t (128 bytes), emf_shape_axes_t (48), emf_shape_extents_t (24),
# emf_shape_frame_t (224) and emf_shape_box_t (584)
SHAPE_MOMENTS_DTYPE = [("solid", "<u8"), ("observed", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("faces_free", "<u8"),
                       ("faces_unknown", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)]
SHAPE_AXES_DTYPE = [("A", "<f4", 9), ("c", "<f4", 3)]
SHAPE_EXTENTS_DTYPE = [("lo", "<f4", 3), ("hi", "<f4", 3)]
SHAPE_FRAME_DTYPE = [("valid", "<i4"), ("reserved", "<i4"), ("centroid", "<f8", 3), ("covariance", "<f8", 6),
                     ("eigenvalues", "<f8", 3), ("axes", "<f8", 9), ("f32", SHAPE_AXES_DTYPE)]
SHAPE_BOX_DTYPE = [("center_vox", "<f8", 3), ("half_vox", "<f8", 3), ("completeness", "<f8"), ("center_obj", "<f8", 3),
                   ("half_m", "<f8", 3), ("corners_obj", "<f8", 24), ("center_world", "<f8", 3), ("axes_world", "<f8", 9),
                   ("corners_world", "<f8", 24)]
SHAPE_JACOBI_SWEEPS = 8
# include/emf_hip.h "Ground map": emf_ground_cell_t (8 bytes)
GROUND_CELL_DTYPE = [("floor", "<i2"), ("top", "<i2"), ("clear", "<i2"), ("levels", "<i2")]
GROUND_MAX_BINS = 256
# include/emf_hip.h "Planes": emf_plane_voxel_t (16 bytes) and emf_plane_moments_t (104)
PLANE_VOXEL_DTYPE = [("index", "<i4"), ("g", "<f4", 3)]
PLANE_MOMENTS_DTYPE = [("count", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("lo", "<i4", 3), ("hi", "<i4", 3)]
PLANE_MAX_K, PLANE_MAX_DIRS, PLANE_MAX_SLOTS, PLANE_MAX_PLANES = 31, 16, 4096, 64
PLANE_SURFACE, PLANE_NORMALS, PLANE_WRITTEN = 0, 1, 2  # the counters of emf_hip_planeSurface
# emf_plane_patch_t (128 bytes), the counters of emf_hip_planePatchLabel / emf_hip_planePatches
PLANE_PATCH_DTYPE = [("id", "<i4"), ("plane", "<i4"), ("count", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("lo", "<i4", 3),
                     ("hi", "<i4", 3), ("ulo", "<f4"), ("uhi", "<f4"), ("vlo", "<f4"), ("vhi", "<f4")]
PLANE_MAX_REACH = 2
PATCH_KEPT, PATCH_PATCHES, PATCH_MEMBERS = 0, 1, 2
# include/emf_hip.h "Object contacts": emf_contact_pair_t (64 bytes), emf_contact_t (144), emf_contact_side_t (68) and
# emf_contact_summary_t (264)
CONTACT_PAIR_DTYPE = [("a", "<i4"), ("b", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3), ("touch", "<f4"), ("reserved", "<i4")]
CONTACT_DTYPE = [("surface", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("sampled", "<u8"),
                 ("inside", "<u8"), ("touching", "<u8"), ("normals", "<u8"), ("sum", "<u8", 3), ("gsum", "<i8", 3),
                 ("lo", "<i4", 3), ("hi", "<i4", 3), ("min_s", "<f4"), ("reserved", "<i4")]
CONTACT_SIDE_DTYPE = [("res", "<i4", 3), ("voxel_size", "<f4"), ("truncdist", "<f4"), ("R", "<f4", 9), ("t", "<f4", 3)]
CONTACT_SUMMARY_DTYPE = [("state", "<i4"), ("saturated", "<i4"), ("direction", "<i4"), ("has_normal", "<i4"),
                         ("distance_m", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3), ("corners", "<f8", 24)]
CONTACT_MAX_PAIRS = 65535
# include/emf_hip.h "Absorbing a volume": emf_absorb_t (88 bytes); emf_absorb_source_t is EmfAbsorbSource below
ABSORB_DTYPE = [("visited", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("saturated", "<u8"),
                ("fused", "<u8"), ("fresh", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)]
# include/emf_hip.h "Lifting a volume": emf_seed_t (88 bytes) and emf_release_t (80)
SEED_DTYPE = [("visited", "<u8"), ("kept", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("saturated", "<u8"),
              ("seeded", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)]
RELEASE_DTYPE = [("visited", "<u8"), ("empty", "<u8"), ("free_space", "<u8"), ("outside", "<u8"), ("unclaimed", "<u8"),
                 ("released", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)]
# include/emf_hip.h "Absorbing a volume": emf_color_moved_t (16 bytes), the second record of the colour entries
COLOR_MOVED_DTYPE = [("colored", "<u8"), ("uncolored", "<u8")]
# include/emf_hip.h "Merging a volume": emf_merge_counts_t (16 bytes), the second record of the count pairs
MERGE_COUNTS_DTYPE = [("foreground", "<u8"), ("gained", "<u8")]
CONTACT_UNSEEN, CONTACT_APART, CONTACT_TOUCHING, CONTACT_PENETRATING = 0, 1, 2, 3
CONTACT_STATES = ("unseen", "apart", "touching", "penetrating")
RAY_REACHED, RAY_BLOCKED, RAY_LEFT, RAY_OUTSIDE, RAY_INVALID = 0, 1, 2, 3, 4
FRONTIER_KEPT, FRONTIER_CLUSTERS, FRONTIER_VOXELS = 0, 1, 2
# include/emf_hip.h "Planning"
PLAN_UNREACHED, PLAN_BLOCKED = 0xffffffff, 0xfffffffe
PLAN_CONVERGED, PLAN_ROUNDS, PLAN_FINITE, PLAN_SEEDS = 0, 1, 2, 3


class EmfPose(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3)]


class EmfTrackParams(C.Structure):
    """Mirror of emf_track_params_t (reference defaults, data.h:36-43)."""

    _fields_ = [("huberThresh", C.c_float), ("maxWeight", C.c_float), ("tau", C.c_float),
                ("eps1", C.c_float), ("eps2", C.c_float), ("nuInit", C.c_float)]

    @classmethod
    def defaults(cls):
        return cls(0.2, 64.0, 1e3, 1e-8, 1e-8, 2.0)


class EmfMotionParams(C.Structure):
    """Mirror of emf_motion_params_t (include/emf_hip.h "Motion masks")."""

    _fields_ = [("band", C.c_float), ("continuity", C.c_float), ("erode", C.c_int32), ("min_pixels", C.c_int32),
                ("max_masks", C.c_int32)]

    @classmethod
    def defaults(cls):
        return cls(0.08, 0.05, 1, 200, 8)


class EmfMotionInfo(C.Structure):
    """Mirror of emf_motion_info_t: one proposal."""

    _fields_ = [("label", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32)]


MOTION_MAX_MASKS = 16


class EmfTrackState(C.Structure):
    """Mirror of emf_track_state_t (device-resident Levenberg-Marquardt state of one model)."""

    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Rtrial", C.c_float * 9),
                ("ttrial", C.c_float * 3), ("A", C.c_float * 36), ("b", C.c_float * 6),
                ("x", C.c_float * 6), ("mu", C.c_float), ("nu", C.c_float), ("rho", C.c_float),
                ("err", C.c_float), ("errNew", C.c_float), ("maxIwBits", C.c_uint32),
                ("maxIwTrialBits", C.c_uint32),
                ("converged", C.c_int32), ("firstIteration", C.c_int32),
                ("evaluateGradient", C.c_int32), ("haveTrial", C.c_int32),
                ("iterations", C.c_int32), ("accepted", C.c_int32), ("iwSel", C.c_int32),
                ("wSel", C.c_int32), ("needAccum", C.c_int32), ("haveSpec", C.c_int32),
                ("spec", C.c_float * 28), ("checkB", C.c_int32),
                ("pending", C.c_int32), ("body", C.c_int32), ("iterTarget", C.c_int32),
                ("logCur", C.c_float), ("logTrial", C.c_float), ("wFac", C.c_float)]

_lib = None


def declared_symbols() -> list[str]:
    """Function names declared in include/emf_hip.h (what the library must export)."""
    text = HEADER_PATH.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(emf_hip_\w+)\s*\(", text)))


def load_variant(suffix: str) -> C.CDLL:
    """A second build of the kernel library beside the product's, e.g. "_fma" = libemf_hip_fma.so
    (`make -C csrc fma`: a*b+c contraction on).  For the tests that measure what contraction alone
    changes; nothing in the product loads it."""
    path = LIB_PATH.with_name(LIB_PATH.stem + suffix + LIB_PATH.suffix)
    if not path.exists():
        raise RuntimeError(f"{path} is missing: build it with `make -C {PKG_DIR / 'csrc'} fma`")
    return _bind(C.CDLL(os.fspath(path)))


def load() -> C.CDLL:
    """Load libemf_hip.so and bind every declared entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library has not been built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C {PKG_DIR / 'csrc'}`."
            " There is no CPU fallback.")
    _lib = _bind(C.CDLL(os.fspath(LIB_PATH)))
    return _lib


def _bind(lib: C.CDLL) -> C.CDLL:
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.emf_hip_trackScratchBytes.restype = C.c_size_t
    lib.emf_hip_unseenTileBytes.restype = C.c_size_t
    lib.emf_hip_pointStatsScratchBytes.restype = C.c_size_t
    lib.emf_hip_meshScratchBytes.restype = C.c_size_t
    lib.emf_hip_meshScratchBytesBatched.restype = C.c_size_t
    lib.emf_hip_meshWeldScratchBytes.restype = C.c_size_t
    lib.emf_hip_meshComponentsScratchBytes.restype = C.c_size_t
    lib.emf_hip_meshSimplifyScratchBytes.restype = C.c_size_t
    lib.emf_hip_packScratchBytes.restype = C.c_size_t
    lib.emf_hip_spillScratchBytes.restype = C.c_size_t
    lib.emf_hip_meshTilesScratchBytes.restype = C.c_size_t
    lib.emf_hip_motionMasksScratchBytes.restype = C.c_size_t
    lib.emf_hip_frontierScratchBytes.restype = C.c_size_t
    lib.emf_hip_nearestSiteScratchBytes.restype = C.c_size_t
    lib.emf_hip_planScratchBytes.restype = C.c_size_t
    lib.emf_hip_planeSurfaceScratchBytes.restype = C.c_size_t
    lib.emf_hip_planePatchScratchBytes.restype = C.c_size_t
    lib.emf_hip_integrateCullScratchBytes.restype = C.c_size_t
    lib.emf_hip_integrateDirtyMapBytes.restype = C.c_size_t
    lib.emf_hip_signMapBytes.restype = C.c_size_t
    lib.emf_hip_raycastFarBoundBytes.restype = C.c_size_t
    lib.emf_hip_relevantTileBytes.restype = C.c_size_t
    lib.emf_hip_peerBufferBytes.restype = C.c_size_t
    lib.emf_hip_peerRaycastSlotBytes.restype = C.c_size_t
    lib.emf_hip_maskAssociationMassBytes.restype = C.c_size_t
    lib.emf_hip_maskAssociationMassScratchBytes.restype = C.c_size_t
    lib.emf_hip_last_error_string.argtypes = []
    lib.emf_hip_last_error_string.restype = C.c_char_p
    return lib


def check(fn_name: str, rc: int) -> None:
    if rc != EMF_OK:
        msg = load().emf_hip_last_error_string().decode(errors="replace")
        raise EmfHipError(fn_name, rc, msg)
