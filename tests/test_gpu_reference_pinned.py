"""The HIP kernels against committed outputs of the REFERENCE'S OWN kernels
(tests/golden/reference_v1.npz, recorded from the reference's device code built for the host) --
directly, with no oracle in between the kernel and the verdict.

The cases are the edges of tests/reference_cases.py: non-finite, negative and zero depth, NaN
association weights, voxels that project exactly onto half pixels, sdf == +-truncdist, weights
that sum to zero, the weight cap, odd and even volume sizes; rays with a zero direction component,
a camera inside the volume, one looking away from it, incoming raylengths, a zero gradient at the
hit; lookups on the last admissible cell; mask bytes 1 and 255.

The integrate cases go through EVERY integrate entry the product uses -- emf_hip_updateTSDF (1 / lambda
inline and from the table, pitched images), emf_hip_integrateBatched, and for the volumes made of
whole tiles emf_hip_integrateBatchedCulled and ...CulledOut with the unseen-tile map in use --
over three frames, each frame compared.  The tile shortcuts of those launches reason about depth
ranges, which is exactly where a NaN or an infinity in a tile's pixels gets forgotten.  The raycast
cases go through emf_hip_raycastTSDF (checked reciprocal and division, with and without a gradient
volume) and emf_hip_raycastBatched.

Reads only tests/golden/.  These are data cases, not stress: each runs once.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import reference_cases as rc
from tests.parity_util import assert_parity, dev_full, to_dev, to_np

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "reference_v1.npz"
SIGMA, ALPHA, PRIOR = 0.02, 0.8, 1.0
INTEGRATE = [n for n, c in rc.CASES.items() if c.kind == "integrate"]
TILED = [n for n in INTEGRATE if n.endswith("_64")]  # whole 32 x 8 x 8 tiles: the culled launches take them
RAYCAST = [n for n, c in rc.CASES.items() if c.kind == "raycast"]


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gold():
    data = dict(np.load(GOLD))
    return json.loads(str(data.pop("digests"))), data


def inputs_of(gold, name):
    inp = rc.CASES[name].inputs()
    assert {k: rc.digest(v) for k, v in inp.items()} == gold[0][name]["inputs"], "the inputs drifted"
    return inp


def expect(gold, name, key, got, what):
    """got == the reference's recorded output: array for array where the whole array is recorded,
    digest for digest otherwise (a mask is compared as zero / non-zero)."""
    digests, arrays = gold
    got = np.asarray(got)
    if key == "mask":
        got = (got != 0).astype(np.uint8)
    if f"{name}/{key}" in arrays:
        assert_parity(got, arrays[f"{name}/{key}"], f"{name} {key} ({what})", exact=True)
    assert rc.digest(got) == digests[name]["outputs"][key], \
        f"{name} {key} ({what}): not the reference's output (only its digest is recorded; " \
        f"tests/test_oracle_pinned.py has the arrays)"


# ---- integrate ----------------------------------------------------------------------------------

def _frames(inp):
    for i in range(rc.nframes(inp)):
        yield i, inp[f"depth{i}"], inp[f"assoc{i}"], inp[f"R{i}"].reshape(-1), inp[f"t{i}"]


@pytest.mark.parametrize("table,pad", [(False, 0), (True, 0), (False, 3), (True, 5)],
                         ids=["inline", "table", "inline_pitched", "table_pitched"])
@pytest.mark.parametrize("name", INTEGRATE)
def test_update_tsdf(ops, dev, gold, name, table, pad):
    inp = inputs_of(gold, name)
    nx, ny, nz = [int(v) for v in inp["res"]]
    vox, trunc, maxw = [float(v) for v in inp["scalars"]]
    h, w = inp["depth0"].shape
    d_t, d_w = dev_full((nz, ny, nx), 0.0), dev_full((nz, ny, nx), 0.0)
    il = None
    if table:
        il = dev_full((h, w), -3.0, pad_cols=pad)
        ops.compute_inv_lambda(inp["K"], il)
    for i, depth, assoc, R, t in _frames(inp):
        ops.update_tsdf(to_dev(depth, dev, pad), to_dev(assoc, dev, pad), d_t, d_w, R, t, inp["K"], vox, trunc,
                        maxw, inv_lambda=il)
        dev.synchronize()
        expect(gold, name, f"tsdf{i}", to_np(d_t), "updateTSDF")
        expect(gold, name, f"wts{i}", to_np(d_w), "updateTSDF")


class TableModel:
    """One volume and the images an emf_model_t names, sized to the case's depth image."""

    def __init__(self, ops, res, w, h, vox, trunc, maxw, unseen=None, tsdf=None, wts=None, grads=None):
        nx, ny, nz = [int(v) for v in res]
        self.ops, self.res = ops, (nx, ny, nz)
        self.vox, self.trunc, self.maxw = float(vox), float(trunc), float(maxw)
        self.d_tsdf = dev_full((nz, ny, nx), 0.0) if tsdf is None else to_dev(tsdf)
        self.d_wts = dev_full((nz, ny, nx), 0.0) if wts is None else to_dev(wts)
        self.d_grads = None if grads is None else to_dev(grads)
        self.d_assoc = dev_full((h, w), 1.0)
        self.d_ray, self.d_hit = dev_full((h, w), 5.0), dev_full((h, w), 5, np.uint8)
        self.d_vert, self.d_nrm = dev_full((h, w, 3), 5.0), dev_full((h, w, 3), 5.0)
        self.d_unseen = unseen

    def entry(self, rcp=0.0):
        return self.ops.make_model(self.d_tsdf, self.d_wts, self.d_assoc, self.d_ray, self.d_vert, self.d_nrm,
                                   self.d_hit, self.vox, self.trunc, self.maxw, SIGMA, ALPHA, PRIOR, model_id=0,
                                   grads=self.d_grads, rcp_voxel=rcp, unseen_tiles=self.d_unseen)


def _model_for(ops, inp, unseen=None):
    h, w = inp["depth0"].shape
    vox, trunc, maxw = inp["scalars"]
    return TableModel(ops, inp["res"], w, h, vox, trunc, maxw, unseen=unseen)


@pytest.mark.parametrize("table", [False, True], ids=["inline", "table"])
@pytest.mark.parametrize("name", INTEGRATE)
def test_integrate_batched(ops, dev, gold, name, table):
    inp = inputs_of(gold, name)
    m = _model_for(ops, inp)
    il = None
    if table:
        il = dev_full(inp["depth0"].shape, -3.0)
        ops.compute_inv_lambda(inp["K"], il)
    visible = dev_full((1,), 1, np.int32)
    for i, depth, assoc, R, t in _frames(inp):
        m.d_assoc.copy_from(assoc)
        ops.integrate_batched(ops.upload_models([m.entry()]), [(R, t)], [m.res], visible, to_dev(depth), inp["K"],
                              inv_lambda=il)
        dev.synchronize()
        expect(gold, name, f"tsdf{i}", to_np(m.d_tsdf), "integrateBatched")
        expect(gold, name, f"wts{i}", to_np(m.d_wts), "integrateBatched")


@pytest.mark.parametrize("unseen_map", ["kept", "rebuilt", "none"])
@pytest.mark.parametrize("name", TILED)
def test_integrate_batched_culled(ops, dev, gold, name, unseen_map):
    """kept: the map starts as "every tile unseen" on the cleared volume and the launches keep it;
    rebuilt: it is rebuilt from the volume before every frame; none: the launch without the map."""
    inp = inputs_of(gold, name)
    unseen = None if unseen_map == "none" else dev_full((ops.unseen_tile_bytes([int(v) for v in inp["res"]]),), 1,
                                                        np.uint8)
    m = _model_for(ops, inp, unseen)
    visible = dev_full((1,), 1, np.int32)
    for i, depth, assoc, R, t in _frames(inp):
        m.d_assoc.copy_from(assoc)
        if unseen_map == "rebuilt":
            ops.rebuild_unseen_tiles(m.d_tsdf, m.d_wts, unseen)
        ops.integrate_batched_culled(ops.upload_models([m.entry()]), [(R, t)], [m.res], visible, to_dev(depth),
                                     inp["K"])
        dev.synchronize()
        expect(gold, name, f"tsdf{i}", to_np(m.d_tsdf), f"integrateBatchedCulled, unseen map {unseen_map}")
        expect(gold, name, f"wts{i}", to_np(m.d_wts), f"integrateBatchedCulled, unseen map {unseen_map}")


@pytest.mark.parametrize("unseen_map", ["kept", "none"])
@pytest.mark.parametrize("name", TILED)
def test_integrate_batched_culled_out(ops, dev, gold, name, unseen_map):
    """Double-buffered as the host classes run it: read the front copy, write the back copy, swap."""
    inp = inputs_of(gold, name)
    res = [int(v) for v in inp["res"]]
    unseen = None if unseen_map == "none" else dev_full((ops.unseen_tile_bytes(res),), 1, np.uint8)
    front, back = _model_for(ops, inp, unseen), _model_for(ops, inp, unseen)  # the copies share the map
    maps = [dev_full((ops.integrate_dirty_map_bytes(res),), 0, np.uint8) for _ in range(2)]
    visible = dev_full((1,), 1, np.int32)
    for i, depth, assoc, R, t in _frames(inp):
        front.d_assoc.copy_from(assoc)
        outs = [(back.d_tsdf, back.d_wts, maps[i % 2], maps[1 - i % 2])]
        ops.integrate_batched_culled_out(ops.upload_models([front.entry()]), [(R, t)], [front.res], visible,
                                         to_dev(depth), inp["K"], outs)
        dev.synchronize()
        front, back = back, front
        expect(gold, name, f"tsdf{i}", to_np(front.d_tsdf), f"integrateBatchedCulledOut, unseen map {unseen_map}")
        expect(gold, name, f"wts{i}", to_np(front.d_wts), f"integrateBatchedCulledOut, unseen map {unseen_map}")


# ---- raycast ------------------------------------------------------------------------------------

def _grad_forms(name):
    # the zeroed gradient block exists only as a gradient volume
    return [True] if name == "ray_zero_grad" else [True, False]


@pytest.mark.parametrize("divide", [False, True], ids=["reciprocal", "divide"])
@pytest.mark.parametrize("name", RAYCAST)
def test_raycast_tsdf(ops, dev, gold, name, divide):
    inp = inputs_of(gold, name)
    h, w = inp["ray0"].shape
    vox, trunc = [float(v) for v in inp["scalars"]]
    rcp = 0.0 if divide else ops.voxel_reciprocal(vox)
    for with_grads in _grad_forms(name):
        pad = 3 if with_grads else 0
        ray = to_dev(inp["ray0"], dev, pad)
        vert, nrm = dev_full((h, w, 3), 0.0, pad_cols=pad), dev_full((h, w, 3), 0.0, pad_cols=pad)
        mask = dev_full((h, w), 0, np.uint8, pad_cols=pad)
        ops.raycast_tsdf(to_dev(inp["tsdf"]), to_dev(inp["grads"]) if with_grads else None, to_dev(inp["wts"]), None,
                         ray, vert, nrm, mask, inp["R"].reshape(-1), inp["t"], inp["K"], vox, trunc, rcp_voxel=rcp)
        dev.synchronize()
        what = f"raycastTSDF, {'gradient volume' if with_grads else 'gradients on the fly'}"
        for key, got in (("mask", mask), ("ray", ray), ("vert", vert), ("nrm", nrm)):
            expect(gold, name, key, to_np(got), what)


@pytest.mark.parametrize("name", [n for n in RAYCAST if n != "ray_prev"])  # the batched launch starts from zeroed images
def test_raycast_batched(ops, dev, gold, name):
    inp = inputs_of(gold, name)
    h, w = inp["ray0"].shape
    vox, trunc = inp["scalars"]
    assert not inp["ray0"].any()
    for with_grads in _grad_forms(name):
        m = TableModel(ops, inp["tsdf"].shape[::-1], w, h, vox, trunc, 64.0, tsdf=inp["tsdf"], wts=inp["wts"],
                       grads=inp["grads"] if with_grads else None)
        table = ops.upload_models([m.entry(rcp=ops.voxel_reciprocal(float(vox)))])
        ops.raycast_batched(table, [(inp["R"].reshape(-1), inp["t"])], [m.res], w, h, inp["K"])
        dev.synchronize()
        what = f"raycastBatched, {'gradient volume' if with_grads else 'gradients on the fly'}"
        for key, got in (("mask", m.d_hit), ("ray", m.d_ray), ("vert", m.d_vert), ("nrm", m.d_nrm)):
            expect(gold, name, key, to_np(got), what)


# ---- lookups and foreground counts --------------------------------------------------------------

def test_volume_lookups_on_the_last_cells(ops, dev, gold):
    name = "lookup_edges"
    inp = inputs_of(gold, name)
    vox = float(inp["scalars"][0])
    h, w = inp["points"].shape[:2]
    R, t, pts = inp["R"].reshape(-1), inp["t"], to_dev(inp["points"])
    for c in (1, 2, 3):
        vals = dev_full((h, w) if c == 1 else (h, w, c), 9.0)
        ops.get_volume_vals(to_dev(inp[f"vol{c}"]), pts, R, t, vox, vals)
        expect(gold, name, f"vals{c}", to_np(vals), "getVolumeVals")
    for grads in (to_dev(rc.forward_grads(inp["vol1"])), None):
        out = dev_full((h * w, 6), 9.0)
        ops.compute_pose_gradients(to_dev(inp["vol1"]), grads, pts, R, t, vox, out)
        expect(gold, name, "pose_grads", to_np(out), "computePoseGradients")


@pytest.mark.parametrize("name", [n for n, c in rc.CASES.items() if c.kind == "fgbg"])
def test_fgbg_counts(ops, dev, gold, name):
    inp = inputs_of(gold, name)
    nx, ny, nz = [int(v) for v in inp["res"]]
    d_fgbg = dev_full((nz, ny, nx, 2), 0.0)
    d_t, d_w = to_dev(inp["tsdf"]), to_dev(inp["wts"])
    for i in range(3):
        ops.update_fgbg_probs(to_dev(inp[f"mask{i}"], dev, 3), to_dev(inp[f"occl{i}"], dev, 3), d_t, d_w, d_fgbg,
                              inp[f"R{i}"].reshape(-1), inp[f"t{i}"], inp["K"], float(inp["scalars"][0]))
    expect(gold, name, "fgbg", to_np(d_fgbg), "updateFgBgProbs")
