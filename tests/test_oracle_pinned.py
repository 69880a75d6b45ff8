"""The CPU oracle against the REFERENCE'S OWN kernels, built for the host -- CPU only.

oracle/build_ref.py compiles the reference's device sources, text unchanged apart from the launch
syntax, into oracle/_ref/libemf_ref.so (oracle/ref_binding.py).  Every group below runs one of its
entry points and the oracle function of the same name on identical inputs and demands equality
bit for bit: no tolerance appears, every one of these operations is IEEE-exact on both sides.
Masks are compared as zero / non-zero (the reference writes ``bool``).

Inputs: first those of the GPU parity suite, imported from it (``frame``, ``BG``, ``CAMS``,
``SPHERES``, the ``bg_state`` of tests/test_gpu_parity.py and the ``world`` of
tests/test_gpu_tracking.py), so that "the GPU equals the oracle here" and "the oracle equals the
reference here" are statements about the same bytes; then the edge cases of
tests/reference_cases.py, each of which asserts that its edge is really exercised.

This module skips only when there is neither a library nor a reference checkout to build it from
(the GPU machine, for one).  With a checkout present, a library that does not build or load FAILS.

Not pinned, because the reference has no kernel text for it: the host-side OpenCV chains
(computeAssociation, Huber weights, normalisation, compositing, the bilateral filter).  And a NaN
point: kernel_getVolumeVals / kernel_computePoseGradients let NaN through both range tests and
index the volume with (int)NaN, which is out of bounds and undefined.
"""
import numpy as np
import pytest

from oracle import ref_binding
from tests import reference_cases as rc
from tests.parity_util import assert_parity
from tests.scenes import Pose, camera_path, rel_CO, rel_OC, rot
from tests.test_gpu_parity import BG, CAMS, H, K, MAXW, SPHERES, W, alloc_vol, bg_state, frame  # noqa: F401
from tests.test_gpu_tracking import _start_pose, world  # noqa: F401
from tests.test_oracle_meshing import sphere_sdf

pytestmark = pytest.mark.skipif(not ref_binding.available() and not ref_binding.reference_present(),
                                reason="no oracle/_ref/libemf_ref.so and no reference checkout to build it from")


@pytest.fixture(scope="module")
def ref():
    """The reference library; built on demand (like the oracle) when only the checkout is there."""
    if not ref_binding.available():
        from oracle import build_ref
        build_ref.build(verbose=False)
    ref_binding.lib()
    return ref_binding


def test_reference_library_builds_and_loads():
    """Fails, never skips, when the reference checkout is present and the library cannot be made."""
    if not ref_binding.available():
        from oracle import build_ref
        assert build_ref.build(verbose=False)
    assert ref_binding.lib().ref_abi_version() == 1


def same(got, want, what):
    """oracle (got) == reference (want), bit for bit in assert_parity's sense."""
    assert np.asarray(got).dtype == np.asarray(want).dtype, what
    assert_parity(got, want, what, exact=True)


def same_mask(got, want, what):
    assert np.array_equal(np.asarray(got) != 0, np.asarray(want) != 0), what


# ---- updateTSDF ---------------------------------------------------------------------------------

def integrate_pair(oracle, ref, res, vox, pose, frames, assoc_fn=None, max_w=MAXW):
    a, b = (alloc_vol(res), alloc_vol(res)), (alloc_vol(res), alloc_vol(res))
    for i in frames:
        cam, depth, ids = frame(i)
        assoc = np.ones((H, W), np.float32) if assoc_fn is None else assoc_fn(i, ids)
        oc = rel_OC(cam, pose)
        for B, (t, w) in ((oracle, a), (ref, b)):
            B.update_tsdf(depth, assoc, t, w, oc.R32, oc.t32, K, vox, 10 * vox, max_w)
    return a, b


@pytest.mark.parametrize("res", [(64, 64, 64), (30, 22, 18), (36, 20, 28), (33, 21, 17)])
def test_integrate_sequence(oracle, ref, res):
    vox = 2.56 / max(res)
    (t, w), (rt, rw) = integrate_pair(oracle, ref, res, vox, BG["pose"], range(3))
    assert (rw > 0).sum() > 1000 and (rt == -1).sum() > 10
    same(t, rt, f"tsdf {res}")
    same(w, rw, f"weights {res}")


def test_integrate_association_weights_cap_and_zero_sum(oracle, ref):
    rng = np.random.default_rng(11)

    def assoc(i, ids):
        a = rng.uniform(0, 1, (H, W)).astype(np.float32)
        a[ids == 1] = 0.0
        return a

    (t, w), (rt, rw) = integrate_pair(oracle, ref, (64, 64, 64), 0.04, BG["pose"], range(5), assoc, 2.5)
    assert rw.max() == 2.5
    same(t, rt, "tsdf")
    same(w, rw, "weights")


def test_integrate_camera_behind_and_rotated_volume(oracle, ref):
    pose = Pose(rot([1, 2, 0.5], 25), [0.1, -0.05, 0.6])
    (t, w), (rt, rw) = integrate_pair(oracle, ref, (48, 40, 56), 0.04, pose, range(2))
    same(t, rt, "tsdf")
    same(w, rw, "weights")


# ---- computeTSDFGrads ---------------------------------------------------------------------------

@pytest.mark.parametrize("res", [(64, 64, 64), (30, 22, 18), (33, 21, 17), (2, 2, 2)])
def test_tsdf_grads(oracle, ref, res):
    rng = np.random.default_rng(4)
    tsdf = rng.uniform(-1, 1, (res[2], res[1], res[0])).astype(np.float32)
    want = ref.compute_tsdf_grads(tsdf)
    same(oracle.compute_tsdf_grads(tsdf), want, "grads")
    same(rc.forward_grads(tsdf), want, "the closed form of tests/reference_cases.py")
    assert not want[-1].any() and not want[:, -1].any() and not want[:, :, -1].any()


# ---- raycastTSDF --------------------------------------------------------------------------------

def raycast_pair(oracle, ref, tsdf, grads, wts, fg, co, vox, ray0=None):
    got = oracle.raycast_tsdf(tsdf, grads, wts, fg, W, H, co.R32, co.t32, K, vox, 10 * vox, raylengths=ray0)
    want = ref.raycast_tsdf(tsdf, grads, wts, fg, W, H, co.R32, co.t32, K, vox, 10 * vox, raylengths=ray0)
    for g, w_, name in zip(got[:3], want[:3], ["raylengths", "vertices", "normals"]):
        same(g, w_, name)
    same_mask(got[3], want[3], "mask")
    return want


@pytest.mark.parametrize("cam_name", list(CAMS))
@pytest.mark.parametrize("use_grad_volume", [False, True])
def test_raycast_background(oracle, ref, bg_state, cam_name, use_grad_volume):
    """use_grad_volume=False: the oracle blends forward differences of the TSDF on the fly, the
    reference samples its own gradient volume -- the values must be the same."""
    tsdf, wts = bg_state
    grads = oracle.compute_tsdf_grads(tsdf) if use_grad_volume else None
    want = raycast_pair(oracle, ref, tsdf, grads, wts, None, rel_CO(CAMS[cam_name], BG["pose"]), BG["vox"])
    if cam_name != "outside_oblique":
        assert want[3].sum() > 2000


def test_raycast_respects_previous_raylength(oracle, ref, bg_state):
    tsdf, wts = bg_state
    ray0 = np.zeros((H, W), np.float32)
    ray0[:, : W // 2] = 1.0
    want = raycast_pair(oracle, ref, tsdf, None, wts, None, rel_CO(CAMS["tracked"], BG["pose"]), BG["vox"], ray0)
    assert want[3][:, : W // 2].sum() < want[3][:, W // 2:].sum()


def test_raycast_empty_and_unseen_volume(oracle, ref):
    tsdf, wts = alloc_vol((32, 32, 32)), alloc_vol((32, 32, 32))
    co = rel_CO(Pose(), Pose(t=[0, 0, 0.8]))
    got = oracle.raycast_tsdf(tsdf, None, wts, None, W, H, co.R32, co.t32, K, 0.01, 0.1)
    want = ref.raycast_tsdf(tsdf, None, wts, None, W, H, co.R32, co.t32, K, 0.01, 0.1)
    assert not want[3].any() and not want[0].any() and not got[3].any() and not got[0].any()


def test_raycast_object_with_foreground_mask(oracle, ref):
    cen, r = SPHERES[0]
    res, vox, pose = (32, 32, 32), 0.8 / 32, Pose(t=cen)
    tsdf, wts, fgbg = alloc_vol(res), alloc_vol(res), alloc_vol(res, 2)
    for i in range(3):
        cam, depth, ids = frame(i)
        oc = rel_OC(cam, pose)
        oracle.update_tsdf(depth, np.ones((H, W), np.float32), tsdf, wts, oc.R32, oc.t32, K, vox, 10 * vox, MAXW)
        oracle.update_fgbg_probs((ids == 1).astype(np.uint8), np.zeros((H, W), np.uint8), tsdf, wts, fgbg,
                                 oc.R32, oc.t32, K, vox)
    probs, vmask = oracle.compute_fg_probs(fgbg)
    assert 0 < (vmask > 0).sum() < vmask.size
    want = raycast_pair(oracle, ref, tsdf, None, wts, vmask, rel_CO(camera_path(3), pose), vox)
    assert want[3].sum() > 200


# ---- getVolumeVals / computePoseGradients -------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 2, 3])
def test_get_volume_vals(oracle, ref, ch):
    rng = np.random.default_rng(20 + ch)
    n = (40, 32, 36)
    vol = rng.standard_normal((n[2], n[1], n[0]) + ((ch,) if ch > 1 else ())).astype(np.float32)
    cam, depth, _ = frame(1)
    pts = oracle.compute_points(depth, K)
    co = rel_CO(cam, Pose(rot([0, 1, 0], 12), [0.1, 0, 1.4]))
    want = ref.get_volume_vals(vol, pts, co.R32, co.t32, 0.03)
    assert (want != 0).mean() > 0.05 and (want == 0).mean() > 0.01
    same(oracle.get_volume_vals(vol, pts, co.R32, co.t32, 0.03), want, f"vals ch={ch}")


@pytest.mark.parametrize("use_grad_volume", [False, True])
def test_pose_gradients(oracle, ref, world, use_grad_volume):
    v = world["vols"][0]
    R, t = _start_pose(world, 0)
    grads = oracle.compute_tsdf_grads(v["tsdf"])
    want = ref.compute_pose_gradients(v["tsdf"], grads, world["points"], R, t, v["vox"])
    got = oracle.compute_pose_gradients(v["tsdf"], grads if use_grad_volume else None, world["points"], R, t,
                                        v["vox"])
    assert (np.abs(want).sum(1) > 0).sum() > 5000
    same(got, want, "pose gradients")


# ---- computeAb / multSingletonCol (folded into orc_reduceAb) ------------------------------------

def test_ab_products_and_their_weighted_sums(oracle, ref, world):
    """The oracle has no function of the shape of computeAb / multSingletonCol: orc_reduceAb forms
    the same float32 per-pixel products and sums them in double.  So: the reference's products
    equal the plain float32 expressions bit for bit, and orc_reduceAb equals the float64 sum of the
    reference's weighted products within the bound tests/test_gpu_tracking.py uses for A and b."""
    v = world["vols"][0]
    R, t = _start_pose(world, 0)
    g = ref.compute_pose_gradients(v["tsdf"], None, world["points"], R, t, v["vox"])
    tv = ref.get_volume_vals(v["tsdf"], world["points"], R, t, v["vox"]).reshape(-1)
    iw = (ref.get_volume_vals(v["wts"], world["points"], R, t, v["vox"]).reshape(-1) / np.float32(MAXW)).astype(np.float32)
    As, bs = ref.compute_ab(g, tv)
    same((g[:, :, None] * g[:, None, :]).reshape(-1, 36), As, "As = g g^T")
    same(tv[:, None] * g, bs, "bs = tsdf * g")
    Aw, bw = ref.mult_singleton_col(iw, As), ref.mult_singleton_col(iw, bs)
    same(As * iw[:, None], Aw, "As * w")
    same(bs * iw[:, None], bw, "bs * w")
    A, b = oracle.reduce_ab(g, tv, iw)
    A64, b64 = Aw.astype(np.float64).sum(0).reshape(6, 6), bw.astype(np.float64).sum(0)
    assert np.abs(A64).max() > 1 and np.abs(b64).max() > 0
    assert np.abs(A - A64).max() <= 2e-5 * np.abs(A64).max(), "Hessian"
    assert np.abs(b - b64).max() <= 2e-5 * np.abs(b64).max(), "gradient"


# ---- copyValues ---------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3])
def test_copy_values(ref, channels):
    """No oracle function either; the plain expression is dst(v - offset) = src(v) where that lies
    inside dst, everything else untouched.  Offsets push part of the source outside on each side."""
    rng = np.random.default_rng(6)
    src = rng.standard_normal((6, 5, 8) if channels == 1 else (6, 5, 8, channels)).astype(np.float32)
    for off, dres in (((-2, 1, 0), (12, 6, 6)), ((3, -1, 2), (4, 8, 4)), ((0, 0, 0), (8, 5, 6)),
                      ((-3, -2, -1), (9, 5, 6)), ((5, 3, 4), (8, 5, 6)), ((8, 0, 0), (8, 5, 6))):
        dshape = (dres[2], dres[1], dres[0]) + (() if channels == 1 else (channels,))
        dst = np.full(dshape, 7.0, np.float32)
        ref.copy_values(src, dst, off)
        want = np.full(dshape, 7.0, np.float32)
        moved = 0
        for z in range(6):
            for y in range(5):
                for x in range(8):
                    xn, yn, zn = x - off[0], y - off[1], z - off[2]
                    if 0 <= xn < dres[0] and 0 <= yn < dres[1] and 0 <= zn < dres[2]:
                        want[zn, yn, xn] = src[z, y, x]
                        moved += 1
        assert (moved == src[..., 0].size if channels > 1 else moved == src.size) == (off == (0, 0, 0)), "part of the source must fall outside"
        assert np.array_equal(dst, want), (off, dres)


# ---- updateFgBgProbs ----------------------------------------------------------------------------

@pytest.mark.parametrize("res", [(32, 32, 32), (30, 22, 18)])
def test_fgbg_counts(oracle, ref, res):
    cen, r = SPHERES[0]
    vox = 0.8 / max(res)
    pose = Pose(rot([0, 0, 1], 10), cen)
    tsdf, wts = alloc_vol(res), alloc_vol(res)
    a, b = alloc_vol(res, 2), alloc_vol(res, 2)
    rng = np.random.default_rng(8)
    for i in range(3):
        cam, depth, ids = frame(i)
        oc = rel_OC(cam, pose)
        oracle.update_tsdf(depth, np.ones((H, W), np.float32), tsdf, wts, oc.R32, oc.t32, K, vox, 10 * vox, MAXW)
        mask = (ids == 1).astype(np.uint8) * (1 if i % 2 else 255)  # any non-zero is "true"
        occl = (rng.random((H, W)) < 0.2).astype(np.uint8)
        oracle.update_fgbg_probs(mask, occl, tsdf, wts, a, oc.R32, oc.t32, K, vox)
        ref.update_fgbg_probs(mask, occl, tsdf, wts, b, oc.R32, oc.t32, K, vox)
    assert b[..., 0].max() >= 2 and b[..., 1].max() >= 2
    same(a, b, "fgBgProbs")


# ---- marchingCubes ------------------------------------------------------------------------------

def _mesh_volumes():
    tiny = np.array([[[-1, 1], [1, 1]], [[1, 1], [1, 1]]], np.float32)
    yield "single cube", tiny, np.ones_like(tiny), None, 1.0
    sdf = sphere_sdf(12, 0.1, 0.35)
    yield "sphere 12", sdf, np.ones_like(sdf), None, 0.1
    w = np.ones_like(sdf)
    w[:, :, 6:] = 0
    yield "sphere 12, unobserved half", sdf, w, None, 0.1
    yield "sphere 12, empty foreground", sdf, np.ones_like(sdf), np.zeros(sdf.shape, np.uint8), 0.1
    fg = np.zeros(sdf.shape, np.uint8)
    fg[:7] = 255
    fg[:, :5] = 1
    yield "sphere 12, foreground mask of 1s and 255s", sdf, np.ones_like(sdf), fg, 0.1
    big = sphere_sdf(24, 0.05, 0.37)
    yield "sphere 24", big, np.ones_like(big), None, 0.05
    rng = np.random.default_rng(2)
    odd = rng.uniform(-1, 1, (7, 10, 13)).astype(np.float32)
    odd[rng.random(odd.shape) < 0.1] = 0.0  # exact zeros: vertexInterp's |val| < 1e-5 branches
    yield "noise 13x10x7", odd, (rng.random(odd.shape) < 0.9).astype(np.float32), None, 0.02
    # the dense fills of tests/mesh_volumes.py (zeros of both signs, denormals, values inside vertexInterp's 1e-5
    # branches, denormal and negative weights), one of them under its foreground mask of bytes 0, 1, 2, 128, 255
    from tests import mesh_volumes as MV
    for shape, masked in (((5, 3, 70), False), ((65, 7, 40), True), ((74, 90, 66), False)):
        t, w, fg, vox = MV.dense(shape)
        yield "dense " + MV.name_of(shape) + (", foreground mask" if masked else ""), t, w, fg if masked else None, vox


@pytest.mark.parametrize("case", list(_mesh_volumes()), ids=lambda c: c[0])
def test_marching_cubes(oracle, ref, case):
    """Vertex, normal and triangle arrays equal AS EMITTED: the host launch runs cubes in a fixed
    order and the reference's offsets come from an exclusive scan in x-fastest cube order, which
    is the order the oracle emits in -- no sorting."""
    name, tsdf, wts, fg, vox = case
    v, n, t = oracle.marching_cubes(tsdf, wts, vox, fg=fg)
    rv, rn, rt = ref.marching_cubes(tsdf, wts, vox, fg=fg)
    if "empty" in name:
        assert len(rv) == 0 and len(rt) == 0
    elif "single" not in name:
        assert len(rv) > 50 and len(rt) > 50
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    with np.errstate(all="ignore"):
        same(v, rv, "vertices")
        same(n, rn, "normals")
    assert np.array_equal(t, rt), "triangles"


# ---- computePoints / renderPhong ----------------------------------------------------------------

def test_compute_points(oracle, ref):
    _, depth, _ = frame(0)
    depth = depth.copy()
    depth[::9, ::7] = np.nan
    depth[1::9, ::7] = np.inf
    depth[2::9, ::7] = -1.0
    with np.errstate(all="ignore"):
        want = ref.compute_points(depth, K)
        got = oracle.compute_points(depth, K)
    assert np.isnan(want).any() and np.isinf(want).any() and (want[..., 2] < 0).any() and (want[..., 2] == 0).any()
    same(got, want, "points")


def test_render_phong(oracle, ref):
    """the reference casts I * 255 to uchar unchecked, which is undefined outside
    [0, 256); the project saturates instead (to_u8).  The images may differ ONLY where the oracle's
    channel is saturated (0 or 255), and must agree on the bulk."""
    rng = np.random.default_rng(12)
    h, w = 61, 83
    pts = rng.uniform(-1, 1, (h, w, 3)).astype(np.float32)
    pts[..., 2] = rng.uniform(0.4, 3.0, (h, w)).astype(np.float32)
    nrm = rng.standard_normal((h, w, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[..., 2] = -np.abs(nrm[..., 2])
    nrm[5, 5] = (0, 0, 1)
    nrm[6, 6] = 0
    nrm[7, 7] = np.nan
    hole = rng.uniform(size=(h, w)) < 0.2
    pts[hole] = 0
    seg = rng.integers(0, 256, (h, w)).astype(np.uint8)
    cmap = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    for light in ((0.0, 0.0, 0.0), (0.5, -0.25, 0.1)):
        with np.errstate(all="ignore"):
            want = ref.render_phong(pts, nrm, seg, cmap, light)
            got = oracle.render_phong(pts, nrm, seg, cmap, light)
        differ = got != want
        assert np.all((got[differ] == 0) | (got[differ] == 255)), "a difference outside the saturation rule"
        assert differ.mean() < 0.02 and np.all(want[hole] == 0) and want[~hole].max() > 100
        unsat = (got > 0) & (got < 255)
        assert unsat.mean() > 0.5 and np.array_equal(got[unsat], want[unsat])


# ---- the edges ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.CASES))
def test_edge_case(oracle, ref, name):
    case = rc.CASES[name]
    inp = case.inputs()
    want = rc.RUN[case.kind](ref, inp)
    case.check(inp, want)  # the reference alone shows that the edge is exercised
    got = rc.RUN[case.kind](oracle, inp)
    assert got.keys() == want.keys()
    for key in want:
        same(got[key], want[key], f"{name}: {key}")
