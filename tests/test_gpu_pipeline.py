"""End-to-end parity of the C++ host classes (emf::EMFusion schedule over the HIP kernels, driven
through include/emf_fusion.h) against the frame-level oracle (tests/oracle_pipeline.py) on the
same synthetic RGB-D stream: E-step x3, raycast + compositing + visibility, association-weighted
integration and fg/bg mask integration, over several frames with moving camera and objects."""
import numpy as np
import pytest

from tests.oracle_pipeline import Affine32, OraclePipeline
from tests.parity_util import assert_parity, to_dev

pytestmark = pytest.mark.gpu

W, H = 160, 120
BG_RES, BG_VOX, OBJ_RES = 64, 0.04, 32
NOBJ, NFRAMES, MASK_EVERY = 2, 6, 3


def run_scenario(path, oracle, W=W, H=H):
    """The scenario on execution path `path` at W x H: yields (fusion, oracle pipeline, object ids, history), closes
    everything afterwards.  Execution paths of emf::EMFusion: batched model-table launches (default), the
    reference-shaped one-stream-per-volume path (EMF_PER_VOLUME=1), and the object-sharded
    multi-GPU path driven through a real RCCL communicator of ONE rank (EMF_FORCE_SHARDED=1):
    E-step partial sum -> ncclAllReduce(sum) -> normalise, hit keys -> ncclAllReduce(min) ->
    composite from keys, indexed device-side visibility gate, per-frame depth broadcast; "peer": the same path
    over the direct peer-write transport with its exchanges fused into the path's kernels (E-step scattering its
    partial sum, wait + reduce + normalise; key packing scattering keys and the background band, wait + min +
    composite + visibility), "peer_unfused": that transport's own two-launch collectives -- what the classes fall back
    to when the group's slots are too small for the fused raycast exchange (13 bytes per pixel)."""
    import os

    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view

    os.environ["EMF_PER_VOLUME"] = "1" if path.endswith("per_volume") else "0"
    # default: the background is kept twice and integrated out of place beside the raycast;
    # "in_place": the reference's sequence raycast -> integrate on one copy
    os.environ["EMF_BG_OVERLAP"] = "0" if path.endswith("in_place") else "1"
    comm = None
    if path.startswith("sharded"):
        os.environ["EMF_FORCE_SHARDED"] = "1"
        if "peer" in path:
            comm = pipeline.Communicator.local_group(1, transport="peer",
                                                     max_bytes=W * H * (8 if path.endswith("unfused") else 16))[0]
        else:
            comm = pipeline.Communicator(pipeline.Communicator.unique_id(), 0, 1)

    # visibility threshold / boundary scaled to the small image (reference: 1600 px, 20 px @ VGA)
    prm = pipeline.make_params(W, H, BG_RES, BG_VOX, OBJ_RES, visibility_thresh=100, boundary=5,
                               mask_frames=MASK_EVERY)
    K = np.array(prm.K, np.float32)
    synth = pipeline.SyntheticStream(W, H, K, NOBJ, seed=0xE3F5)
    fus = pipeline.Fusion(prm, comm)
    if comm is not None:
        fus.set_depth_broadcast(0)  # the per-frame ncclBroadcast of the depth image (rank 0 = source)
    orc = OraclePipeline(oracle, W, H, K, BG_RES, BG_VOX, list(prm.volume_pose_t), OBJ_RES,
                         visibility_thresh=100, boundary=5)
    fus.enable_raycast_stats(True)
    ids = []
    for k in range(NOBJ):
        c, r, vs = synth.sphere(k, 0)
        ids.append(fus.add_object(c, vs))
        assert orc.add_object(c, vs) == ids[-1]
    history = []
    for f in range(NFRAMES):
        depth, sid = synth.render(f)
        R, t = synth.camera_pose(f)
        poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(i - 1, f)[0])
                 for i in ids}
        run_masks = f % MASK_EVERY == 0
        masks = {i: (sid == i).astype(np.uint8) for i in ids} if run_masks else {}
        d_depth = to_dev(depth)
        d_masks = {i: to_dev(m) for i, m in masks.items()}
        fus.process_frame(image_view(d_depth), R, t, poses,
                          {i: image_view(m) for i, m in d_masks.items()}, run_masks)
        fus.synchronize()
        orc.process_frame(depth, Affine32(R.reshape(3, 3), t),
                          {i: Affine32(p[0].reshape(3, 3), p[1]) for i, p in poses.items()},
                          masks, run_masks)
        history.append(dict(vis=sorted(fus.visible_objects()), ovis=sorted(orc.vis)))
    os.environ.pop("EMF_PER_VOLUME", None)
    os.environ.pop("EMF_BG_OVERLAP", None)
    os.environ.pop("EMF_FORCE_SHARDED", None)
    yield fus, orc, ids, history
    fus.close()
    if comm is not None:
        comm.close()
    synth.close()


@pytest.fixture(scope="module", params=["batched", "batched_in_place", "per_volume", "sharded_1rank",
                                         "sharded_1rank_per_volume", "sharded_1rank_peer", "sharded_1rank_peer_unfused"])
def run(request, oracle, dev):
    yield from run_scenario(request.param, oracle)


def test_frames_were_processed(run):
    fus, orc, ids, history = run
    assert fus.frame_index() == NFRAMES == orc.frame
    assert all(fus.owns_object(i) for i in ids)


def test_visible_sets_match_every_frame(run):
    _, _, _, history = run
    for f, hrec in enumerate(history):
        assert hrec["vis"] == hrec["ovis"], f"frame {f}"
    assert any(hrec["vis"] for hrec in history[1:]), "no object ever became visible"


def test_background_volume(run):
    fus, orc, _, _ = run
    t = fus.volume("tsdf", 0)
    w = fus.volume("weights", 0)
    assert (orc.bg["wts"] > 0).sum() > 10000
    # association weights pass through expf (few-ulp library differences), then through the
    # running average: allow the north-star tolerance with a small outlier budget
    assert_parity(w, orc.bg["wts"], "bg weights", rtol=1e-4, atol=1e-6, budget=1e-3)
    assert_parity(t, orc.bg["tsdf"], "bg tsdf", rtol=1e-4, atol=1e-6, budget=1e-3)


def test_object_volumes_and_foreground(run):
    fus, orc, ids, _ = run
    for v in orc.objects:
        i = v["id"]
        assert_parity(fus.volume("weights", i), v["wts"], f"obj {i} weights", rtol=1e-4, atol=1e-6,
                      budget=1e-3)
        assert_parity(fus.volume("tsdf", i), v["tsdf"], f"obj {i} tsdf", rtol=1e-4, atol=1e-6,
                      budget=1e-3)
        assert_parity(fus.volume("fgprobs", i), v["probs"], f"obj {i} fgProbs", rtol=1e-4,
                      atol=1e-6, budget=1e-3)
        got_mask = fus.volume("fgmask", i)
        assert (got_mask != v["vmask"]).mean() < 1e-3
        assert (v["vmask"] > 0).sum() > 50


def test_association_weights(run):
    fus, orc, ids, _ = run
    assert_parity(fus.image("points"), orc.points, "points", exact=True)
    assert_parity(fus.image("assoc_norm"), orc.norm, "associationNorm", rtol=1e-4, budget=1e-3)
    assert_parity(fus.image("bg_assoc"), orc.bg_assoc, "bg association", rtol=1e-4, atol=1e-7,
                  budget=1e-3)
    total = fus.image("bg_assoc").astype(np.float64)
    for v in orc.objects:
        a = fus.image("obj_assoc", v["id"])
        assert_parity(a, v["assoc"], f"obj {v['id']} association", rtol=1e-4, atol=1e-7,
                      budget=1e-3)
        total += a
    valid = orc.norm != 0
    assert np.allclose(total[valid], 1.0, atol=1e-5) and np.all(total[~valid] == 0)
    assert any((v["assoc"] > 0.5).sum() > 100 for v in orc.objects), "objects never win pixels"


def test_raycast_and_segmentation(run):
    fus, orc, ids, _ = run
    seg = fus.image("segmentation")
    assert (seg != orc.seg).mean() < 2e-3
    assert set(np.unique(orc.seg)) >= {0, 1} and (orc.seg > 0).sum() > 200
    same = seg == orc.seg
    ray = fus.image("raylengths")
    assert_parity(ray[same], orc.ray[same], "composite raylengths", rtol=1e-4, budget=5e-3)
    assert_parity(fus.image("bg_raylengths"), orc.bg_ray, "bg raylengths", rtol=1e-4, budget=5e-3)
    for v in orc.objects:
        assert_parity(fus.image("obj_raylengths", v["id"]), v["ray"], f"obj {v['id']} raylengths",
                      rtol=1e-4, budget=5e-3)
    nrm = fus.image("normals")
    hit = (orc.ray > 0) & same
    assert_parity(nrm[hit], orc.nrm[hit], "normals", rtol=1e-3, atol=1e-4, budget=1e-2)


def test_march_sample_count_close_to_oracle(run):
    fus, orc, _, _ = run
    samples, hits, gathered, skipped = fus.raycast_stats()
    assert hits > 0
    # the oracle marches every ray to the end of its range; the batched path cuts a march where nothing
    # can be hit any more (far bounds): never more samples than the oracle, and not wildly fewer
    assert 0.5 * orc.march_samples <= samples <= 1.01 * orc.march_samples


def test_reset_in_the_middle_of_a_run_starts_over_exactly(dev):
    """EMFusion::reset (reference EMFusion.cpp:58-68) with everything the native path keeps beside the
    volumes -- second copy of the background and its dirty maps, fills done a frame ahead, sign maps,
    relevant-tile lists, streams with work in flight: a run after reset() equals a run on a fresh instance
    byte for byte."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm = pipeline.make_params(W, H, 128, 0.02, OBJ_RES, visibility_thresh=100, boundary=5, mask_frames=MASK_EVERY)
    K = np.array(prm.K, np.float32)
    synth = pipeline.SyntheticStream(W, H, K, NOBJ, seed=0xE3F5)
    keep = []

    def run(fus, frames):
        ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(NOBJ)]
        for f in frames:
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(i - 1, f)[0]) for i in ids}
            masks = {i: to_dev((sid == i).astype(np.uint8)) for i in ids} if f % MASK_EVERY == 0 else {}
            d = to_dev(depth)
            keep.append((d, masks))
            fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, bool(masks))
        fus.synchronize()
        return dict(t=fus.volume("tsdf", 0), w=fus.volume("weights", 0), ray=fus.image("raylengths"),
                    seg=fus.image("segmentation"), obj={i: fus.volume("tsdf", i) for i in ids},
                    assoc=fus.image("bg_assoc"))

    fresh = pipeline.Fusion(prm, None)
    want = run(fresh, range(5))
    fresh.close()
    fus = pipeline.Fusion(prm, None)
    run(fus, range(2, 6))  # another stretch of the stream first, left without waiting for anything
    fus.reset()
    got = run(fus, range(5))
    fus.close()
    synth.close()
    for k in ("t", "w", "ray", "seg", "assoc"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for i in want["obj"]:
        assert got["obj"][i].tobytes() == want["obj"][i].tobytes(), i
    assert (want["w"] > 0).sum() > 10000 and (want["seg"] > 0).sum() > 100
