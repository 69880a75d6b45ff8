"""Motion masks through the host classes (Fusion.set_motion_masks): a sphere that enters a scene of which only the
wall is known is discovered, created as an object on its first frame, matched on the following ones and kept alive
by clean-up -- from nothing but depth.  The proposals of every frame are compared with the restatement
(tests/motion_reference.py) on the images of that frame; with the mode off nothing changes; queued masks take
precedence; the sharded path refuses the mode.

The scene is rendered here: a tilted wall z = 1.9 + 0.1 x for six frames, then a sphere of radius 0.152 m (20 pixels at
its distance of 1 m, its surface 0.9 m and more in front of the wall) that moves 1 cm per frame for eight more."""
import numpy as np
import pytest
from scipy import ndimage

from tests import motion_reference as mr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

W, H, WALL_FRAMES, FRAMES = 160, 120, 6, 14
EYE, ZERO = np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)
RADIUS = 0.152
MOTION = dict(band=0.4, continuity=0.05, erode=1, min_pixels=100, max_masks=8)  # band: the background's 10 voxels
IMAGES = ("points", "bg_assoc", "assoc_norm", "raylengths", "vertices", "normals", "segmentation", "bg_raylengths")


def params():
    from emfusion_amd import pipeline
    return pipeline.make_params(W, H, 64, 0.04, 32, visibility_thresh=100, boundary=5, mask_frames=1)


def render(frame):
    """(depth (H, W) f32, true sphere mask) of one frame; the camera sits at the origin and looks down +z."""
    K = np.array(params().K, np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]  # ray (dx, dy, 1): the ray parameter is z
    depth = 1.9 / (1.0 - 0.1 * dx)
    inside = np.zeros((H, W), bool)
    if frame >= WALL_FRAMES:
        c = np.array([-0.05 + 0.01 * (frame - WALL_FRAMES), 0.02, 1.0])
        a = dx * dx + dy * dy + 1.0
        b = -2.0 * (dx * c[0] + dy * c[1] + c[2])
        disc = b * b - 4.0 * a * (c @ c - RADIUS * RADIUS)
        inside = disc > 0
        z = (-b - np.sqrt(np.where(inside, disc, 0.0))) / (2.0 * a)
        depth = np.where(inside, z, depth)
    return depth.astype(np.float32), inside


@pytest.fixture(scope="module")
def frames():
    return [render(f) for f in range(FRAMES)]


def run_session(frames, setup=None, queue=None, n=FRAMES):
    """A session over the first n frames; setup(fusion) before the first one; queue: {frame: [u8 masks]} of queued
    instance masks.  Returns the per-frame log and the final state."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    fus = pipeline.Fusion(params())
    fus.set_cleanup(True)
    if setup:
        setup(fus)
    log, keep = [], []
    for f in range(n):
        d = to_dev(frames[f][0])
        keep.append(d)
        if queue and f in queue:
            dm = [to_dev(m) for m in queue[f]]
            keep.append(dm)
            fus.queue_instance_masks([image_view(m) for m in dm])
        fus.process_frame(image_view(d), EYE, ZERO, {}, {}, True)
        fus.synchronize()
        labels, proposals = fus.last_motion_masks()
        log.append(dict(created=fus.last_created(), assigned=fus.last_mask_assignment(), deleted=fus.last_deleted(),
                        ids=fus.object_ids(), labels=labels, proposals=proposals, points=fus.image("points"),
                        bg_ray=fus.image("bg_raylengths")))
    final = dict(tsdf=fus.volume("tsdf", 0), weights=fus.volume("weights", 0),
                 images={k: fus.image(k) for k in IMAGES}, last_masks=fus.last_masks())
    fus.close()
    return log, final


@pytest.fixture(scope="module")
def discovered(dev, frames):
    return run_session(frames, lambda fus: fus.set_motion_masks(True, **MOTION))


@pytest.fixture(scope="module")
def plain(dev, frames):
    return run_session(frames)


def test_sphere_is_discovered_created_once_matched_and_kept(discovered):
    log, final = discovered
    for f in range(WALL_FRAMES):  # (a) nothing but the wall: no proposal, no object
        assert log[f]["ids"] == [] and log[f]["proposals"] == [] and log[f]["created"] == [], f
    first = log[WALL_FRAMES]
    assert len(first["proposals"]) == 1 and first["created"] == [1] and first["ids"] == [1]
    assert first["assigned"] == [1]
    for f in range(WALL_FRAMES + 1, FRAMES):  # matched, not created again
        assert log[f]["created"] == [] and log[f]["assigned"] == [1], (f, log[f]["created"], log[f]["assigned"])
        assert log[f]["deleted"] == [] and log[f]["ids"] == [1], f
    # get_last_masks draws the last frame's proposal in the first instance colour
    n, img = final["last_masks"]
    assert n == 1
    inside = log[-1]["labels"] == 0
    assert (img[inside] == (0, 0, 255)).all() and not img[~inside].any()


def test_proposals_equal_the_restatement_on_every_frame(discovered):
    log, _ = discovered
    seen = 0
    for f, fr in enumerate(log):  # (b)
        ref = mr.motion_masks(fr["points"], fr["bg_ray"], **MOTION)
        assert fr["labels"].dtype == np.int32 and fr["labels"].tobytes() == ref["labels"].tobytes(), f
        assert fr["proposals"] == mr.proposals(ref), f
        seen += ref["count"]
    assert seen == FRAMES - WALL_FRAMES


def test_the_proposal_is_the_sphere(discovered, frames):
    log, _ = discovered
    square = np.ones((3, 3), bool)
    for f in range(WALL_FRAMES, FRAMES):  # (c) bounds that follow from the band and the erosion alone
        truth = frames[f][1]
        got = log[f]["labels"] == 0
        assert not (got & ~ndimage.binary_dilation(truth, square)).any(), f
        core = ndimage.binary_erosion(truth, square, iterations=MOTION["erode"] + 2)
        assert core.sum() > 500 and not (core & ~got).any(), f


def same_state(a, b):
    assert a["tsdf"].tobytes() == b["tsdf"].tobytes() and a["weights"].tobytes() == b["weights"].tobytes()
    for k in IMAGES:
        assert a["images"][k].tobytes() == b["images"][k].tobytes(), k


def test_mode_off_changes_nothing(dev, frames, plain, discovered):
    def on_and_off(fus):
        fus.set_motion_masks(True, **MOTION)
        fus.set_motion_masks(False)

    log, final = run_session(frames, on_and_off)  # (d)
    same_state(final, plain[1])
    for a, b in zip(log, plain[0]):
        assert a["proposals"] == b["proposals"] == [] and (a["labels"] == -1).all() and (b["labels"] == -1).all()
        assert a["ids"] == b["ids"] == []
    same_state(run_session(frames)[1], plain[1])  # what the comparison rests on: a session repeats itself
    assert discovered[0][-1]["ids"] == [1]  # ... and with the mode on the same frames do give an object


def test_queued_masks_take_precedence(dev, frames):
    f0 = WALL_FRAMES
    queued = frames[f0][1].astype(np.uint8)
    log, _ = run_session(frames, lambda fus: fus.set_motion_masks(True, **MOTION), queue={f0: [queued]}, n=f0 + 2)  # (e)
    assert log[f0]["proposals"] == [] and (log[f0]["labels"] == -1).all()
    assert log[f0]["created"] == [1] and log[f0]["assigned"] == [1]  # from the queued mask
    assert len(log[f0 + 1]["proposals"]) == 1 and log[f0 + 1]["assigned"] == [1]  # the next frame proposes again


def test_refusals(dev, frames):
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):  # (f) thread-ranks of a sharded session
        fus = pipeline.Fusion(params(), comm)
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.set_motion_masks(True, **MOTION)
        assert err.value.code == -4
        fus.set_motion_masks(False)  # switching it off is no error anywhere
        ready.wait(timeout=JOIN_S)
        for f in range(2):  # the session goes on
            d = to_dev(frames[f][0])
            fus.process_frame(image_view(d), EYE, ZERO, {}, {}, True)
            fus.synchronize()
        labels, proposals = fus.last_motion_masks()
        hits = int((fus.image("bg_raylengths") > 0).sum())
        fus.close()
        return hits, proposals, bool((labels == -1).all())

    for hits, proposals, empty in run_ranks(2, body):
        assert hits > W * H // 2 and proposals == [] and empty
    fus = pipeline.Fusion(params())
    for bad in (dict(erode=4), dict(max_masks=0), dict(max_masks=17), dict(min_pixels=-1), dict(continuity=-1.0)):
        with pytest.raises(pipeline.FusionError) as err:
            fus.set_motion_masks(True, **bad)
        assert err.value.code == -4, bad
    fus.close()
