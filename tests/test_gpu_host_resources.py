"""The host classes own their pinned host memory and HIP events through emf::PinnedBuffer / emf::Event (core/types.hpp):
~EMFusion waits for the device and the members release themselves, and a constructor that throws releases what it had
built.  One small session reaches every owner -- the visibility mirrors, the tracking states and progress words, the
life-cycle read-backs, the view poses, the mesh table and staging, both upload slots with their events -- and is
repeated over constructions in one process: the last must give the bytes of the first, also right after a
construction that was refused (EMF_MARCH_ROWS=3: an argument error raised before any launch).

Scene: 160 x 120, background 64^3 at 0.04 m, two objects 32^3, four frames -- two on device depth maps with masks (the second is
tracked and ends with clean-up), two through process_rgbd (host depth: one upload slot each)."""
import os

import numpy as np
import pytest
import xxhash

from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu
W, H = 160, 120
EYE = np.eye(3, dtype=np.float32).reshape(-1)


def _digest(a):
    return xxhash.xxh3_128(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).hexdigest()


@pytest.fixture(scope="module")
def scene(dev):
    from emfusion_amd import pipeline
    prm = pipeline.make_params(W, H, 64, 0.04, 32, visibility_thresh=100, boundary=5, mask_frames=100)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    frames = []
    for f in range(4):
        depth, sid = synth.render(f)
        frames.append((depth, sid, synth.camera_pose(f), [synth.sphere(k, f)[0] for k in range(2)]))
    first = [synth.sphere(k, 0) for k in range(2)]
    synth.close()
    return prm, frames, first


def _session(scene):
    """every call that allocates one of the owners; any failure raises"""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    prm, frames, first = scene
    fus = pipeline.Fusion(prm, None)
    try:
        ids = [fus.add_object(c, vs) for c, _, vs in first]
        fus.set_tracking(camera=True, objects=True)
        keep = []
        for f in (0, 1):
            depth, sid, (R, t), centres = frames[f]
            d = to_dev(depth)
            masks = {i: to_dev((sid == i).astype(np.uint8)) for i in ids}
            keep += [d, masks]
            fus.set_cleanup(f == 1)  # both are mask frames (an object is ray-cast through its foreground mask); frame 1
            fus.process_frame(image_view(d), R, t, {i: (EYE, centres[i - 1]) for i in ids},  # is tracked and ends with cleanUpObjs
                              {i: image_view(m) for i, m in masks.items()}, True)
        fus.set_cleanup(False)
        for f in (2, 3):  # host depth maps: the two upload slots, their staging buffers and events
            fus.process_rgbd(frames[f][0])
        fus.synchronize()
        out = {"ids": tuple(fus.object_ids()), "vis": tuple(sorted(fus.visible_objects())), "uploads": fus.upload_host_time()[1],
               "seen": int((fus.volume("weights", 0) > 0).sum())}
        out["render"] = _digest(fus.render()[0])
        R, t = frames[3][2]
        rgb, ray, seg = fus.render_view(R, t)
        out["view"] = _digest(rgb) + _digest(ray) + _digest(seg)
        out["view_hits"] = int((ray > 0).sum())
        meshes = fus.meshes()
        out["mesh_ids"] = tuple(sorted(meshes))
        out["vertices"] = sum(len(v) for v, _, _ in meshes.values())
        for i, (v, n, tri) in meshes.items():
            out[f"mesh {i}"] = _digest(v) + _digest(n) + _digest(tri)
        for i in (0,) + out["ids"]:
            out[f"tsdf {i}"] = _digest(fus.volume("tsdf", i))
            out[f"weights {i}"] = _digest(fus.volume("weights", i))
            out[f"pose {i}"] = _digest(np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in fus.pose(i)]))
        for i in out["ids"]:
            out[f"fgprobs {i}"] = _digest(fus.volume("fgprobs", i))
        for im in ("raylengths", "segmentation", "assoc_norm", "bg_assoc", "bg_raylengths"):
            out[im] = _digest(fus.image(im))
        return out
    finally:
        fus.close()


def test_constructions_in_one_process_give_the_same_bytes_also_after_a_refused_one(scene):
    from emfusion_amd import pipeline
    runs = [_session(scene) for _ in range(6)]
    base = runs[0]
    # the session is not vacuous: both objects live through the clean-up and are meshed, both upload slots were used
    assert base["ids"] == (1, 2) and base["mesh_ids"] == (0, 1, 2) and base["uploads"] == 2, base
    assert base["seen"] > 10000 and base["view_hits"] > 1000 and base["vertices"] > 1000, base
    assert runs[-1] == base, sorted(k for k in base if base[k] != runs[-1][k])
    # a constructor that throws: refused with the documented error, nothing left behind that disturbs the next one
    os.environ["EMF_MARCH_ROWS"] = "3"
    try:
        with pytest.raises(pipeline.FusionError) as e:
            pipeline.Fusion(scene[0], None)
    finally:
        os.environ.pop("EMF_MARCH_ROWS", None)
    assert e.value.code == -4 and "EMFusion: EMF_MARCH_ROWS=3 (1, 2 or 4 lanes per background ray)" in str(e.value)  # EMF_E_ARG
    again = _session(scene)
    assert again == base, sorted(k for k in base if base[k] != again[k])
