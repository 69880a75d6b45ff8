"""The in-process scenarios of tests/test_gpu_components_pipeline.py, run in a process of their own:
python tests/components_pipeline_probe.py switch|switch_color|cleanup DIR.  Every assertion is made here; the process
ends with "PROBE_RESULT ok" or a traceback.
Why its own process: these scenarios create and destroy fusion instances with their streams, and which hardware queue a
later stream of the process lands on depends on that history (tests/test_gpu_peer_exchange.py, tests/dynamic_probe.py).
The thread-rank tests that follow in the suite's process keep one rank's kernel waiting for another's; they keep the
stream history they have always had."""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tests.components_reference import components, filter_mesh, kept_labels  # noqa: E402
from tests.parity_util import to_dev  # noqa: E402

FW, FH = 160, 120
# Small enough to leave every model its surface, large enough to drop the fragments three frames of this scene leave
# beside it (the switch scenario asserts that at least one mesh loses some).
MIN_TRIANGLES = 8


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def _setup(color=False):
    """The frame-mesh tests' scene: a 64^3 background and two 32^3 objects over the synthetic stream."""
    from emfusion_amd import pipeline
    prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5)
    synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), 2)
    fus = pipeline.Fusion(prm)
    if color:
        fus.enable_color()
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(2)]
    return synth, fus, ids


def _frame(fus, synth, ids, f, mask_frame, color=False):
    from emfusion_amd.ops import image_view
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    masks = {i: to_dev((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if mask_frame else {}
    keep = [to_dev(depth)]
    if color:
        keep.append(to_dev(np.random.default_rng(0xC0105 + f).integers(0, 256, (FH, FW, 3), dtype=np.uint8)))
        fus.set_color_image(image_view(keep[1]))
    fus.process_frame(image_view(keep[0]), R, t, poses, {i: image_view(m) for i, m in masks.items()}, mask_frame)
    fus.synchronize()


def _ply_bytes(tmp, mesh):
    from emfusion_amd import pipeline
    p = tmp / "expected.ply"
    pipeline.write_mesh(p, *mesh[:3], colors=mesh[3] if len(mesh) > 3 else None)
    return p.read_bytes()


def _stats(welded, filtered, largest):
    labels, sizes = components(welded[2], len(welded[0]))
    return dict(components=int((labels == np.arange(len(labels))).sum()),
                kept_components=len(kept_labels(labels, sizes, MIN_TRIANGLES, largest)),
                triangles=len(welded[2]), kept_triangles=len(filtered[2]))


def switch_scenario(tmp_path, color):
    """With set_mesh_filter on, mesh(), meshes(), the result files and the last frame's meshes equal the restatement's
    filter of what the same calls return with the filter off and the weld on; mesh_components() and last_mesh_filter()
    agree with it."""
    synth, fus, ids = _setup(color)
    try:
        fus.setup_output(True, False)
        fus.set_mesh_filter(MIN_TRIANGLES, largest_objects=True)     # (the weld switch stays off: the filter implies it)
        for f in range(3):
            _frame(fus, synth, ids, f, f == 0, color)
        filtered_one, stats_one = {}, {}
        for i in [0] + ids:
            filtered_one[i] = fus.mesh(i, colors=color)
            stats_one[i] = fus.last_mesh_filter()
        filtered_all = fus.meshes(colors=color)
        stats_all = fus.last_mesh_filter()
        fus.write_results(str(tmp_path / "on"), volumes=False)
        fus.set_mesh_filter()
        assert fus.last_mesh_filter() == stats_all                    # (the last extraction's, until the next one)
        fus.set_mesh_weld(True)
        welded_all = fus.meshes(colors=color)
        assert fus.last_mesh_filter() == {}
        differs = []
        for i in [0] + ids:
            welded = fus.mesh(i, colors=color)
            same(welded_all[i], welded, i)
            assert len(welded[0]) > 100
            labels, sizes = components(welded[2], len(welded[0]))
            print(f"model {i}: {len(welded[0])} welded vertices, component sizes "
                  f"{sorted(sizes[labels == np.arange(len(labels))].tolist(), reverse=True)}")
            same(fus.mesh_components(i), (labels, sizes), i)
            want = filter_mesh(*welded[:3], c=welded[3] if color else None, min_triangles=MIN_TRIANGLES,
                               largest_only=i != 0)
            same(filtered_one[i], want, i)
            same(filtered_all[i], want, i)
            expected_stats = _stats(welded, want, i != 0)
            assert stats_one[i] == {i: expected_stats} and stats_all[i] == expected_stats
            assert len(want[0]) > 100                                  # the surface stays
            differs.append(len(want[0]) != len(welded[0]))
            name = "mesh_bg.ply" if i == 0 else f"mesh_{i}.ply"
            frame = tmp_path / "on" / "frame_meshes" / ("bg" if i == 0 else str(i)) / "0002.ply"
            expected = _ply_bytes(tmp_path, want)
            assert (tmp_path / "on" / name).read_bytes() == expected, i
            assert frame.read_bytes() == expected, i
        assert sorted(stats_all) == [0] + ids
        assert any(differs)                                            # otherwise this test shows nothing
    finally:
        fus.close()
        synth.close()


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _files(d):
    return {str(p.relative_to(d)): hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(Path(d).rglob("*"))
            if p.is_file()}


def _cleanup_run(tmp, filter_on):
    """The frame-mesh tests' clean-up scenario: object 2 is reported behind the camera in frame 3 and deleted there."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 320, 240
    prm = pipeline.make_params(Wf, Hf, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_cleanup(True)
    if filter_on:
        fus.set_mesh_filter(MIN_TRIANGLES, largest_objects=True)
    fus.setup_output(True, False)
    centers, keep, log = {}, [], []
    try:
        for f in range(5):
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            d = to_dev(depth)
            masks = {i: to_dev((sid == i).astype(np.uint8)) for i in centers}
            keep += [d, masks]
            poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), c) for i, c in centers.items()}
            if f == 3:
                poses[2] = (poses[2][0], np.array([0, 0, -30], np.float32))
            if f == 0:
                new = [to_dev((sid == k).astype(np.uint8)) for k in (1, 2)]
                keep.append(new)
                fus.queue_new_object_masks([image_view(m) for m in new])
            fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, True)
            fus.synchronize()
            if f == 0:
                centers = {k: fus.pose(k)[1] for k in (1, 2)}
            if f == 3:
                del centers[2]
            live = fus.object_ids()
            log.append((live, fus.last_deleted(), [_digest(np.concatenate([x.reshape(-1) for x in fus.pose(i)]))
                                                  for i in [0] + live],
                        [_digest(fus.volume(v, i)) for i in [0] + live for v in ("tsdf", "weights")]))
        fus.write_results(str(tmp), volumes=False)
        return log, _files(tmp)
    finally:
        fus.close()
        synth.close()


def cleanup_scenario(tmp_path):
    """The clean-up run with the filter on and off: poses, object_ids(), last_deleted(), image logs and volumes have
    identical digests; only mesh files differ."""
    off_log, off_files = _cleanup_run(tmp_path / "off", False)
    on_log, on_files = _cleanup_run(tmp_path / "on", True)
    assert off_log[3][1] == [2] and off_log[4][0] == [1]      # the scenario happened
    assert on_log == off_log                                   # poses, object_ids(), last_deleted(), volumes
    assert sorted(on_files) == sorted(off_files)
    ply = {k for k in on_files if k.endswith(".ply")}
    assert {k for k in on_files if on_files[k] != off_files[k]} <= ply   # poses-*.txt and every image log: same bytes
    assert any(k.endswith(".png") for k in on_files)
    assert on_files["mesh_bg.ply"] != off_files["mesh_bg.ply"] and on_files["mesh_1.ply"] != off_files["mesh_1.ply"]
    # the deleted object's last mesh is the soup the life cycle took
    assert on_files["mesh_2.ply"] == off_files["mesh_2.ply"]


if __name__ == "__main__":
    from emfusion_amd import devmem
    assert devmem.device_count() >= 1, "no HIP device is visible (there is no CPU fallback)"
    devmem.set_device(0)
    what, out = sys.argv[1], Path(sys.argv[2])
    out.mkdir(parents=True, exist_ok=True)
    if what == "cleanup":
        cleanup_scenario(out)
    else:
        switch_scenario(out, what == "switch_color")
    print("PROBE_RESULT ok")
