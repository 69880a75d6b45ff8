"""The in-process scenarios of tests/test_gpu_simplify_pipeline.py, run in a process of their own:
python tests/simplify_pipeline_probe.py switch|switch_color|cleanup DIR.  Every assertion is made here; the process ends
with "PROBE_RESULT ok" or a traceback.  Its own process for the reason tests/components_pipeline_probe.py gives; the
session, the frames and the helpers are that file's."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tests.components_pipeline_probe import MIN_TRIANGLES, _digest, _files, _frame, _ply_bytes, _setup, same  # noqa: E402
from tests.parity_util import to_dev  # noqa: E402
from tests.simplify_reference import simplify  # noqa: E402

CELL = 0.06   # metres: one and a half background voxels of the scene, a few object voxels


def _expected(ops, mesh, color):
    """ops.simplify_mesh of a welded (filtered) mesh -- and the restatement's, which must agree."""
    want = ops.simplify_mesh(*mesh[:3], colors=mesh[3] if color else None, cell=CELL)
    same(want, simplify(*mesh[:3], mesh[3] if color else None, cell=np.float32(CELL)))
    return want


def _stats(mesh, want):
    v, _, t = mesh[:3]
    keys = np.unique(np.floor(v.astype(np.float64) / np.float64(np.float32(CELL))), axis=0)
    return dict(vertices_in=len(v), triangles_in=len(t), vertices_out=len(want[0]), triangles_out=len(want[2]),
                clusters=len(keys))


def switch_scenario(tmp_path, color):
    """With set_mesh_simplify on, mesh(), meshes(), the result files and the last frame's meshes equal
    ops.simplify_mesh of what the same calls return with it off (welded, and filtered where the filter is on);
    last_mesh_simplify() agrees with the arrays; set back to 0 it restores the welded bytes."""
    from emfusion_amd import ops
    synth, fus, ids = _setup(color)
    try:
        fus.setup_output(True, False)
        fus.set_mesh_simplify(CELL)                                   # (the weld switch stays off: a cell implies it)
        assert fus.last_mesh_simplify() == {}
        for f in range(3):
            _frame(fus, synth, ids, f, f == 0, color)
        one, stats_one = {}, {}
        for i in [0] + ids:
            one[i] = fus.mesh(i, colors=color)
            stats_one[i] = fus.last_mesh_simplify()
        every = fus.meshes(colors=color)
        stats_all = fus.last_mesh_simplify()
        assert fus.last_mesh_filter() == {}
        fus.write_results(str(tmp_path / "on"), volumes=False)
        fus.set_mesh_filter(MIN_TRIANGLES, largest_objects=True)      # behind the filter
        both_one = {i: fus.mesh(i, colors=color) for i in [0] + ids}
        both = fus.meshes(colors=color)
        stats_both = fus.last_mesh_simplify()
        fus.set_mesh_simplify(0.0)                                    # back to 0: the filtered, then the welded bytes
        assert fus.last_mesh_simplify() == stats_both                 # (the last extraction's, until the next one)
        filtered = fus.meshes(colors=color)
        assert fus.last_mesh_simplify() == {}
        fus.set_mesh_filter()
        fus.set_mesh_weld(True)
        welded = fus.meshes(colors=color)
        for i in [0] + ids:
            same(fus.mesh(i, colors=color), welded[i], i)
            assert len(welded[i][0]) > 100
            want = _expected(ops, welded[i], color)
            print(f"model {i}: {len(welded[i][0])} welded vertices / {len(welded[i][2])} triangles -> "
                  f"{len(want[0])} / {len(want[2])}; filtered {len(filtered[i][0])} / {len(filtered[i][2])}")
            assert 0 < len(want[0]) < len(welded[i][0]) and 0 < len(want[2]) < len(welded[i][2])
            same(one[i], want, i)
            same(every[i], want, i)
            expected_stats = _stats(welded[i], want)
            assert stats_one[i] == {i: expected_stats} and stats_all[i] == expected_stats, (stats_one[i], expected_stats)
            want_both = _expected(ops, filtered[i], color)
            same(both[i], want_both, (i, "filtered"))
            same(both_one[i], want_both, (i, "filtered"))
            assert stats_both[i] == _stats(filtered[i], want_both)
            name = "mesh_bg.ply" if i == 0 else f"mesh_{i}.ply"
            frame = tmp_path / "on" / "frame_meshes" / ("bg" if i == 0 else str(i)) / "0002.ply"
            expected = _ply_bytes(tmp_path, want)
            assert (tmp_path / "on" / name).read_bytes() == expected, i
            assert frame.read_bytes() == expected, i
        assert sorted(stats_all) == [0] + ids
        fus.set_mesh_weld(False)
        soup = fus.mesh(0)
        assert len(soup[0]) > len(welded[0][0]) and len(soup[2]) == len(welded[0][2])   # everything off: the soup again
    finally:
        fus.close()
        synth.close()


def _cleanup_run(tmp, simplify_on):
    """The frame-mesh tests' clean-up scenario (object 2 is reported behind the camera in frame 3 and deleted there),
    with a checkpoint written after the last frame."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 320, 240
    prm = pipeline.make_params(Wf, Hf, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_cleanup(True)
    if simplify_on:
        fus.set_mesh_simplify(CELL)
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
        Path(tmp).mkdir(parents=True, exist_ok=True)
        fus.save_checkpoint(str(tmp) + ".ckpt")   # (before write_results, which keeps the live models' meshes as written)
        fus.write_results(str(tmp), volumes=False)
        return log, _files(tmp), Path(str(tmp) + ".ckpt").read_bytes()
    finally:
        fus.close()
        synth.close()


def cleanup_scenario(tmp_path):
    """The clean-up run with the switch on and off: poses, object_ids(), last_deleted(), image logs, volumes and the
    checkpoint are the same bytes; only mesh files differ, and not the deleted object's."""
    off_log, off_files, off_ckpt = _cleanup_run(tmp_path / "off", False)
    on_log, on_files, on_ckpt = _cleanup_run(tmp_path / "on", True)
    assert off_log[3][1] == [2] and off_log[4][0] == [1]      # the scenario happened
    assert on_log == off_log                                   # poses, object_ids(), last_deleted(), volumes
    assert on_ckpt == off_ckpt and len(on_ckpt) > 1000         # not stored in a checkpoint, and nothing else moved
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
