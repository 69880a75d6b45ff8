"""The sharded pipeline at its edges, rehearsed once each on threads of one GPU after the kernels involved have passed rank by
rank on emulated ranks (tests/test_gpu_peer_kernels.py):

  * thirty-one objects on two ranks: rank 0 holds 17 association maps and takes the unfused E-step, rank 1 holds 16 and takes
    the fused one, under the same sequence numbers (EMFusion::estepSharded chooses by the rank's own count, DESIGN.md
    section 7).  The peer transport must equal the host-staged one bit for bit;
  * ragged image sizes: 164 x 77 (area % 4 == 0) on both transports, 161 x 77 (odd area) on the host-staged transport, against
    the single-GPU run with the bounds of tests/test_gpu_rehearsal.py;
  * 161 x 77 on the peer transport: refused when the communicator is attached, on every rank, before any exchange
    (DESIGN.md section 3).

As in tests/test_gpu_peer_exchange.py every scenario runs in a child process of its own with that file's environment, rank
threads are joined with a time-out, the child has a time-out, and nothing is retried."""
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tests.test_gpu_peer_exchange import ENV  # noqa: E402

pytestmark = pytest.mark.gpu

JOIN_S = 240
IMAGES = ("seg", "ray", "bg_ray", "bg_assoc", "bg_tsdf", "bg_w")


def same_results(a, b, what):
    """Two runs of run_job / _boundary_job, rank by rank: every image, the background volume and every object volume."""
    for r, (x, y) in enumerate(zip(a, b)):
        assert x["mine"] == y["mine"] and x["vis"] == y["vis"], (what, r)
        for k in IMAGES:
            assert x[k].tobytes() == y[k].tobytes(), (what, r, k)
        for i in x["mine"]:
            for u, v in zip(x["obj"][i], y["obj"][i]):
                assert u.tobytes() == v.tobytes(), (what, r, i)


# ---- 1. the 16-map boundary ------------------------------------------------------------------------------------------

def _boundary_job(transport):
    """31 objects on 2 ranks as tests/test_gpu_sharded_lifecycle.py::test_uneven_ownership_many_objects builds its scene:
    80 x 60, a 32^3 background, 8^3 objects, 3 frames."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    from tests.parity_util import to_dev
    W, H, world, nobj = 80, 60, 2, 31
    prm = pipeline.make_params(W, H, 32, 0.08, 8, visibility_thresh=20, boundary=2)
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 1, seed=0xE3F5)
    frames = [(synth.render(f)[0],) + tuple(synth.camera_pose(f)) for f in range(3)]
    centre = synth.sphere(0, 0)[0]
    synth.close()
    rng = np.random.default_rng(7)
    centres = [centre + rng.uniform(-0.2, 0.2, 3).astype(np.float32) for _ in range(nobj)]
    comms = pipeline.Communicator.local_group(world, transport, W * H * 16)
    out, errors = [None] * world, []
    ready = threading.Barrier(world)

    def rank_main(r):
        try:
            fus = pipeline.Fusion(prm, comms[r])
            ids = [fus.add_object(c, 0.4) for c in centres]
            mine = [i for i in ids if fus.owns_object(i)]
            keep, per_frame, before = [], [], comms[r].exchanges()
            ready.wait(timeout=JOIN_S)
            for depth, R, t in frames:
                d = to_dev(depth)
                keep.append(d)
                fus.process_frame(image_view(d), R, t, {}, {}, False)
                fus.synchronize()
                per_frame.append(comms[r].exchanges() - before)
                before = comms[r].exchanges()
            out[r] = dict(mine=mine, maps=1 + len(mine), per_frame=per_frame, alive=fus.object_ids(),
                          seg=fus.image("segmentation"), ray=fus.image("raylengths"), bg_ray=fus.image("bg_raylengths"),
                          bg_assoc=fus.image("bg_assoc"), bg_tsdf=fus.volume("tsdf", 0), bg_w=fus.volume("weights", 0),
                          vis=sorted(fus.visible_objects()),
                          obj={i: (fus.volume("tsdf", i), fus.volume("weights", i), fus.image("obj_assoc", i)) for i in mine})
            fus.close()
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((r, repr(e)))
            ready.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=JOIN_S)
    assert not any(th.is_alive() for th in threads), "a rank hangs"
    assert not errors, errors
    for c in comms:
        c.close()
    return out


def _boundary_scenario(_):
    from emfusion_amd import devmem
    devmem.set_device(0)
    host, peer = _boundary_job("host"), _boundary_job("peer")
    for ranks in (host, peer):
        assert [r["maps"] for r in ranks] == [17, 16]  # first of all: the two protocols really do meet
        assert len(ranks[0]["alive"]) == 31 and ranks[0]["alive"] == ranks[1]["alive"]
        # (frame 0 has no E-step and no raycast: it exchanges nothing)
        assert ranks[0]["per_frame"] == ranks[1]["per_frame"] and all(n > 0 for n in ranks[0]["per_frame"][1:]), ranks[0]["per_frame"]
        for k in IMAGES:
            assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), k
    same_results(peer, host, "peer against host-staged")
    assert (host[0]["bg_assoc"] < 1).any(), "the objects take no part in the normaliser: nothing was exchanged"
    print("SCENARIO_OK boundary 0")


# ---- 2. ragged sizes ---------------------------------------------------------------------------------------------------

def _sizes_scenario(which):
    import tests.test_gpu_rehearsal as reh
    from emfusion_amd import devmem
    devmem.set_device(0)
    size, world, peer_too = {1642: ((164, 77), 2, True), 1643: ((164, 77), 3, True), 1612: ((161, 77), 2, False)}[which]
    nobj = 4
    single = reh.run_job(1, nobj, False, size=size)[0]
    host = reh.run_job(world, nobj, False, size=size)
    reh.check_against_single(host, single, nobj, world)
    if peer_too:
        peer = reh.run_job(world, nobj, False, size=size, transport="peer")
        same_results(peer, host, "peer against host-staged")
        assert len({r["exchanges"] for r in peer}) == 1 and peer[0]["exchanges"] > 0
    print("SCENARIO_OK sizes", which)


# ---- 3. the refusal ----------------------------------------------------------------------------------------------------

def _refusal_scenario(_):
    from emfusion_amd import devmem, pipeline
    devmem.set_device(0)

    def attach(size, world, bytes_per_pixel=16):
        """Every rank's attempt to attach a peer communicator to a session of `size`: (error code, message) per rank.
        16 bytes per pixel hold the fused raycast exchange, 8 only the hit keys: such a session exchanges unfused."""
        w, h = size
        prm = pipeline.make_params(w, h, 32, 0.08, 8)
        comms = pipeline.Communicator.local_group(world, "peer", w * h * bytes_per_pixel)
        got = [None] * world

        def rank_main(r):
            try:
                pipeline.Fusion(prm, comms[r]).close()
                got[r] = (0, "")
            except pipeline.FusionError as e:
                got[r] = (e.code, str(e))
        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=JOIN_S)
        assert not any(th.is_alive() for th in threads), "a rank hangs"
        assert all(c.exchanges() == 0 for c in comms)  # refused or not: attaching exchanges nothing
        for c in comms:
            c.close()
        return got

    for world in (2, 3):
        got = attach((161, 77), world)
        assert all(code == -2 for code, _ in got), got  # EMF_E_SHAPE, the same on every rank
        assert all("width * height % 4 == 0" in msg and "161 x 77" in msg for _, msg in got), got
    assert all(code == 0 for code, _ in attach((164, 77), 2))
    # the unfused collectives move the bands of the u8 hit mask: whole units only if width * height % 16 == 0
    got = attach((164, 77), 2, bytes_per_pixel=8)
    assert all(code == -2 and "width * height % 16 == 0" in msg for code, msg in got), got
    assert all(code == 0 for code, _ in attach((160, 120), 2, bytes_per_pixel=8))
    print("SCENARIO_OK refusal 0")


SCENARIOS = {"boundary": _boundary_scenario, "sizes": _sizes_scenario, "refusal": _refusal_scenario}


def _in_own_process(what, arg=0):
    run = subprocess.run([sys.executable, str(Path(__file__).resolve()), what, str(arg)], cwd=ROOT,
                         env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and f"SCENARIO_OK {what} {arg}" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]


def test_seventeen_and_sixteen_maps_meet_under_one_sequence_number(dev):
    _in_own_process("boundary")


@pytest.mark.parametrize("which", [1642, 1643, 1612], ids=["164x77-w2-host-peer", "164x77-w3-host-peer", "161x77-w2-host"])
def test_sharded_job_at_ragged_sizes(dev, which):
    _in_own_process("sizes", which)


def test_peer_communicator_refuses_a_session_it_cannot_serve(dev):
    _in_own_process("refusal")


if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](int(sys.argv[2]))
