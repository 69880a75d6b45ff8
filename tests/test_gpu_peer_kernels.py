"""The kernels of the direct peer-write exchanges, rank by rank on emulated ranks (tests/peer_emulation.py): every rank's
producer, the flags, every rank's consumer, on one stream -- no kernel ever waits for another.  Everything is compared byte
for byte: the consumers' outputs with a plain numpy restatement (float32, sums in table order and in rank order), the
receive buffers with what every sender must have stored, poison everywhere else.

Sizes (width x height) against the 64 x 4 tiles of the fused kernels and the 16-byte units of the transport:
  160 x 120  the size of every other sharded test          164 x 77   ragged against every tile, area % 4 == 0
  161 x 77, 47 x 33  odd areas: slots that end in a partial unit, u64 / f32 / u8 sub-arrays at odd offsets
  17 x 130   one tile column, 33 tile rows                  5 x 3      less than one tile, less than one band
Worlds 1, 2, 3 and 8; at 47 x 33 (3 bands of 16 rows) and 5 x 3 (one band) most of 8 ranks own an empty band.
Every scenario plays four consecutive sequence numbers with fresh data and the slots poisoned in between, once with the
wait as a launch of its own (waitInFront = 1) and once inside the consumer (0), in the default and the contraction-on
library."""
import numpy as np
import pytest

from emfusion_amd import _lib, sharding
from tests.frame_scenes import ALPHA, MAXW, PRIOR, SIGMA, SPHERES, frame
from tests.parity_util import assert_parity, dev_full, to_dev, to_np
from tests.peer_emulation import KEY_POISON, NAN_POISON, SEQUENCES, PeerEmulation
from tests.scenes import Pose, camera_path, intrinsics, rel_CO, rel_OC, rot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


@pytest.fixture(params=["", "_fma"], ids=["default", "fma"])
def lib(request, ops):
    """ops.* through libemf_hip.so, then through libemf_hip_fma.so (a * b + c contraction on)."""
    plain = ops._L
    if request.param:
        ops._L = _lib.load_variant(request.param)
    try:
        yield request.param
    finally:
        ops._L = plain


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at byte {int(bad[0])} of {got.nbytes}")


def raises_code(code, call, *args, **kwargs):
    with pytest.raises(_lib.EmfHipError) as e:
        call(*args, **kwargs)
    assert e.value.code == code, e.value
    return str(e.value)


# ---- 1. the E-step's exchange ----------------------------------------------------------------------------------------
# (size, world, maps per rank -- the background's included --, pad_cols of points / objSum / norm)
ESTEP_CASES = [((160, 120), 2, (2, 16), 0),
               ((164, 77), 3, (2, 1, 16), 0),
               ((161, 77), 2, (16, 2), 3),
               ((47, 33), 3, (1, 2, 2), 0),
               ((47, 33), 8, (2, 1, 1, 2, 1, 16, 1, 2), 0),
               ((17, 130), 2, (2, 2), 5),
               ((5, 3), 2, (2, 1), 0),
               ((5, 3), 8, (1, 2, 1, 2, 2, 1, 2, 16), 1),
               ((160, 120), 1, (2,), 0)]


class Volumes:
    """A 32^3 background and three small objects after two integrated frames, on the device."""
    SPECS = [((32, 32, 32), 0.08, Pose(t=[0, 0, 1.28]), 0),
             ((24, 20, 16), 0.03, Pose(t=SPHERES[0][0]), 1),
             ((16, 16, 16), 0.035, Pose(rot([0, 1, 0], 7), SPHERES[1][0]), 2),
             ((12, 16, 20), 0.04, Pose(rot([1, 0, 0], -5), SPHERES[0][0]), 1)]

    def __init__(self, ops, size):
        w, h = size
        self.size, self.K = size, intrinsics(w, h)
        self.vols = []
        for res, vox, pose, sphere in self.SPECS:
            shape = (res[2], res[1], res[0])
            v = dict(vox=np.float32(vox), trunc=np.float32(10) * np.float32(vox), pose=pose, tsdf=dev_full(shape, 0.0),
                     wts=dev_full(shape, 0.0), probs=None, vmask=None)
            fgbg = dev_full(shape + (2,), 0.0) if sphere else None
            for i in range(2):
                cam, depth, ids = frame(size, i)
                oc = rel_OC(cam, pose)
                ops.update_tsdf(to_dev(depth), dev_full((h, w), 1.0), v["tsdf"], v["wts"], oc.R32, oc.t32, self.K, float(v["vox"]),
                                float(v["trunc"]), MAXW)
                if sphere:
                    ops.update_fgbg_probs(to_dev((ids == sphere).astype(np.uint8)), dev_full((h, w), 0, np.uint8), v["tsdf"],
                                          v["wts"], fgbg, oc.R32, oc.t32, self.K, float(v["vox"]))
            if sphere:
                v["probs"], v["vmask"] = dev_full(shape, 0.0), dev_full(shape, 0, np.uint8)
                ops.compute_fg_probs(fgbg, v["probs"], v["vmask"])
            self.vols.append(v)
        # what the E-step never touches, but a table entry must name
        self.unused = (dev_full((h, w), 0.0), dev_full((h, w, 3), 0.0), dev_full((h, w, 3), 0.0), dev_full((h, w), 0, np.uint8))


_volumes = {}


def volumes(ops, size):
    if size not in _volumes:
        plain, ops._L = ops._L, _lib.load()  # the volumes are the same whichever library a test then runs
        try:
            _volumes[size] = Volumes(ops, size)
        finally:
            ops._L = plain
    return _volumes[size]


class RankTable:
    """The model table of one rank: the background replica and nmaps - 1 objects, one association map each.  A long table
    lists ONE small object many times, each entry at a pose of its own (as the ragged tracker test fills its table)."""

    def __init__(self, ops, vs, rank, nmaps):
        w, h = vs.size
        self.which = [0] + [1 + (rank + (k if nmaps <= 3 else 0)) % 3 for k in range(nmaps - 1)]
        self.shift = [np.zeros(3)] + [np.array([0.01 * k, -0.004 * k, 0.002 * k]) for k in range(nmaps - 1)]
        self.maps = [dev_full((h, w), 7.0) for _ in self.which]
        entries = []
        for k, (m, a) in enumerate(zip(self.which, self.maps)):
            v = vs.vols[m]
            entries.append(ops.make_model(v["tsdf"], v["wts"], a, *vs.unused, float(v["vox"]), float(v["trunc"]), MAXW, SIGMA,
                                          ALPHA, PRIOR, model_id=k, fg_probs=v["probs"], fg_mask=v["vmask"],
                                          rcp_voxel=ops.voxel_reciprocal(v["vox"])))
        self.table = ops.upload_models(entries)
        self.vs = vs

    def poses(self, cam):
        out = []
        for m, d in zip(self.which, self.shift):
            p = self.vs.vols[m]["pose"]
            co = rel_CO(cam, Pose(p.R, np.asarray(p.t, np.float64) + d))
            out.append((co.R32, co.t32))
        return out

    def poison(self):
        for a in self.maps:
            a.copy_from(np.full(a.shape, 7, np.float32))


def estep_reference(ops, tables, seq, size, pad):
    """Points and poses of sequence `seq`; every rank's un-normalised maps from ops.estep_batched(normalize=False), which the
    batched tests pin to the oracle; then, in float32 numpy: every rank's partial (table-order sum of its object maps), e (the
    partials in rank order), s = bg + e and every map as where(s != 0, v / s, 0)."""
    w, h = size
    cam = camera_path(4 + seq)
    points = dev_full((h, w, 3), 0.0, pad_cols=pad)
    ops.compute_points(to_dev(frame(size, 2 + seq)[1]), intrinsics(w, h), points)
    poses, raw, partials = [], [], []
    for t in tables:
        poses.append(t.poses(cam))
        t.poison()
        ops.estep_batched(t.table, poses[-1], points, normalize=False)
        raw.append([to_np(a) for a in t.maps])
        part = np.zeros((h, w), np.float32)
        if len(raw[-1]) > 1:
            part = raw[-1][1].copy()
            for v in raw[-1][2:]:
                part = part + v
        partials.append(part)
    e = partials[0].copy()
    for p in partials[1:]:
        e = e + p
    want = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for maps in raw:
            s = maps[0] + e
            want.append(dict(norm=s, maps=[np.where(s != 0, v / s, np.float32(0)).astype(np.float32) for v in maps]))
    assert all(np.isfinite(p).all() for p in partials) and float(e.max()) > 0, "degenerate scene"
    return dict(points=points, poses=poses, raw=raw, partials=partials, e=e, want=want)


def check_estep_outputs(tables, outs, ref, what):
    for r, t in enumerate(tables):
        for k, a in enumerate(t.maps):
            same_bytes(to_np(a), ref["want"][r]["maps"][k], f"{what}: map {k} of rank {r}")
        same_bytes(to_np(outs[r][0]), ref["e"], f"{what}: objSum of rank {r}")
        same_bytes(to_np(outs[r][1]), ref["want"][r]["norm"], f"{what}: norm of rank {r}")


@pytest.mark.parametrize("size,world,nmaps,pad", ESTEP_CASES,
                         ids=[f"{s[0]}x{s[1]}-w{w}-{'_'.join(map(str, n))}" for s, w, n, _ in ESTEP_CASES])
def test_estep_exchange_on_emulated_ranks(ops, dev, lib, size, world, nmaps, pad):
    w, h = size
    vs = volumes(ops, size)
    tables = [RankTable(ops, vs, r, nmaps[r]) for r in range(world)]
    refs = {seq: estep_reference(ops, tables, seq, size, pad) for seq in SEQUENCES}
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, world, w * h * 4, wait_in_front, NAN_POISON)
        for seq in SEQUENCES:
            ref = refs[seq]
            emu.poison()
            outs = [(dev_full((h, w), 5.0, pad_cols=pad), dev_full((h, w), 5.0, pad_cols=pad)) for _ in tables]
            for r, t in enumerate(tables):
                t.poison()
                emu.expect(seq, r, ref["partials"][r])  # a rank that owns nothing contributes exact zeros
            emu.play(seq,
                     lambda r, g: ops.estep_batched_peer(tables[r].table, ref["poses"][r], ref["points"], g, seq),
                     lambda r, g: ops.peer_normalize_association(g, seq, tables[r].maps, outs[r][0], outs[r][1]))
            check_estep_outputs(tables, outs, ref, f"waitInFront {wait_in_front}, sequence {seq}")


def test_a_seventeenth_map_is_refused_by_the_fused_normalisation(ops, dev, lib):
    """17 maps exceed the kernel's table (kNormMaps = 16): EMF_E_LIMIT, nothing launched -- slots, flags and images keep
    their poison.  (The host classes send such a rank down the unfused route: the mixed-protocol test below.)"""
    w, h = 47, 33
    maps = [dev_full((h, w), 7.0) for _ in range(17)]
    obj_sum, norm = dev_full((h, w), 5.0), dev_full((h, w), 5.0)
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, 2, w * h * 4, wait_in_front, NAN_POISON)
        msg = raises_code(_lib.EMF_E_LIMIT, ops.peer_normalize_association, emu.groups[1], 1, maps, obj_sum, norm)
        assert "17 maps" in msg
        emu.check_guards("behind the refusal")
        emu.check_slots("behind the refusal")
        assert all((to_np(a) == 7).all() for a in maps) and (to_np(obj_sum) == 5).all() and (to_np(norm) == 5).all()


@pytest.mark.parametrize("size", [(160, 120), (164, 77)], ids=["160x120", "164x77"])
def test_mixed_estep_protocols_under_one_sequence_number(ops, dev, lib, size):
    """Thirty-one objects on two ranks: rank 0 holds 17 maps and runs the UNFUSED sequence (estep_batched with obj_sum,
    peer_scatter, peerWaitReduceSumF32, normalize_association with the reduced sum), rank 1 holds 16 and runs the fused
    pair, under the same sequence number (EMFusion::estepSharded chooses by the rank's own map count).  Both put a dense
    float partial at offset 0 of their slot and both signal once and wait once: both must end with the reference's bytes."""
    w, h = size
    vs = volumes(ops, size)
    tables = [RankTable(ops, vs, 0, 17), RankTable(ops, vs, 1, 16)]
    pad = 3 if size == (164, 77) else 0  # pitched points and norm at 164 x 77 (the exchanged sum itself is dense)
    refs = {seq: estep_reference(ops, tables, seq, size, pad) for seq in SEQUENCES}
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, 2, w * h * 4, wait_in_front, NAN_POISON)
        for seq in SEQUENCES:
            ref = refs[seq]
            emu.poison()
            outs = [(dev_full((h, w), 5.0), dev_full((h, w), 5.0, pad_cols=pad)) for _ in tables]
            for r, t in enumerate(tables):
                t.poison()
                emu.expect(seq, r, ref["partials"][r])

            def producer(r, g):
                if r == 0:
                    ops.estep_batched(tables[0].table, ref["poses"][0], ref["points"], normalize=False, obj_sum=outs[0][0])
                    ops.peer_scatter(g, outs[0][0], w * h * 4, 0, seq)
                else:
                    ops.estep_batched_peer(tables[1].table, ref["poses"][1], ref["points"], g, seq)

            def consumer(r, g):
                if r == 0:
                    ops.peer_reduce_sum_f32(g, seq, w * h, outs[0][0], wait=True)
                    ops.normalize_association(tables[0].maps, extra_sum=outs[0][0], norm=outs[0][1], nsum=1)
                else:
                    ops.peer_normalize_association(g, seq, tables[1].maps, outs[1][0], outs[1][1])

            emu.play(seq, producer, consumer)
            check_estep_outputs(tables, outs, ref, f"waitInFront {wait_in_front}, sequence {seq}")


# ---- 2. the raycast's exchange ---------------------------------------------------------------------------------------
# (size, world, objects, pad_cols of every image, slot guard: 0 = slotBytes == emf_hip_peerRaycastSlotBytes exactly)
RAYCAST_CASES = [((160, 120), 2, 5, 0, 0),
                 ((164, 77), 3, 7, 5, 256),
                 ((161, 77), 2, 5, 0, 0),
                 ((47, 33), 3, 4, 0, 0),
                 ((47, 33), 8, 9, 3, 0),    # bands of 16 rows: ranks 3..7 own none
                 ((17, 130), 3, 5, 0, 256),
                 ((5, 3), 2, 4, 0, 0),
                 ((5, 3), 8, 3, 1, 0),      # one band: ranks 1..7 own none, ranks 3..7 no object either
                 ((160, 120), 1, 3, 0, 0)]


def raycast_scene(size, nobj, seed):
    """tests/test_gpu_multirank.py's _scene at a given size: random hits, ties across ranks."""
    w, h = size
    rng = np.random.default_rng(seed)
    ids = list(range(1, nobj + 1))
    hit = [(rng.random((h, w)) < 0.3).astype(np.uint8) for _ in ids]
    ray = [(rng.uniform(0.5, 3, (h, w)).astype(np.float32) * s) for s in hit]
    top = min(20, (h + 1) // 2)
    if nobj >= 4:
        ray[3][:top], hit[3][:top] = ray[0][:top], hit[0][:top]  # ties across ranks (ids 1 and 4)
    if nobj >= 2:
        ray[1][h - top:], hit[1][h - top:] = ray[0][h - top:], hit[0][h - top:]  # ... and between ranks 0 and 1 in any world
    vert = [rng.standard_normal((h, w, 3)).astype(np.float32) for _ in ids]
    nrm = [rng.standard_normal((h, w, 3)).astype(np.float32) for _ in ids]
    bg_mask = (rng.random((h, w)) < 0.8).astype(np.uint8)
    bg_ray = rng.uniform(0.5, 3, (h, w)).astype(np.float32) * bg_mask
    bg_vert = rng.standard_normal((h, w, 3)).astype(np.float32)
    bg_norm = rng.standard_normal((h, w, 3)).astype(np.float32)
    diff0 = (rng.uniform(-1, 1, (h, w)) * (rng.random((h, w)) < 0.3)).astype(np.float32)
    return dict(ids=ids, hit=hit, ray=ray, vert=vert, nrm=nrm, bg_mask=bg_mask, bg_ray=bg_ray, bg_vert=bg_vert, bg_norm=bg_norm,
                diff0=diff0)


def band_of(rank, world, h):
    """(rows per rank, first row, rows) as EMFusion::compositeAcrossRanks passes them; sharding.bg_band where non-empty."""
    per_rank = (((h + 15) // 16 + world - 1) // world) * 16  # Communicator.hpp bgBandRows
    row0 = min(rank * per_rank, h)
    rows = min(per_rank, h - row0)
    r0, n = sharding.bg_band(rank, world, h)
    assert n == rows and (n == 0 or r0 == row0)
    return per_rank, row0, rows


def raycast_reference(oracle, size, world, nobj, seq, boundary):
    w, h = size
    sc = raycast_scene(size, nobj, 1000 * seq + 7 * w + h + nobj)
    diff = sc["diff0"].copy()
    ray, vert, nrm, seg, no_obj, vis = oracle.composite_raycast(sc["ids"], sc["ray"], sc["vert"], sc["nrm"], sc["hit"], sc["bg_ray"],
                                                                sc["bg_vert"], sc["bg_norm"], sc["bg_mask"], diff, boundary)
    sc.update(w_ray=ray, w_vert=vert, w_nrm=nrm, w_seg=seg, w_noobj=no_obj, w_vis=np.asarray(vis), w_diff=diff)
    sc["pos"] = {i: k for k, i in enumerate(sc["ids"])}
    sc["mine"] = [sharding.local_objects(sc["ids"], r, world) for r in range(world)]
    sc["keys"] = [sharding.pack_hit_keys([sc["ray"][sc["pos"][i]] for i in mine], [sc["hit"][sc["pos"][i]] for i in mine],
                                         [sc["pos"][i] for i in mine]) if mine else np.full((h, w), sharding.NO_HIT, np.uint64)
                  for mine in sc["mine"]]
    return sc


class RaycastRank:
    """What one rank brings to the raycast's exchange: its objects' images, the background raycast with only its own band
    filled in (every other row poisoned), and poisoned outputs."""

    def __init__(self, sc, rank, world, size, pad):
        w, h = size
        d = lambda a: to_dev(a, pad_cols=pad)
        self.lp = [sc["pos"][i] for i in sc["mine"][rank]]
        self.obj_ray, self.obj_seg = [d(sc["ray"][p]) for p in self.lp], [d(sc["hit"][p]) for p in self.lp]
        self.obj_vert, self.obj_nrm = [d(sc["vert"][p]) for p in self.lp], [d(sc["nrm"][p]) for p in self.lp]
        self.per_rank, self.row0, self.rows = band_of(rank, world, h)
        bg_ray, bg_mask = np.full((h, w), 9, np.float32), np.full((h, w), 9, np.uint8)
        bg_ray[self.row0:self.row0 + self.rows] = sc["bg_ray"][self.row0:self.row0 + self.rows]
        bg_mask[self.row0:self.row0 + self.rows] = sc["bg_mask"][self.row0:self.row0 + self.rows]
        self.bg_ray, self.bg_mask, self.bg_vert, self.bg_norm = d(bg_ray), d(bg_mask), d(sc["bg_vert"]), d(sc["bg_norm"])
        full = lambda shape, v, t=np.float32: dev_full(shape, v, t, pad_cols=pad)
        self.ray, self.vert, self.nrm = full((h, w), 5.0), full((h, w, 3), 5.0), full((h, w, 3), 5.0)
        self.seg, self.no_obj = full((h, w), 5, np.uint8), full((h, w), 5, np.uint8)
        self.diff = d(sc["diff0"])
        self.vis = dev_full((len(sc["ids"]),), 0, np.int32)

    def pack(self, ops, g, seq):
        ops.pack_hit_keys_peer(self.lp, self.obj_ray, self.obj_seg, self.bg_ray, self.bg_mask, self.row0, self.rows, g, seq)

    def composite(self, ops, g, seq, sc, boundary):
        ops.composite_from_keys_peer(g, seq, self.per_rank, sc["ids"], self.lp, self.obj_ray, self.obj_vert, self.obj_nrm,
                                     self.bg_ray, self.bg_vert, self.bg_norm, self.bg_mask, self.ray, self.vert, self.nrm,
                                     self.seg, self.diff, self.no_obj, boundary, self.vis)

    def outputs(self):
        return [self.ray, self.vert, self.nrm, self.seg, self.no_obj, self.diff, self.bg_ray, self.bg_mask, self.vis]


def expect_raycast_slots(emu, seq, sc, ranks, size):
    w, h = size
    P = w * h
    for r, rk in enumerate(ranks):
        emu.expect(seq, r, sc["keys"][r])
        if rk.rows:
            rows = slice(rk.row0, rk.row0 + rk.rows)
            emu.expect(seq, r, sc["bg_ray"][rows], 8 * P + 4 * rk.row0 * w)
            emu.expect(seq, r, sc["bg_mask"][rows], 12 * P + rk.row0 * w)


@pytest.mark.parametrize("size,world,nobj,pad,guard", RAYCAST_CASES,
                         ids=[f"{s[0]}x{s[1]}-w{w}-n{n}" + ("-exact" if not g else "") for s, w, n, _, g in RAYCAST_CASES])
def test_raycast_exchange_on_emulated_ranks(ops, oracle, dev, lib, size, world, nobj, pad, guard):
    w, h = size
    boundary = 10 if min(w, h) >= 40 else 1
    need = ops.peer_raycast_slot_bytes(w, h)
    assert need == (13 * w * h + 15) // 16 * 16
    refs = {seq: raycast_reference(oracle, size, world, nobj, seq, boundary) for seq in SEQUENCES}
    assert any(r["w_vis"].sum() > 0 and (r["w_seg"] > 0).any() for r in refs.values())
    if world == 8:
        assert sum(band_of(r, world, h)[2] == 0 for r in range(world)) >= 5  # most ranks own no band
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, world, need, wait_in_front, KEY_POISON, slot_guard=guard)
        assert emu.slot_bytes == need + guard
        for seq in SEQUENCES:
            sc = refs[seq]
            ranks = [RaycastRank(sc, r, world, size, pad) for r in range(world)]
            emu.poison()
            expect_raycast_slots(emu, seq, sc, ranks, size)
            emu.play(seq, lambda r, g: ranks[r].pack(ops, g, seq), lambda r, g: ranks[r].composite(ops, g, seq, sc, boundary))
            for r, rk in enumerate(ranks):
                what = f"waitInFront {wait_in_front}, sequence {seq}, rank {r}"
                assert_parity(to_np(rk.seg), sc["w_seg"], f"segmentation ({what})", exact=True)
                same_bytes(to_np(rk.ray), sc["w_ray"], f"raylengths ({what})")
                assert_parity(to_np(rk.no_obj), sc["w_noobj"], f"noObj ({what})", exact=True)
                same_bytes(to_np(rk.diff), sc["w_diff"], f"diffRaylengths ({what})")
                counts = to_np(rk.vis)
                assert counts.tolist() == sc["w_vis"].tolist(), f"visibility counts ({what})"
                local_or_bg = (sc["w_seg"] == 0) | np.isin(sc["w_seg"], sc["mine"][r])
                got_v, got_n = to_np(rk.vert), to_np(rk.nrm)
                assert_parity(got_v[local_or_bg], sc["w_vert"][local_or_bg], f"vertices ({what})", exact=True)
                assert_parity(got_n[local_or_bg], sc["w_nrm"][local_or_bg], f"normals ({what})", exact=True)
                assert np.all(got_v[~local_or_bg] == 0) and np.all(got_n[~local_or_bg] == 0), f"remote winners ({what})"
                same_bytes(to_np(rk.bg_ray), sc["bg_ray"], f"background raylengths, all bands ({what})")
                same_bytes(to_np(rk.bg_mask), sc["bg_mask"], f"background mask, all bands ({what})")
                # the gate from the counts: flags as visibility_flags_indexed gives them, the counts mirrored, then cleared
                thresh = int(np.median(sc["w_vis"]))
                index = [0] + rk.lp
                want_flags = dev_full((len(index),), -1, np.int32)
                ops.visibility_flags_indexed(to_dev(counts), index, thresh, want_flags)
                flags, mirror = dev_full((len(index),), -1, np.int32), dev_full((nobj,), -1, np.int32)
                ops.visibility_flags_mirror(rk.vis, nobj, index, thresh, flags, mirror)
                assert to_np(flags).tolist() == to_np(want_flags).tolist() == [1] + [int(sc["w_vis"][p] > thresh) for p in rk.lp]
                assert to_np(mirror).tolist() == sc["w_vis"].tolist() and not to_np(rk.vis).any(), what


@pytest.mark.parametrize("size,world", [((161, 77), 2), ((164, 77), 3), ((5, 3), 2)], ids=["161x77", "164x77", "5x3"])
def test_raycast_slots_one_unit_short_are_refused(ops, oracle, dev, lib, size, world):
    """slotBytes one 16-byte unit below emf_hip_peerRaycastSlotBytes: both entries return EMF_E_ARG and launch nothing."""
    w, h = size
    need = ops.peer_raycast_slot_bytes(w, h)
    sc = raycast_reference(oracle, size, world, 3, 1, 1)
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, world, need - 16, wait_in_front, KEY_POISON, slot_guard=0)
        assert emu.slot_bytes == need - 16
        for r in range(world):
            rk = RaycastRank(sc, r, world, size, 0)
            before = [to_np(a) for a in rk.outputs()]
            assert "needs" in raises_code(_lib.EMF_E_ARG, rk.pack, ops, emu.groups[r], 1)
            assert "needs" in raises_code(_lib.EMF_E_ARG, rk.composite, ops, emu.groups[r], 1, sc, 1)
            for a, b in zip(rk.outputs(), before):
                same_bytes(to_np(a), b, "an output of a refused call")
        emu.check_guards("behind the refusals")
        emu.check_slots("behind the refusals")


# ---- 3. the exchanges on their own -----------------------------------------------------------------------------------
# element counts: one 16-byte unit; not a multiple of the grid stride; more units than the 2048-workgroup grid covers in one
# pass (2048 x 256 lanes: 524288 float4 units, and twice over for the u64 pairs)
STANDALONE_CASES = [(4, 3), (4, 8), (4100, 3), (4100, 8), (4100, 1), (1024 * 2048 + 4, 2)]


def consume(ops, wait_in_front, g, seq, fused_wait, run):
    """The two-launch form (peerWait*: run(wait=True)) or the three-launch form (peerSignalWait, then the plain consumer)."""
    if fused_wait:
        run(True)
    else:
        ops.peer_signal_wait(g, seq)
        run(False)


@pytest.mark.parametrize("n,world", STANDALONE_CASES, ids=[f"n{n}-w{w}" for n, w in STANDALONE_CASES])
def test_reductions_on_emulated_ranks(ops, dev, lib, n, world):
    rng = np.random.default_rng(n + world)
    sequences = SEQUENCES if n < 1 << 20 else SEQUENCES[:3]  # (the large buffers: three sequences still use both parities)
    for wait_in_front in (1, 0):
        sums = PeerEmulation(ops, world, n * 4, wait_in_front, NAN_POISON)
        mins = PeerEmulation(ops, world, n * 8, wait_in_front, KEY_POISON)
        for seq in sequences:
            f = [(rng.standard_normal(n) * 10.0 ** int(rng.integers(-3, 4))).astype(np.float32) for _ in range(world)]
            k = [rng.integers(0, 2 ** 63, n, dtype=np.uint64) for _ in range(world)]
            want_f = f[0].copy()
            for r in range(1, world):
                want_f = want_f + f[r]  # rank order, float32
            want_k = np.minimum.reduce(k)
            d_f, d_k = [to_dev(a) for a in f], [to_dev(a) for a in k]
            out_f, out_k = [dev_full((n,), 5.0) for _ in f], [dev_full((n,), 5, np.uint64) for _ in k]
            fused = seq % 2 == 1  # both forms meet both producer orders; in place (as the communicator) in the fused form
            for emu, data in ((sums, f), (mins, k)):
                emu.poison()
                for r in range(world):
                    emu.expect(seq, r, data[r])
            sums.play(seq, lambda r, g: ops.peer_scatter(g, d_f[r], n * 4, 0, seq),
                      lambda r, g: consume(ops, wait_in_front, g, seq, fused, lambda wait: ops.peer_reduce_sum_f32(
                          g, seq, n, d_f[r] if fused else out_f[r], wait=wait)))
            mins.play(seq, lambda r, g: ops.peer_scatter(g, d_k[r], n * 8, 0, seq),
                      lambda r, g: consume(ops, wait_in_front, g, seq, fused, lambda wait: ops.peer_reduce_min_u64(
                          g, seq, n, d_k[r] if fused else out_k[r], wait=wait)))
            for r in range(world):
                same_bytes(to_np(d_f[r] if fused else out_f[r]), want_f, f"sum, sequence {seq}, rank {r}")
                same_bytes(to_np(d_k[r] if fused else out_k[r]), want_k, f"min, sequence {seq}, rank {r}")


@pytest.mark.parametrize("n,world", STANDALONE_CASES, ids=[f"n{n}-w{w}" for n, w in STANDALONE_CASES])
def test_copies_on_emulated_ranks(ops, dev, lib, n, world):
    """peer_copy_from_slot (a broadcast of rank seq % world's buffer) and the multi-part wait-copy (a gather of the ranks'
    parts of an array, split at 16-byte units; with few units most parts are empty)."""
    rng = np.random.default_rng(7 * n + world)
    units = n // 4
    cuts = [units * r // world * 4 for r in range(world + 1)]  # element bounds of the ranks' parts
    sequences = SEQUENCES if n < 1 << 20 else SEQUENCES[:2]  # (two exchanges each: four sequence numbers, both parities twice)
    for wait_in_front in (1, 0):
        emu = PeerEmulation(ops, world, n * 4, wait_in_front, NAN_POISON)
        for seq in sequences:
            data = [rng.standard_normal(n).astype(np.float32) for _ in range(world)]
            # (a) broadcast from the root's slot, three launches
            root = seq % world
            d, out = [to_dev(a) for a in data], [dev_full((n,), 5.0) for _ in data]
            emu.poison()
            emu.expect(2 * seq - 1, root, data[root])
            emu.play(2 * seq - 1, lambda r, g: ops.peer_scatter(g, d[r], n * 4, 0, 2 * seq - 1) if r == root else None,
                     lambda r, g: (ops.peer_signal_wait(g, 2 * seq - 1),
                                   ops.peer_copy_from_slot(g, 2 * seq - 1, root, 0, out[r], n * 4)))
            for r in range(world):
                same_bytes(to_np(out[r]), data[root], f"copy from the slot of rank {root}, sequence {2 * seq - 1}, rank {r}")
            # (b) every rank scatters its part to the part's own offset; one launch waits and copies the others' parts
            want = np.concatenate([data[r][cuts[r]:cuts[r + 1]] for r in range(world)])
            emu.poison()
            for r in range(world):
                emu.expect(2 * seq, r, data[r][cuts[r]:cuts[r + 1]], 4 * cuts[r])
            emu.play(2 * seq,
                     lambda r, g: ops.peer_scatter(g, d[r], 4 * (cuts[r + 1] - cuts[r]), 4 * cuts[r], 2 * seq, src_offset=4 * cuts[r]),
                     lambda r, g: ops.peer_wait_copy_from_slots(g, 2 * seq, [(p, 4 * cuts[p], d[r], 4 * cuts[p], 4 * (cuts[p + 1] - cuts[p]))
                                                                            for p in range(world) if p != r]))
            for r in range(world):
                same_bytes(to_np(d[r]), want, f"gathered parts, sequence {2 * seq}, rank {r}")


def test_standalone_rejections_leave_their_outputs_alone(ops, dev, lib):
    n = 64
    emu = PeerEmulation(ops, 2, n * 4, 1, NAN_POISON)
    g = emu.groups[0]
    src, out = dev_full((n + 64,), 1.0), dev_full((n,), 5.0)
    out64 = dev_full((n // 2,), 5, np.uint64)
    ARG, LIMIT = _lib.EMF_E_ARG, _lib.EMF_E_LIMIT
    raises_code(ARG, ops.peer_reduce_sum_f32, g, 1, 6, out)                 # float count 6
    raises_code(ARG, ops.peer_reduce_sum_f32, g, 1, 6, out, wait=True)
    raises_code(ARG, ops.peer_reduce_min_u64, g, 1, 3, out64)               # odd u64 count
    raises_code(ARG, ops.peer_reduce_min_u64, g, 1, 3, out64, wait=True)
    raises_code(ARG, ops.peer_scatter, g, src, 16, 8, 1)                    # offset 8
    raises_code(ARG, ops.peer_copy_from_slot, g, 1, 1, 8, out, 16)
    raises_code(ARG, ops.peer_wait_copy_from_slots, g, 1, [(1, 8, out, 0, 16)])
    raises_code(ARG, ops.peer_scatter, g, src, emu.slot_bytes + 16, 0, 1)   # message larger than the slot
    raises_code(ARG, ops.peer_reduce_sum_f32, g, 1, emu.slot_bytes // 4 + 4, out)
    raises_code(ARG, ops.peer_copy_from_slot, g, 1, 1, emu.slot_bytes - 16, out, 32)
    raises_code(LIMIT, ops.peer_wait_copy_from_slots, g, 1, [(1, 0, out, 0, 16)] * 17)  # 17 copy parts
    emu.check_guards("behind the rejections")
    emu.check_slots("behind the rejections")
    assert (to_np(out) == 5).all() and (to_np(out64) == 5).all() and (to_np(src) == 1).all()
