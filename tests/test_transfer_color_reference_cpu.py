"""tests/transfer_color_reference.py against itself (include/emf_hip.h "Absorbing a volume" and "Lifting a volume",
DESIGN.md 5.31): the vectorised statements of the colour rules and the loops agree byte for byte on the cases the GPU test
runs (the loops over at most 12 x 6 x 5 voxels of each case's box), with the count identities; the sweep the GPU test runs
reaches every kind of voxel the rules tell apart; identity pose, equal lattices and an unobserved destination copy the
source's coloured entries with Wc capped; a second seed and a second release change no colour byte; a constant colour
absorbed into the same constant colour stays, whatever the weights; the weight cap; pipeline.absorbed_line and
pipeline.lifted_line round-trip an event with its colour counts."""
import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import lift_reference as lr
from tests import shape_reference as sr
from tests import transfer_color_reference as tc

f32 = np.float32


def loop_box(box, limit=(12, 6, 5)):
    lo, size = box
    return lo, tuple(min(s, m) for s, m in zip(size, limit))


def unchanged_outside(color, dst, box, name):
    lo, size = box
    keep = np.ones(dst["tsdf"].shape, bool)
    keep[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = False
    assert color[keep].tobytes() == dst["color"][keep].tobytes(), name


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_of_the_absorption_agree(shape, content):
    for name, dst, src, pose, box in tc.absorb_cases(shape, content):
        box = loop_box(box)
        a, b = tc.absorb_color(dst, src, pose, box), tc.absorb_color_loop(dst, src, pose, box)
        assert a[3].tobytes() == b[0].tobytes() and a[4].tobytes() == b[1].tobytes(), (name, a[4], b[1])
        tc.check_identities(a[2], a[4], "fused")
        unchanged_outside(a[3], dst, box, name)
        assert int((a[3] != dst["color"]).any(axis=3).sum()) <= a[2]["fused"], name
        if src["color"] is None:
            assert a[4]["colored"] == 0, name


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_of_the_seed_agree(shape, content):
    for name, dst, src, pose, box in tc.seed_cases(shape, content):
        box = loop_box(box)
        a, b = tc.seed_color(dst, src, pose, box), tc.seed_color_loop(dst, src, pose, box)
        assert a[3].tobytes() == b[0].tobytes() and a[4].tobytes() == b[1].tobytes(), (name, a[4], b[1])
        tc.check_identities(a[2], a[4], "seeded")
        unchanged_outside(a[3], dst, box, name)
        with np.errstate(invalid="ignore"):
            had = dst["weights"] > 0
        assert a[3][had].tobytes() == dst["color"][had].tobytes(), name  # KEPT: the entry is not touched
        # a second seed finds its voxels KEPT and changes no colour byte
        again = tc.seed_color(dict(dst, tsdf=a[0], weights=a[1], color=a[3]), src, pose, box)
        assert again[3].tobytes() == a[3].tobytes() and again[4].tobytes() == tc.moved().tobytes(), name


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_of_the_release_agree(shape, content):
    for name, dst, claim, pose, box in tc.release_cases(shape, content):
        box = loop_box(box)
        a, b = tc.release_color(dst, claim, pose, box), tc.release_color_loop(dst, claim, pose, box)
        assert a[3].tobytes() == b[0].tobytes() and a[4].tobytes() == b[1].tobytes(), (name, a[4], b[1])
        tc.check_identities(a[2], a[4], "released")
        unchanged_outside(a[3], dst, box, name)
        gone = a[1].view(np.uint32) != dst["weights"].view(np.uint32)  # a released weight was > 0 and is +0.0
        assert not a[3][gone].any() and a[3][~gone].tobytes() == dst["color"][~gone].tobytes(), name
        again = tc.release_color(dict(dst, tsdf=a[0], weights=a[1], color=a[3]), claim, pose, box)
        assert again[3].tobytes() == a[3].tobytes() and again[4].tobytes() == tc.moved().tobytes(), name


def test_the_planted_wall_under_the_three_ratios():
    box = ((6, 2, 1), (18, 9, 6))
    for name, ratio, dst, src, pose in tc.planted_cases():
        for vec, loop, which in ((tc.absorb_color, tc.absorb_color_loop, "fused"), (tc.seed_color, tc.seed_color_loop, "seeded")):
            a, b = vec(dst, src, pose, box), loop(dst, src, pose, box)
            assert a[3].tobytes() == b[0].tobytes() and a[4].tobytes() == b[1].tobytes(), (name, which)
            full = vec(dst, src, pose)
            tc.check_identities(full[2], full[4], which)
            assert full[2][which] > 0, (name, which)


def test_the_sweep_reaches_every_kind_of_voxel():
    """Over all cases the GPU test runs (tests/test_gpu_transfer_color.py: the same generators, whole boxes as they come)
    the restatement meets each kind of voxel the rules tell apart; otherwise that test proves less than it claims."""
    absorb, seed, release = {}, {}, {}
    for shape in ar.SHAPES:
        for content in sr.CONTENTS:
            for _, dst, src, pose, box in tc.absorb_cases(shape, content):
                tc.absorb_color(dst, src, pose, box, kinds=absorb)
            for _, dst, src, pose, box in tc.seed_cases(shape, content):
                tc.seed_color(dst, src, pose, box, kinds=seed)
            for _, dst, claim, pose, box in tc.release_cases(shape, content):
                tc.release_color(dst, claim, pose, box, kinds=release)
    for kinds, names in ((absorb, tc.ABSORB_KINDS), (seed, tc.SEED_KINDS), (release, tc.RELEASE_KINDS)):
        for name in names:
            assert kinds.get(name, 0) > 0, (name, kinds)


def test_identity_copies_the_coloured_entries_with_the_weight_capped():
    """Identity pose, equal lattices, equal truncation, an unobserved destination: every fused (seeded) voxel holds the
    source's entry with Wc capped where the source is coloured and (0, 0, 0, 0) where it is not; nothing else changes."""
    shape = (33, 17, 9)
    st, sw, _ = sr.volume(shape, "half_shell")
    dt, dw, _ = sr.volume(shape, "unobserved")
    for max_weight, capq in ((64.0, 16384), (10.0, 2560), (300.0, 65535), (0.001, 1)):
        assert tc.capq_of(max_weight) == capq
        dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, max_weight), color=tc.color_volume(shape, "hostile", 3))
        src = dict(ar.src_vol(st, sw, None, 0.01, 0.04), color=tc.color_volume(shape, "weighted", 4, 65535))
        for statement, which in ((tc.absorb_color, "fused"), (tc.seed_color, "seeded")):
            tsdf, weights, rec, color, crec = statement(dst, src, ar.pose_of())
            changed = weights.view(np.uint32) != dw.view(np.uint32)
            assert rec[which] == changed.sum() > 50
            want = src["color"][changed].copy()
            uncolored = want[:, 3] == 0
            want[:, 3] = np.minimum(want[:, 3], capq)
            want[uncolored] = 0
            assert color[changed].tobytes() == want.tobytes() and color[~changed].tobytes() == dst["color"][~changed].tobytes()
            assert crec["uncolored"] == uncolored.sum() > 0 and crec["colored"] == (~uncolored).sum() > 0
            assert (want[:, 3] == capq).any() or capq == 65535


def test_a_constant_colour_absorbed_into_itself_stays():
    """(De * c + Sw * c + (De + Sw) / 2) / (De + Sw) == c for any weights: the running average of one colour."""
    shape = (33, 17, 9)
    st, sw, _ = sr.volume(shape, "all_solid")
    dt, dw, _ = sr.volume(shape, "random")
    dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, 64.0), color=tc.color_volume(shape, "constant", 5, 65535))
    src = dict(ar.src_vol(st, sw, None, 0.01, 0.04), color=tc.color_volume(shape, "constant", 6, 65535))
    src["color"][..., 3] = np.maximum(src["color"][..., 3], 1)
    for pose in (ar.pose_of(), ar.pose_of(None, (0.0031, 0.0047, 0.0013))):
        _, _, rec, color, crec = tc.absorb_color(dst, src, pose)
        assert rec["fused"] == crec["colored"] > 1000 and crec["uncolored"] == 0
        assert (color[..., :3] == (0x1234, 0xFFFF, 0x0001)).all()
        changed = color[..., 3] != dst["color"][..., 3]  # only weights move, and a written one is capped
        assert changed.sum() > 500 and color[..., 3][changed].max() <= 16384


def test_the_quotient_is_exact_where_64_bits_are_needed():
    """The vectorised quotient against Python integers at the corners of the u16 range."""
    edge = (0, 1, 2, 255, 256, 32767, 32768, 65534, 65535)
    for De in edge:
        for Sw in edge[1:]:
            for Dc in edge:
                for Sc in edge:
                    den = De + Sw
                    want = (De * Dc + Sw * Sc + den // 2) // den
                    a, b = De * Dc, Sw * Sc  # each below 2^32: the three 32-bit divisions of the kernel
                    assert a // den + b // den + (a % den + b % den + den // 2) // den == want <= 65535


def test_the_lines_round_trip_an_event_with_its_colour_counts():
    from emfusion_amd import pipeline
    rec, seed, rel = np.zeros((), ar.ABSORB), np.zeros((), lr.SEED), np.zeros((), lr.RELEASE)
    for k, name in enumerate(ar.COUNTS):
        rec[name] = 500 + k
    for k, name in enumerate(lr.SEED_COUNTS):
        seed[name] = 1000 + k
    for k, name in enumerate(lr.RELEASE_COUNTS):
        rel[name] = 2 ** 33 + k
    R, t = np.arange(9, dtype=f32) / 7, np.array([0.1, -1e-9, 3.0000002], f32)
    absorbed = dict(id=3, frame=9, clipped=False, R=R, t=t, lo=(1, 2, 3), size=(4, 5, 6), record=rec)
    lifted = dict(id=7, frame=12, clipped=True, seed_R=R, seed_t=t, release_R=R, release_t=-t, lo=(60, 61, 62), size=(40, 41, 42),
                  seed=seed, release=rel)
    a, b, c = tc.moved(2 ** 40 + 1, 17), tc.moved(5, 0), tc.moved(0, 2 ** 33)
    plain = pipeline.absorbed_line(absorbed)
    line = pipeline.absorbed_line(absorbed, color=a)
    assert line.startswith(plain + " ") and pipeline.absorbed_line(absorbed, color=None) == plain
    assert [int(v) for v in line.split()[-2:]] == [2 ** 40 + 1, 17] and len(line.split()) == len(plain.split()) + 2
    plain = pipeline.lifted_line(lifted)
    line = pipeline.lifted_line(lifted, color=(b, c))
    assert line.startswith(plain + " ") and pipeline.lifted_line(lifted, color=None) == plain
    assert [int(v) for v in line.split()[-4:]] == [5, 0, 0, 2 ** 33] and len(line.split()) == len(plain.split()) + 4
    from emfusion_amd import ops
    assert ops.COLOR_MOVED_DTYPE == tc.COLOR_MOVED
