"""The follow policy (pipeline.follow_shift = emf_fusion_follow_shift): a pure function of floats that
needs no device.  Per axis shift_i = trunc(q_i / (float(step_i) * voxel)) * step_i, in single precision, for the
followed point q in the background's frame."""
import numpy as np
import pytest

from emfusion_amd import pipeline

VOX = 0.01
STEP = (64, 64, 64)  # a cell of 0.64 m


def test_inside_the_dead_zone_nothing_moves():
    assert pipeline.follow_shift((0.0, 0.0, 0.0), STEP, VOX) == (0, 0, 0)
    assert pipeline.follow_shift((0.63, -0.63, 0.3), STEP, VOX) == (0, 0, 0)
    assert pipeline.follow_shift((-0.0, 1e-30, -1e-30), STEP, VOX) == (0, 0, 0)


def test_exactly_on_a_boundary():
    # a voxel size and steps that are exact in binary: the boundary itself belongs to the next cell, on both sides
    vox, step = 1.0 / 64, (64, 32, 8)  # cells of 1, 0.5, 0.125 m
    assert pipeline.follow_shift((1.0, 0.5, 0.125), step, vox) == (64, 32, 8)
    assert pipeline.follow_shift((-1.0, -0.5, -0.125), step, vox) == (-64, -32, -8)
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert pipeline.follow_shift((below, -below / 2, below / 8), step, vox) == (0, 0, 0)


def test_beyond_two_steps_negative_coordinates_and_mixed_axes():
    assert pipeline.follow_shift((1.5, 0.0, 0.0), STEP, VOX) == (128, 0, 0)
    assert pipeline.follow_shift((-2.0, 0.0, 0.0), STEP, VOX) == (-192, 0, 0)
    assert pipeline.follow_shift((0.7, -0.1, -1.3), STEP, VOX) == (64, 0, -128)
    # per-axis steps: cells of 0.32, 0.08 and 0.16 m
    assert pipeline.follow_shift((0.33, -0.17, 0.15), (32, 8, 16), VOX) == (32, -16, 0)


@pytest.mark.parametrize("step", [(48, 64, 64), (64, 12, 64), (64, 64, 4), (0, 8, 8), (-32, 8, 8), (32, 8, 0)])
def test_steps_that_are_not_positive_tile_multiples_are_refused(step):
    with pytest.raises(pipeline.FusionError) as err:
        pipeline.follow_shift((0.1, 0.2, 0.3), step, VOX)
    assert err.value.code == -4  # EMF_E_ARG


def test_bad_voxel_sizes_and_points_are_refused():
    for q, vox in (((0.0, 0.0, 0.0), 0.0), ((0.0, 0.0, 0.0), -0.01), ((np.nan, 0.0, 0.0), VOX), ((0.0, np.inf, 0.0), VOX)):
        with pytest.raises(pipeline.FusionError):
            pipeline.follow_shift(q, STEP, vox)


def test_result_is_a_step_multiple_and_brings_the_point_back():
    rng = np.random.default_rng(0xF0110)
    steps = [(32, 8, 8), (64, 64, 64), (96, 24, 40), (32, 64, 8)]
    for n in range(400):
        step = steps[n % len(steps)]
        vox = np.float32((0.004, 0.01, 0.02)[n % 3])
        q = rng.uniform(-6.0, 6.0, 3).astype(np.float32)
        k = pipeline.follow_shift(q, step, float(vox))
        for i in range(3):
            assert k[i] % step[i] == 0
            cell = np.float64(np.float32(step[i]) * vox)
            # after the roll the point sits at q - k * voxel in the new frame: inside one cell of the centre
            assert abs(np.float64(q[i]) - k[i] * np.float64(vox)) < cell, (q, step, vox, k)
            assert k[i] == 0 or np.sign(k[i]) == np.sign(q[i])  # towards the point, never past the centre
