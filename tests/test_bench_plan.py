"""bench.py's frame plan (CPU only): --steps is the number of timed steps for any length of run, --warmup the number of
untimed steps before the first timed one, runs that fit the synthetic sequence are one pass as before, longer runs
repeat it from the seeded map without going past its last frame, and every run length sees the same scene."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.mark.parametrize("warmup,steps", [(5, 20), (10, 60), (2, 298), (2, 299), (0, 301), (5, 1000), (10, 20000),
                                          (150, 151), (400, 1000), (1000, 5)])
def test_frame_plan_times_exactly_the_steps_asked_for(warmup, steps):
    cap = bench.SEQ_FRAMES_MAX
    n, plan = bench.frame_plan(warmup, steps)
    assert n == min(warmup + steps, cap)
    assert all(0 <= w <= t <= n for w, t in plan)
    assert sum(t - w for w, t in plan) == steps
    first = next(i for i, (w, t) in enumerate(plan) if t > w)
    assert all(t == w for w, t in plan[:first]) and all(t > w for w, t in plan[first:])
    assert sum(w for w, _ in plan[:first]) + plan[first][0] == warmup
    if warmup + steps <= cap:
        assert plan == [(warmup, warmup + steps)]
    else:  # every timed pass replays the same warm-up frames
        assert len({w for w, _ in plan[first:]}) == 1


def test_the_synthetic_sequence_exists_at_the_plan_cap():
    from openekfmonoslam_amd.synth import SyntheticSequence

    seq = SyntheticSequence(50, bench.SEQ_FRAMES_MAX)
    assert len(seq.frames) == bench.SEQ_FRAMES_MAX


def test_every_run_length_sees_the_same_scene():
    """the parity gate and the timed frames start from the same map and frames whatever --steps is"""
    import numpy as np

    from openekfmonoslam_amd.synth import SyntheticSequence

    ref = SyntheticSequence(50, bench.frame_plan(5, 20)[0])
    for warmup, steps in ((5, 150), (10, 290), (5, 2000)):
        seq = SyntheticSequence(50, bench.frame_plan(warmup, steps)[0])
        np.testing.assert_array_equal(seq.points, ref.points)
        np.testing.assert_array_equal(seq.P0, ref.P0)
        for (k1, d1), (k2, d2) in zip(seq.frames, ref.frames):
            np.testing.assert_array_equal(k1, k2)
            np.testing.assert_array_equal(d1, d2)
