"""GPU: the second update's gather / assembly launch is enqueued behind the rescue stage's partition BEFORE the host has read the
rescued count (device-count steps, step.cpp step_device_counts): its grid is sized by the outlier count and the kernel reads the count
(k_gather_assemble with d_M).  A device-count step must give what a host-count step gives (ekf_keep_step_predictions forces the
host counts, and with them the host-sized launch) bit for bit, at every size of the second update where the device-side decoding
of the grid changes.

The scenes were chosen on the CPU with the oracle's step (ALGORITHMIC variant); (n_outliers, n_rescued) per frame:

  A  SyntheticSequence(100, 5, seed=2, outlier_fraction=0.1, pixel_sigma=0.02, distractors_per_feature=0, max_bit_flips=0)
     (72, 67) (33, 22) (12, 6) (10, 0) (8, 2)   rescued counts that are no multiple of 16; outliers and NONE rescued (frame 3)
  B  SyntheticSequence(100, 5, seed=9, outlier_fraction=0.03, pixel_sigma=0.02, distractors_per_feature=0, max_bit_flips=0)
     (78, 77) (14, 11) (7, 7) (10, 4) (0, 0)    every outlier rescued (frame 2); NO outliers, no rescue stage at all (frame 4)
  C  SyntheticSequence(40, 3, seed=2)
     (31, 31) (20, 20) (19, 17)                 2 * 31 = 62 rows, just below 64; 2 * 17 = 34, just above 32
  D  SyntheticSequence(40, 3, seed=3)
     (33, 33) (16, 16) (15, 15)                 66 rows, just above 64; 32 rows exactly; 30, just below 32

The fp64 engine takes the oracle's decisions on these scenes, so the recorded counts are asserted for precision 0; in
EKF_PRECISION_F32_EXACT the two engines must agree with each other."""
import numpy as np
import pytest

from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import rel_max, state_err
from tests.oracle_lib import ALGORITHMIC
from tests.test_gpu_exact_edge_cases import EXACT, assert_parity
from tests.test_gpu_edge_cases import _same_info
from tests.test_gpu_parity import eng_mod, make_pair  # noqa: F401
from tests.test_gpu_step_counts import INFO_FIELDS

pytestmark = pytest.mark.gpu

CLEAN = dict(pixel_sigma=0.02, distractors_per_feature=0.0, max_bit_flips=0)
SCENES = {
    "A": ((100, 5), dict(seed=2, outlier_fraction=0.1, **CLEAN), [(72, 67), (33, 22), (12, 6), (10, 0), (8, 2)]),
    "B": ((100, 5), dict(seed=9, outlier_fraction=0.03, **CLEAN), [(78, 77), (14, 11), (7, 7), (10, 4), (0, 0)]),
    "C": ((40, 3), dict(seed=2), [(31, 31), (20, 20), (19, 17)]),
    "D": ((40, 3), dict(seed=3), [(33, 33), (16, 16), (15, 15)]),
}
_SEQS = {}


def sequence(name):
    if name not in _SEQS:
        args, kw, _ = SCENES[name]
        _SEQS[name] = SyntheticSequence(*args, **kw)
    return _SEQS[name]


def test_the_recorded_sizes_cover_the_cases():
    sizes = [s for _, _, per_frame in SCENES.values() for s in per_frame]
    assert any(no > 0 and nr == 0 for no, nr in sizes)
    assert any(no > 0 and nr == no for no, nr in sizes)
    assert any(no == 0 for no, nr in sizes)
    assert any(nr % 16 not in (0, 1, 15) and nr > 0 for no, nr in sizes)
    assert any((2 * nr) % 32 == 30 for no, nr in sizes) and any((2 * nr) % 32 == 2 and nr > 1 for no, nr in sizes)
    assert any(nr > 0 and (2 * nr) % 32 == 0 for no, nr in sizes)


def _engine(eng_mod, seq, precision, sweep_mode):
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    if sweep_mode is not None:
        e.set_sweep_mode(sweep_mode)
    e.upload_frames(seq.frames)
    return e


def _run_pair(eng_mod, name, precision, sweep_mode, async_errors=False):
    seq = sequence(name)
    dev, host = _engine(eng_mod, seq, precision, sweep_mode), _engine(eng_mod, seq, precision, sweep_mode)
    dev.set_async_errors(async_errors)
    host.keep_step_predictions(True)
    sizes = []
    for t in range(len(seq.frames)):
        a, b = dev.step_frame(t), host.step_frame(t)
        for f in INFO_FIELDS:
            assert getattr(a, f) == getattr(b, f), (name, t, f, getattr(a, f), getattr(b, f))
        assert a.status == 0
        sizes.append((a.n_outliers, a.n_rescued))
    dev.synchronize()
    return dev, host, sizes


@pytest.mark.parametrize("async_errors", [False, True], ids=["sync", "async"])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_count_steps_equal_host_count_steps_at_the_second_updates_sizes(eng_mod, name, precision, async_errors):
    dev, host, sizes = _run_pair(eng_mod, name, precision, 4, async_errors)  # (bitwise: the launch-per-panel sweep)
    if precision == 0:
        assert sizes == SCENES[name][2], (name, sizes)
    for u, v in zip(dev.get_state(), host.get_state()):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(dev.get_map_features(), host.get_map_features()):
        np.testing.assert_array_equal(u, v)
    dev.close()
    host.close()


def test_default_sweep_mode_agrees_to_1e_12(eng_mod):
    """the persistent sweep (the default, and what the early launch leaves the first diagonal block to) is not bitwise repeatable:
    fp64 engine, same decisions, state and covariance to 1e-12"""
    dev, host, sizes = _run_pair(eng_mod, "A", 0, None)
    assert sizes == SCENES["A"][2]
    (x, fp, P), (xh, fph, Ph) = dev.get_state(), host.get_state()
    assert state_err(x, fp, xh, fph) <= 1e-12
    assert rel_max(P, Ph) <= 1e-12
    for u, v in zip(dev.get_map_features(), host.get_map_features()):
        np.testing.assert_array_equal(u, v)
    dev.close()
    host.close()


@pytest.mark.parametrize("async_errors", [False, True], ids=["sync", "async"])
def test_stalled_first_update_behind_which_the_early_launch_ran_frozen(eng_mod, oracle_lib, async_errors):
    """ekf_debug_stall_next_sweep on the FIRST update of frame 1: the rescue stage behind it -- re-prediction, partition and the early
    gather / assembly launch -- runs frozen, the failure is seen at that stage's read-back, the update is run again and the stage
    repeated with its early launch.  Decisions, state, covariance and the map's counters are the oracle's after every frame."""
    seq = SyntheticSequence(170, 3, seed=5)
    e, o = make_pair(eng_mod, oracle_lib, seq, precision=EXACT)
    e.upload_frames(seq.frames)
    e.set_async_errors(async_errors)
    e.stall_sweep(2)  # persistent sweeps from now on: frame 0 LI, frame 0 HI, frame 1 LI
    for t in range(3):
        gi = e.step_frame(t)
        oi = o.step(*seq.frames[t], ALGORITHMIC)
        assert gi.status == 0
        _same_info(gi, oi, f"frame {t}")
        assert oi.n_inliers > 0 and oi.n_rescued > 0, "the scene must exercise both updates"
    e.synchronize()
    assert e.sweep_retries == 1, e.sweep_retries
    assert_parity(e, o, f"stalled first update, async {async_errors}", 170)
    _, tp, tm = e.get_map_features()
    _, otp, otm = o.map_features()
    assert np.array_equal(tm, otm) and np.array_equal(tp, otp)
    e.close()
