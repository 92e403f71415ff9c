"""Frame intervals on the device: k_predict_prepare with dt a kernel argument through ekf_predict_dt,
ekf_set_frame_interval and ekf_set_staged_intervals, and the look-ahead k_camera_ahead through ekf_predict_camera_ahead -- PER ENTRY
against tests/predict_dt_ref.py (numpy, np.longdouble; bounds derived there, not measured), and bit for bit against the paths that
must not change: dt = 1 is the engine that was never told an interval, a step over the set interval is the stage calls over it, a
staged table is the setter called before every step, the look-ahead is the corner a prediction over tau leaves.

The sizes are predict_ref.COV_SIZES' reasons: m = n - 13 = 3 the smallest map (one strip workgroup with three threads at work),
258 a strip that crosses into a second workgroup, 768 a last workgroup that is exactly full.  The tests print the worst
|device - reference| / tolerance per output, as tests/test_gpu_prediction_stages.py does."""
import numpy as np
import pytest

import predict_dt_ref as pdr
import predict_ref as pr
from openekfmonoslam_amd.ekftypes import DESC_BYTES, KEYPOINT_DTYPE
from openekfmonoslam_amd.synth import SyntheticSequence

pytestmark = pytest.mark.gpu

F64, F32, F32_EXACT, F64_EXACT = 0, 1, 2, 3
ALL_PRECISIONS = [F64, F32, F32_EXACT, F64_EXACT]
EKF_ERR_INVALID_ARG = 1
BAD_INTERVALS = [0.0, -1.0, float("nan"), float("inf")]


def p_is_f32(precision):
    return precision in (F32, F32_EXACT)


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def make_engine(eng_mod, s, precision, x13=None):
    e = eng_mod.EkfEngine(s.cam, s.par, s.n_features + 8, max_keypoints=64, precision=precision)
    e.set_state(s.x13 if x13 is None else x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    return e


def report(what, precision, n, dt, dev, ref, tol):
    r, at = pr.worst_ratio(dev, ref, tol)
    print(f"prediction over dt: {what:13s} precision {precision} n {n:5d} dt {dt:4.2f}: worst |dev - ref| / tol = {r:.3f} at {at}")
    return r, at


def assert_states_equal(a, b, msg=""):
    for name, u, v in zip(("x13", "feature_pos", "P"), a, b):
        np.testing.assert_array_equal(u, v, err_msg=f"{msg} {name}")


def _check_prediction_over_dt(e, s, precision, dt):
    """e holds any state: predict(dt) from it, every output per entry against the reference evaluated on what get_state() returned"""
    x1, f1, P1 = e.get_state()
    e.predict(dt=dt)
    x2, f2, P2 = e.get_state()
    ref = pdr.predict_cov_ref(x1, P1, s.par, dt, pr.U32 if p_is_f32(precision) else 0.0)
    bad = []
    for name, got, (want, tol) in (("x13", x2, pdr.state_ref(x1, dt)), ("corner", P2[:13, :13], ref["corner"]),
                                   ("row strip", P2[:13, 13:], ref["row strip"]), ("column strip", P2[13:, :13], ref["column strip"])):
        r, at = report(name, precision, s.n, dt, got, want, tol)
        if not (r <= 1.0):  # (a NaN is a failure)
            bad.append((name, r, at))
    assert not bad, bad
    np.testing.assert_array_equal(x2[7:13], x1[7:13])  # v and w are carried over
    np.testing.assert_array_equal(f2, f1)
    np.testing.assert_array_equal(P2[13:, 13:], P1[13:, 13:])  # the untouched block: bit for bit
    np.testing.assert_array_equal(P2, P2.T)
    return (x1, P1), (x2, P2)


# ------------------------------------------------------------------------------------------------ 1. per entry
@pytest.mark.parametrize("precision", ALL_PRECISIONS)
@pytest.mark.parametrize("m", [3, 258, 768])
@pytest.mark.parametrize("dt", [0.37, 2.5])
def test_prediction_over_dt_per_entry(eng_mod, dt, m, precision):
    s = pr.scene_for_n(13 + m)
    e = make_engine(eng_mod, s, precision)
    e.predict()  # (as the stage tests: strips that a prediction has already mixed)
    (_, P1), (_, P2) = _check_prediction_over_dt(e, s, precision, dt)
    assert np.abs(P2[:13, 13:] - P1[:13, 13:]).max() > 0  # (the strips did change)
    assert e.frame_interval() == 1.0  # predict(dt) leaves the set interval alone


# ------------------------------------------------------------------------------------------------ 2. threshold branches
@pytest.mark.parametrize("w,dt,q_moves", [((0.0, 0.0, 0.0), 2.5, False), ((3e-16, 0.0, 0.0), 0.5, False), ((1.5e-16, 0.0, 0.0), 2.5, True)],
                         ids=["w-zero-dt-2.5", "w-dt-below-w-above", "w-below-w-dt-above"])
def test_small_angle_branches(eng_mod, w, dt, q_moves):
    """exact w = 0 over a long interval, and the two combinations of the small-angle tests a dt != 1 makes reachable
    (tests/test_predict_dt_ref_cpu.py pins what the reference does in each): |w dt| < eps <= |w_x| -- the quaternion is carried
    over bit for bit while F keeps its angular-velocity diagonal and its Qm D block -- and |w_i| < eps <= |w dt| -- the quaternion
    turns while that diagonal and the quaternion block of G are zero.  The wrong branch misses the corner by a diagonal entry of
    P or by a whole G Q G' block, many orders above the tolerance."""
    s = pr.scene_for_n(13 + 3)
    x = np.array(s.x13, dtype=np.float64)
    x[10:13] = w
    e = make_engine(eng_mod, s, F64, x13=x)
    (x1, _), (x2, _) = _check_prediction_over_dt(e, s, F64, dt)
    np.testing.assert_array_equal(x1, x)
    assert (x2[3:7] != x1[3:7]).any() == q_moves


# ------------------------------------------------------------------------------------------------ 3. dt = 1 is today's path
@pytest.mark.parametrize("precision", [F64, F32_EXACT])
def test_unit_interval_is_the_plain_prediction(eng_mod, precision):
    s = pr.scene_for_n(13 + 258)
    plain, by_arg, by_set = (make_engine(eng_mod, s, precision) for _ in range(3))
    by_set.set_frame_interval(1.0)
    for _ in range(2):  # (twice: the second prediction starts from strips the first has mixed)
        plain.predict()
        by_arg.predict(dt=1.0)
        by_set.predict()
        want = plain.get_state()
        assert_states_equal(by_arg.get_state(), want, "predict(dt=1.0)")
        assert_states_equal(by_set.get_state(), want, "set_frame_interval(1.0) + predict()")
    assert by_set.frame_interval() == 1.0


# ------------------------------------------------------------------------------------------------ 4. the set interval reaches the step
@pytest.mark.parametrize("precision", [F64, F32_EXACT])
def test_step_predicts_over_the_set_interval(eng_mod, precision):
    """test_step_prediction_equals_stage_calls (tests/test_gpu_prediction_stages.py) over dt = 2.5 at N = 257: k_predict_cov_features
    with two workgroups of features, fused (counts on the device) and kept (counts on the host, the stage kernels), against a twin's
    predict(dt=2.5) + predict_measurements(), bit for bit.  The frame has no keypoints: nothing is matched, nothing updated."""
    N, dt = 257, 2.5
    s = pr.xyz_scene(N)
    kps, desc = np.zeros(0, dtype=KEYPOINT_DTYPE), np.zeros((0, DESC_BYTES), dtype=np.uint8)
    fused, kept, staged, unit = (make_engine(eng_mod, s, precision) for _ in range(4))
    kept.keep_step_predictions(True)
    for e in (fused, kept):
        e.set_frame_interval(dt)
        assert e.frame_interval() == dt
    infos = [fused.step(kps, desc), kept.step(kps, desc)]
    staged.predict(dt=dt)
    want, _, _ = staged.predict_measurements()
    idx = want["featureIndex"]
    assert len(idx) > 0
    every = np.arange(N, dtype=np.int32)
    ref_state = staged.get_state()
    HPs, HPcs = staged.hp_rows(every)
    for name, e, info in (("fused", fused, infos[0]), ("kept", kept, infos[1])):
        assert (info.n_predicted, info.n_matches, info.status) == (len(idx), 0, 0), name
        assert_states_equal(e.get_state(), ref_state, name)
        np.testing.assert_array_equal(e.unseen_features(), staged.unseen_features(), err_msg=name)
        HP, HPc = e.hp_rows(every)
        np.testing.assert_array_equal(HP, HPs, err_msg=name)
        np.testing.assert_array_equal(HPc, HPcs, err_msg=name)
    got = kept.step_predictions()
    np.testing.assert_array_equal(got["featureIndex"], idx)
    np.testing.assert_array_equal(got["imagePos"], want["imagePos"])
    np.testing.assert_array_equal(got["covarianceMatrix"], want["covarianceMatrix"])
    unit.predict()  # (and the interval mattered: a unit prediction leaves another state)
    assert np.abs(unit.get_state()[0][:3] - ref_state[0][:3]).max() > 0


# ------------------------------------------------------------------------------------------------ 5. staged intervals
def test_staged_intervals_equal_the_setter_before_every_step(eng_mod):
    """three staged frames with their own intervals, and a fourth beyond the table that falls back to the set interval, against a
    twin that is told the interval before every step on the same frames: x, the features and P bit for bit after every frame"""
    seq = SyntheticSequence(50, 4)
    assert len(seq.frames) >= 4
    table, fallback = [1.0, 0.5, 2.0], 1.5

    def engine():
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=F64)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        e.set_sweep_mode(4)  # bitwise run-to-run comparisons need the launch-per-panel sweep
        return e

    staged, twin, unit = engine(), engine(), engine()
    staged.upload_frames(seq.frames[:4])
    unit.upload_frames(seq.frames[:4])
    staged.set_frame_interval(fallback)
    staged.set_staged_intervals(table)
    assert staged.frame_interval() == fallback  # the table is its own thing
    for t in range(4):
        dt = table[t] if t < len(table) else fallback
        twin.set_frame_interval(dt)
        a, b = staged.step_frame(t), twin.step(*seq.frames[t])
        assert (a.n_predicted, a.n_matches, a.n_inliers, a.n_rescued, a.status) == (b.n_predicted, b.n_matches, b.n_inliers, b.n_rescued, b.status), t
        assert_states_equal(staged.get_state(), twin.get_state(), f"frame {t}")
        unit.step_frame(t)
        if t == 0:  # dt[0] = 1: the engine without a table
            assert_states_equal(staged.get_state(), unit.get_state(), "frame 0")
    assert np.abs(staged.get_state()[0] - unit.get_state()[0]).max() > 0  # (the other intervals mattered)
    staged.set_staged_intervals([])  # cleared: frame 1 of a fresh run would use the set interval
    staged.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    twin.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    twin.set_frame_interval(fallback)
    staged.step_frame(1)
    twin.step(*seq.frames[1])
    assert_states_equal(staged.get_state(), twin.get_state(), "cleared table")


# ------------------------------------------------------------------------------------------------ 6. look-ahead
@pytest.mark.parametrize("precision", ALL_PRECISIONS)
@pytest.mark.parametrize("m", [3, 258])
@pytest.mark.parametrize("tau", [0.37, 2.5])
def test_camera_ahead(eng_mod, tau, m, precision):
    s = pr.scene_for_n(13 + m)
    e, twin = make_engine(eng_mod, s, precision), make_engine(eng_mod, s, precision)
    for eng in (e, twin):
        eng.predict()
    before = e.get_state()
    x_a, P_a = e.camera_ahead(tau)
    assert_states_equal(e.get_state(), before, "camera_ahead wrote the filter:")
    x0, _, P0 = before
    (x_ref, x_tol), (c_ref, c_tol) = pdr.camera_ahead_ref(x0, P0, s.par, tau)
    bad = []
    for name, got, want, tol in (("ahead x13", x_a, x_ref, x_tol), ("ahead corner", P_a, c_ref, c_tol)):
        r, at = report(name, precision, s.n, tau, got, want, tol)
        if not (r <= 1.0):
            bad.append((name, r, at))
    assert not bad, bad
    np.testing.assert_array_equal(P_a, P_a.T)
    twin.predict(dt=tau)
    x_t, _, P_t = twin.get_state()
    np.testing.assert_array_equal(x_a, x_t)
    if p_is_f32(precision):  # the prediction rounds the same fp64 value to the storage type of P
        np.testing.assert_array_equal(P_a.astype(np.float32), P_t[:13, :13].astype(np.float32))
        assert (P_a != P_t[:13, :13]).any()  # (the look-ahead itself is not rounded)
    else:
        np.testing.assert_array_equal(P_a, P_t[:13, :13])
    x_b, P_b = e.camera_ahead(tau)  # asking twice changes nothing
    np.testing.assert_array_equal(x_b, x_a)
    np.testing.assert_array_equal(P_b, P_a)


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("bad", BAD_INTERVALS, ids=["zero", "negative", "nan", "inf"])
def test_bad_intervals_are_refused(eng_mod, bad):
    s = pr.scene_for_n(13 + 3)
    e = make_engine(eng_mod, s, F64)
    e.set_frame_interval(1.25)
    before = e.get_state()
    calls = (("set_frame_interval", lambda: e.set_frame_interval(bad)), ("predict", lambda: e.predict(dt=bad)),
             ("camera_ahead", lambda: e.camera_ahead(bad)), ("set_staged_intervals", lambda: e.set_staged_intervals([1.0, bad, 2.0])))
    for name, call in calls:
        with pytest.raises(eng_mod.EkfError) as err:
            call()
        assert err.value.code == EKF_ERR_INVALID_ARG, name
        assert "interval" in str(err.value), (name, str(err.value))
        assert_states_equal(e.get_state(), before, name)
        assert e.frame_interval() == 1.25, name
    e.predict()  # and the engine still predicts over the interval it had
    twin = make_engine(eng_mod, s, F64)
    twin.predict(dt=1.25)
    assert_states_equal(e.get_state(), twin.get_state(), "after the refusals")
