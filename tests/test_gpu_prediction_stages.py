"""Stage tests of the prediction (csrc/kernels_predict.hip): k_predict_prepare, k_predict_cov<T>, k_predict_cov_features<T>,
k_predict_features, k_compact and k_hp_rows<T, TO> with the compaction that rides in it, through the C ABI, PER ENTRY against
tests/predict_ref.py (numpy, np.longdouble) in all four precisions, at the sizes where the launches change shape.

Every bound is derived, not measured (predict_ref.py: u_store |ref| + K u64 sum|terms|, K counted from the kernel's operations);
the tests print the worst |device - reference| / tolerance per output so that the margin is on record (DESIGN.md lists what the
MI355X gave).  tests/test_predict_ref_cpu.py holds the reference equal to the oracle within the same bounds and checks the
input conditions assumed here: sizes reached with both feature types, the visibility pattern around every wavefront, workgroup
and 1024 boundary, >= 1 px between every feature and every threshold of the visibility test.
"""
import numpy as np
import pytest

import predict_ref as pr
from openekfmonoslam_amd.ekftypes import DESC_BYTES, KEYPOINT_DTYPE

pytestmark = pytest.mark.gpu

F64, F32, F32_EXACT, F64_EXACT = 0, 1, 2, 3
ALL_PRECISIONS = [F64, F32, F32_EXACT, F64_EXACT]


def p_is_f32(precision):
    return precision in (F32, F32_EXACT)


def hp_is_f32(precision):  # F32_EXACT keeps P in fp32 and the row pairs in fp64
    return precision == F32


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def make_engine(eng_mod, s, precision, x13=None):
    e = eng_mod.EkfEngine(s.cam, s.par, s.n_features + 8, max_keypoints=64, precision=precision)
    P0 = s.P0 if s.P0 is not None else np.zeros((s.n, s.n))
    e.set_state(s.x13 if x13 is None else x13, s.feature_pos, s.feature_type, s.desc, P0)
    return e


def report(what, precision, n, dev, ref, tol):
    r, at = pr.worst_ratio(dev, ref, tol)
    print(f"prediction stages: {what:13s} precision {precision} n {n:5d}: worst |dev - ref| / tol = {r:.3f} at {at}")
    return r, at


# ------------------------------------------------------------------------------------------------ a. covariance prediction
def _check_covariance_prediction(eng_mod, s, precision):
    e = make_engine(eng_mod, s, precision)
    e.predict()
    x1, _, P1 = e.get_state()
    e.predict()
    _, _, P2 = e.get_state()
    ref = pr.predict_cov_ref(x1, P1, s.par, pr.U32 if p_is_f32(precision) else 0.0)
    bad = []
    for name, got in (("corner", P2[:13, :13]), ("row strip", P2[:13, 13:]), ("column strip", P2[13:, :13])):
        r, at = report(name, precision, s.n, got, *ref[name])
        if not (r <= 1.0):  # (a NaN is a failure)
            bad.append((name, r, at))
    assert not bad, bad
    np.testing.assert_array_equal(P2[13:, 13:], P1[13:, 13:])  # the untouched block: bit for bit
    np.testing.assert_array_equal(P2, P2.T)  # both strips are the same products in the same order; the corner is mirrored
    assert np.abs(P2[:13, 13:] - P1[:13, 13:]).max() > 0  # (the strips did change)


@pytest.mark.parametrize("precision", ALL_PRECISIONS)
@pytest.mark.parametrize("m", pr.COV_SIZES)
def test_covariance_prediction_per_entry(eng_mod, m, precision):
    """n - 13 = m columns in the strips: 255 fills one strip workgroup but for one thread, 258 puts two threads into the second,
    513 one into the third, 768 fills the third to its last thread (columns n-3 .. n-1 belong to its last three threads)."""
    _check_covariance_prediction(eng_mod, pr.scene_for_n(13 + m), precision)


def test_covariance_prediction_zero_angular_velocity(eng_mod):
    """the |w| < eps branch of F and G (no quaternion-by-omega block, zeroed omega diagonal), fp32 storage"""
    _check_covariance_prediction(eng_mod, pr.scene_for_n(13 + 258, omega_zero=True), F32)


# ------------------------------------------------------------------------------------------------ b. row pairs, S, HPc
HP_CASES = [(n, p) for p in (F64, F64_EXACT) for n in pr.HP_SIZES_F64] + [(n, p) for p in (F32, F32_EXACT) for n in pr.HP_SIZES_F32]


@pytest.mark.parametrize("n,precision", HP_CASES)
def test_row_pairs_S_and_camera_columns_per_entry(eng_mod, n, precision):
    """fp64 P: 2 columns per lane, 512 per chunk; fp32 P: 4 and 1024.  1021 leaves one valid lane in the tail, 1024 is a full last
    vector, 1027 / 1030 put 3 columns / a full vector and 2 into a second chunk; 511 / 514 the same for fp64.

    Rows of features the prediction does not reach must not be written.  They are poisoned first: a measurement prediction from
    the scene's poison pose (same position, turned 52 degrees) sees every feature the real pose does not see; the values it leaves
    in their rows -- and in their HPc columns -- are what those rows must still hold, bit for bit, after the real prediction."""
    s = pr.scene_for_n(n)
    N = s.n_features
    every = np.arange(N, dtype=np.int32)
    e = make_engine(eng_mod, s, precision, x13=s.x_poison)
    pp, _, _ = e.predict_measurements()
    unseen = np.nonzero(~s.vis)[0]
    assert np.isin(unseen, pp["featureIndex"]).all()
    HP0, HPc0 = (a.copy() for a in e.hp_rows(every))
    assert (np.abs(HP0[unseen]).max(axis=(1, 2)) > 0).all() and (np.abs(HPc0[unseen]).max(axis=(1, 2)) > 0).all()

    e.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    e.predict()
    _, _, P1 = e.get_state()
    preds, Hs, Hf = e.predict_measurements()
    idx = preds["featureIndex"]
    np.testing.assert_array_equal(idx, np.nonzero(s.vis)[0])
    HP, HPc = e.hp_rows(every)
    (rHP, tHP), (rHPc, tHPc), (rS, tS) = pr.hp_ref(P1, Hs, Hf, idx, s.feature_type, s.covpos, pr.U32 if hp_is_f32(precision) else 0.0)
    bad = []
    for name, got, ref, tol in (("HP", HP[idx], rHP, tHP), ("HPc", HPc[idx], rHPc, tHPc), ("S", preds["covarianceMatrix"], rS, tS)):
        r, at = report(name, precision, n, got, ref, tol)
        if not (r <= 1.0):  # (a NaN is a failure)
            bad.append((name, r, at))
    assert not bad, bad
    if not hp_is_f32(precision):  # the camera columns are the same fp64 values as the row pairs' first 13 columns
        np.testing.assert_array_equal(HPc[idx], HP[idx][:, :, :13])
    np.testing.assert_array_equal(HP[unseen], HP0[unseen])
    np.testing.assert_array_equal(HPc[unseen], HPc0[unseen])


# ------------------------------------------------------------------------------------------------ c. lists
def _oracle_list(ol, s, idx=None):
    o = ol.Oracle(s.cam, s.par, s.n_features + 8)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, np.zeros((s.n, s.n)))
    o.predict()
    if idx is not None:
        return o.predict_measurements(idx)[0]["featureIndex"]
    return o.predict_measurement_state(o.x13(), o.rotation(), o.feature_pos())["featureIndex"]


@pytest.mark.parametrize("N", pr.LIST_SIZES)
def test_full_prediction_list(eng_mod, oracle_lib, N):
    """256 / 257: compaction in the launch of k_predict_features / a separate k_compact; 1025: k_compact with two items per thread"""
    s = pr.xyz_scene(N, with_P0=False)
    e = make_engine(eng_mod, s, F64)
    e.predict()
    np.testing.assert_array_equal(e.unseen_features(), np.arange(N))  # nothing has been predicted yet
    got = e.predict_measurements()[0]["featureIndex"]
    want = _oracle_list(oracle_lib, s)
    np.testing.assert_array_equal(want, np.nonzero(s.vis)[0])
    assert len(got) == len(want)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(e.unseen_features(), np.nonzero(~s.vis)[0])


@pytest.mark.parametrize("count", [256, 257])
def test_subset_and_state_only_lists(eng_mod, oracle_lib, count):
    """a permuted index list of 256 / 257 of a map of 300, and predict_measurement_state on a map of 256 / 257: the oracle's list in
    the oracle's order; neither touches the list of unseen features (which, before any full prediction, is the whole map: a subset
    prediction that wrote it would shorten it)"""
    s = pr.xyz_scene(300, with_P0=False)
    idx = np.random.default_rng(count).permutation(300)[:count].astype(np.int32)
    assert 0 < s.vis[idx].sum() < count
    e = make_engine(eng_mod, s, F64)
    e.predict()
    got = e.predict_measurements(idx)[0]["featureIndex"]
    want = _oracle_list(oracle_lib, s, idx)
    np.testing.assert_array_equal(want, idx[s.vis[idx]])
    assert len(got) == len(want)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(e.unseen_features(), np.arange(300))

    s = pr.xyz_scene(count, with_P0=False)
    e = make_engine(eng_mod, s, F64)
    e.predict()
    ps = e.predict_measurement_state()
    want = _oracle_list(oracle_lib, s)
    assert len(ps) == len(want)
    np.testing.assert_array_equal(ps["featureIndex"], want)
    np.testing.assert_array_equal(e.unseen_features(), np.arange(count))
    full = e.predict_measurements()[0]
    np.testing.assert_array_equal(full["featureIndex"], want)
    np.testing.assert_array_equal(ps["imagePos"], full["imagePos"])
    np.testing.assert_array_equal(e.unseen_features(), np.nonzero(~s.vis)[0])
    e.predict_measurement_state()
    e.predict_measurements(np.nonzero(~s.vis)[0][:5].astype(np.int32))
    np.testing.assert_array_equal(e.unseen_features(), np.nonzero(~s.vis)[0])


# ------------------------------------------------------------------------------------------------ d. the step's fused path
@pytest.mark.parametrize("precision", [F64, F32_EXACT])
@pytest.mark.parametrize("N", pr.FUSED_SIZES)
def test_step_prediction_equals_stage_calls(eng_mod, N, precision):
    """EKF::step's prediction -- k_predict_cov_features, and above 256 features the compaction as one more workgroup of k_hp_rows
    (2 and 5 flags per thread at 257 and 1025) -- against ekf_predict + ekf_predict_measurements on the same state, bit for bit.
    The frame has no keypoints: nothing is matched, nothing updated (S and the row pairs are formed before the matcher runs).

    ekf_keep_step_predictions makes a step count its predictions on the host, and that path launches the STAGE kernels; so one
    engine steps without it (the fused launches: state, P, row pairs, unseen list and counters are compared) and one with it
    (imagePos and S of the step's predictions are compared)."""
    s = pr.xyz_scene(N)
    kps, desc = np.zeros(0, dtype=KEYPOINT_DTYPE), np.zeros((0, DESC_BYTES), dtype=np.uint8)
    fused, kept, staged = (make_engine(eng_mod, s, precision) for _ in range(3))
    kept.keep_step_predictions(True)
    infos = [fused.step(kps, desc), kept.step(kps, desc)]
    staged.predict()
    want, _, _ = staged.predict_measurements()
    idx = want["featureIndex"]
    np.testing.assert_array_equal(idx, np.nonzero(s.vis)[0])
    every = np.arange(N, dtype=np.int32)
    xs, fs, Ps = staged.get_state()
    HPs, HPcs = staged.hp_rows(every)
    assert (np.abs(HPs[idx]).max(axis=(1, 2)) > 0).all()
    for name, e, info in (("fused", fused, infos[0]), ("kept", kept, infos[1])):
        assert (info.n_predicted, info.n_matches, info.status) == (len(idx), 0, 0), name
        x, f, P = e.get_state()
        np.testing.assert_array_equal(x, xs, err_msg=name)
        np.testing.assert_array_equal(f, fs, err_msg=name)
        np.testing.assert_array_equal(P, Ps, err_msg=name)
        np.testing.assert_array_equal(e.unseen_features(), staged.unseen_features(), err_msg=name)
        HP, HPc = e.hp_rows(every)
        np.testing.assert_array_equal(HP, HPs, err_msg=name)
        np.testing.assert_array_equal(HPc, HPcs, err_msg=name)
        tp = e.get_map_features()[1]
        np.testing.assert_array_equal(tp, s.vis.astype(np.uint32), err_msg=name)  # one more for exactly the predicted features
    assert (staged.get_map_features()[1] == 0).all()
    got = kept.step_predictions()
    np.testing.assert_array_equal(got["featureIndex"], idx)
    np.testing.assert_array_equal(got["imagePos"], want["imagePos"])
    np.testing.assert_array_equal(got["covarianceMatrix"], want["covarianceMatrix"])
    assert (want["covarianceMatrix"][:, 0] > 1.0).all()  # (S was formed: I plus something)
