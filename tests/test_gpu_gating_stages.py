"""GPU: the three stages that decide which rows enter the covariance update -- descriptor matcher (k_match), 1-point RANSAC
(k_ransac_hyp, k_ransac_select) and outlier rescue (k_rescue) -- through the C ABI on a CONVERGED filter, against the CPU oracle and
the numpy restatement of one hypothesis (tests/ransac_ref.py).  Scenes, lists and the conditions they meet (margins of the
reference's decisions, batch edges, ties, planted thresholds, live matcher cases) are built and asserted in
tests/test_ransac_ref_cpu.py; the measured values are in its docstring.

RANSAC, per hypothesis: an engine and an oracle with ransacAllInliersProbability = 1e-9 stop behind the first hypothesis that has
support, so ekf_ransac on the list rotated by h returns hypothesis h's own support mask -- compared bit for bit with D[h] < thr of
the reference (with the reference loop on the rotated rows where the rotated list starts with unsupported hypotheses).
RANSAC, full loop: mask and hypothesis count equal the oracle's for ransac_batch in {1, 2, 3, 5, 8, 32}, on lists that end on a
launch edge, first in a launch and inside one, on rotations that hold ties of the best support, at N = 300 (512-thread launch) and
N = 420 (third launch).  A third of the features is XYZ.  Precisions 1-3 get the state with P rounded to fp32 and only decisions
the reference takes 5e-4 px or more from the threshold; equality is exact in every precision.

Reference margins (pixels, min |D - thr| over the evaluated hypotheses): N = 50 plain 9.1e-4, adversarial 3.4e-2; N = 300 plain
1.5e-3, adversarial 6.6e-3; N = 420 plain 3.6e-4, adversarial 2.6e-2.  Rescue: planted v = chi2 (1 -+ eps), eps = 1e-6 (fp64) and
1e-3 (other precisions); the outliers' own v are further from chi2 than that."""
import numpy as np
import pytest

import ransac_ref as rr
from test_ransac_ref_cpu import (BATCHES, MATCH_COUNTS, TINY_PROBABILITY, TRUNCATED, MatchScene, RescueScene, Scene, f32_rotations,
                                 tie_rotations, with_probability)

pytestmark = pytest.mark.gpu

PRECISIONS = [0, 1, 2, 3]  # F64, F32 (H P table in fp32), F32_EXACT, F64_EXACT
STEP_FIELDS = ("n_predicted", "n_matches", "n_hypotheses", "n_inliers", "n_outliers", "n_rescued", "status")


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


@pytest.fixture(scope="module")
def scenes(oracle_lib):
    cache = {}

    def get(N, p_f32=False, prob=None):
        key = (N, p_f32, prob)
        if key not in cache:
            cache[key] = Scene(oracle_lib, N, p_f32, prob)
        return cache[key]
    return get


def engine_on(eng_mod, sc, precision=0, ransac_batch=0):
    """an engine on the scene's state, predicted like the scene's oracle"""
    N = sc.seq.n_features
    e = eng_mod.EkfEngine(sc.seq.cam, sc.par, N + 8, max_keypoints=4 * N + 64, precision=precision, ransac_batch=ransac_batch)
    e.set_state(*sc.state)
    e.predict()
    pe, _, _ = e.predict_measurements()
    np.testing.assert_array_equal(pe["featureIndex"], sc.preds["featureIndex"])
    return e


def hp_dtype(precision):
    return np.float32 if precision == 1 else np.float64  # EKF_PRECISION_F32 keeps the H P table, the gain columns, in fp32


def assert_ransac_equal(e, m, mask, nh, what):
    mask_e, nh_e = e.ransac(m)
    assert nh_e == nh, (what, nh_e, nh)
    np.testing.assert_array_equal(mask_e, mask, err_msg=str(what))


# ------------------------------------------------------------------------------------------------------ RANSAC
@pytest.mark.parametrize("N,precision", [(50, p) for p in PRECISIONS] + [(300, 0)])
def test_ransac_support_mask_per_hypothesis(eng_mod, scenes, N, precision):
    sc = scenes(N, precision != 0, TINY_PROBABILITY)
    thr = sc.par.ransacThresholdPredictDistance
    e = engine_on(eng_mod, sc, precision)
    for name, m in sc.lists().items():
        M = len(m)
        D = sc.distances(m, hp_dtype(precision))
        if precision != 0:
            hs = f32_rotations(sc.distances(m), thr, TINY_PROBABILITY)
        else:
            hs = range(M) if N == 50 else np.unique(np.linspace(0, M - 1, 32).astype(int))
        own, single = rr.support(D, thr)[0], 0
        for h in hs:
            masks, counts = rr.support(rr.rotated(D, h), thr)
            mask, nh = rr.sequential_loop(counts, masks, M, TINY_PROBABILITY)
            if nh == 1:  # the mask IS hypothesis h's support, seen from the rotated list
                single += 1
                np.testing.assert_array_equal(np.roll(mask, h), own[h])
            assert_ransac_equal(e, np.roll(m, -h), mask, nh, (name, h))
        assert single >= (25 if name == "plain" else 1), (name, single)


@pytest.mark.parametrize("N,precision", [(50, p) for p in PRECISIONS] + [(300, 0)])
def test_ransac_full_loop_batch_widths(eng_mod, scenes, N, precision):
    sc = scenes(N, precision != 0)
    thr, prob = sc.par.ransacThresholdPredictDistance, sc.par.ransacAllInliersProbability
    lists = sc.lists()
    D = sc.distances(lists["plain"])
    ties = tie_rotations(D, thr, prob)
    rot = []
    if N == 50:  # rotations of the plain list: other supports, other ends of the loop, ties of the best support
        rot = [h for h in range(len(D)) if rr.margin(rr.rotated(D, h), thr, len(sc.ransac(np.roll(lists["plain"], -h))[1])) >= 5e-4]
        assert set(ties) & set(rot), (ties, rot)
    for batch in BATCHES:
        e = engine_on(eng_mod, sc, precision, batch)
        for name, m in lists.items():
            mask, counts = sc.ransac(m)
            assert_ransac_equal(e, m, mask, len(counts), (batch, name))
        for h in rot:
            m = np.roll(lists["plain"], -h)
            mask, counts = sc.ransac(m)
            assert_ransac_equal(e, m, mask, len(counts), (batch, "plain rotated", h))
        e.close()


def test_ransac_full_loop_third_launch(eng_mod, scenes):
    """N = 420, default ransac_batch: the adversarial list ends inside the launch that starts at hypothesis 288"""
    sc = scenes(420)
    e = engine_on(eng_mod, sc)
    for name, m in sc.lists().items():
        mask, counts = sc.ransac(m)
        assert name == "plain" or len(counts) > 288
        assert_ransac_equal(e, m, mask, len(counts), name)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ransac_truncated_lists(eng_mod, scenes, precision):
    """the last M matches of the adversarial list: 32 hypotheses = the first launch exactly (M = 34), one hypothesis in the second
    launch (M = 35), a single match"""
    sc = scenes(50, precision != 0)
    e = engine_on(eng_mod, sc, precision)
    adv = sc.lists()["adversarial"]
    for M in TRUNCATED:
        mask, counts = sc.ransac(adv[-M:])
        assert_ransac_equal(e, adv[-M:], mask, len(counts), M)


@pytest.mark.parametrize("N", [50, 300])
def test_step_path_batch_widths(eng_mod, oracle_lib, scenes, N):
    """EKF::step with the match count on the device launches its first batch before the host knows anything: engines with
    ransac_batch 1 and 5 (the loop continues in wide launches) step like the default one (it ends inside the first launch), bit for bit"""
    sc = scenes(N)
    frames = sc.seq.frames[sc.t : sc.t + 3]
    runs = []
    for batch in (0, 1, 5):
        e = eng_mod.EkfEngine(sc.seq.cam, sc.par, N + 8, max_keypoints=4 * N + 64, ransac_batch=batch)
        e.set_state(*sc.state)
        infos = [tuple(getattr(i, f) for f in STEP_FIELDS) for i in (e.step(k, d) for k, d in frames)]
        runs.append((infos, e.get_state()))
        e.close()
    for infos, (x, fp, P) in runs[1:]:
        assert infos == runs[0][0]
        np.testing.assert_array_equal(x, runs[0][1][0])
        np.testing.assert_array_equal(fp, runs[0][1][1])
        np.testing.assert_array_equal(P, runs[0][1][2])
    assert all(i[2] >= 2 and i[3] >= N // 4 for i in runs[0][0]), runs[0][0]
    if N == 50:
        o = oracle_lib.Oracle(sc.seq.cam, sc.par, N + 8)
        o.set_state(*sc.state)
        ref = [tuple(getattr(i, f) for f in STEP_FIELDS) for i in (o.step(k, d, oracle_lib.LITERAL) for k, d in frames)]
        assert runs[0][0] == ref


# ------------------------------------------------------------------------------------------------------ rescue
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rescue_at_the_threshold(eng_mod, oracle_lib, precision):
    sc = RescueScene(oracle_lib, precision == 0)
    e = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, 58, max_keypoints=264, precision=precision)
    e.set_state(*sc.state_visible)
    seen, _, _ = e.predict_measurements()  # leaves a prediction of the feature that is hidden next in the per-feature tables
    assert seen["featureIndex"][0] == 0 and np.abs(sc.lists["outliers"]["imagePos"][1] - seen["imagePos"][0]).max() < 0.6
    e.set_state(*sc.state)
    e.predict()
    e.predict_measurements()
    e.update(sc.inliers)
    pe, _, _ = e.predict_measurements(sc.idx)
    np.testing.assert_array_equal(pe["featureIndex"], sc.preds["featureIndex"])  # (the hidden feature is not re-predicted)
    for name in ("outliers", "inside", "outside"):
        got = e.rescue(sc.lists[name])
        np.testing.assert_array_equal(got, sc.expected[name], err_msg=name)
    assert sc.expected["outliers"].any() and not sc.expected["outliers"].all()


def test_rescue_is_strict_at_equality(eng_mod, oracle_lib):
    """v == chi2 exactly is not rescued (EKF.cpp:94: `<`).  P = 0 makes S_i = I exactly, so v = d0 d0 + d1 d1 of the innovation the
    device itself forms from its own prediction: the threshold is set to that very number, then to the next double above it."""
    from openekfmonoslam_amd import synth
    from openekfmonoslam_amd.ekftypes import DESC_BYTES, MATCH_DTYPE, s3_camera, s3_params

    cam, par = s3_camera(), s3_params()
    x = np.zeros(13)
    x[3] = 1.0
    fpos, _, _ = synth.new_feature(cam, par, x, np.array([cam.cx + 31.3, cam.cy - 17.9]))

    def engine(chi2):
        p2 = with_probability(par, par.ransacAllInliersProbability)
        p2.ransacChi2Threshold = chi2
        e = eng_mod.EkfEngine(cam, p2, 8, max_keypoints=64)
        e.set_state(x, fpos.reshape(1, 6), None, np.zeros((1, DESC_BYTES), np.uint8), np.zeros((19, 19)))
        p, _, _ = e.predict_measurements()
        return e, p, p2

    e, p, _ = engine(par.ransacChi2Threshold)
    assert len(p) == 1
    np.testing.assert_array_equal(p["covarianceMatrix"][0], [1.0, 0.0, 0.0, 1.0])
    m = np.zeros(1, dtype=MATCH_DTYPE)
    m["imagePos"][0] = p["imagePos"][0] + np.array([1.7, 1.3])
    d = m["imagePos"][0] - p["imagePos"][0]
    v = d[0] * d[0] + d[1] * d[1]  # inv(I) = I and t = d I = d exactly; the kernels are built without FMA contraction
    assert 4.0 < v < par.ransacChi2Threshold and e.rescue(m)[0]
    e.close()
    for chi2, expect in ((v, False), (np.nextafter(v, np.inf), True)):
        e, p_again, p2 = engine(chi2)
        np.testing.assert_array_equal(p_again["imagePos"], p["imagePos"])
        assert oracle_lib.Oracle(cam, p2, 8).rescue(m, p)[0] == expect
        assert e.rescue(m)[0] == expect, chi2
        e.close()


# ------------------------------------------------------------------------------------------- descriptor matcher
def assert_matcher_equal(eng_mod, sc):
    e = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, 58, max_keypoints=4200, descriptor_cols_f32=sc.cols_f32)
    e.set_state(*sc.state)
    e.predict()
    pe, _, _ = e.predict_measurements()
    np.testing.assert_array_equal(pe["featureIndex"], sc.preds["featureIndex"])
    total = 0
    for n_kp in MATCH_COUNTS:
        me = e.match(sc.kps[:n_kp], sc.kdesc[:n_kp])
        mo = sc.oracle_matches(n_kp)
        for f in ("featureIndex", "keypointIndex", "imagePos", "distance"):
            np.testing.assert_array_equal(me[f], mo[f], err_msg=f"{f} n_kp={n_kp}")
        total += len(mo)
    assert total >= 8
    e.close()


@pytest.mark.parametrize("layout", ["edges", "passes"])
@pytest.mark.parametrize("pattern", ["accept", "reject"])
def test_match_candidate_order_across_boundaries(eng_mod, oracle_lib, pattern, layout):
    assert_matcher_equal(eng_mod, MatchScene(oracle_lib, pattern, layout))


@pytest.mark.parametrize("pattern", ["accept", "reject"])
def test_match_candidate_order_f32_descriptors(eng_mod, oracle_lib, pattern):
    assert_matcher_equal(eng_mod, MatchScene(oracle_lib, pattern, "passes", cols_f32=64))
