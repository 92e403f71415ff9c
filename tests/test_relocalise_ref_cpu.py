"""The relocalisation's numpy contract (tests/relocalise_ref.py) on its own, the constants the GPU tests assert against (tests/relocalise_scenes.py), and
the ABI of the engine library (ctypes only; no GPU is touched)."""
import ctypes as C

import numpy as np
import pytest

import relocalise_ref as rr
from openekfmonoslam_amd.ekftypes import EkfRelocHypothesis, EkfRelocParams, EkfRelocResult, s3_camera
from openekfmonoslam_amd.synth import angles_to_quat

LD = np.longdouble
EPS64, EPSLD = float(np.finfo(np.float64).eps), float(np.finfo(LD).eps)


def pose_error(sols, r, q):
    """the smallest error of a solution against (r, q): largest component of r, and of q up to its sign"""
    errs = [max(float(np.max(np.abs(s[0] - r))), float(min(np.max(np.abs(s[1] - q)), np.max(np.abs(s[1] + q))))) for s in sols]
    return min(errs) if errs else np.inf


def bearings_of(X, r, q, dt):
    Rq = rr.quat_to_rot(np.asarray(q, dtype=dt), dt)
    return np.stack([rr._unit(rr._mtv(Rq, np.asarray(X[i], dtype=dt) - np.asarray(r, dtype=dt))) for i in range(3)])


# ------------------------------------------------------------------------------------------------------------ P3P
def test_p3p_returns_the_true_pose_for_200_random_triples():
    """Tolerance from the same run in longdouble: the error of a float64 run is the longdouble run's error scaled by the ratio of
    the two machine epsilons (the conditioning of a triple is the same in both), up to the constant by which two different
    sequences of roundings differ -- 100 is allowed -- and never below 100 float64 epsilons of the scene's size (10)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for it in range(200):
        X = rng.uniform(-3, 3, (3, 3)) + np.array([0, 0, 6.0])
        q = angles_to_quat(rng.normal(0, 0.5, 3))
        r = rng.normal(0, 0.5, 3)
        e64 = pose_error(rr.p3p(X, bearings_of(X, r, q, np.float64), np.float64), r, q)
        eld = pose_error(rr.p3p(X.astype(LD), bearings_of(X, r, q, LD), LD), r.astype(LD), q.astype(LD))
        tol = 100.0 * (EPS64 / EPSLD) * max(eld, 10.0 * EPSLD)
        worst = max(worst, e64 / tol)
        assert e64 <= tol, (it, e64, eld)
    print(f"worst float64 error / tolerance over 200 triples: {worst:.3f}")


def test_quartic_roots_agree_with_numpy_roots():
    rng = np.random.default_rng(9)
    for _ in range(200):
        roots = np.sort(rng.uniform(-3, 3, 4))
        if np.min(np.diff(roots)) < 0.05:
            continue
        k = np.poly(roots)[::-1] * rng.uniform(0.5, 2.0)
        got = rr.quartic_real_roots(k.astype(np.float64))
        assert len(got) == 4 and np.allclose(got, roots, rtol=0, atol=1e-9)
    two = np.poly([0.5, 2.0])  # two real roots and a complex pair
    k = np.polymul(two, [1.0, 0.2, 1.5])[::-1]
    want = sorted(z.real for z in np.roots(k[::-1]) if abs(z.imag) < 1e-12)
    assert np.allclose(rr.quartic_real_roots(k), want, rtol=0, atol=1e-12)
    assert rr.quartic_real_roots(np.array([1.0, 0.0, 2.0, 0.0, 1.0])) == []  # (v^2 + 1)^2: biquadratic, no real root
    assert np.allclose(rr.quartic_real_roots(np.array([4.0, 0.0, -5.0, 0.0, 1.0])), [-2, -1, 1, 2])  # biquadratic branch
    assert rr.quartic_real_roots(np.array([1.0, 1.0, 1.0, 1.0, 0.0])) == []  # no quartic
    assert rr.quartic_real_roots(np.array([1.0, np.nan, 1.0, 1.0, 1.0])) == []


def test_degenerate_triples_return_nothing_and_no_nan():
    cam = s3_camera()
    f = np.stack([rr.bearing(cam, u, v) for u, v in ((100.0, 80.0), (320.0, 240.0), (500.0, 400.0))])
    line = np.outer([-1.0, 0.0, 2.0], [1.0, 0.5, 0.25]) + np.array([0.0, 0.0, 5.0])
    X = np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 6.0], [0.0, 1.0, 7.0]])
    cases = {"collinear world points": (line, f),
             "two identical candidates": (X[[0, 0, 2]], f[[0, 0, 2]]),
             "a bearing pair with cos(gamma) = 1": (X, f[[0, 0, 2]])}
    for name, (Xc, fc) in cases.items():
        for dt in (np.float64, LD):
            sols = rr.p3p(Xc, fc, dt)
            assert sols == [], name
    # ... and whatever a solver returns for any input is finite
    rng = np.random.default_rng(2)
    for _ in range(100):
        for r, q in rr.p3p(rng.normal(0, 1, (3, 3)), np.stack([rr._unit(v) for v in rng.normal(0, 1, (3, 3))])):
            assert np.all(np.isfinite(r)) and np.all(np.isfinite(q))


# ------------------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("C_", [3, 4, 1000])
def test_sampled_triples_are_distinct(C_):
    for seed in (0, 1, 2 ** 64 - 5):
        for h in range(rr.MAX_HYPOTHESES):
            t = rr.sample_triple(seed, h, C_)
            assert len(set(t)) == 3 and all(0 <= i < C_ for i in t)
    assert rr.splitmix64(0) == 0xE220A8397B1DCDAF  # the published first output of splitmix64 seeded with 0


# ---------------------------------------------------------------------------------------------------------- match
def test_global_match_threshold_ratio_and_ties():
    feat = np.zeros((3, 32), dtype=np.uint8)
    kp = np.zeros((4, 32), dtype=np.uint8)
    kp[0, 0] = 0b111         # distance 3 to every feature
    kp[1, 0] = 0b1           # distance 1
    kp[2, 0] = 0b10          # distance 1: a tie with keypoint 1
    kp[3] = 255              # far
    xy = np.arange(8, dtype=np.float64).reshape(4, 2)
    used = np.array([True, False, True])
    got = rr.global_match(feat, used, xy, kp, 48.0, 0.0)
    assert [(c[0], c[1], c[3]) for c in got] == [(0, 1, 1), (2, 1, 1)]  # ascending features, the lower keypoint of a tie, no unused one
    assert got[0][2] == (2.0, 3.0)
    assert rr.global_match(feat, used, xy, kp, 48.0, 1.0) == []          # d1 < 1.0 * d2 fails at d1 = d2
    assert rr.global_match(feat, used, xy, kp, 0.5, 0.0) == []           # d1 <= max_distance
    assert len(rr.global_match(feat, used, xy[:1], kp[:1], 3.0, 0.8)) == 2  # one keypoint: no second best, d1 = max_distance passes
    assert rr.global_match(feat, used, xy[:0], kp[:0], 48.0, 0.0) == []


# ---------------------------------------------------------------------------------------------------------- score
def test_scoring_threshold_and_tie_order():
    cam = s3_camera()
    r, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    X = np.array([[0.0, 0.0, 5.0], [0.5, 0.2, 4.0], [-0.4, 0.3, 6.0], [0.0, 0.0, -5.0]])
    ok, uv = rr.predict_pixel(cam, r, q, X)
    assert list(ok) == [True, True, True, False]  # the last one is behind the camera
    pix = uv.copy()
    pix[1, 0] += 3.0          # exactly on the threshold of 3 px: an inlier (<=)
    pix[2, 0] += 3.0 + 1e-9   # just outside
    n, sse, e2 = rr.score_pose(cam, r, q, X, pix, 3.0)
    assert n == 2 and np.isinf(e2[3]) and e2[2] > 9.0 and abs(float(sse) - 9.0) < 1e-9
    assert rr.better(3, 5.0, 2, 1.0) and rr.better(3, 1.0, 3, 2.0)
    assert not rr.better(3, 2.0, 3, 2.0) and not rr.better(2, 0.0, 3, 9.0)  # equal keeps the earlier solution / hypothesis


def test_whole_reference_selects_by_the_stated_order():
    """with the same triple forced on every hypothesis all records are equal, and the lowest h wins"""
    import relocalise_scenes as t

    sc = t.Scene(12)
    xy = np.stack([sc.kps["x"], sc.kps["y"]], -1).astype(np.float64)
    ref = rr.relocalise(sc.seq.cam, sc.feature_pos, sc.feature_type, sc.covpos, sc.P, sc.seq.feature_desc, xy, sc.desc,
                        dict(t.PARAMS, hypotheses=4), triples=[[0, 5, 9]] * 4)
    assert ref["n_valid_hypotheses"] in (0, 4)
    if ref["n_valid_hypotheses"]:
        assert ref["best_hypothesis"] == 0 and ref["n_inliers"] == ref["hypotheses"][3]["inliers"]
        assert int(ref["inlier_mask"].sum()) == ref["n_inliers"]


def test_constants_of_the_gpu_test_are_current():
    """what tests/relocalise_scenes.py carries as constants for the GPU tests, measured again: for both seeds the reference alone stays inside the
    5 % cap (no hypothesis of them is solved differently in float64 and in longdouble beyond it)"""
    import relocalise_scenes as t

    s65 = t.Scene(65)
    for seed in t.HYP_SEEDS:
        disc = t.hypothesis_discrepancies(s65, s65.reference(seed=seed))
        keep = t.kept_hypotheses(disc)  # asserts that the kept ones are finite
        assert len(keep) >= (1 - t.LEFT_OUT) * len(disc)
        assert abs(disc[keep].max() / t.REF_DISCREPANCY[seed] - 1) < 1e-6
    s257 = t.Scene(257)
    ref = s257.reference(seed=t.PARAMS["seed"])
    disc = t.hypothesis_discrepancies(s257, ref)
    assert abs(disc[t.kept_hypotheses(disc)].max() / t.REF_DISCREPANCY["e2e"] - 1) < 1e-6
    assert ref["found"] == 1
    assert abs(np.max(np.abs(ref["r"] - s257.seq.truth_r[t.FRAME])) / t.E2E_REF_ERROR_R - 1) < 1e-6
    assert abs(np.max(np.abs(ref["q"] - s257.seq.truth_q[t.FRAME])) / t.E2E_REF_ERROR_Q - 1) < 1e-6


def test_install_covariance_is_block_diagonal_and_psd():
    import relocalise_scenes as t

    sc = t.Scene(12)
    P = sc.P + 1e-6  # cross terms everywhere
    P2 = rr.install_covariance(P, sc.seq.par, 0.05, 0.02, np.float32)
    assert not np.any(P2[:13, 13:]) and not np.any(P2[13:, :13]) and np.array_equal(P2[13:, 13:], P[13:, 13:])
    assert np.array_equal(np.diag(P2)[:7], np.array([np.float32(0.05 ** 2)] * 3 + [np.float32(0.25 * 0.02 ** 2)] * 4, dtype=np.float64))
    assert np.all(np.linalg.eigvalsh(P2) >= 0)


# ------------------------------------------------------------------------------------------------------------ ABI
def test_library_exports_the_relocalisation_abi():
    """fails on a tree without the feature: the symbol is not there"""
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    for name in ("ekf_relocalise", "ekf_relocalise_image", "ekf_get_relocalise_candidates", "ekf_get_relocalise_hypotheses"):
        assert hasattr(lib, name), name
        assert name in engine.ABI
    assert lib.ekf_abi_version() == 1
    assert (C.sizeof(EkfRelocParams), C.sizeof(EkfRelocResult), C.sizeof(EkfRelocHypothesis)) == (72, 96, 88)
