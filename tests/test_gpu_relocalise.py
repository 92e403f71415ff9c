"""Relocalisation on the device (ekf_relocalise, kernels_reloc.hip) against its numpy contract
(tests/relocalise_ref.py): the match table entry for entry, the hypotheses record for record, the installed pose end to end, and
what the call leaves alone.

The map is SyntheticSequence(...).points as depth features with a small diagonal P (one test: as converged inverse-depth features),
in fp64 and in EKF_PRECISION_F32_EXACT storage.  The scenes, the parameters and the measured constants behind the pose tolerances
are in tests/relocalise_scenes.py, where the tolerances are explained.
"""
import ctypes as C

import numpy as np
import pytest

import relocalise_ref as rr
from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, KEYPOINT_DTYPE
from relocalise_scenes import (E2E_REF_ERROR_Q, E2E_REF_ERROR_R, FRAME, HYP_SEEDS, PARAMS, REF_DISCREPANCY, InverseDepthScene, Scene,
                               hypothesis_discrepancies, kept_hypotheses, pose_tolerance)

pytestmark = pytest.mark.gpu

PRECISIONS = [0, 2]  # EKF_PRECISION_F64, EKF_PRECISION_F32_EXACT


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


@pytest.fixture(scope="module")
def scene65():
    return Scene(65)


@pytest.fixture(scope="module")
def scene257():
    return Scene(257)


@pytest.fixture(scope="module")
def ref65(scene65):
    """the float64 reference of test 2 and the hypotheses it keeps, per seed; computed once"""
    out = {}
    for seed in HYP_SEEDS:
        ref = scene65.reference(seed=seed)
        disc = hypothesis_discrepancies(scene65, ref)
        out[seed] = (ref, disc)
    return out


@pytest.fixture(scope="module")
def ref257(scene257):
    return scene257.reference(seed=PARAMS["seed"])


def snapshot(e):
    """every byte the call must leave alone when it installs nothing"""
    x, fp, P = e.get_state()
    desc, tp, tm = e.get_map_features()
    t, c = e.feature_layout()
    return [x, fp, P, desc, tp, tm, t, c]


def same_bytes(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


def finite_result(res, hyp):
    return (np.all(np.isfinite(res["r"])) and np.all(np.isfinite(res["q"])) and np.isfinite(res["rms_px"]) and np.all(np.isfinite(hyp["sse"]))
            and np.all(np.isfinite(hyp["r"])) and np.all(np.isfinite(hyp["q"])))


# ------------------------------------------------------------------------------------------- 1. the match table, exact
def match_case(n, k, rng):
    """n features and k keypoints: about half of min(n, k) keypoints are a feature's descriptor with a few bits flipped, the
    rest are random; feature 1's best distance occurs twice (keypoints 0 and k - 1 carry its descriptor) when k >= 2"""
    feat = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    owners = rng.permutation(k)[: max(1, min(n, k) // 2)]
    for i, kp in enumerate(owners):
        d = feat[i % n].copy()
        for bit in rng.integers(0, 256, rng.integers(0, 30)):
            d[bit // 8] ^= np.uint8(1 << (bit % 8))
        desc[kp] = d
    if k >= 2:
        desc[0] = feat[1]
        desc[k - 1] = feat[1]
    kps = np.zeros(k, dtype=KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(1, 639, k).astype(np.float32)
    kps["y"] = rng.uniform(1, 479, k).astype(np.float32)
    return feat, kps, desc


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [1, 255, 2049])
@pytest.mark.parametrize("n", [3, 65, 257])
def test_match_table_is_exact(eng_mod, n, k, precision):
    """N x K at the lane (K = 1), workgroup (255 of 256 threads) and pass (2049 = 8 x 256 + 1) edges; equal best distances go to
    the lower keypoint index, with the ratio test (which then rejects: d1 < coef d2 fails at d1 = d2) and without it"""
    sc = Scene(n)
    rng = np.random.default_rng(1000 * n + k)
    feat, kps, desc = match_case(n, k, rng)
    e = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, n + 16, max_keypoints=2049, precision=precision)
    e.set_state(sc.x_true, sc.feature_pos, sc.feature_type, feat, sc.P)
    xy = np.stack([kps["x"], kps["y"]], -1).astype(np.float64)
    used = np.ones(n, dtype=bool)
    for coef in (0.8, 0.0):
        res = e.relocalise(kps, desc, **dict(PARAMS, hypotheses=1, second_best_coef=coef))
        want = rr.global_match(feat, used, xy, desc, PARAMS["max_distance"], coef)
        got, _ = e.relocalise_candidates()
        assert res["n_features_used"] == n and res["n_candidates"] == len(want) == len(got)
        assert [int(f) for f in got["featureIndex"]] == [c[0] for c in want]
        assert [int(f) for f in got["keypointIndex"]] == [c[1] for c in want]
        assert np.array_equal(got["imagePos"], np.array([c[2] for c in want]).reshape(-1, 2))
        assert np.array_equal(got["distance"], np.array([c[3] for c in want], dtype=np.float32))
        if k >= 2:
            tie = [c for c in want if c[0] == 1]
            assert (tie == [] and coef > 0) or (tie[0][1] == 0 and tie[0][3] == 0 and coef == 0)


# --------------------------------------------------------------------------------------- 2. the hypotheses, per record
def pose_difference(r1, q1, r2, q2):
    return max(float(np.max(np.abs(r1 - r2))), float(np.max(np.abs(q1 - q2))))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed", HYP_SEEDS)
def test_hypotheses_match_reference(eng_mod, scene65, ref65, seed, precision):
    ref, disc = ref65[seed]
    keep = kept_hypotheses(disc)
    assert disc[keep].max() <= REF_DISCREPANCY[seed] * 1.0000001, "the constants in tests/relocalise_scenes.py are stale"
    e = scene65.engine(eng_mod, precision)
    res = e.relocalise(scene65.kps, scene65.desc, **dict(PARAMS, seed=seed))
    hyp = e.relocalise_hypotheses()
    assert res["n_candidates"] == ref["n_candidates"] and len(hyp) == 256 == res["n_hypotheses"]
    assert [list(map(int, h)) for h in hyp["cand"]] == [list(r["cand"]) for r in ref["hypotheses"]]  # every triple, none left out
    worst = 0.0
    for h in keep:
        want, got = ref["hypotheses"][h], hyp[h]
        assert got["n_solutions"] == want["n_solutions"], h
        if want["n_solutions"] == 0:
            continue
        worst = max(worst, pose_difference(got["r"], got["q"], want["r"], want["q"]))
        # inliers: equal once the candidates whose reference error is within 1e-6 px of the threshold are set aside
        err = np.sqrt(want["errs"])
        unsure = int(np.sum(np.abs(err - PARAMS["inlier_px"]) <= 1e-6))
        assert abs(int(got["inliers"]) - want["inliers"]) <= unsure, h
    tol = pose_tolerance(seed)  # 100 x the reference's own float64-vs-longdouble difference among the hypotheses kept in THIS run
    print(f"seed {seed} precision {precision}: {len(keep)} hypotheses kept, worst pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


# ------------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("precision", PRECISIONS)
def test_end_to_end_recovers_tracking(eng_mod, scene257, ref257, precision):
    sc, N = scene257, 257
    e = sc.engine(eng_mod, precision, x13=sc.displaced())
    lost = e.step(sc.kps, sc.desc)
    assert lost.n_inliers < 0.1 * N  # from 1 m and 40 degrees off, a plain step finds nothing: the test means something
    e = sc.engine(eng_mod, precision, x13=sc.displaced())
    res = e.relocalise(sc.kps, sc.desc, **dict(PARAMS, install=1))
    assert res["found"] == 1 and res["installed"] == 1
    assert res["best_hypothesis"] == ref257["best_hypothesis"] and res["n_inliers"] == ref257["n_inliers"]
    tol = pose_tolerance("e2e")  # this scene's own figure: 100 x the reference's float64-vs-longdouble difference at N = 257, seed 11
    assert pose_difference(res["r"], res["q"], ref257["r"], ref257["q"]) <= tol
    # the reference's own pose error against the truth, measured on the CPU, is the bound (the device may differ from the reference
    # by tol)
    assert np.max(np.abs(res["r"] - sc.seq.truth_r[FRAME])) <= E2E_REF_ERROR_R + tol
    assert np.max(np.abs(res["q"] - sc.seq.truth_q[FRAME])) <= E2E_REF_ERROR_Q + tol
    x, _, _ = e.get_state(want_P=False)
    assert np.array_equal(x[0:3], res["r"]) and np.array_equal(x[3:7], res["q"])
    info = e.step(sc.kps, sc.desc)
    assert info.status == 0 and info.n_inliers + info.n_rescued >= 0.8 * N


# ------------------------------------------------------------------------------- 4. nothing moves unless installed
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_moves_unless_installed(eng_mod, scene65, precision):
    sc = scene65
    e = sc.engine(eng_mod, precision, x13=sc.displaced())
    before = snapshot(e)
    rnd = np.random.default_rng(7).integers(0, 256, sc.desc.shape, dtype=np.uint8)
    res = e.relocalise(sc.kps, rnd, **dict(PARAMS, install=1))
    assert res["found"] == 0 and res["installed"] == 0
    assert same_bytes(before, snapshot(e))
    res = e.relocalise(sc.kps, sc.desc, **dict(PARAMS, install=0))
    assert res["found"] == 1 and res["installed"] == 0
    assert same_bytes(before, snapshot(e))


# ------------------------------------------------------------------------------- 5. install writes the strip only
@pytest.mark.parametrize("precision", PRECISIONS)
def test_install_writes_the_camera_strip_only(eng_mod, scene65, precision):
    sc = scene65
    x_prev = sc.x_true.copy()
    x_prev[0:3], x_prev[3:7] = sc.seq.truth_r[FRAME - 1], sc.seq.truth_q[FRAME - 1]
    e = sc.engine(eng_mod, precision, x13=x_prev)
    info = e.step(sc.kps, sc.desc)  # one tracked frame: P now has cross terms everywhere
    assert info.status == 0 and info.n_inliers > sc.N // 2
    P0 = e.get_state()[2]
    assert np.any(P0[:13, 13:]) and np.count_nonzero(P0[13:, 13:]) > P0[13:, 13:].size // 2
    before = snapshot(e)
    res = e.relocalise(sc.kps, sc.desc, **dict(PARAMS, install=1, sigma_position=0.07, sigma_angle=0.03))
    assert res["installed"] == 1
    after = snapshot(e)
    assert same_bytes(before[3:], after[3:]) and same_bytes([before[1]], [after[1]])  # the map's tables and parameters
    P = after[2]
    storage = np.float32 if precision == 2 else np.float64
    want = rr.install_covariance(P0, sc.seq.par, 0.07, 0.03, storage)
    assert P[13:, 13:].tobytes() == P0[13:, 13:].tobytes()
    assert not np.any(P[:13, 13:]) and not np.any(P[13:, :13])
    assert P[:13, :13].tobytes() == want[:13, :13].tobytes()
    assert P[:13, :].tobytes() == np.ascontiguousarray(P[:, :13].T).tobytes()
    x = after[0]
    assert np.array_equal(x[0:7], np.concatenate([res["r"], res["q"]])) and not np.any(x[7:10]) and np.all(x[10:13] == 2.22e-16)
    e.set_fixed_map(True)
    for _ in range(2):
        info = e.step(sc.kps, sc.desc)
        assert info.status == 0
    assert np.all(np.isfinite(e.get_state()[0]))


# ------------------------------------------------------------------------------------------------------ 6. edges
def assert_not_found(e, res):
    hyp = e.relocalise_hypotheses()
    assert res["found"] == 0 and res["installed"] == 0 and finite_result(res, hyp)
    e.synchronize()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_cand", [0, 1, 2])
def test_edge_few_candidates(eng_mod, scene65, precision, n_cand):
    sc = scene65
    e = sc.engine(eng_mod, precision)
    desc = np.random.default_rng(3).integers(0, 256, sc.desc.shape, dtype=np.uint8)
    desc[:n_cand] = sc.seq.feature_desc[:n_cand]
    res = e.relocalise(sc.kps, desc, **PARAMS)
    assert res["n_candidates"] == n_cand and res["n_valid_hypotheses"] == 0 and res["best_hypothesis"] == -1
    assert_not_found(e, res)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edge_collinear_map_and_no_keypoints(eng_mod, scene65, precision):
    sc = scene65
    fp = sc.feature_pos.copy()
    fp[:, 0:3] = np.outer(np.linspace(-1.0, 1.0, sc.N), [1.0, 0.5, 0.25]) + np.array([0.0, 0.0, 5.0])
    e = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, sc.N + 16, max_keypoints=4 * sc.N + 64, precision=precision)
    e.set_state(sc.x_true, fp, sc.feature_type, sc.seq.feature_desc, sc.P)
    res = e.relocalise(sc.kps, sc.desc, **PARAMS)
    assert res["n_candidates"] >= 3 and res["n_valid_hypotheses"] == 0
    assert_not_found(e, res)
    res = e.relocalise(sc.kps[:0], sc.desc[:0], **PARAMS)  # K = 0
    assert res["n_features_used"] == sc.N and res["n_candidates"] == 0
    assert_not_found(e, res)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edge_fresh_inverse_depth_map(eng_mod, scene65, precision):
    """a map as it is seeded: rho = 1 with sd(rho) = 1, no usable depth; max_rel_depth_sd = 0.3 keeps every feature out"""
    seq = scene65.seq
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=4 * seq.n_features + 64, precision=precision)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    assert np.all(seq.feature_type == FEATURE_INVERSE_DEPTH)
    res = e.relocalise(scene65.kps, scene65.desc, **dict(PARAMS, max_rel_depth_sd=0.3))
    assert res["n_features_used"] == 0 and res["n_candidates"] == 0
    assert_not_found(e, res)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_rel", [0.3, 0.0])
def test_converged_inverse_depth_features_take_part(eng_mod, precision, max_rel):
    """the inverse-depth branch of k_reloc_match with features that DO take part: world points through m(theta, phi) / rho, and
    sd(rho) / rho <= max_rel_depth_sd read from P in its storage type, with features on both sides of 0.3 and two with rho < 0
    (one of them with a small sd); max_rel_depth_sd = 0 filters by the sign of rho alone"""
    sc = InverseDepthScene(65)
    e = sc.engine(eng_mod, precision, x13=sc.displaced())
    P = e.get_state()[2]  # as stored (rounded to fp32 in EKF_PRECISION_F32_EXACT): what the device compares
    res = e.relocalise(sc.kps, sc.desc, **dict(PARAMS, max_rel_depth_sd=max_rel))
    ref = sc.reference(P=P, max_rel_depth_sd=max_rel)
    usable = (sc.feature_pos[:, 5] > 0) & ((sc.rel_sd <= max_rel) if max_rel else True)
    assert ref["n_features_used"] == int(usable.sum()) == res["n_features_used"] and 0 < res["n_features_used"] < 65
    got, mask = e.relocalise_candidates()
    want = ref["candidates"]
    assert res["n_candidates"] == len(want) == len(got) >= 3
    assert all(usable[c[0]] for c in want)
    assert [int(f) for f in got["featureIndex"]] == [c[0] for c in want]
    assert [int(f) for f in got["keypointIndex"]] == [c[1] for c in want]
    assert np.array_equal(got["imagePos"], np.array([c[2] for c in want]).reshape(-1, 2))
    assert np.array_equal(got["distance"], np.array([c[3] for c in want], dtype=np.float32))
    # the world points went through the device's sin / cos: the hypotheses' triples are the reference's, the pose is the scene's
    hyp = e.relocalise_hypotheses()
    assert [list(map(int, h)) for h in hyp["cand"]] == [list(r["cand"]) for r in ref["hypotheses"]]
    assert res["found"] == ref["found"] == 1 and res["best_hypothesis"] == ref["best_hypothesis"]
    err = np.sqrt(ref["hypotheses"][ref["best_hypothesis"]]["errs"])
    unsure = int(np.sum(np.abs(err - PARAMS["inlier_px"]) <= 1e-6))
    assert abs(res["n_inliers"] - ref["n_inliers"]) <= unsure


# ------------------------------------------------------------------------------------------------ 7. determinism
@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_call_twice_is_byte_identical(eng_mod, scene65, precision):
    e = scene65.engine(eng_mod, precision, x13=scene65.displaced())
    runs = []
    for _ in range(2):
        res = e.relocalise(scene65.kps, scene65.desc, **PARAMS)
        cand, mask = e.relocalise_candidates()
        runs.append([np.concatenate([res["r"], res["q"], [res["rms_px"]]]), np.array([res[k] for k in sorted(res) if k not in ("r", "q", "rms_px")]),
                     e.relocalise_hypotheses(), cand, mask])
    assert same_bytes(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------- 8. image form
@pytest.mark.parametrize("precision", PRECISIONS)
def test_image_form_equals_keypoint_form(eng_mod, scene65, precision):
    sc = scene65
    e = sc.engine(eng_mod, precision, x13=sc.displaced(), max_keypoints=4096)
    e.upload_image(sc.seq.render_image(FRAME))
    thr = 1e10  # synthetic renders: above the background noise's corners
    kps, desc = e.detect_keypoints(thr, masked=False, capacity=4096)
    assert 0 < len(kps) == e.last_found
    # the map's descriptors: that of the detected keypoint nearest to each point's patch (so that the frame has candidates at all)
    px = sc.seq.pixel_positions(FRAME).astype(np.float64)
    d2 = (px[:, None, 0] - kps["x"][None, :]) ** 2 + (px[:, None, 1] - kps["y"][None, :]) ** 2
    e.set_state(sc.displaced(), sc.feature_pos, sc.feature_type, desc[np.argmin(d2, axis=1)], sc.P)
    params = dict(PARAMS, inlier_px=10.0, second_best_coef=0.0)
    a = e.relocalise_image(thr, **params)
    ha, (ca, ma) = e.relocalise_hypotheses(), e.relocalise_candidates()
    assert a["n_candidates"] >= 3 and a["n_valid_hypotheses"] > 0
    b = e.relocalise(kps, desc, **params)
    hb, (cb, mb) = e.relocalise_hypotheses(), e.relocalise_candidates()
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert same_bytes([ha, ca, ma], [hb, cb, mb])


# ------------------------------------------------------------------------------------------ 9. invalid arguments
BAD_PARAMS = [dict(hypotheses=0), dict(hypotheses=4097), dict(min_inliers=3), dict(max_distance=-1.0), dict(max_distance=float("nan")),
              dict(second_best_coef=-0.1), dict(second_best_coef=1.5), dict(second_best_coef=float("nan")), dict(inlier_px=0.0),
              dict(inlier_px=float("nan")), dict(max_rel_depth_sd=-1.0), dict(max_rel_depth_sd=float("nan")), dict(sigma_position=0.0),
              dict(sigma_position=float("nan")), dict(sigma_angle=0.0), dict(sigma_angle=float("nan"))]


def test_invalid_arguments_are_refused(eng_mod, scene65):
    sc = scene65
    e = sc.engine(eng_mod, 0, x13=sc.displaced(), max_keypoints=len(sc.kps))
    before = snapshot(e)
    for bad in BAD_PARAMS:
        assert e.relocalise(sc.kps, sc.desc, allow_errors=(1,), **dict(PARAMS, install=1, **bad)) == {"code": 1}, bad
        assert e.relocalise_image(1e7, allow_errors=(1,), **dict(PARAMS, install=1, **bad)) == {"code": 1}, bad
    p, out = e._reloc_params(**PARAMS), eng_mod.EkfRelocResult()
    assert e.L.ekf_relocalise(e.h, None, None, -1, C.byref(p), C.byref(out)) == 1  # n_kp < 0
    more = np.zeros(len(sc.kps) + 1, dtype=KEYPOINT_DTYPE)
    assert e.relocalise(more, np.zeros((len(more), 32), dtype=np.uint8), allow_errors=(1,), **PARAMS) == {"code": 1}  # n_kp > max_keypoints
    assert b"ekf_relocalise" in e.L.ekf_last_error(e.h)
    assert same_bytes(before, snapshot(e))
    f32 = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, 32, max_keypoints=64, descriptor_cols_f32=64)  # not EKF_DESCRIPTOR_U8_HAMMING
    assert f32.relocalise(sc.kps[:0], sc.desc[:0], allow_errors=(1,), **PARAMS) == {"code": 1}
    sh = eng_mod.EkfEngine(sc.seq.cam, sc.seq.par, 32, max_keypoints=64, shard=(0, 2))  # a sharded engine
    assert sh.relocalise(sc.kps[:0], sc.desc[:0], allow_errors=(1,), **PARAMS) == {"code": 1}
    assert sh.relocalise_image(1e7, allow_errors=(1,), **PARAMS) == {"code": 1}
