"""CPU-only checks of the template warp: the numpy reference (tests/template_warp_ref.py) on the
textured-plane scenes of tests/warp_scene.py, and the exported symbols."""
import ctypes as C

import numpy as np
import pytest

import template_warp_ref as tw
import warp_scene as ws
from openekfmonoslam_amd import build, engine
from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH, EkfCamera, EkfParams

N_FEAT = 40
ROLL_ANGLES, APPROACH_RATIOS = (10, 20, 30, 45), (1.25, 1.5, 2)
ROLL_DEG, APPROACH_RATIO = 20, 1.5  # the smallest listed values that pass test_problem_and_cure (its docstring)
APPROACH_MARGIN = 170.0             # seeds that stay in the frame while their offsets from the centre double
IDENTITY = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))


@pytest.fixture(scope="module")
def scene():
    return ws.PlaneScene()


def captured(scene, n=N_FEAT, margin=120.0):
    """frame 0: seeds, their world points, pyramid"""
    uv0, pts, _, _, _, _ = scene.seed_features(n, margin=margin)
    return uv0, pts, tw.pyramid(scene.render(IDENTITY, 0))


def state_of(pose):
    x = np.zeros(13)
    x[0:3], x[3:7] = pose
    return x


def shares(scene, kind, amount, margin):
    """(share of features whose stored level-0 template passes ZNCC >= 0.8 at the true pixel of the last frame, the same
    for the reference-warped template, fall-back levels, share of pixels within 1e-6 of a rounding boundary)"""
    uv0, pts, pyr0 = captured(scene, margin=margin)
    pose = ws.trajectory(kind, 1, amount)[1]
    pyr = tw.pyramid(scene.render(pose, 1))
    uv, _ = scene.true_pixels(pose, pts)
    stored_ok = warped_ok = n_fb = close = total = 0
    for i in range(len(uv0)):
        stored = tw.stored_templates(pyr0, uv0[i])
        fp = np.concatenate([pts[i], np.zeros(3)])
        out, fb, dist, _ = tw.warp_templates(scene.cam, state_of(pose), fp, FEATURE_DEPTH, IDENTITY[0], IDENTITY[1], uv0[i],
                                             tw.source_patches(pyr0, uv0[i]), uv[i], stored)
        now = tw.window(pyr[0], tw.to_level(uv[i, 0], 0), tw.to_level(uv[i, 1], 0), tw.R)
        stored_ok += tw.zncc(stored[0], now) >= 0.8
        warped_ok += tw.zncc(out[0], now) >= 0.8
        n_fb += int(fb.sum())
        close += int((dist < 1e-6).sum())
        total += dist.size
    return stored_ok / len(uv0), warped_ok / len(uv0), n_fb, close / total


def test_identity_pose_returns_the_centre_of_the_source(scene):
    """current pose = capture pose: the ray through a template pixel meets the plane on the capture camera's own ray
    through that pixel, so the sample is the integer source pixel and the bilinear value is exact"""
    uv0, pts, pyr0 = captured(scene)
    for i in range(len(uv0)):
        src = tw.source_patches(pyr0, uv0[i])
        fp = np.concatenate([pts[i], np.zeros(3)])
        out, fb, dist, _ = tw.warp_templates(scene.cam, state_of(IDENTITY), fp, FEATURE_DEPTH, IDENTITY[0], IDENTITY[1], uv0[i], src, uv0[i])
        assert not fb.any()
        assert (dist >= 1e-6).all(), "a pixel within 1e-6 of a rounding boundary at the identity pose"
        np.testing.assert_array_equal(out, src[:, 15:26, 15:26])
        np.testing.assert_array_equal(out, tw.stored_templates(pyr0, uv0[i]))


def test_problem_and_cure(scene):
    """True poses, true feature positions, committed scene seed, 40 features, reference alone.  Share of features whose
    level-0 template reaches ZNCC >= 0.8 at the true pixel, stored / warped:
        roll      10 deg 0.925 / 1.0    20 deg 0.025 / 1.0    30 deg 0.0 / 1.0    45 deg 0.0 / 1.0
        approach  1.25   0.9   / 1.0    1.5    0.15  / 1.0    2      0.0 / 1.0
    so the smallest listed values at which the stored template fails (< 0.8) for at least three quarters of the features
    and the warped one holds (>= 0.8) for at least three quarters are 20 degrees and a ratio of 1.5.  (With texture
    cells of 6 px instead of 3 px no listed ratio made the stored template fail for three quarters -- 0.75 still passed
    at ratio 2; a stored template is the more robust the LARGER the texture's features are, so the cells were made
    smaller, not larger, and the thresholds were left alone.)"""
    def passes(s):
        return s[0] <= 0.25 and s[1] >= 0.75

    roll = {a: shares(scene, "roll", a, 120.0) for a in ROLL_ANGLES}
    appr = {a: shares(scene, "approach", a, APPROACH_MARGIN) for a in APPROACH_RATIOS}
    print("roll (stored, warped, fall-backs, close share):", roll)
    print("approach:", appr)
    assert min(a for a in ROLL_ANGLES if passes(roll[a])) == ROLL_DEG, roll
    assert min(a for a in APPROACH_RATIOS if passes(appr[a])) == APPROACH_RATIO, appr
    for s in list(roll.values()) + list(appr.values()):
        assert s[3] <= 0.01  # the committed scenes put (essentially) no pixel within 1e-6 of a rounding boundary


def test_fallback_is_per_level(scene):
    """A level falls back exactly when one of its samples leaves the 41 x 41 source, and then only that level.  Samples
    leave the source on a RETREAT (the template's +-5 pixels cover +-5 k source pixels at k times the capture distance,
    > 20 from k = 4 on); an approach contracts them.  The centres of the two windows are rounded to whole level pixels
    (to_level), which moves the samples by up to about one more source pixel times k, so between k = 20/6 and 4 the
    levels of one feature differ.  Concretely, at k = 3.5 on the committed scene: feature 5 loses level 2 alone, feature 3
    loses levels 0 and 1 and keeps level 2, feature 1 warps all three."""
    uv0, pts, pyr0 = captured(scene, n=8)
    single = 0
    seen = {}
    for k in np.arange(3.0, 4.25, 0.05):
        pose = (np.array([0.0, 0.0, ws.PLANE_Z * (1.0 - k)]), IDENTITY[1])
        uv, _ = scene.true_pixels(pose, pts)
        for i in range(len(uv0)):
            stored = tw.stored_templates(pyr0, uv0[i])
            fp = np.concatenate([pts[i], np.zeros(3)])
            out, fb, _, co = tw.warp_templates(scene.cam, state_of(pose), fp, FEATURE_DEPTH, IDENTITY[0], IDENTITY[1], uv0[i],
                                               tw.source_patches(pyr0, uv0[i]), uv[i], stored)
            for l in range(3):
                assert fb[l] == bool(((co[l] < 0) | (co[l] > 40)).any())
                if fb[l]:
                    np.testing.assert_array_equal(out[l], stored[l])
            single += int(fb.sum() == 1)
            seen[(int(round(k * 100)), i)] = tuple(bool(f) for f in fb)
    assert single > 0
    assert seen[(350, 5)] == (False, False, True), seen[(350, 5)]
    assert seen[(350, 3)] == (True, True, False), seen[(350, 3)]
    assert seen[(350, 1)] == (False, False, False), seen[(350, 1)]
    assert all(seen[(300, i)] == (False, False, False) and seen[(420, i)] == (True, True, True) for i in range(len(uv0)))
    # no source patch: every level falls back to the stored bytes
    out, fb, _, _ = tw.warp_templates(scene.cam, state_of(IDENTITY), np.concatenate([pts[0], np.zeros(3)]), FEATURE_DEPTH,
                                      IDENTITY[0], IDENTITY[1], uv0[0], None, uv0[0], tw.stored_templates(pyr0, uv0[0]))
    assert fb.all()
    np.testing.assert_array_equal(out, tw.stored_templates(pyr0, uv0[0]))


def test_inverse_depth_and_depth_features_warp_alike(scene):
    """X is the same point for both feature kinds (the conversion keeps the tables)"""
    uv0, pts, fpos, ftype, _, _ = scene.seed_features(6)
    pyr0 = tw.pyramid(scene.render(IDENTITY, 0))
    pose = ws.trajectory("roll", 1, ROLL_DEG)[1]
    uv, _ = scene.true_pixels(pose, pts)
    for i in range(6):
        np.testing.assert_allclose(tw.feature_xyz(fpos[i], ftype[i]), pts[i], rtol=0, atol=1e-12)
        src = tw.source_patches(pyr0, uv0[i])
        a = tw.warp_templates(scene.cam, state_of(pose), fpos[i], ftype[i], IDENTITY[0], IDENTITY[1], uv0[i], src, uv[i])
        b = tw.warp_templates(scene.cam, state_of(pose), np.concatenate([pts[i], np.zeros(3)]), FEATURE_DEPTH, IDENTITY[0],
                              IDENTITY[1], uv0[i], src, uv[i])
        np.testing.assert_array_equal(a[0], b[0])


def test_library_exports_the_warp_calls():
    build.build_engine()
    lib = engine.load_library()
    for name in ("ekf_set_template_warp", "ekf_get_template_warp_counts", "ekf_get_match_templates"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    # struct sizes as in test_abi_and_host.py: nothing existing changed size
    assert C.sizeof(EkfCamera) == 8 + 12 * 8
    assert C.sizeof(EkfParams) == 12 * 8
    assert C.sizeof(engine.EkfEngineConfig) == C.sizeof(EkfCamera) + C.sizeof(EkfParams) + 6 * 4
    assert C.sizeof(engine.EkfStageTimes) == 11 * 8
    assert lib.ekf_set_template_warp(None, 1) == 1  # EKF_ERR_INVALID_ARG: no engine
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_get_template_warp_counts(None, C.byref(a), C.byref(b)) == 1
    assert lib.ekf_get_match_templates(None, None, 0, None) == 1
