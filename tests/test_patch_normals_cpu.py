"""CPU-only checks of the patch-normal estimator: the numpy restatement (tests/patch_normal_ref.py)
on the tilted plane of tests/tilted_scene.py with true poses and true feature positions, and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import patch_normal_ref as pn
import template_warp_ref as tw
import tilted_scene as ts
from openekfmonoslam_amd import build, engine
from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH

R0, Q0 = ts.IDENTITY


def state_of(pose):
    x = np.zeros(13)
    x[0:3], x[3:7] = pose
    return x


def angles(est, pts):
    """angle to the true normal per feature; a feature without an estimate stands at the rule"""
    return np.array([pn.angle_deg(pn.normal_of(Q0, pn.rule_pq(R0, Q0, X) if e is None else e[0]), ts.NORMAL) for e, X in zip(est, pts)])


def run(scene, poses, pts_used=None, frames=None):
    """the estimator over a trajectory, anchored at the rounded true pixels.  pts_used: the feature positions handed to the
    estimator (default: the true ones).  Returns (uv0, true points, source patches, estimates [(pq, info) or None])."""
    uv0, pts, _, _, _, _ = scene.seed_features()
    used = pts if pts_used is None else pts_used(pts)
    pyr0 = tw.pyramid(scene.render(ts.IDENTITY, 0))
    src = [tw.source_patches(pyr0, uv) for uv in uv0]
    est = [None] * len(uv0)
    for t in (range(1, len(poses)) if frames is None else frames):
        pyr = tw.pyramid(scene.render(poses[t], t))
        uv, _ = scene.true_pixels(poses[t], pts)
        for i in range(len(uv0)):
            out = pn.refine(scene.cam, state_of(poses[t]), np.concatenate([used[i], np.zeros(3)]), FEATURE_DEPTH, R0, Q0, uv0[i], src[i],
                            pyr, np.rint(uv[i]).astype(int), est[i])
            if out is not None:
                est[i] = (out[0], out[1])
    return uv0, pts, src, est


@pytest.fixture(scope="module")
def scene():
    return ts.TiltedScene()


@pytest.fixture(scope="module")
def orbit_run(scene):
    return run(scene, ts.orbit())


def converged(start, end):
    return float(np.mean(end < start / 3.0))


def test_scene_is_what_the_issue_describes(scene):
    assert (scene.cam.pixelsX, scene.cam.pixelsY) == (320, 240) and ts.N_FEAT == 16
    poses = ts.orbit()
    assert len(poses) == ts.ORBIT_FRAMES + 1 == 13 and abs(poses[-1][0][0] - 1.2) < 1e-15
    for pose in poses:  # the yaw keeps the plane's centre on the optical axis
        uv, _ = scene.true_pixels(pose, ts.CENTRE[None, :])
        np.testing.assert_allclose(uv[0], [scene.cam.cx, scene.cam.cy], atol=1e-9)
    _, pts, _, _, _, _ = scene.seed_features()
    np.testing.assert_allclose((pts - ts.CENTRE) @ ts.NORMAL, 0.0, atol=1e-12)  # the seeds lie on the tilted plane
    start = angles([None] * len(pts), pts)
    assert np.median(start) > 35.0, start  # the rule is about 40 degrees off and more
    # the rule as a slope is the rule of section 4.6
    for X in pts:
        np.testing.assert_allclose(pn.normal_of(Q0, pn.rule_pq(R0, Q0, X)), (R0 - X) / np.linalg.norm(R0 - X), atol=1e-15)


def test_convergence(scene, orbit_run):
    """True poses, true X, the orbit: the angle between the estimated and the true normal ends below a third of where
    the rule starts for at least three quarters of the features.  Measured on the committed scene: all 16 features pass;
    median 1.8 degrees, worst 2.7 degrees, from a median of 43 degrees."""
    _, pts, _, est = orbit_run
    start, end = angles([None] * len(pts), pts), angles(est, pts)
    print("start", np.round(start, 1), "end", np.round(end, 1), "median", np.median(end), "worst", end.max())
    assert converged(start, end) >= 0.75, (start, end)


def test_benefit(scene, orbit_run):
    """Last orbit frame, true pixel: the level-0 template warped with the estimated normal reaches a higher ZNCC than
    the one warped with the rule for at least three quarters of the features.  Share of features at ZNCC >= 0.8 on the
    committed scene: 0.625 with the rule, 1.0 with the estimate; the estimate is higher for all 16."""
    uv0, pts, src, est = orbit_run
    pose = ts.orbit()[-1]
    pyr = tw.pyramid(scene.render(pose, ts.ORBIT_FRAMES))
    uv, _ = scene.true_pixels(pose, pts)
    z_rule, z_est = [], []
    for i in range(len(uv0)):
        fp = np.concatenate([pts[i], np.zeros(3)])
        now = tw.window(pyr[0], tw.to_level(uv[i, 0], 0), tw.to_level(uv[i, 1], 0), tw.R)
        for z, pq in ((z_rule, None), (z_est, est[i][0] if est[i] else None)):
            out, fb, _, _ = pn.warp_templates(scene.cam, state_of(pose), fp, FEATURE_DEPTH, R0, Q0, uv0[i], src[i], uv[i], pq=pq)
            z.append(-1.0 if fb[0] else tw.zncc(out[0], now))
    z_rule, z_est = np.array(z_rule), np.array(z_est)
    print("ZNCC rule", np.round(z_rule, 3), "estimate", np.round(z_est, 3))
    print("share at 0.8: rule", np.mean(z_rule >= 0.8), "estimate", np.mean(z_est >= 0.8))
    assert np.mean(z_est > z_rule) >= 0.75, (z_rule, z_est)


def test_no_baseline_leaves_the_prior(scene):
    """pure roll: the image motion does not depend on the normal, so A = J'J is about zero: every slope stays within
    1e-6 of the rule and the information grows by less than 1e-6 of the prior's norm"""
    _, pts, _, est = run(scene, ts.roll())
    prior_norm = np.linalg.norm(pn.PRIOR_INFO * np.eye(2))
    assert all(e is not None for e in est)
    for e, X in zip(est, pts):
        assert np.abs(e[0] - pn.rule_pq(R0, Q0, X)).max() <= 1e-6, (e[0], pn.rule_pq(R0, Q0, X))
        growth = np.array([[e[1][0] - pn.PRIOR_INFO, e[1][1]], [e[1][1], e[1][2] - pn.PRIOR_INFO]])
        assert np.linalg.norm(growth) < 1e-6 * prior_norm, growth


def test_translation_compensation(scene):
    """X displaced so that the prediction is 3 px off while the anchor sits at the true pixel: the shift is removed, not
    fitted as a slope, and the estimate still meets the convergence condition (against the true normal)"""
    poses = ts.orbit()

    def displaced(pts):  # along the world x axis; 3 px at the depth of each point, seen from the last pose
        out = pts.copy()
        out[:, 0] += 3.0 * np.linalg.norm(pts - poses[-1][0], axis=1) / scene.cam.fx
        return out

    _, pts, _, est = run(scene, poses, displaced)
    off = scene.true_pixels(poses[-1], displaced(pts))[0] - scene.true_pixels(poses[-1], pts)[0]
    assert 2.0 < np.median(np.linalg.norm(off, axis=1)) < 4.0, off
    start, end = angles([None] * len(pts), pts), angles(est, pts)
    print("displaced X: end", np.round(end, 1), "median", np.median(end), "worst", end.max())
    assert converged(start, end) >= 0.75, (start, end)


def test_constants_match_the_header():
    hdr = open(os.path.join(build.CSRC, "patch_normal.h")).read()
    vals = {k: eval(v) for k, v in re.findall(r"constexpr double (PN_[A-Z_]+) = ([^;]+);", hdr)}
    assert vals == {"PN_FD_STEP": pn.FD_STEP, "PN_S_MIN": pn.S_MIN, "PN_STEP_MAX": pn.STEP_MAX, "PN_PRIOR_INFO": pn.PRIOR_INFO,
                    "PN_MIN_SS": pn.MIN_SS}, vals


def test_library_exports_the_patch_normal_calls():
    build.build_engine()
    lib = engine.load_library()
    for name in ("ekf_set_patch_normals", "ekf_refine_patch_normals", "ekf_get_patch_normals", "ekf_set_patch_normal",
                 "ekf_get_patch_normal_counts"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    assert C.sizeof(engine.EkfPatchNormal) == 72
    assert lib.ekf_set_patch_normals(None, 1) == 1  # EKF_ERR_INVALID_ARG: no engine
    assert lib.ekf_refine_patch_normals(None, None, 0) == 1
    assert lib.ekf_get_patch_normals(None, None, 0, None) == 1
    assert lib.ekf_set_patch_normal(None, 0, None, None) == 1
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_get_patch_normal_counts(None, C.byref(a), C.byref(b)) == 1
