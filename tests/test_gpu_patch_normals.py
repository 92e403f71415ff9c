"""Patch normals on the device (ekf_set_patch_normals, k_ncc_normal) against the numpy restatement
(tests/patch_normal_ref.py) on the tilted plane of tests/tilted_scene.py: the estimator, the warp that uses its estimate, the
bookkeeping through map management, the untouched paths with the mode off or no estimate yet, and the filter on the orbit."""
import os
import subprocess

import numpy as np
import pytest

import patch_normal_ref as pn
import template_warp_ref as tw
import tilted_scene as ts
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_map_points import s3_config_320
from tests.test_gpu_parity import eng_mod  # noqa: F401
from tests.test_patch_normals_cpu import angles, converged

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
N = ts.N_FEAT
R0, Q0 = ts.IDENTITY


class Orbit:
    """the scene, its orbit frames and the seeded map, rendered once for the module and never changed"""

    def __init__(self):
        self.scene = ts.TiltedScene()
        self.poses = ts.orbit()
        self.frames = [self.scene.render(p, t) for t, p in enumerate(self.poses)]
        self.uv0, self.pts, self.fpos, self.ftype, self.x13, self.P = self.scene.seed_features()
        v, w = ts.orbit_velocity()
        self.x13[7:10], self.x13[10:13] = v, np.where(w != 0, w, 2.22e-16)
        pyr0 = tw.pyramid(self.frames[0])
        self.src = np.stack([tw.source_patches(pyr0, uv) for uv in self.uv0])
        self.stored = np.stack([tw.stored_templates(pyr0, uv) for uv in self.uv0])

    def truth(self, t):
        return self.scene.true_pixels(self.poses[t], self.pts)[0]

    def engine(self, eng_mod, warp=True, normals=True, rho_sd=None):
        """map seeded on frame 0 at the true depths with the orbit's velocity as prior, templates captured there"""
        e = eng_mod.EkfEngine(self.scene.cam, self.scene.par, N + 8)
        if warp:
            e.set_template_warp(True)
        if normals:
            e.set_patch_normals(True)
        P = self.P.copy()
        if rho_sd is not None:
            k = rho_sd / self.scene.par.inverseDepthRhoSD
            rows = 13 + 6 * np.arange(N) + 5
            P[rows, :] *= k
            P[:, rows] *= k
        e.set_state(self.x13, self.fpos, self.ftype, None, P)
        e.upload_image(self.frames[0])
        e.capture_templates(np.arange(N), self.uv0)
        return e

    def matches(self, t, idx=None):
        idx = np.arange(N) if idx is None else np.asarray(idx)
        m = np.zeros(len(idx), dtype=MATCH_DTYPE)
        m["featureIndex"], m["imagePos"] = idx, np.rint(self.truth(t)[idx])
        return m


@pytest.fixture(scope="module")
def orbit():
    return Orbit()


def reference_step(o, e, t, before, bump=False):
    """the restatement for every feature: current state of e, frame t, anchors at the rounded true pixels, estimates
    `before` (patch_normals() read before the device step).  bump: every input double moved one ulp."""
    up = (lambda a: np.nextafter(np.asarray(a, dtype=np.float64), np.inf)) if bump else (lambda a: np.asarray(a, dtype=np.float64))
    x, fp, _ = e.get_state(want_P=False)
    ftype, _ = e.feature_layout()
    pyr = tw.pyramid(o.frames[t])
    anchors = np.rint(o.truth(t)).astype(int)
    out = []
    for i in range(N):
        est = (up(before["pq"][i]), up(before["info"][i])) if before["updates"][i] > 0 else None
        out.append(pn.refine(o.scene.cam, up(x), up(fp[i]), ftype[i], up(R0), up(Q0), o.uv0[i], o.src[i], pyr, anchors[i], est))
    return out


def test_estimator_equals_the_restatement(eng_mod, orbit):
    """Frame 0 captured; the state is carried to frames 3 and 8 by the motion model alone (ekf_predict: the orbit is close to
    a constant velocity); refine_patch_normals at the rounded true pixels: a first update from the rule at frame 3, a second
    from the stored estimate at frame 8.  Tolerance: the device's sin / cos may differ from the host's in the last bit of X,
    so the restatement is run again with every input double one ulp up, and 16 x the largest change of (p, q) and of the
    information it shows is allowed, with a floor of 1e-12 relative.  Measured on one MI355X: (p, q) differ by at most
    7.0e-13 (allowed 9.6e-11 there), the information by 9.6e-10 at a scale of 2.5e3 (allowed 1.3e-7)."""
    e = orbit.engine(eng_mod)
    done = 0
    for t in (3, 8):
        while done < t:
            e.predict()
            done += 1
        e.upload_image(orbit.frames[t])
        before = e.patch_normals()
        e.refine_patch_normals(orbit.matches(t))
        got = e.patch_normals()
        upd, skip = e.patch_normal_counts()
        want, moved = reference_step(orbit, e, t, before), reference_step(orbit, e, t, before, bump=True)
        assert all(w is not None for w in want) and all(m is not None for m in moved)
        assert (upd, skip) == (N, 0)
        np.testing.assert_array_equal(got["updates"], before["updates"] + 1)
        for k, field in ((0, "pq"), (1, "info")):
            ref = np.array([w[k] for w in want])
            sens = np.abs(np.array([m[k] for m in moved]) - ref).max()
            tol = max(16.0 * sens, 1e-12 * np.abs(ref).max())
            diff = np.abs(got[field] - ref).max()
            print(f"frame {t} {field}: device - restatement {diff:.3e}, one-ulp sensitivity {sens:.3e}, tolerance {tol:.3e}, scale {np.abs(ref).max():.3e}")
            assert diff <= tol, (t, field, diff, tol)
        for i in range(N):  # the reported normal is the slope's
            np.testing.assert_allclose(got["normal"][i], pn.normal_of(Q0, got["pq"][i]), atol=1e-14)


def check_templates(o, e, t, pqs, label):
    """match on frame t; the compared templates against the reference warp with the slopes pqs (None: the rule), with the
    exemption of tests/test_gpu_template_warp.py for samples within 1e-6 of a rounding boundary"""
    preds, _, _ = e.predict_measurements()
    e.upload_image(o.frames[t])
    e.match_ncc()
    got = e.match_templates(np.arange(N))
    x, fp, _ = e.get_state(want_P=False)
    ftype, _ = e.feature_layout()
    want, dist = o.stored.copy(), np.full((N, 3, 11, 11), np.inf)
    for p in preds:
        i = int(p["featureIndex"])
        want[i], _, dist[i], _ = pn.warp_templates(o.scene.cam, x, fp[i], ftype[i], R0, Q0, o.uv0[i], o.src[i], p["imagePos"], o.stored[i], pq=pqs[i])
    close = dist < 1e-6
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert len(preds) > 0 and np.isfinite(dist).any(), label
    assert not (diff[~close] != 0).any(), (label, int((diff[~close] != 0).sum()))
    assert (diff[close] <= 1).all() and close.sum() <= 0.01 * np.isfinite(dist).sum(), label
    return got


def test_the_warp_uses_the_estimate(eng_mod, orbit):
    e = orbit.engine(eng_mod)
    for _ in range(3):
        e.predict()
    pqs = [None] * N
    for i in range(0, N, 2):  # every other feature: a slope well away from the rule; the others keep the rule
        pqs[i] = np.array([0.8 - 0.02 * i, 0.05 * (i % 3) - 0.05])
        e.set_patch_normal(i, pqs[i])
    with_est = check_templates(orbit, e, 3, pqs, "chosen slopes")
    rule = orbit.engine(eng_mod, normals=False)
    for _ in range(3):
        rule.predict()
    without = check_templates(orbit, rule, 3, [None] * N, "warp only")
    assert (with_est[0::2] != without[0::2]).any()  # the slope changes the rendering
    np.testing.assert_array_equal(with_est[1::2], without[1::2])


def test_no_estimate_means_the_same_bytes(eng_mod, orbit):
    both = [orbit.engine(eng_mod, normals=on) for on in (True, False)]
    out = []
    for e in both:
        for _ in range(4):
            e.predict()
        e.predict_measurements()
        e.upload_image(orbit.frames[4])
        m = e.match_ncc()
        out.append((m, e.match_templates(np.arange(N)), e.template_warp_counts()))
    assert out[0][2] == out[1][2] and out[0][2][0] > 0
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert (both[0].patch_normals()["updates"] == 0).all()


def test_mode_off_changes_nothing(eng_mod, orbit):
    """image steps after the mode was on and off again: states bitwise equal to an engine that never had it on
    (launch-per-panel sweep: the run-to-run reproducible one)"""
    states = []
    for toggled in (False, True):
        e = orbit.engine(eng_mod, normals=False)
        e.set_sweep_mode(4)
        if toggled:
            e.set_patch_normals(True)
            e.set_patch_normals(False)
        infos = [e.step_image(orbit.frames[t]) for t in (1, 2, 3)]
        states.append((e.get_state(), [(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1] and states[0][1][-1][1] > 0
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_through_the_filter(eng_mod, orbit):
    """The orbit through ekf_step_image, one engine per setting, the same frames.  With the mode on: the normals meet the
    CPU convergence condition, at least three quarters of the features in view are matched in the last frame, and strictly
    more than with the warp alone."""
    on, off = orbit.engine(eng_mod), orbit.engine(eng_mod, normals=False)
    for t in range(1, len(orbit.frames)):
        i_on, i_off = on.step_image(orbit.frames[t]), off.step_image(orbit.frames[t])
        assert i_on.status == 0 and i_off.status == 0
        upd, skip = on.patch_normal_counts()
        assert upd + skip == i_on.n_inliers + i_on.n_rescued, (t, upd, skip, i_on.n_inliers, i_on.n_rescued)
        print(f"frame {t}: matches on / off {i_on.n_matches} / {i_off.n_matches}, normals updated {upd} skipped {skip}")
    got = on.patch_normals()
    est = [(g["pq"], g["info"]) if g["updates"] > 0 else None for g in got]
    start, end = angles([None] * N, orbit.pts), angles(est, orbit.pts)
    truth, cam = orbit.truth(len(orbit.frames) - 1), orbit.scene.cam
    in_view = int(((truth[:, 0] > 0) & (truth[:, 0] < cam.pixelsX) & (truth[:, 1] > 0) & (truth[:, 1] < cam.pixelsY)).sum())
    msg = (f"{in_view} features in view; last frame: {i_on.n_matches} matches with the patch normals, {i_off.n_matches} with the warp "
           f"alone; normals: median {np.median(end):.1f} deg, worst {end.max():.1f} deg, from a median of {np.median(start):.1f} deg")
    print(msg)
    assert converged(start, end) >= 0.75, msg
    assert i_on.n_matches >= 0.75 * in_view, msg
    assert i_on.n_matches > i_off.n_matches, msg


def test_tables_follow_map_management(eng_mod, orbit):
    e = orbit.engine(eng_mod, rho_sd=0.002)  # depths known well enough for the conversion (tests/test_gpu_template_warp.py)
    for i in range(N):
        e.set_patch_normal(i, [0.01 * i, -0.02 * i], [2.0 + i, 0.5, 3.0 + i])
    keep = np.arange(N)

    def check(label):
        got = e.patch_normals()
        np.testing.assert_array_equal(got["pq"], np.stack([0.01 * keep, -0.02 * keep], axis=1), err_msg=label)
        np.testing.assert_array_equal(got["info"], np.stack([2.0 + keep, np.full(len(keep), 0.5), 3.0 + keep], axis=1), err_msg=label)
        assert (got["updates"] == 1).all(), label

    drop = np.array([1, 2, 9], dtype=np.int32)
    e.remove_features(drop)
    keep = np.setdiff1d(keep, drop)
    check("after remove_features")
    converted = e.convert_inverse_depth_to_depth()
    assert converted >= 0 and e.feature_layout()[0][converted] == 1
    check("after a conversion")
    # remove_bad_features: two features are re-captured on a frame that shows nothing (which resets their estimates and leaves
    # them unmatchable); one image step with the mode off (the tables stay) and they are the bad ones
    e.set_patch_normals(False)
    e.upload_image(np.full_like(orbit.frames[0], 118))
    e.capture_templates(np.array([0, 1], dtype=np.int32), orbit.uv0[keep[:2]])
    assert e.step_image(orbit.frames[1]).n_matches >= len(keep) - 4
    before = e.patch_normals()
    removed = e.remove_bad_features()
    after = e.patch_normals()
    assert removed >= 2 and len(after) == len(before) - removed and (after["updates"] == 1).all()
    rows = [tuple(r) for r in before["pq"][before["updates"] == 1]]
    it = iter(rows)
    assert all(any(tuple(a) == b for b in it) for a in after["pq"]), "the survivors keep their records, in map order"
    # a re-capture resets the estimate
    e2 = orbit.engine(eng_mod)
    e2.predict()
    e2.upload_image(orbit.frames[1])
    e2.refine_patch_normals(orbit.matches(1))
    assert (e2.patch_normals()["updates"] == 1).all()
    e2.capture_templates(np.array([0, 5], dtype=np.int32), orbit.truth(1)[[0, 5]])
    upd = e2.patch_normals()["updates"]
    assert upd[0] == 0 and upd[5] == 0 and upd.sum() == N - 2


def test_refusals_and_mode_switches(eng_mod, orbit):
    seq = SyntheticSequence(12, 1)
    s = eng_mod.EkfEngine(seq.cam, seq.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_patch_normals(True)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.close()
    e = eng_mod.EkfEngine(orbit.scene.cam, orbit.scene.par, N)
    with pytest.raises(eng_mod.EkfError) as ex:  # the warp is off
        e.set_patch_normals(True)
    assert ex.value.code == 1
    e.set_template_warp(True)
    e.set_patch_normals(True)
    e.set_template_warp(False)  # clears the mode
    e.set_template_warp(True)
    e.set_state(orbit.x13, orbit.fpos, orbit.ftype, None, orbit.P)
    e.upload_image(orbit.frames[0])
    e.capture_templates(np.arange(N), orbit.uv0)
    with pytest.raises(eng_mod.EkfError) as ex:  # the mode is off: no estimator stage
        e.refine_patch_normals(orbit.matches(0))
    assert ex.value.code == 1
    e.step_image(orbit.frames[1])
    assert (e.patch_normals()["updates"] == 0).all()


def test_keypoint_matcher_ignores_the_mode(eng_mod):
    seq = SyntheticSequence(50, 3)
    states = []
    for normals in (False, True):
        e = eng_mod.EkfEngine(seq.cam, seq.par, 64, max_keypoints=4096)
        e.set_sweep_mode(4)
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, 1e9)
        if normals:
            e.set_template_warp(True)
            e.set_patch_normals(True)
        e.upload_image(seq.render_image(0))
        desc = e.describe(seq.pixel_positions(0).astype(np.float64))
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc, seq.P0)
        infos = [e.step_image(seq.render_image(t)) for t in (1, 2, 3)]
        assert e.patch_normal_counts() == (0, 0)
        states.append((e.get_state(), [(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1] and states[0][1][-1][1] > 0
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_counters(eng_mod, orbit):
    """updated + skipped = the features handed to the estimator; a feature without a source patch is skipped"""
    e = orbit.engine(eng_mod)
    e.set_template_warp(False)  # a capture with the warp off keeps no source patch (and clears the mode)
    e.capture_templates(np.array([3, 4], dtype=np.int32), orbit.uv0[[3, 4]])
    e.set_template_warp(True)
    e.set_patch_normals(True)
    e.predict()
    e.upload_image(orbit.frames[1])
    idx = np.array([0, 3, 4, 7, 11])
    e.refine_patch_normals(orbit.matches(1, idx))
    assert e.patch_normal_counts() == (3, 2)
    np.testing.assert_array_equal(e.patch_normals(idx)["updates"], [1, 0, 0, 1, 1])
    e.refine_patch_normals(orbit.matches(1, idx[:0]))
    assert e.patch_normal_counts() == (0, 0)


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setPatchNormals on the committed frames, ekf_sequence --patch-normals, and nx ny nz in map.ply with the
    mode on only"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check, sample = str(tmp_path / "patch_normals_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "patch_normals_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check, str(cfg), SEQ + "/", "1e10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 7 and sum(int(s[-3]) for s in steps) > 0, r.stdout  # "... normals updated U skipped S"
    for flag, has in (("--patch-normals", True), ("--warp-templates", False)):
        out = tmp_path / ("out" + flag)
        out.mkdir()
        r = subprocess.run([sample, str(cfg), SEQ + "/", str(out) + "/", flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (sum("patch normals updated" in ln for ln in r.stdout.splitlines()) == 7) == has
        header = (out / "map.ply").read_text().split("end_header")[0]
        assert ("property double nx" in header or "property float nx" in header) == has, header
