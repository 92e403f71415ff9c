"""Sub-pixel NCC matches on the device (ekf_set_subpixel_matches, k_ncc_match<true>) against the numpy restatement of the
fit (tests/ncc_subpixel_ref.py): the positions bit for bit, the counts, the rule's fall-back cases on crafted frames, the
untouched mode-off path against the oracle, the mode through the filter, the refusals and the C++ seam.

The reference takes the integer best pixel as an input.  It comes from the same engine's mode-off match of the same state
and frame, which the oracle defines (test_gpu_ncc.py); the mode may not change which features match, their order or their
distances, and that is asserted first."""
import os
import subprocess

import numpy as np
import pytest

import ncc_subpixel_ref as sp
import template_warp_ref as tw
import warp_scene as ws
from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, s3_camera, s3_params
from openekfmonoslam_amd.synth import SyntheticSequence, initial_state_and_covariance, seed_map
from tests.test_gpu_map_points import s3_config_320
from tests.test_gpu_parity import eng_mod, make_pair  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
IDENTITY = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))
N_FEAT, FRAMES = 24, 10
# sideways: 0.0213 world units in 8 frames, ~0.35 px of image motion per frame (test_ncc_subpixel_cpu.py); roll: 2 degrees per frame
SCENES = {"sideways": 0.0213 * FRAMES / 8, "roll": 20.0}


@pytest.fixture(scope="module")
def scene():
    return ws.PlaneScene()


class Run:
    """an engine on one scene: map seeded on frame 0 with the true velocity as prior, templates captured there"""

    def __init__(self, eng_mod, scene, kind, warp=False, subpix=False):
        amount = SCENES[kind]
        self.scene = scene
        self.poses = ws.trajectory(kind, FRAMES, amount)
        self.uv0, self.pts, fpos, ftype, x13, P = scene.seed_features(N_FEAT)
        v, w = ws.velocity(kind, FRAMES, amount)
        x13[7:10] = v
        x13[10:13] = np.where(w != 0, w, 2.22e-16)
        self.e = e = eng_mod.EkfEngine(scene.cam, scene.par, N_FEAT + 16)
        if warp:
            e.set_template_warp(True)
        if subpix:
            e.set_subpixel_matches(True)
        e.set_state(x13, fpos, ftype, None, P)
        e.upload_image(scene.render(IDENTITY, 0))
        e.capture_templates(np.arange(N_FEAT), self.uv0)

    def frame(self, t):
        return self.scene.render(self.poses[t], t)


def off_and_on(e):
    """the match of the uploaded frame from the engine's current predictions, mode off and then on"""
    e.set_subpixel_matches(False)
    off = e.match_ncc().copy()
    assert e.subpixel_counts() == (0, 0)
    e.set_subpixel_matches(True)
    on = e.match_ncc().copy()
    counts = e.subpixel_counts()
    e.set_subpixel_matches(False)
    return off, on, counts


def check_against_reference(e, off, on, counts, label):
    """-> (reference positions float32 [M, 2], fitted flags bool [M, 2])"""
    assert len(on) == len(off) and len(on) > 0, (label, len(on), len(off))
    for f in ("featureIndex", "keypointIndex", "distance"):
        np.testing.assert_array_equal(on[f], off[f], err_msg=f"{label}: {f}")
    np.testing.assert_array_equal(off["imagePos"], np.rint(off["imagePos"]), err_msg=f"{label}: mode off is not at integer pixels")
    level0 = e.image_level(0)
    tmpl = e.match_templates(on["featureIndex"])[:, 0]  # what the last match compared: re-rendered with the template warp
    want, fitted = np.zeros((len(on), 2), dtype=np.float32), np.zeros((len(on), 2), dtype=bool)
    for j in range(len(on)):
        bx, by = off["imagePos"][j]
        want[j, 0], want[j, 1], fitted[j, 0], fitted[j, 1] = sp.refine(level0, tmpl[j], int(bx), int(by))
    got = on["imagePos"]
    print(f"{label}: {len(on)} matches, axes fitted {int(fitted.sum())} of {fitted.size}, device counts {counts}, "
          f"largest move {np.abs(got - off['imagePos']).max():.4f} px")
    np.testing.assert_array_equal(got.astype(np.float32), want, err_msg=label)
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{label}: positions are not float32 values")
    assert np.abs(got - off["imagePos"]).max() <= 0.5
    assert counts == (int(fitted.sum()), int((~fitted).sum())), (label, counts)
    assert counts[0] + counts[1] == 2 * len(on)
    return want, fitted


def test_device_equals_reference(eng_mod, scene):
    """sideways scene, frames 1 to 4: from one state, the mode changes imagePos only, to the reference's float32 bits"""
    run = Run(eng_mod, scene, "sideways")
    e = run.e
    fitted_axes = axes = 0
    for t in range(1, 5):
        e.predict_measurements()
        e.upload_image(run.frame(t))
        off, on, counts = off_and_on(e)
        assert len(on) >= 0.75 * N_FEAT
        _, fitted = check_against_reference(e, off, on, counts, f"sideways, frame {t}")
        fitted_axes += int(fitted.sum())
        axes += fitted.size
        assert e.step_image(run.frame(t)).status == 0  # (mode off) the filter moves on to the next frame
    # the CPU experiment fits every axis of this scene; a kernel that always falls back must not pass
    assert fitted_axes >= 0.9 * axes, (fitted_axes, axes)


def test_warp_and_fit_together(eng_mod, scene):
    """roll scene with the template warp: the fit uses the re-rendered level-0 template"""
    run = Run(eng_mod, scene, "roll", warp=True)
    e = run.e
    for t in (1, 2):
        assert e.step_image(run.frame(t)).status == 0
    e.predict_measurements()
    e.upload_image(run.frame(3))
    off, on, counts = off_and_on(e)
    ok, _ = e.template_warp_counts()
    assert ok > 0
    stored = np.stack([tw.stored_templates(tw.pyramid(scene.render(IDENTITY, 0)), uv)[0] for uv in run.uv0])
    assert (e.match_templates(on["featureIndex"])[:, 0] != stored[on["featureIndex"]]).any()  # the warp changed what is compared
    _, fitted = check_against_reference(e, off, on, counts, "roll with the template warp, frame 3")
    assert fitted.any()


def crafted_frame(w=320, h=240, seed=21):
    """random values, 3 x 3 box-blurred so that windows one pixel apart correlate"""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    return np.rint(sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0).astype(np.uint8)


def test_border_and_flat_cases(eng_mod):
    """no motion, templates captured from the matched frame itself, 320 x 240.
    Features 0..3 sit in the outermost column / row (the prediction stage admits 0 < u < W, 0 < v < H, so a feature at
    u = 0.3 is predicted and its level-0 pixel is column 0): the axis whose neighbour leaves the frame stays at the integer,
    the other one equals the reference.  Feature 4's best pixel is (115, 120) in a frame that is constant over columns
    80..119: the window of (114, 120) is constant, its key is -1, and x stays at the integer.  Feature 5 is an ordinary one."""
    W, H = 320, 240
    cam, par = s3_camera(W, H), s3_params()
    img = crafted_frame(W, H)
    img[:, 80:120] = 100
    uv0 = np.array([[0.3, 100.3], [W - 0.7, 60.0], [150.0, 0.3], [200.0, H - 0.7], [115.0, 120.0], [250.0, 150.0]])
    cells = [(0, 100), (W - 1, 60), (150, 0), (200, H - 1), (115, 120), (250, 150)]
    want_fit = [(False, True), (False, True), (True, False), (True, False), (False, None), (True, True)]
    n = len(uv0)
    x13, P13 = initial_state_and_covariance(par)
    fpos, P = seed_map(cam, par, x13, P13, uv0)
    e = eng_mod.EkfEngine(cam, par, n + 8)
    e.set_state(x13, fpos, np.full(n, FEATURE_INVERSE_DEPTH, dtype=np.int32), None, P)
    e.upload_image(img)
    e.capture_templates(np.arange(n), uv0)
    preds, _, _ = e.predict_measurements()
    assert len(preds) == n, "the prediction stage did not admit a border feature"
    off, on, counts = off_and_on(e)
    np.testing.assert_array_equal(off["featureIndex"], np.arange(n))
    np.testing.assert_array_equal(off["imagePos"], np.array(cells, dtype=np.float64))
    _, fitted = check_against_reference(e, off, on, counts, "border and flat cases")
    for i, (fx, fy) in enumerate(want_fit):
        assert fitted[i, 0] == fx and (fy is None or fitted[i, 1] == fy), (i, fitted[i])
    for i, (cx, cy) in enumerate(cells):  # the axis that fell back is the integer, exactly
        if not fitted[i, 0]:
            assert on["imagePos"][i, 0] == cx
        if not fitted[i, 1]:
            assert on["imagePos"][i, 1] == cy
    lvl = e.image_level(0)
    assert sp.neighbour_key(lvl, e.match_templates([4])[0, 0], 114, 120) == -1.0


@pytest.mark.parametrize("nfeat", [12, 50])
def test_mode_off_is_todays_path(eng_mod, oracle_lib, nfeat):
    """enabled and then disabled: matches identical to the oracle's, as test_gpu_ncc.test_match_ncc_identical checks them"""
    seq = SyntheticSequence(nfeat, 3)
    e, o = make_pair(eng_mod, oracle_lib, seq)
    e.set_subpixel_matches(True)
    e.set_subpixel_matches(False)
    img0, uv0 = seq.render_image(0), seq.pixel_positions(0).astype(np.float64)
    e.upload_image(img0)
    e.capture_templates(np.arange(nfeat), uv0)
    o.set_image(img0)
    o.capture_templates(np.arange(nfeat), uv0)
    for t in (1, 2):
        e.predict()
        o.predict()
        e.predict_measurements()
        preds, _, _ = o.predict_measurements()
        img = seq.render_image(t)
        e.upload_image(img)
        o.set_image(img)
        mg, mo = e.match_ncc(), o.match_ncc(preds)
        assert len(mg) == len(mo) and len(mo) > 0.6 * nfeat
        for f in ("featureIndex", "keypointIndex", "imagePos", "distance"):
            np.testing.assert_array_equal(mg[f], mo[f])
        assert e.subpixel_counts() == (0, 0)


def test_through_the_filter(eng_mod, scene):
    """ten sideways frames through ekf_step_image with the mode on: every step EKF_OK, counts consistent, and on frame 1
    (where both engines hold the same state) no fewer matches than with the mode off.  The final camera-position errors
    are printed for DESIGN.md 4.7; nothing is promised about them."""
    on, off = Run(eng_mod, scene, "sideways", subpix=True), Run(eng_mod, scene, "sideways")
    for t in range(1, FRAMES + 1):
        img = on.frame(t)
        i_on, i_off = on.e.step_image(img), off.e.step_image(img)
        assert i_on.status == 0 and i_off.status == 0
        a, b = on.e.subpixel_counts()
        assert a + b == 2 * i_on.n_matches and a > 0, (t, a, b, i_on.n_matches)
        assert off.e.subpixel_counts() == (0, 0)
        if t == 1:
            assert i_on.n_matches >= i_off.n_matches and i_on.n_matches >= 0.75 * N_FEAT
    r_true = on.poses[FRAMES][0]
    errs = [float(np.linalg.norm(r.e.get_state(want_P=False)[0][:3] - r_true)) for r in (on, off)]
    print(f"sideways, {FRAMES} frames, camera moved {np.linalg.norm(r_true):.5f}: final position error with the fit {errs[0]:.3e}, "
          f"without {errs[1]:.3e}; matches in the last frame {i_on.n_matches} / {i_off.n_matches}")


def test_sharded_engine_refuses(eng_mod):
    seq = SyntheticSequence(12, 1)
    s = eng_mod.EkfEngine(seq.cam, seq.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_subpixel_matches(True)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.close()


def test_keypoint_matcher_ignores_the_mode(eng_mod):
    seq = SyntheticSequence(50, 3)
    states = []
    for subpix in (False, True):
        e = eng_mod.EkfEngine(seq.cam, seq.par, 64, max_keypoints=4096)
        e.set_sweep_mode(4)  # the run-to-run reproducible sweep (test_gpu_ncc.test_staged_images_equal_direct_steps)
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, 1e9)
        if subpix:
            e.set_subpixel_matches(True)
        e.upload_image(seq.render_image(0))
        desc = e.describe(seq.pixel_positions(0).astype(np.float64))
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc, seq.P0)
        infos = [e.step_image(seq.render_image(t)) for t in (1, 2, 3)]
        assert e.subpixel_counts() == (0, 0)
        states.append((e.get_state(), [(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1] and states[0][1][-1][1] > 0
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setSubpixelMatches(true) on the committed frames: non-integer imagePos; ekf_sequence --subpixel prints the counts"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check, sample = str(tmp_path / "subpixel_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "subpixel_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check, str(cfg), SEQ + "/", "1e10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 7
    assert all(int(s[7]) + int(s[9]) == 2 * int(s[5]) for s in steps) and sum(int(s[7]) for s in steps) > 0
    last = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("match")]
    assert len(last) == 1 and int(last[0][1]) > 0 and int(last[0][3]) > 0  # matches, axes at a non-integer position
    r = subprocess.run([sample, str(cfg), SEQ + "/", "--subpixel"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum("axes refined" in ln for ln in r.stdout.splitlines()) == 7
