"""Wide search on the device (ekf_set_ncc_wide_search: k_ncc_wide_classify, k_ncc_wide_coarse, k_ncc_wide_finish) against the
numpy restatement of the whole NCC search (tests/ncc_wide_ref.py, pinned to the oracle by test_ncc_wide_cpu.py): which
features match, their positions and their distance bits, and the wide counts; the threshold between the two paths, gates
larger than the frame, ties across tiles, the three modes together, the untouched mode-off path, the mode through the
filter, the refusals and the C++ seam.

The reference is fed what the engine returns: its pyramid levels, its predictions and the templates its last match
compared."""
import os
import subprocess

import numpy as np
import pytest

import ncc_wide_ref as wr
import warp_scene as ws
import wide_scene as wsn
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_map_points import s3_config_320
from tests.test_gpu_parity import eng_mod, make_pair  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
IDENTITY = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))


@pytest.fixture(scope="module")
def displaced():
    return wsn.DisplacedScene()


def device(e, wide, subpix=False):
    """the match of the uploaded frame from the engine's current predictions -> (matches, wide counts)"""
    e.set_ncc_wide_search(wide)
    e.set_subpixel_matches(subpix)
    m = e.match_ncc().copy()
    return m, e.ncc_wide_counts()


def reference(e, oracle_lib, preds, max_rad, subpix=False):
    """after a device match: the restatement on the engine's own pyramid, predictions and compared templates"""
    o = oracle_lib.Oracle(wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params(), 1)  # the gate functions only: they take no camera
    levels = [e.image_level(l) for l in range(3)]
    return wr.match_all(o, levels, preds, e.match_templates(preds["featureIndex"]), max_rad, subpix)


def engine_with(eng_mod, cam, par, uv, P, frame0, frame1):
    x13, fpos, ftype = wsn.seeded(cam, par, uv)
    e = eng_mod.EkfEngine(cam, par, len(uv) + 8)
    e.set_state(x13, fpos, ftype, None, P)
    e.upload_image(frame0)
    e.capture_templates(np.arange(len(uv)), uv)
    e.upload_image(frame1)
    preds, _, _ = e.predict_measurements()
    assert len(preds) == len(uv)
    return e, preds


def test_device_equals_reference(eng_mod, oracle_lib, displaced):
    """displaced targets 100 px away in gates of about 150 px: on = the uncapped reference (all eight found, at a distance
    of exactly 0), off = the capped one (none found)"""
    sc = displaced
    e = eng_mod.EkfEngine(sc.cam, sc.par, 16)
    sc.load(e)
    preds, _, _ = e.predict_measurements()
    on, counts = device(e, True)
    want, slots, want_counts, _ = reference(e, oracle_lib, preds, None)
    print(f"on: {len(on)} matches, wide counts {counts}; reference {len(want)} matches, {want_counts}")
    wr.assert_matches_equal(on, want, "mode on")
    assert counts == want_counts and counts[0] == sc.n
    np.testing.assert_array_equal(on["imagePos"], sc.target)
    off, counts = device(e, False)
    want, _, _, _ = reference(e, oracle_lib, preds, wr.MAXRAD)
    wr.assert_matches_equal(off, want, "mode off")
    assert counts == (0, 0) and len(off) <= 1


def test_threshold(eng_mod, oracle_lib, displaced):
    """gates whose rounded major semi-axis straddles 63 / 64, matched on the frame the templates come from (every feature
    matches at its prediction): <= 63 is today's path and is not counted, >= 64 is counted"""
    sc = displaced
    target = np.array([61.0, 62.0, 62.8, 63.3, 63.7, 64.3, 65.0, 66.0])
    o = oracle_lib.Oracle(sc.cam, sc.par, 1)
    axes = target.copy()
    e, preds = engine_with(eng_mod, sc.cam, sc.par, sc.UV, wsn.diag_P(sc.cam, sc.n, axes, 0.5 * axes), sc.frame0, sc.frame0)
    x13, fpos, ftype = wsn.seeded(sc.cam, sc.par, sc.UV)
    for _ in range(3):  # S is not exactly the diagonal diag_P aims at (R, the projection off the centre): scale P towards the targets
        axes *= target / np.array([o.ellipse(p["covarianceMatrix"])[0].max() for p in preds])
        e.set_state(x13, fpos, ftype, None, wsn.diag_P(sc.cam, sc.n, axes, 0.5 * axes))
        preds, _, _ = e.predict_measurements()
    major = np.array([int(np.rint(o.ellipse(p["covarianceMatrix"])[0].max())) for p in preds])
    print("rounded major semi-axes:", major.tolist())
    assert (major <= 63).sum() >= 2 and (major >= 64).sum() >= 2 and 63 in major and 64 in major
    off, _ = device(e, False)
    on, counts = device(e, True)
    want, slots, want_counts, _ = reference(e, oracle_lib, preds, None)
    assert [s["wide"] for s in slots] == (major >= 64).tolist()
    assert counts == want_counts and counts[0] == int((major >= 64).sum())
    wr.assert_matches_equal(on, want, "mode on")
    assert len(off) == sc.n
    narrow = major[off["featureIndex"]] <= 63
    wr.assert_matches_equal(on[np.isin(on["featureIndex"], off["featureIndex"][narrow])], off[narrow], "slots below the threshold")


def test_gate_larger_than_frame_and_off_frame(eng_mod, oracle_lib):
    """feature 0: a gate of about 2000 px, the box is the whole 80 x 60 level (all six tiles) and the target anywhere in the
    frame is found; feature 1: predicted 3 px from the corner with a gate of about 120 px; feature 2: a gate whose minor
    semi-axis rounds to 0.  The prediction stage returns S = H P H' + I, so a covariance cannot bring an axis below 4.9 px; the
    degenerate S comes from a P whose phi variance c is negative.  S is linear in c: two predictions give S(c) = Sa + c Sb, and
    c is bisected in numpy until the smaller eigenvalue of S(c) is 0.002.  Nothing but the prediction stage sees that P."""
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
    uv = np.array([[160.0, 120.0], [3.0, 3.0], [200.0, 60.0]])
    frame0 = wr.blurred_noise(wsn.H, wsn.W, 51)
    frame1 = wr.blurred_noise(wsn.H, wsn.W, 52)
    frame1[8:72, 240:304] = frame0[88:152, 128:192]      # feature 0: (160, 120) -> (272, 40)
    frame1[60:124, 40:104] = frame0[0:64, 0:64]          # feature 1: (3, 3) -> (43, 63)
    frame1[28:92, 108:172] = frame0[28:92, 168:232]      # feature 2: (200, 60) -> (140, 60), along its gate's only axis
    P = wsn.diag_P(cam, 3, [2000.0, 88.0, 150.0], [2000.0, 88.0, 50.0])
    e, preds = engine_with(eng_mod, cam, par, uv, P, frame0, frame1)
    i, state = 13 + 6 * 2 + 4, wsn.seeded(cam, par, uv)
    c0, S0 = P[i, i], preds[2]["covarianceMatrix"].reshape(2, 2).copy()
    P[i, i] = 0.0
    e.set_state(*state, None, P)
    Sa = e.predict_measurements()[0][2]["covarianceMatrix"].reshape(2, 2).copy()
    Sb = (S0 - Sa) / c0
    lo, hi = -c0, 0.0  # smallest eigenvalue: negative at lo, >= 1 at hi, increasing in c
    assert np.linalg.eigvalsh(Sa + lo * Sb)[0] < 0.0
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if np.linalg.eigvalsh(Sa + mid * Sb)[0] < 0.002 else (lo, mid)
    P[i, i] = hi
    e.set_state(*state, None, P)
    preds, _, _ = e.predict_measurements()
    assert 0.001 < np.linalg.eigvalsh(preds[2]["covarianceMatrix"].reshape(2, 2))[0] < 0.004
    on, counts = device(e, True)
    want, slots, want_counts, _ = reference(e, oracle_lib, preds, None)
    print([(s["major"], s["minor"], s["ncand"], s["valid"], s["bx"], s["by"]) for s in slots], counts)
    assert slots[0]["major"] >= 1900 and slots[0]["ncand"] == 80 * 60
    assert 100 <= slots[1]["major"] <= 140 and slots[2]["minor"] == 0 and all(s["wide"] for s in slots)
    wr.assert_matches_equal(on, want, "mode on")
    assert counts == want_counts
    assert on["featureIndex"][0] == 0
    np.testing.assert_array_equal(on["imagePos"][0], [272.0, 40.0])


def test_ties_across_tiles(eng_mod, oracle_lib):
    """a frame that repeats every 32 px (8 coarse pixels), a template cut from it and a gate over more than three periods:
    coarse candidates in different tiles have identical integer sums, and the first in raster order has to win"""
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
    frame = wsn.periodic_frame(32)
    uv = np.array([[160.0, 120.0]])
    e, preds = engine_with(eng_mod, cam, par, uv, wsn.diag_P(cam, 1, 150.0, 150.0), frame, frame)
    on, counts = device(e, True)
    want, slots, want_counts, _ = reference(e, oracle_lib, preds, None)
    s = slots[0]
    print(f"{len(s['best'])} coarse candidates share the best key {s['key']}, in tiles {s['tiles']}; first {s['best'][0]}")
    assert len(s["best"]) >= 2 and len(s["tiles"]) >= 2, "the reference saw no tie across tiles: the test would pass vacuously"
    assert s["valid"] and len(on) == 1
    wr.assert_matches_equal(on, want, "ties")
    assert counts == want_counts
    assert (on["imagePos"][0] != uv[0]).any()  # not the prediction itself: an earlier period in raster order


def test_with_warp_and_subpixel(eng_mod, oracle_lib):
    """the 20 degree roll scene of tests/warp_scene.py at 320 x 240 with direction uncertainty added to every feature:
    template warp, sub-pixel fit and wide search in one match equal the reference fed the re-rendered templates"""
    n_feat, frames = 16, 10
    scene = ws.PlaneScene(wsn.W, wsn.H)
    poses = ws.trajectory("roll", frames, 20.0)
    uv0, _, fpos, ftype, x13, P = scene.seed_features(n_feat, margin=60.0)
    v, w = ws.velocity("roll", frames, 20.0)
    x13[7:10], x13[10:13] = v, np.where(w != 0, w, 2.22e-16)
    axes = np.where(np.arange(n_feat) % 4 == 3, 40.0, 110.0)  # three in four beyond the threshold
    e = eng_mod.EkfEngine(scene.cam, scene.par, n_feat + 8)
    e.set_template_warp(True)
    e.set_state(x13, fpos, ftype, None, P + wsn.diag_P(scene.cam, n_feat, axes, axes))
    e.upload_image(scene.render(IDENTITY, 0))
    e.capture_templates(np.arange(n_feat), uv0)
    for _ in range(3):
        e.predict()
    preds, _, _ = e.predict_measurements()
    e.upload_image(scene.render(poses[3], 3))
    off, _ = device(e, False, subpix=True)
    warp_off = e.template_warp_counts()
    on, counts = device(e, True, subpix=True)
    assert e.template_warp_counts() == warp_off and warp_off[0] > 0
    fit = e.subpixel_counts()
    want, slots, want_counts, want_fit = reference(e, oracle_lib, preds, None, subpix=True)
    print(f"{len(on)} matches (mode off {len(off)}), wide counts {counts}, axes fitted / integer {fit}")
    assert sum(s["wide"] for s in slots) >= len(preds) / 2
    wr.assert_matches_equal(on, want, "warp + sub-pixel + wide")
    assert counts == want_counts and fit == want_fit and fit[0] + fit[1] == 2 * len(on) and len(on) > 0


@pytest.mark.parametrize("nfeat", [12, 50])
def test_mode_off_is_todays_path(eng_mod, oracle_lib, nfeat):
    """enabled and then disabled: matches identical to the oracle's, as test_gpu_ncc.test_match_ncc_identical checks them;
    and on a frame without a wide gate the mode changes nothing and counts nothing"""
    seq = SyntheticSequence(nfeat, 3)
    e, o = make_pair(eng_mod, oracle_lib, seq)
    e.set_ncc_wide_search(True)
    e.set_ncc_wide_search(False)
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
        mo = o.match_ncc(preds)
        assert len(mo) > 0.6 * nfeat
        wr.assert_matches_equal(e.match_ncc(), mo, f"frame {t}, before the toggle")
        assert e.ncc_wide_counts() == (0, 0)
        on, counts = device(e, True)
        off, _ = device(e, False)
        wr.assert_matches_equal(off, mo, f"frame {t}, on -> off")
        assert e.ncc_wide_counts() == (0, 0)
        n_wide = sum(((int(np.rint(o.ellipse(p["covarianceMatrix"])[0].max())) >> 2) + 1) > wr.MAXRAD for p in preds)
        assert counts[0] == n_wide
        if n_wide == 0:
            wr.assert_matches_equal(on, mo, f"frame {t}, mode on without a wide gate")
            assert counts == (0, 0)
        elif t == 1:
            pytest.fail("frame 1 was chosen for having no wide gate")


def test_reacquires_through_the_filter(eng_mod, oracle_lib):
    """Six frames of the textured plane at 320 x 240 through ekf_step_image.  The camera rests for frames 0 and 1 and has
    jumped sideways by 90 px of image motion (a translation parallel to the plane: the whole frame shifts) from frame 2
    on.  Before frame 2 the camera position's variance is inflated once through set_state (gates of about 150 px).
    Mode on: the filter re-acquires, at least half the map are RANSAC inliers at frame 3.  Mode off: at most 1.
    How the scene was checked: before frame 2 is stepped, the numpy reference is run on each engine's own predictions
    and frame -- uncapped it finds at least half the map within 1.5 px of the true pixels, capped at most one -- so what
    the filter is asked to do is decided by the matching stage alone; both are asserted below."""
    n_feat, jump_px = 16, 90.0
    scene = ws.PlaneScene(wsn.W, wsn.H)
    uv0, pts, fpos, ftype, x13, P = scene.seed_features(n_feat, margin=100.0, min_sep=12)
    moved = (np.array([jump_px * ws.PLANE_Z / scene.cam.fx, 0.0, 0.0]), IDENTITY[1])
    poses = [IDENTITY, IDENTITY] + [moved] * 4
    truth, _ = scene.true_pixels(moved, pts)
    sigma = 150.0 / wsn.AXIS_PER_SIGMA * ws.PLANE_Z / scene.cam.fx  # camera position, world units
    inliers = {}
    for wide in (True, False):
        e = eng_mod.EkfEngine(scene.cam, scene.par, n_feat + 8)
        e.set_ncc_wide_search(wide)
        e.set_state(x13, fpos, ftype, None, P)
        e.upload_image(scene.render(poses[0], 0))
        e.capture_templates(np.arange(n_feat), uv0)
        for t in range(1, 6):
            if t == 2:
                x, fp, Pe = e.get_state()
                Pe[0, 0] += sigma ** 2
                Pe[1, 1] += sigma ** 2
                e.set_state(x, fp, ftype, None, Pe)
                # the matching stage alone, on what the step is about to see (predict + predict_measurements as the step does)
                e.predict()
                preds, _, _ = e.predict_measurements()
                e.upload_image(scene.render(poses[2], 2))
                e.match_ncc()
                for max_rad in (None, wr.MAXRAD):
                    m, _, _, _ = reference(e, oracle_lib, preds, max_rad)
                    near = int((np.abs(m["imagePos"] - truth[m["featureIndex"]]).max(axis=1) <= 1.5).sum()) if len(m) else 0
                    print(f"reference before frame 2, max_rad {max_rad}: {len(m)} matches, {near} at the true pixels")
                    assert near >= n_feat / 2 if max_rad is None else near <= 1
                e.set_state(x, fp, ftype, None, Pe)  # undo the prediction
            info = e.step_image(scene.render(poses[t], t))
            assert info.status == 0
            print(f"wide {wide} frame {t}: predicted {info.n_predicted} matches {info.n_matches} inliers {info.n_inliers} rescued {info.n_rescued}")
            if t == 3:
                inliers[wide] = info.n_inliers
    assert inliers[True] >= n_feat / 2 and inliers[False] <= 1, inliers


def test_sharded_engine_refuses(eng_mod):
    seq = SyntheticSequence(12, 1)
    s = eng_mod.EkfEngine(seq.cam, seq.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_ncc_wide_search(True)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.close()


def test_keypoint_matcher_ignores_the_mode(eng_mod):
    seq = SyntheticSequence(50, 3)
    states = []
    for wide in (False, True):
        e = eng_mod.EkfEngine(seq.cam, seq.par, 64, max_keypoints=4096)
        e.set_sweep_mode(4)  # the run-to-run reproducible sweep (test_gpu_ncc.test_staged_images_equal_direct_steps)
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, 1e9)
        if wide:
            e.set_ncc_wide_search(True)
        e.upload_image(seq.render_image(0))
        desc = e.describe(seq.pixel_positions(0).astype(np.float64))
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc, seq.P0)
        infos = [e.step_image(seq.render_image(t)) for t in (1, 2, 3)]
        assert e.ncc_wide_counts() == (0, 0)
        states.append((e.get_state(), [(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1] and states[0][1][-1][1] > 0
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setWideSearch(true) on the committed frames gives the C ABI's result; ekf_sequence --wide-search runs them
    and writes output.yml"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check, sample = str(tmp_path / "wide_search_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "wide_search_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check, str(cfg), SEQ + "/", "1e10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum(ln.startswith("step") for ln in r.stdout.splitlines()) == 7
    last = {ln.split()[1]: ln.split() for ln in r.stdout.splitlines() if ln.startswith("match")}
    assert set(last) == {"off", "class", "abi"} and last["class"][2:] == last["abi"][2:] and int(last["class"][4]) > 0
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sample, str(cfg), SEQ + "/", str(out) + "/", "--wide-search"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum("gates searched wide" in ln for ln in r.stdout.splitlines()) == 7
    assert (out / "output.yml").exists()
