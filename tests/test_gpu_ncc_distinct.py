"""The NCC matcher's distinctiveness test on the device (ekf_set_ncc_distinct: k_ncc_match<.., true>, k_ncc_wide_coarse<true>,
k_ncc_wide_finish<.., true>) against its numpy restatement (tests/ncc_distinct_ref.py): the match list, the per-slot rival
records to the bit and the counts, on the narrow and the wide path; the edge of the exclusion block; all modes together; the
untouched mode-off path; the mode through the filter; the refusals and the C++ seam.

The reference is fed what the engine returns: its pyramid levels, its predictions and the templates its last match compared."""
import os
import subprocess

import numpy as np
import pytest

import ncc_distinct_ref as dr
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


def device(e, coef, wide, subpix=False):
    """the match of the uploaded frame from the engine's current predictions -> (matches, rival records, distinct counts)"""
    e.set_ncc_wide_search(wide)
    e.set_subpixel_matches(subpix)
    e.set_ncc_distinct(coef)
    m = e.match_ncc().copy()
    return m, e.ncc_rivals(), e.ncc_distinct_counts()


def reference(e, oracle_lib, preds, coef, wide, subpix=False):
    """after a device match: the restatement on the engine's own pyramid, predictions and compared templates"""
    o = oracle_lib.Oracle(wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params(), 1)  # the gate functions only: they take no camera
    levels = [e.image_level(l) for l in range(3)]
    return dr.match_all(o, levels, preds, e.match_templates(preds["featureIndex"]), None if wide else wr.MAXRAD, subpix, coef)


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


def check(e, oracle_lib, preds, coef, wide, label, subpix=False):
    """device == reference: list, records, counts -> (device matches, reference slots, records)"""
    m, riv, counts = device(e, coef, wide, subpix)
    want, slots, _, fit, want_riv, want_counts = reference(e, oracle_lib, preds, coef, wide, subpix)
    print(f"{label}: {len(m)} matches, counts {counts}, states {riv['state'].tolist()}")
    wr.assert_matches_equal(m, want, label)
    dr.assert_rivals_equal(riv, want_riv, label)
    assert counts == want_counts, label
    return m, slots, riv


@pytest.mark.parametrize("wide", [True, False])
def test_periodic_match_is_rejected(eng_mod, oracle_lib, wide):
    """the scene of test_gpu_ncc_wide.test_ties_across_tiles: a frame that repeats every 32 px under a 150 px gate.  The one
    confident wrong match leaves the list; with coef 0 it is back"""
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
    frame = wsn.periodic_frame(32)
    uv = np.array([[160.0, 120.0]])
    e, preds = engine_with(eng_mod, cam, par, uv, wsn.diag_P(cam, 1, 150.0, 150.0), frame, frame)
    m, slots, riv = check(e, oracle_lib, preds, 0.5, wide, f"periodic, wide {wide}")
    assert len(m) == 0 and e.ncc_distinct_counts() == (1, 1)
    assert riv["state"].tolist() == [3] and riv["distance"][0] == 0 and riv["rivalDistance"][0] == 0
    s = slots[0]
    assert (s["rx"] - s["bx"]) % 32 == 0 and (s["ry"] - s["by"]) % 32 == 0 and (s["rx"], s["ry"]) != (s["bx"], s["by"])
    m0, riv0, counts0 = device(e, 0.0, wide)
    assert len(m0) == 1 and m0["distance"][0] == 0 and (m0["imagePos"][0] != uv[0]).any()
    assert len(riv0) == 0 and counts0 == (0, 0)


def test_displaced_scene_equals_reference(eng_mod, oracle_lib):
    """the eight displaced targets in gates of about 150 px, wide search on: every rival lies in another tile than the best (the
    second coarse pass), none comes close, the list is the coef-0 list"""
    sc = wsn.DisplacedScene()
    e = eng_mod.EkfEngine(sc.cam, sc.par, 16)
    sc.load(e)
    preds, _, _ = e.predict_measurements()
    m0, _, _ = device(e, 0.0, True)
    m, slots, riv = check(e, oracle_lib, preds, 0.5, True, "displaced")
    wr.assert_matches_equal(m, m0, "coef 0.5 against coef 0")
    assert len(m) == sc.n and riv["state"].tolist() == [2] * sc.n and (riv["rivalDistance"] > 0.5).all()
    other = 0
    for p, s in zip(preds, slots):  # tiles of the slot's candidate box, as k_ncc_wide_classify lays them out
        x_lo, y_lo = (max(wr.to_level(p["imagePos"][a], 2) - ((s["major"] >> 2) + 1), 0) for a in (0, 1))
        tile = lambda c: ((c[0] - x_lo) // wr.TILE, (c[1] - y_lo) // wr.TILE)
        other += tile(s["b2"]) != tile(s["coarse_rival"])
    print(f"{other} of {sc.n} rivals lie in another tile than the best")
    assert other >= sc.n // 2


class TwoCopies:
    """Four features seeded on blurred noise; frame1 is other noise into which each feature's surroundings are pasted at two
    places 48 px apart (24 px either side of the prediction, features 0 and 1 along x, 2 and 3 along y) under a 150 px gate, and 1
    is added to one pixel of one copy's level-0 template footprint: the second copy in raster order for features 0 and 2, the
    first for 1 and 3.  The pasted surroundings are 48 x 48 -- the whole footprint of the three templates, 44 px at level 2 --:
    at 48 px apart two 64 x 64 squares would overwrite each other inside those footprints.  Everything is a multiple of 4."""
    UV = np.array([[80.0, 60.0], [240.0, 60.0], [80.0, 180.0], [240.0, 180.0]])

    def __init__(self):
        self.cam, self.par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
        self.frame0, self.frame1 = wr.blurred_noise(wsn.H, wsn.W, 61), wr.blurred_noise(wsn.H, wsn.W, 62)
        self.copies = []
        for i, (u, v) in enumerate(self.UV.astype(int)):
            d = np.array([24, 0]) if i < 2 else np.array([0, 24])
            pair = [np.array([u, v]) - d, np.array([u, v]) + d]  # raster order
            for cu, cv in pair:
                self.frame1[cv - 24:cv + 24, cu - 24:cu + 24] = self.frame0[v - 24:v + 24, u - 24:u + 24]
            pu, pv = pair[1 - i % 2]
            assert self.frame1[pv + 1, pu + 2] < 255
            self.frame1[pv + 1, pu + 2] += 1
            self.copies.append(pair)


@pytest.mark.parametrize("wide", [True, False])
def test_two_repetitions(eng_mod, oracle_lib, wide):
    """Features 0 and 2 (the later copy is the perturbed one): the first copy wins with distance 0, the other is the rival with a
    small positive distance, and the rule keeps the match at both coefficients: 0 < d2 * coef.  Features 1 and 3 (the first copy is
    perturbed): the two copies are best and rival again, and the match stays exactly where d1 < d2 * coef -- nowhere when the
    perturbed copy wins the coarse tie.  (The gate of 150 px is wide; with the mode off the cap of 66 px holds both copies too.)"""
    sc = TwoCopies()
    e, preds = engine_with(eng_mod, sc.cam, sc.par, sc.UV, wsn.diag_P(sc.cam, 4, 150.0, 150.0), sc.frame0, sc.frame1)
    for coef in (0.5, 1.0):
        m, slots, riv = check(e, oracle_lib, preds, coef, wide, f"two copies, coef {coef}, wide {wide}")
        for i, (s, r) in enumerate(zip(slots, riv)):
            places = {(s["bx"], s["by"]), (s["rx"], s["ry"])}
            assert places == {tuple(c) for c in sc.copies[i]}, (i, places)
            assert r["state"] == (2 if np.float64(r["distance"]) < np.float64(r["rivalDistance"]) * coef else 3)
            assert sorted([r["distance"] == 0, r["rivalDistance"] == 0]) == [False, True]
            assert 0 < max(r["distance"], r["rivalDistance"]) < 1e-3
            if i % 2 == 0:
                assert (s["bx"], s["by"]) == tuple(sc.copies[i][0]) and r["distance"] == 0 and r["state"] == 2
        assert sorted(m["featureIndex"].tolist()) == [i for i in range(4) if riv["state"][i] == 2]
    assert set(riv["state"][[1, 3]].tolist()) <= {2, 3}


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("period", [8, 12])
def test_exclusion_edge(eng_mod, oracle_lib, wide, period):
    """frames that repeat every 8 and 12 px: 2 and 3 coarse pixels.  The repetitions 2 coarse pixels from the coarse best have
    its key and are not rivals (the rival is the one 4 away); the one 3 away is.  The gates were chosen with the reference: 30 px
    (narrow path; the first repetition in raster order still refines to a pixel inside the gate) and 48 x 150 px (wide path), whose
    top row begins where the best and that rival fall into two tiles of the slot's box."""
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
    frame = wsn.periodic_frame(period, seed=43)
    uv = np.array([[160.0, 120.0]])
    axes = (48.0, 150.0) if wide else (30.0, 30.0)
    e, preds = engine_with(eng_mod, cam, par, uv, wsn.diag_P(cam, 1, *axes), frame, frame)
    m, slots, riv = check(e, oracle_lib, preds, 0.5, wide, f"period {period}, wide {wide}")
    s = slots[0]
    assert s["wide"] == wide and s["state"] == 3 and s["d1"] == 0 and s["d2"] == 0
    b2, cr = s["b2"], s["coarse_rival"]
    step = 3 if period == 12 else 4
    print(f"coarse best {b2}, coarse rival {cr}")
    assert max(abs(cr[0] - b2[0]), abs(cr[1] - b2[1])) == step
    if wide:
        x_lo = max(wr.to_level(uv[0, 0], 2) - ((s["major"] >> 2) + 1), 0)
        assert (b2[0] - x_lo) // wr.TILE != (cr[0] - x_lo) // wr.TILE, "best and rival share a tile: the edge is not across tiles"


def test_all_modes_together(eng_mod, oracle_lib):
    """template warp, sub-pixel fit, wide search and the distinctiveness test in one match on the 20 degree roll scene of
    tests/test_gpu_ncc_wide.test_with_warp_and_subpixel: list, records and counts equal the reference fed the re-rendered
    templates, and the sub-pixel counts cover the kept matches only"""
    n_feat, frames = 16, 10
    scene = ws.PlaneScene(wsn.W, wsn.H)
    poses = ws.trajectory("roll", frames, 20.0)
    uv0, _, fpos, ftype, x13, P = scene.seed_features(n_feat, margin=60.0)
    v, w = ws.velocity("roll", frames, 20.0)
    x13[7:10], x13[10:13] = v, np.where(w != 0, w, 2.22e-16)
    axes = np.where(np.arange(n_feat) % 4 == 3, 40.0, 110.0)
    e = eng_mod.EkfEngine(scene.cam, scene.par, n_feat + 8)
    e.set_template_warp(True)
    e.set_state(x13, fpos, ftype, None, P + wsn.diag_P(scene.cam, n_feat, axes, axes))
    e.upload_image(scene.render(IDENTITY, 0))
    e.capture_templates(np.arange(n_feat), uv0)
    for _ in range(3):
        e.predict()
    preds, _, _ = e.predict_measurements()
    e.upload_image(scene.render(poses[3], 3))
    m, slots, riv = check(e, oracle_lib, preds, 0.5, True, "warp + sub-pixel + wide + distinct", subpix=True)
    fit = e.subpixel_counts()
    want_fit = reference(e, oracle_lib, preds, 0.5, True, True)[3]
    assert e.template_warp_counts()[0] > 0 and sum(s["wide"] for s in slots) >= len(preds) / 2
    assert fit == want_fit and fit[0] + fit[1] == 2 * len(m) and len(m) > 0
    assert len(riv) == len(preds) and (riv["state"] >= 2).sum() > 0


@pytest.mark.parametrize("nfeat", [12, 50])
def test_mode_off_is_todays_path(eng_mod, oracle_lib, nfeat):
    """enabled and then disabled: matches identical to the oracle's, as test_gpu_ncc.test_match_ncc_identical checks them"""
    seq = SyntheticSequence(nfeat, 3)
    e, o = make_pair(eng_mod, oracle_lib, seq)
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
        e.set_ncc_distinct(0.5)
        on = e.match_ncc().copy()
        assert len(e.ncc_rivals()) == len(preds) and len(on) <= len(mo)
        e.set_ncc_distinct(0)
        wr.assert_matches_equal(e.match_ncc(), mo, f"frame {t}, on -> off")
        assert len(e.ncc_rivals()) == 0 and e.ncc_distinct_counts() == (0, 0)


def test_through_the_filter(eng_mod):
    """ekf_step_image over the eight golden frames with coef 0.5, the coef-0 run beside it: every step succeeds and the test
    takes less than a tenth of a frame's matches"""
    from PIL import Image

    frames = [np.asarray(Image.open(os.path.join(SEQ, f"{k:05d}.png"))) for k in range(8)]
    cam, par = wsn.s3_camera(320, 240), wsn.s3_params()
    runs = {}
    for coef in (0.0, 0.5):
        e = eng_mod.EkfEngine(cam, par, 96)
        e.set_ncc_distinct(coef)
        e.reset()
        e.upload_image(frames[0])
        uv = e.detect_new_features(40, min_response=1e10)
        e.add_features(uv)
        e.capture_templates(np.arange(40), uv)
        runs[coef] = []
        for t in range(1, 8):
            info = e.step_image(frames[t])
            with_rival, rejected = e.ncc_distinct_counts()
            runs[coef].append((info.status, info.n_predicted, info.n_matches, info.n_inliers, with_rival, rejected))
            assert info.status == 0
    for t, (a, b) in enumerate(zip(runs[0.0], runs[0.5]), 1):
        print(f"frame {t}: coef 0 (status, predicted, matches, inliers, rivals, rejected) {a}; coef 0.5 {b}")
        assert a[4:] == (0, 0) and b[5] <= b[4]
        assert b[5] < 0.10 * (b[2] + b[5])


def test_refusals(eng_mod):
    seq = SyntheticSequence(12, 1)
    s = eng_mod.EkfEngine(seq.cam, seq.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_ncc_distinct(0.5)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.set_ncc_distinct(0)  # off is what a sharded engine runs
    s.close()
    e = eng_mod.EkfEngine(seq.cam, seq.par, 12)
    e.set_ncc_distinct(0.25)
    for bad in (-0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(eng_mod.EkfError) as ex:
            e.set_ncc_distinct(bad)
        assert ex.value.code == 1
    e.set_ncc_distinct(1.0)


def test_keypoint_matcher_ignores_the_mode(eng_mod):
    seq = SyntheticSequence(50, 3)
    states = []
    for coef in (0.0, 0.5):
        e = eng_mod.EkfEngine(seq.cam, seq.par, 64, max_keypoints=4096)
        e.set_sweep_mode(4)  # the run-to-run reproducible sweep (test_gpu_ncc.test_staged_images_equal_direct_steps)
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, 1e9)
        e.set_ncc_distinct(coef)
        e.upload_image(seq.render_image(0))
        desc = e.describe(seq.pixel_positions(0).astype(np.float64))
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc, seq.P0)
        infos = [e.step_image(seq.render_image(t)) for t in (1, 2, 3)]
        assert e.ncc_distinct_counts() == (0, 0) and len(e.ncc_rivals()) == 0
        states.append((e.get_state(), [(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1] and states[0][1][-1][1] > 0
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setNccDistinct(0.5) on the committed frames gives the C ABI's result; ekf_sequence --ncc-distinct 0.5 runs them
    and writes output.yml"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check_bin, sample = str(tmp_path / "ncc_distinct_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check_bin, os.path.join(ROOT, "tests", "cpp", "ncc_distinct_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check_bin, str(cfg), SEQ + "/", "1e10", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum(ln.startswith("step") for ln in r.stdout.splitlines()) == 7
    last = {ln.split()[1]: ln.split() for ln in r.stdout.splitlines() if ln.startswith("match")}
    assert set(last) == {"off", "class", "abi"} and last["class"][2:] == last["abi"][2:] and int(last["class"][2]) > 0
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sample, str(cfg), SEQ + "/", str(out) + "/", "--ncc-distinct", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum("matches with a rival in the gate" in ln for ln in r.stdout.splitlines()) == 7
    assert (out / "output.yml").exists()
