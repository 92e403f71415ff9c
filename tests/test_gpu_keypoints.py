"""GPU tests of the image-in descriptor matcher: the device keypoint detector and BRIEF-32 (kernels_detect.hip) against
the numpy reference (tests/keypoint_ref.py) bit for bit, the gate mask against the oracle's ellipse test, and the
KEYPOINTS-mode image step against the keypoint step fed the reference's unmasked keypoints (bitwise) and against the
oracle on real frames."""
import numpy as np
import pytest

import keypoint_ref as kr
from openekfmonoslam_amd.ekftypes import s3_camera, s3_params
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.oracle_lib import ALGORITHMIC
from tests.test_gpu_parity import assert_state_close, eng_mod  # noqa: F401
from tests.test_keypoints_cpu import (S3_INIT_FEATURES, S3_INIT_RESPONSE, S3_KP_RESPONSE, S3_MATCH_FLOOR,
                                      oracle_s3_run, s3_frames)

pytestmark = pytest.mark.gpu

SYN_RESPONSE = 1e10  # synthetic renders: above the background noise's corners
INFO_FIELDS = ("n_predicted", "n_matches", "n_hypotheses", "n_inliers", "n_outliers", "n_rescued", "status",
               "n_sweep_retries")


def _uv(kps):
    return np.stack([kps["x"], kps["y"]], axis=1).astype(np.float64)


def _engine(eng_mod, cam, par, nfeat, precision=0, max_keypoints=8192):
    return eng_mod.EkfEngine(cam, par, nfeat, max_keypoints=max_keypoints, precision=precision)


def _images():
    out = [("s3_%d" % k, f, None) for k, f in enumerate(s3_frames())]
    for w, h in ((640, 480), (1920, 1080)):
        seq = SyntheticSequence(200, 2, width=w, height=h)
        out.append((f"syn_{w}x{h}", seq.render_image(1), seq))
    seq = SyntheticSequence(40, 2, width=321, height=243)
    out.append(("rgba_321x243", seq.render_image(1, channels=4), seq))
    return out


def test_detect_unmasked_equals_reference(eng_mod, oracle_lib):
    cam, par = s3_camera(320, 240), s3_params()
    for name, img, seq in _images():
        e = _engine(eng_mod, seq.cam if seq else cam, par, 16)
        e.upload_image(img)
        if img.ndim == 3:  # the gray level 0 of the pyramid (bit-checked against the oracle by test_gpu_ncc)
            o = oracle_lib.Oracle(seq.cam, par, 16)
            o.set_image(img)
            gray = o.image_level(0)
        else:
            gray = img
        for mr in (1e9, SYN_RESPONSE):
            kps, desc = e.detect_keypoints(mr, masked=False)
            rk, rd = kr.keypoints_and_descriptors(gray, mr)
            assert len(rk) > 0, name
            assert e.last_found == len(rk), name
            np.testing.assert_array_equal(kps["x"], rk["x"], err_msg=name)
            np.testing.assert_array_equal(kps["y"], rk["y"], err_msg=name)
            np.testing.assert_array_equal(desc, rd, err_msg=name)
        # capacity: the first ones in raster order, all of them counted
        k5, d5 = e.detect_keypoints(SYN_RESPONSE, capacity=5)
        np.testing.assert_array_equal(_uv(k5), _uv(rk[:5]))
        np.testing.assert_array_equal(d5, rd[:5])
        assert e.last_found == len(rk)
        e.close()


@pytest.mark.parametrize("w,h", [(640, 480), (321, 243)])
def test_describe_arbitrary_pixels_equals_reference(eng_mod, w, h):
    seq = SyntheticSequence(60, 2, width=w, height=h)
    img = seq.render_image(0)
    e = _engine(eng_mod, seq.cam, seq.par, 16)
    e.upload_image(img)
    rng = np.random.default_rng(7)
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (2, 3), (w - 3, h - 4), (3.7, h - 0.6), (w - 0.2, 1.2),
           (10.5, 20.5), (10.4999, 20.4999), (-0.5, 7), (-0.51, 7.5), (-3.2, -2.6), (w + 2.0, h + 3.0), (w / 2, h / 2)]
    pts += [(x, y) for x, y in rng.uniform([-4, -4], [w + 4, h + 4], size=(300, 2))]
    uv = np.array(pts, dtype=np.float64)
    np.testing.assert_array_equal(e.describe(uv), kr.describe(img, uv))
    # the same pixels through the detector path: describe at the keypoints == the detector's descriptors
    kps, desc = e.detect_keypoints(SYN_RESPONSE)
    np.testing.assert_array_equal(e.describe(_uv(kps)), desc)


def _inside_any_gate(o, preds, kps):
    keep = np.zeros(len(kps), dtype=bool)
    gates = []
    for p in preds:
        ax, ang = o.ellipse(p["covarianceMatrix"])
        aw, ah = int(np.rint(ax[0])), int(np.rint(ax[1]))  # round half to even, as cv::Size(Size2f)
        gates.append((float(np.float32(p["imagePos"][0])), float(np.float32(p["imagePos"][1])), aw, ah, ang))
    for i, k in enumerate(kps):
        for cx, cy, aw, ah, ang in gates:
            if o.point_in_ellipse(float(k["x"]), float(k["y"]), cx, cy, aw, ah, ang):
                keep[i] = True
                break
    return keep


@pytest.mark.parametrize("nfeat", [50, 200])
def test_masked_detection_is_the_gated_reference_list(eng_mod, oracle_lib, nfeat):
    seq = SyntheticSequence(nfeat, 2)
    e = _engine(eng_mod, seq.cam, seq.par, nfeat + 8)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    img = seq.render_image(1)
    e.upload_image(img)  # before the prediction: its gates are kept for the mask
    e.predict()
    preds, _, _ = e.predict_measurements()
    assert len(preds) > 0
    o = oracle_lib.Oracle(seq.cam, seq.par, 8)
    for mr in (1e9, SYN_RESPONSE):
        rk, rd = kr.keypoints_and_descriptors(img, mr)
        keep = _inside_any_gate(o, preds, rk)
        assert 0 < keep.sum() < len(rk)
        kps, desc = e.detect_keypoints(mr, masked=True)
        np.testing.assert_array_equal(_uv(kps), _uv(rk[keep]))
        np.testing.assert_array_equal(desc, rd[keep])


def _seeded_pair(eng_mod, seq, precision, max_keypoints=8192):
    """two engines with the same map, whose descriptors are the BRIEF-32 of frame 0 at the features' pixels"""
    desc0 = kr.describe(seq.render_image(0), seq.pixel_positions(0).astype(np.float64))
    out = []
    for _ in range(2):
        e = _engine(eng_mod, seq.cam, seq.par, seq.n_features + 8, precision, max_keypoints)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc0, seq.P0)
        e.set_sweep_mode(4)  # bitwise run-to-run comparisons need the launch-per-panel sweep
        out.append(e)
    return out


def _assert_same_filter(a, b):
    xa, fa, Pa = a.get_state()
    xb, fb, Pb = b.get_state()
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(fa, fb)
    np.testing.assert_array_equal(Pa, Pb)
    for u, v in zip(a.get_map_features(), b.get_map_features()):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("nfeat", [50, 200, 1000])
def test_keypoint_step_equals_step_with_reference_keypoints(eng_mod, nfeat, precision):
    """engine A: KEYPOINTS image step (masked device detection); engine B: ekf_step with the reference's UNMASKED list
    -- identical counters, bitwise x, P and map descriptors: the mask loses nothing the matcher could accept"""
    seq = SyntheticSequence(nfeat, 3)
    a, b = _seeded_pair(eng_mod, seq, precision)
    a.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, SYN_RESPONSE)
    total = 0
    for t in range(1, 4):
        img = seq.render_image(t)
        ia = a.step_image(img)
        kps, desc = kr.keypoints_and_descriptors(img, SYN_RESPONSE)
        b.upload_image(img)  # the same step path (image loaded) fed host keypoints
        ib = b.step(kps, desc)
        for f in INFO_FIELDS:
            assert getattr(ia, f) == getattr(ib, f), (t, f, getattr(ia, f), getattr(ib, f))
        det, kept = a.step_keypoints()
        assert det == kept and 0 < det <= len(kps)
        total += ia.n_matches
    assert total >= nfeat  # the map's own descriptors are found again
    _assert_same_filter(a, b)


def test_real_frames_keypoint_matcher_equals_oracle(eng_mod, oracle_lib):
    """s3 frames: init (detect_new -> describe -> add), then seven KEYPOINTS image steps; the oracle is fed the
    reference's unmasked keypoints and descriptors (tests/test_keypoints_cpu.py)"""
    frames = s3_frames()
    o, infos, uv_o, desc_o = oracle_s3_run(oracle_lib)
    e = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), 96, max_keypoints=2048)
    e.reset()
    e.upload_image(frames[0])
    uv = e.detect_new_features(S3_INIT_FEATURES, min_response=S3_INIT_RESPONSE)
    np.testing.assert_array_equal(uv, uv_o)
    desc = e.describe(uv)
    np.testing.assert_array_equal(desc, desc_o)
    e.add_features(uv, desc)
    e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, S3_KP_RESPONSE)
    for t in range(1, 8):
        gi, oi = e.step_image(frames[t]), infos[t - 1]
        for f in INFO_FIELDS[:7]:
            assert getattr(gi, f) == getattr(oi, f), (t, f, getattr(gi, f), getattr(oi, f))
        assert gi.n_matches >= S3_MATCH_FLOOR[t - 1]
    assert_state_close(e, o, 1e-8, "seven real frames, keypoint matcher")
    np.testing.assert_array_equal(e.get_map_features()[0], o.map_features()[0])


def test_staged_keypoint_steps_equal_direct_steps(eng_mod):
    seq = SyntheticSequence(50, 5)
    a, b = _seeded_pair(eng_mod, seq, 0)
    for e in (a, b):
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, SYN_RESPONSE)
    imgs = [seq.render_image(t) for t in range(1, 6)]
    b.upload_images(imgs)
    for t in range(5):
        ia, ib = a.step_image(imgs[t]), b.step_staged_image(t)
        for f in INFO_FIELDS:
            assert getattr(ia, f) == getattr(ib, f), (t, f)
        assert a.step_keypoints() == b.step_keypoints()
    _assert_same_filter(a, b)


def test_keypoint_capacity(eng_mod):
    """max_keypoints below the masked count: the step keeps the first kcap in raster order and reports both numbers"""
    kcap = 24
    seq = SyntheticSequence(200, 2)
    a, ref = _seeded_pair(eng_mod, seq, 0, max_keypoints=kcap)
    probe, _ = _seeded_pair(eng_mod, seq, 0, max_keypoints=kcap)
    img = seq.render_image(1)
    # the masked list of this very prediction, truncated to kcap
    probe.upload_image(img)
    probe.predict()
    probe.predict_measurements()
    kps, desc = probe.detect_keypoints(SYN_RESPONSE, masked=True, capacity=kcap)
    found = probe.last_found
    assert len(kps) == kcap < found
    a.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, SYN_RESPONSE)
    ia = a.step_image(img)
    assert a.step_keypoints() == (found, kcap)
    ref.upload_image(img)
    ib = ref.step(kps, desc)
    for f in INFO_FIELDS:
        assert getattr(ia, f) == getattr(ib, f), f
    _assert_same_filter(a, ref)


def test_keypoint_matcher_errors(eng_mod):
    seq = SyntheticSequence(12, 2)
    img = seq.render_image(1)
    INVALID = 1
    # CV_32F / L2 descriptors: no BRIEF-32
    e = eng_mod.EkfEngine(seq.cam, seq.par, 20, descriptor_cols_f32=64)
    with pytest.raises(eng_mod.EkfError) as ex:
        e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS)
    assert ex.value.code == INVALID
    e.upload_image(img)
    with pytest.raises(eng_mod.EkfError) as ex:
        e.describe(np.array([[20.0, 20.0]]))
    assert ex.value.code == INVALID
    kps, _ = e.detect_keypoints(SYN_RESPONSE, descriptors=False)  # positions alone are fine
    assert len(kps) > 0
    e.set_image_matcher(eng_mod.IMAGE_MATCHER_NCC)
    e.close()
    # sharded engine
    s = eng_mod.EkfEngine(seq.cam, seq.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS)
    assert ex.value.code == INVALID
    s.set_image_matcher(eng_mod.IMAGE_MATCHER_NCC)
    s.close()
    # no image yet
    f = eng_mod.EkfEngine(seq.cam, seq.par, 20)
    f.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for call in (lambda: f.detect_keypoints(SYN_RESPONSE), lambda: f.describe(np.array([[20.0, 20.0]]))):
        with pytest.raises(eng_mod.EkfError) as ex:
            call()
        assert ex.value.code == INVALID
    # ... and the engine goes on: image, detection, a KEYPOINTS step
    f.upload_image(seq.render_image(0))
    assert len(f.detect_keypoints(SYN_RESPONSE)[0]) > 0
    f.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, SYN_RESPONSE)
    assert f.step_image(img).status == 0
