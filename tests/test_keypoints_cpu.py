"""CPU side of the image-in descriptor matcher (keypoint detector + BRIEF-32): the pattern table
is what its generator writes, the numpy reference (tests/keypoint_ref.py) computes the oracle's corner measure, and the
oracle tracks the reference's sample frames when fed the reference's keypoints and descriptors.  The per-frame match
counts measured here are the floor tests/test_gpu_keypoints.py asserts for the engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

import keypoint_ref as kr
from openekfmonoslam_amd.ekftypes import PREDICTION_DTYPE, s3_camera, s3_params
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.oracle_lib import ALGORITHMIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
S3_KP_RESPONSE = 1e9    # keypoint threshold on the s3 frames
S3_INIT_RESPONSE = 1e10  # new-feature threshold of the initial map (as test_gpu_ncc.test_real_frames_engine_equals_oracle)
S3_INIT_FEATURES = 40
# n_matches of frames 1..7 of the oracle run below: the floor of the engine's KEYPOINTS-mode run on the same frames
S3_MATCH_FLOOR = [33, 32, 30, 32, 31, 32, 32]


def s3_frames():
    from PIL import Image

    return [np.asarray(Image.open(os.path.join(SEQ, f"{k:05d}.png"))) for k in range(8)]


def test_pattern_header_is_generated():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_brief_pattern.py"), "--stdout"],
                         capture_output=True, check=True).stdout
    with open(kr.PATTERN_H, "rb") as f:
        assert f.read() == out


def test_pattern_table_properties():
    p = kr.brief_pattern()
    assert p.shape == (256, 4)
    assert p.min() >= -19 and p.max() <= 19
    assert not np.any(np.all(p[:, :2] == p[:, 2:], axis=1)), "a test compares a point with itself"
    assert len({tuple(r) for r in p.tolist()}) == 256, "repeated pair"


def test_threshold_conversion():
    assert kr.threshold(-5.0) == 0 and kr.threshold(0.0) == 0
    assert kr.threshold(1e9) == 1000000000 and kr.threshold(2.7) == 2
    assert kr.threshold(1e30) == kr.INT64_MAX


@pytest.mark.parametrize("source", ["s3", "synthetic"])
@pytest.mark.parametrize("min_response", [0.0, 1e9, 1e10])
def test_response_matches_the_oracle_detector(oracle_lib, source, min_response):
    """the per-16x16-cell argmax of the numpy R (border 16, threshold) == the oracle's new-feature detector without
    predictions, which returns every cell candidate in cell order when there are fewer than max_new"""
    if source == "s3":
        img = s3_frames()[0]
        cam = s3_camera(320, 240)
    else:
        seq = SyntheticSequence(200, 2)
        img = seq.render_image(1)
        cam = seq.cam
    o = oracle_lib.Oracle(cam, s3_params(), 16)
    o.set_image(img)
    h, w = img.shape
    max_new = (w // 16) * (h // 16) + 1
    got = o.detect_new_features(np.zeros(0, dtype=PREDICTION_DTYPE), max_new, min_response=min_response)
    ref = kr.cell_maxima(img, min_response)
    assert len(ref) > 0
    np.testing.assert_array_equal(ref, got)


def test_reference_keypoints_are_local_maxima():
    img = s3_frames()[3]
    R = kr.response(img)
    kps = kr.keypoints(img, S3_KP_RESPONSE)
    assert 100 < len(kps) < 2000
    order = kps["y"].astype(np.int64) * img.shape[1] + kps["x"].astype(np.int64)
    assert np.all(np.diff(order) > 0), "not in raster order"
    for k in kps[::17]:
        x, y = int(k["x"]), int(k["y"])
        win = R[y - 2 : y + 3, x - 2 : x + 3]
        assert R[y, x] == win.max() and R[y, x] >= S3_KP_RESPONSE


def test_reference_descriptor_bits():
    """bit packing and clamping of the numpy BRIEF on a hand-checkable image: a left-to-right ramp"""
    img = np.tile(np.arange(64, dtype=np.uint8) * 3, (40, 1))
    p = kr.brief_pattern()
    d = kr.describe(img, [[32.0, 20.0]])
    bits = np.unpackbits(d[0])
    # on an unclamped ramp S grows with x: test i is set exactly when ax < bx
    np.testing.assert_array_equal(bits, (p[:, 0] < p[:, 2]).astype(np.uint8))
    # half-integers round up (floor(u + 0.5)); positions off the frame read the edge
    np.testing.assert_array_equal(kr.describe(img, [[31.5, 19.5]]), d)
    np.testing.assert_array_equal(kr.describe(img, [[-40.0, 5.0]]), kr.describe(img, [[-60.0, 5.0]]))


def oracle_s3_run(oracle_lib):
    """the oracle on the s3 frames, fed tests/keypoint_ref.py: init on frame 0 (40 new features + their descriptors),
    then seven keypoint steps (ALGORITHMIC).  Returns (oracle, per-frame infos, initial uv, initial descriptors)."""
    frames = s3_frames()
    o = oracle_lib.Oracle(s3_camera(320, 240), s3_params(), 96)
    o.reset()
    o.set_image(frames[0])
    uv = o.detect_new_features(np.zeros(0, dtype=PREDICTION_DTYPE), S3_INIT_FEATURES, min_response=S3_INIT_RESPONSE)
    desc = kr.describe(frames[0], uv)
    for p, d in zip(uv, desc):
        o.add_feature(p, d)
    infos = []
    for t in range(1, 8):
        kps, kd = kr.keypoints_and_descriptors(frames[t], S3_KP_RESPONSE)
        infos.append(o.step(kps, kd, ALGORITHMIC))
    return o, infos, uv, desc


def test_oracle_tracks_s3_with_reference_keypoints(oracle_lib):
    o, infos, uv, _ = oracle_s3_run(oracle_lib)
    assert len(uv) == S3_INIT_FEATURES
    assert [i.n_matches for i in infos] == S3_MATCH_FLOOR
    for i in infos:
        assert i.status == 0 and i.n_predicted == S3_INIT_FEATURES
        assert i.n_inliers + i.n_rescued >= 0.85 * i.n_matches
    x = o.x13()
    assert np.all(np.isfinite(x)) and x[0] < -0.005  # the camera of this sequence slides sideways
