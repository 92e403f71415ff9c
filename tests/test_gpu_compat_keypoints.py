"""ekf_compat::ImageEKF with the keypoint matcher, driven by tests/cpp/keypoint_image_check.cpp over the s3 frames: the
C++ driver class reproduces, frame by frame, the counters of the Python-driven engine run of
tests/test_gpu_keypoints.py::test_real_frames_keypoint_matcher_equals_oracle (map management off in its config)."""
import os
import subprocess

import numpy as np
import pytest

from openekfmonoslam_amd.ekftypes import s3_camera
from tests.test_io_host import CONFIG
from tests.test_keypoints_cpu import S3_INIT_FEATURES, S3_INIT_RESPONSE, S3_KP_RESPONSE, oracle_s3_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")


def s3_config_320():
    """the test configuration with the S3 camera scaled to the 320 x 240 frames and no map management"""
    c = s3_camera(320, 240)
    text = CONFIG % {"min_matches": S3_INIT_FEATURES}
    for key, old, new in [("PixelsX", "640", c.pixelsX), ("PixelsY", "480", c.pixelsY), ("FX", "525.060143149240389", c.fx),
                          ("FY", "524.245488213640215", c.fy), ("CX", "308.649343121753361", c.cx),
                          ("CY", "236.536005491807288", c.cy), ("DX", "0.007021618750000", c.dx),
                          ("DY", "0.007027222916667", c.dy), ("MapManagementFrequency", "1", 0)]:
        a, b = f'{key}: "{old}"', f'{key}: "{new!r}"'
        assert a in text, a
        text = text.replace(a, b)
    return text


def test_image_ekf_keypoint_matcher_over_s3(tmp_path, oracle_lib):
    exe = str(tmp_path / "keypoint_image_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "keypoint_image_check.cpp"),
                           "-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"])
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320())
    r = subprocess.run([exe, str(cfg), SEQ + "/", repr(S3_INIT_RESPONSE), repr(S3_KP_RESPONSE)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"init {S3_INIT_FEATURES}"
    steps = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("step ")]
    _, infos, _, _ = oracle_s3_run(oracle_lib)  # = the engine's counters (test_gpu_keypoints asserts them equal)
    assert len(steps) == len(infos) == 7
    for t, (s, i) in enumerate(zip(steps, infos)):
        assert s[:7] == [i.n_predicted, i.n_matches, i.n_hypotheses, i.n_inliers, i.n_outliers, i.n_rescued, i.status], t
        assert s[8] == s[7] > 0  # detected == kept (capacity 4 x max_features)
    x = np.array([float(v) for v in lines[-1].split()[1:]])
    assert x[0] < -0.005
