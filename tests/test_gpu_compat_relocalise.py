"""ekf_compat::ImageEKF::setRelocalise, driven by tests/cpp/relocalise_check.cpp over the s3 frames with the keypoint matcher: with
lostBelow above any inlier count every step counts as lost, so after lostFrames = 2 such steps the next step relocalises on its image
before it steps, logs the outcome, and the count starts again.  What the relocalisation finds on this young map is not asserted
(tests/test_gpu_relocalise.py covers the numbers); the bookkeeping around it is."""
import os
import subprocess

import pytest

from tests.test_gpu_compat_keypoints import PKG, ROOT, SEQ, s3_config_320
from tests.test_keypoints_cpu import S3_INIT_FEATURES, S3_INIT_RESPONSE, S3_KP_RESPONSE

pytestmark = pytest.mark.gpu


def test_image_ekf_relocalises_after_lost_frames(tmp_path):
    exe = str(tmp_path / "relocalise_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "relocalise_check.cpp"),
                           "-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"])
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320())
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(cfg), SEQ + "/", str(out) + "/", repr(S3_INIT_RESPONSE), repr(S3_KP_RESPONSE), "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"init {S3_INIT_FEATURES}"
    steps = [dict(zip(ln.split()[0::2], (int(v) for v in ln.split()[1::2]))) for ln in lines[1:]]
    assert len(steps) == 7 and all(s["status"] == 0 for s in steps)
    assert [s["relocalised"] for s in steps] == [0, 0, 1, 0, 1, 0, 1]  # two lost steps, then the third relocalises first
    assert [s["lost"] for s in steps] == [1, 2, 1, 2, 1, 2, 1]
    done = [s for s in steps if s["relocalised"]]
    assert all(s["hypotheses"] == 128 and s["installed"] == s["found"] for s in done)  # setRelocalise installs what it finds
    log = (out / "log.txt").read_text().splitlines()
    outcome = [ln for ln in log if ln.startswith("Relocalised: inliers=") or ln == "Relocalise failed"]
    assert [ln.startswith("Relocalised") for ln in outcome] == [bool(s["found"]) for s in done]
