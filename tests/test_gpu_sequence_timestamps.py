"""`ekf_sequence --timestamps FILE [--time-unit SECONDS]` (samples/ekf_sequence.cpp) on the rendered sequence of
tests/test_gpu_sequence.py: times on the unit beat change nothing, a dropped frame is stepped over dt = 2, and a time that does not
increase is refused before the first frame.

output.yml is compared byte for byte EXCEPT the seven "Running time (microseconds)" values of every frame (Prediction, Matching,
Ransac, UpdateLI, RescueOutliers, UpdateHI, MapManagement): they are wall-clock measurements and differ between any two runs of
the same command.  Every count, state and covariance digit is compared as text."""
import os
import re
import shutil
import subprocess

import pytest

from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_io_host import CONFIG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
FRAMES = 7
TIMED = ("Prediction", "Matching", "Ransac", "UpdateLI", "RescueOutliers", "UpdateHI", "MapManagement")


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """the sample program, the configuration and the seven rendered frames, once for the module"""
    from PIL import Image

    base = tmp_path_factory.mktemp("timestamps")
    exe = str(base / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", exe, os.path.join(ROOT, "samples", "ekf_sequence.cpp"),
                           "-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"])
    seq = SyntheticSequence(80, FRAMES - 1)
    imgdir = base / "img"
    imgdir.mkdir()
    for t in range(FRAMES):
        frame = seq.render_image(t, outlier_fraction=0.0, channels=3 if t % 2 == 0 else 1)
        Image.fromarray(frame[..., ::-1] if frame.ndim == 3 else frame).save(str(imgdir / f"{t:05d}.png"))
    cfg = base / "config.yml"
    cfg.write_text(CONFIG % {"min_matches": 40})
    return exe, str(cfg), imgdir, base


def run(sample, name, imgdir=None, times=None, extra=()):
    exe, cfg, default_imgdir, base = sample
    outdir = base / name
    outdir.mkdir()
    cmd = [exe, cfg, str(imgdir or default_imgdir) + "/", str(outdir) + "/"]
    if times is not None:
        tfile = base / (name + "_times.txt")
        tfile.write_text("# seconds, one per frame\n" + "".join(f"{t!r}\n" for t in times))
        cmd += ["--timestamps", str(tfile)]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300), outdir


def untimed(text):
    """output.yml without the values of the measured running times"""
    return re.sub(r"^(\s*(?:%s):).*$" % "|".join(TIMED), r"\1", text, flags=re.M)


def test_unit_beat_timestamps_change_nothing(sample):
    plain, plain_out = run(sample, "plain")
    assert plain.returncode == 0, plain.stdout + plain.stderr
    timed, timed_out = run(sample, "beat", times=[float(t) for t in range(FRAMES)])
    assert timed.returncode == 0, timed.stdout + timed.stderr
    a, b = (plain_out / "output.yml").read_text(), (timed_out / "output.yml").read_text()
    assert a.count("StateEstimation") == FRAMES - 1 and untimed(a) != a
    assert untimed(a) == untimed(b)
    log = (timed_out / "log.txt").read_text()
    assert log.count("Frame interval: dt = 1\n") == FRAMES - 1
    assert "Frame interval" not in (plain_out / "log.txt").read_text()
    # the same beat in milliseconds
    ms, ms_out = run(sample, "beat_ms", times=[40e-3 * t for t in (0, 1, 2, 3, 4, 5, 6)], extra=["--time-unit", "0.04"])
    assert ms.returncode == 0, ms.stdout + ms.stderr
    dts = [float(v) for v in re.findall(r"Frame interval: dt = (\S+)", (ms_out / "log.txt").read_text())]
    assert len(dts) == FRAMES - 1 and all(abs(d - 1.0) < 1e-12 for d in dts)


def test_a_dropped_frame_is_stepped_over_two_intervals(sample):
    """frame 3 is dropped: the files that remain are numbered 0..5 (the sample reads consecutive numbers up to the first missing
    one), the time file keeps the gap -- 0 1 2 4 5 6 -- and the step on the frame after it runs over dt = 2"""
    _, _, imgdir, base = sample
    gapdir = base / "img_gap"
    gapdir.mkdir()
    kept = [t for t in range(FRAMES) if t != 3]
    for k, t in enumerate(kept):
        shutil.copyfile(str(imgdir / f"{t:05d}.png"), str(gapdir / f"{k:05d}.png"))
    r, outdir = run(sample, "gap", imgdir=gapdir, times=[float(t) for t in kept])
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == len(kept) - 1  # to the end
    log = (outdir / "log.txt").read_text()
    per_step = re.findall(r"~~~~~~~~~~~~ STEP (\d+) ~~~~~~~~~~~~\n(?:Fixed map: on\n)?Frame interval: dt = (\S+)\n", log)
    assert per_step == [("1", "1"), ("2", "1"), ("3", "2"), ("4", "1"), ("5", "1")]
    assert r.stdout.count("frame interval: dt = 2\n") == 1
    assert (outdir / "output.yml").read_text().count("StateEstimation") == len(kept) - 1


@pytest.mark.parametrize("times,what", [([0.0, 1.0, 2.0, 2.0, 4.0, 5.0, 6.0], "increase"), ([0.0, 1.0, 2.0, 3.0, 4.0, 5.0], "6 times for 7 frames")],
                         ids=["repeated-time", "one-time-short"])
def test_bad_time_files_are_refused_before_the_first_frame(sample, times, what):
    r, outdir = run(sample, "bad_" + what.split()[0], times=times)
    assert r.returncode != 0
    assert what in r.stderr, r.stderr
    assert "init:" not in r.stdout and "step" not in r.stdout
    assert not (outdir / "output.yml").exists() and not (outdir / "log.txt").exists()  # nothing was opened, no frame was read
