"""The map export on the device (ekf_get_map_points, k_map_points) against its numpy restatement
(tests/map_points_ref.py), against the conversion it mirrors, and through the C++ driver class and the sample program.

Tolerance: 1e-12 x the absolute-value bound of each sum (B = |J| |Z| |J|' for a covariance), the fp64 parity gate of
test_gpu_map_management.py / test_gpu_parity.py.  Worst error / bound measured on an MI355X (printed by
test_export_matches_reference, seq50 and a 200-feature sequence, precisions 0, 1, 2): 4.8e-16 over cov, 7.8e-16 over
cov_cam, 2.4e-16 over xyz, 3.7e-16 over cam, 1.3e-16 over the linearity index."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_points_ref as mp
from openekfmonoslam_amd.ekftypes import EkfMapPoint, s3_camera
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_io_host import CONFIG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
TOL = 1e-12
SWEEP_LAUNCHES = 4  # EKF_SWEEP_LAUNCHES: the run-to-run reproducible mode


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


@pytest.fixture(scope="module")
def seq200():
    return SyntheticSequence(200, 2)


def make(eng_mod, seq, precision=0, steps=2, sweep_mode=None):
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=4 * seq.n_features + 64, precision=precision)
    if sweep_mode is not None:
        e.set_sweep_mode(sweep_mode)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for kps, desc in seq.frames[:steps]:
        e.step(kps, desc)
    return e


def reference(e):
    x, fp, P = e.get_state()
    t, c = e.feature_layout()
    return mp.map_points_ref(x, fp, t, c, P), (x, fp, P, t, c)


def worst_ratio(got, want, bound):
    """max |got - want| / bound; an entry whose bound is 0 (a structurally zero sum) has to be exact"""
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max())


def linearity_bound(ref, state):
    """|L| (1 + k_dot + 2 k_c): the index is 4 sigma (tc.tf) / (|tf| |tc|^2); k_dot = sum|tc_k tf_k| / |tc.tf| is the
    condition of the dot product, k_c = bound(X - r) / |tc| that of tc = X - r (it enters squared through |tc|)."""
    x, fp, _, t, _ = state
    out = np.zeros(len(t))
    for i in np.flatnonzero(t == mp.FEATURE_INVERSE_DEPTH):
        tc, tf = ref["xyz"][i] - x[:3], ref["xyz"][i] - fp[i, :3]
        k_dot = np.abs(tc * tf).sum() / abs(tc @ tf)
        k_c = np.linalg.norm(ref["xyz_bound"][i] + np.abs(x[:3])) / np.linalg.norm(tc)
        out[i] = abs(ref["linearity"][i]) * (1 + k_dot + 2 * k_c)
    return out


# ---------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("which", ["seq50", "seq200"])
def test_export_matches_reference(eng_mod, seq50, seq200, which, precision):
    seq = seq50 if which == "seq50" else seq200
    e = make(eng_mod, seq, precision)
    pts = e.map_points()
    ref, (x, fp, P, t, c) = reference(e)
    assert len(pts) == e.N == seq.n_features
    ratios = {
        "cov": worst_ratio(pts["cov"], ref["cov"], ref["B"]),
        "cov_cam": worst_ratio(pts["cov_cam"], ref["cov_cam"], ref["B_cam"]),
        "xyz": worst_ratio(pts["xyz"], ref["xyz"], ref["xyz_bound"]),
        "cam": worst_ratio(pts["cam"], ref["cam"], ref["cam_bound"]),
    }
    inv = t == mp.FEATURE_INVERSE_DEPTH
    ratios["linearity"] = worst_ratio(pts["linearity"][inv], ref["linearity"][inv], linearity_bound(ref, (x, fp, P, t, c))[inv])
    print(f"map export {which} precision {precision}: worst |error| / bound =", {k: f"{v:.2e}" for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= TOL, (k, v)
    _, tp, tm = e.get_map_features()
    np.testing.assert_array_equal(pts["type"], t)
    np.testing.assert_array_equal(pts["covpos"], c)
    np.testing.assert_array_equal(pts["times_predicted"], tp)
    np.testing.assert_array_equal(pts["times_matched"], tm)
    assert tp.max() > 0  # two steps: the counters are not trivially zero


# ------------------------------------------------------------------------------------------------------- 2. mixed map
def test_mixed_map_depth_features_are_copied_exactly(eng_mod):
    seq = SyntheticSequence(50, 4)
    seq.par.inverseDepthLinearityIndexThreshold = 1e9  # every call converts the first remaining inverse-depth feature
    e = eng_mod.EkfEngine(seq.cam, seq.par, 66, max_keypoints=264)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for t, (kps, desc) in enumerate(seq.frames):
        e.step(kps, desc)
        assert e.convert_inverse_depth_to_depth() == t
    pts = e.map_points()
    ref, (x, fp, P, t, c) = reference(e)
    depth = np.flatnonzero(t == mp.FEATURE_DEPTH)
    assert list(depth) == [0, 1, 2, 3] and e.n == 313 - 3 * 4
    for i in depth:
        np.testing.assert_array_equal(pts["xyz"][i], fp[i, :3])
        np.testing.assert_array_equal(pts["cov"][i], P[c[i]:c[i] + 3, c[i]:c[i] + 3])
        assert pts["linearity"][i] == 1e300
    assert np.all(pts["linearity"][4:] < 1e300)
    np.testing.assert_array_equal(pts["type"], t)
    np.testing.assert_array_equal(pts["covpos"], c)
    for k, b in (("cov", "B"), ("cov_cam", "B_cam"), ("xyz", "xyz_bound"), ("cam", "cam_bound")):
        assert worst_ratio(pts[k], ref[k], ref[b]) <= TOL, k


# ------------------------------------------------------------------------------- 3. the conversion the export mirrors
def test_export_agrees_with_conversion(eng_mod, seq50):
    seq = SyntheticSequence(50, 2)
    seq.par.inverseDepthLinearityIndexThreshold = 1e9
    e = make(eng_mod, seq)
    before = e.map_points().copy()
    ref, _ = reference(e)
    i = e.convert_inverse_depth_to_depth()
    assert i == 0
    _, fp, P = e.get_state()
    _, c = e.feature_layout()
    pos = c[i]
    assert np.all(np.abs(fp[i, :3] - before["xyz"][i]) <= TOL * ref["xyz_bound"][i])
    assert np.all(np.abs(P[pos:pos + 3, pos:pos + 3] - before["cov"][i]) <= TOL * ref["B"][i])
    after = e.map_points()
    assert after["type"][i] == mp.FEATURE_DEPTH and after["linearity"][i] == 1e300
    np.testing.assert_array_equal(after["xyz"][i], fp[i, :3])
    # default threshold: the conversion picks the first feature whose exported linearity index is below it
    e = make(eng_mod, seq50)
    thr = seq50.par.inverseDepthLinearityIndexThreshold
    picked = []
    for _ in range(3):
        below = np.flatnonzero(e.map_points()["linearity"] < thr)
        want = int(below[0]) if len(below) else -1
        assert e.convert_inverse_depth_to_depth() == want
        picked.append(want)
    print("conversions picked from the exported linearity index (default threshold):", picked)
    # and with a threshold that splits this map (the median index), so that the rule has something to pick
    lin = e.map_points()["linearity"]
    seq = SyntheticSequence(50, 2)
    seq.par.inverseDepthLinearityIndexThreshold = thr = float(np.median(lin))
    e = make(eng_mod, seq)
    picked = []
    for _ in range(3):
        below = np.flatnonzero(e.map_points()["linearity"] < thr)
        assert len(below) > 0
        assert e.convert_inverse_depth_to_depth() == int(below[0])
        picked.append(int(below[0]))
    assert len(set(picked)) == 3
    print(f"conversions picked from the exported linearity index (threshold {thr:.3e}):", picked)


# ------------------------------------------------------------------------------------------------------ 4. read-only
def test_export_is_read_only(eng_mod, seq50):
    e = make(eng_mod, seq50)
    a = e.get_state()
    ta = e.feature_layout()
    e.map_points()
    e.map_points()
    b = e.get_state()
    tb = e.feature_layout()
    for u, v in zip(a + ta, b + tb):
        np.testing.assert_array_equal(u, v)
    # two engines on the same frames in the reproducible sweep mode, one of them exporting after every step
    seq = SyntheticSequence(50, 5)
    plain = make(eng_mod, seq, steps=0, sweep_mode=SWEEP_LAUNCHES)
    exporting = make(eng_mod, seq, steps=0, sweep_mode=SWEEP_LAUNCHES)
    for kps, desc in seq.frames:
        plain.step(kps, desc)
        exporting.step(kps, desc)
        assert len(exporting.map_points()) == exporting.N
    for u, v in zip(plain.get_state(), exporting.get_state()):
        np.testing.assert_array_equal(u, v)


# ----------------------------------------------------------------------------------------------------------- 5. edges
def test_export_edges(eng_mod, seq12):
    seq = seq12
    e = eng_mod.EkfEngine(seq.cam, seq.par, 40, max_keypoints=64)
    e.reset()
    pts = e.map_points()
    assert len(pts) == 0 and pts.dtype.names[0] == "xyz"
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    N = e.N
    n = C.c_int(-1)
    assert e.L.ekf_get_map_points(e.h, None, 0, C.byref(n)) == 0 and n.value == N  # points = NULL: count only
    buf = (EkfMapPoint * N)()
    n = C.c_int(-1)
    assert e.L.ekf_get_map_points(e.h, buf, N - 1, C.byref(n)) == 2  # EKF_ERR_CAPACITY, and the count needed
    assert n.value == N and b"capacity" in e.L.ekf_last_error(e.h)
    assert all(p.covpos == 0 for p in buf)  # nothing was written
    assert e.L.ekf_get_map_points(e.h, buf, N, C.byref(n)) == 0 and n.value == N
    assert [p.covpos for p in buf] == [13 + 6 * i for i in range(N)]
    assert e.L.ekf_get_map_points(e.h, buf, N, None) == 1  # EKF_ERR_INVALID_ARG
    # a sharded engine refuses it, as it refuses the other map calls
    grp = LocalShardGroup(seq.cam, seq.par, seq.n_features, 2, max_keypoints=4 * seq.n_features + 64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, 0.5 * (seq.P0 + seq.P0.T))
    with pytest.raises(eng_mod.EkfError) as ei:
        grp.engines[0].map_points()
    assert ei.value.code == 1 and "sharded" in str(ei.value)
    grp.close()


# -------------------------------------------------------------------------------------------------------- 6. symmetry
@pytest.mark.parametrize("precision", [0, 2])
def test_covariances_are_exactly_symmetric(eng_mod, seq200, precision):
    pts = make(eng_mod, seq200, precision).map_points()
    for k in ("cov", "cov_cam"):
        np.testing.assert_array_equal(pts[k], pts[k].transpose(0, 2, 1))
        assert np.all(np.diagonal(pts[k], axis1=1, axis2=2) >= 0)


# -------------------------------------------------------------------------------------------------- 7. sample program
def s3_config_320(min_matches):
    """the test configuration with the S3 camera scaled to the 320 x 240 frames (map management on)"""
    c = s3_camera(320, 240)
    text = CONFIG % {"min_matches": min_matches}
    for key, old, new in [("PixelsX", "640", c.pixelsX), ("PixelsY", "480", c.pixelsY), ("FX", "525.060143149240389", c.fx),
                          ("FY", "524.245488213640215", c.fy), ("CX", "308.649343121753361", c.cx),
                          ("CY", "236.536005491807288", c.cy), ("DX", "0.007021618750000", c.dx),
                          ("DY", "0.007027222916667", c.dy)]:
        a, b = f'{key}: "{old}"', f'{key}: "{new!r}"'
        assert a in text, a
        text = text.replace(a, b)
    return text


def read_ply(path):
    lines = open(path).read().splitlines()
    end = lines.index("end_header")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    count = [int(ln.split()[2]) for ln in lines[:end] if ln.startswith("element vertex")]
    props = [ln.split()[1:] for ln in lines[:end] if ln.startswith("property")]
    assert props == [["double", n] for n in ("x", "y", "z", "sx", "sy", "sz")] + [["uchar", "inverse_depth"]]
    rows = [ln.split() for ln in lines[end + 1:] if ln]
    assert len(count) == 1 and len(rows) == count[0]
    return np.array([[float(v) for v in r[:6]] for r in rows]).reshape(-1, 6), np.array([int(r[6]) for r in rows], dtype=int)


def test_sample_program_writes_the_map(tmp_path):
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    sample, check = str(tmp_path / "ekf_sequence"), str(tmp_path / "map_points_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "map_points_check.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    outdir = tmp_path / "out"
    outdir.mkdir()
    threshold = "1e10"  # new-feature threshold on these frames (test_gpu_ncc.test_real_frames_engine_equals_oracle)
    r = subprocess.run([sample, str(cfg), SEQ + "/", str(outdir) + "/", "0", "99999", threshold], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 7
    final_features = int(steps[-1].split("features")[1].split()[0])
    assert (outdir / "output.yml").exists() and (outdir / "log.txt").exists()
    ply, inv = read_ply(str(outdir / "map.ply"))
    assert len(ply) == final_features > 0
    assert np.all(ply[:, 3:] >= 0) and set(inv) <= {0, 1}
    # the same run through the driver class, exported at the end: ImageEKF::writeMapPly against ImageEKF::mapPoints in one
    # process, and the sample's file against that export
    own = str(tmp_path / "own.ply")
    r = subprocess.run([check, str(cfg), SEQ + "/", threshold, own], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"features {final_features}"
    exported = np.array([[float(v) for v in ln.split()[1:7]] for ln in lines[1:]])
    types = np.array([int(ln.split()[7]) for ln in lines[1:]])
    ply2, inv2 = read_ply(own)
    np.testing.assert_array_equal(ply2[:, :3], exported[:, :3])  # %.17g round-trips
    np.testing.assert_array_equal(ply2[:, 3:], np.sqrt(exported[:, 3:]))
    np.testing.assert_array_equal(inv2, (types == mp.FEATURE_INVERSE_DEPTH).astype(int))
    np.testing.assert_array_equal(ply[:, :3], exported[:, :3])
    np.testing.assert_array_equal(inv, inv2)
