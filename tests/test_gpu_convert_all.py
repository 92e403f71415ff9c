"""ekf_convert_all_inverse_depth_to_depth (k_convert_all_prepare, k_convert_all_P in csrc/kernels_map.hip; host half in
csrc/map_host.cpp) through the C ABI, PER ENTRY against tests/convert_all_ref.py (numpy, np.longdouble): every entry of P' and of
the new positions, the layout, and everything the call must leave alone, at the sizes where 3-row features straddle the kernel's
64-row tiles; then the selection, an asymmetric P, the single route's map, history independence, the refusals, the driver class
and the sample program.

Every bound is derived, not measured (convert_all_ref.py: u_store |ref| + K u64 sum|terms| with map_ref.convert_ref's counts; moved
entries: bit for bit); the tests print the worst |device - reference| / tolerance per output (DESIGN.md 9.2 lists what the MI355X
gave).  tests/test_convert_all_ref_cpu.py holds the reference to the single-conversion reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import convert_all_ref as car
import map_ref as mr
import predict_ref as pr
from openekfmonoslam_amd.ekftypes import DESC_BYTES, FEATURE_DEPTH, FEATURE_INVERSE_DEPTH, s3_params
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
FRAMES = os.path.join(ROOT, "tests", "golden", "s3_frames")
F64, F32, F32_EXACT, F64_EXACT = 0, 1, 2, 3
INVALID_ARG, NOT_POSITIVE_DEFINITE = 1, 3

# (n, pos) of map_ref.convert_scene -> n' with every inverse-depth feature converted: 3-row features across every 64-tile seam, old
# and new indices on both sides of 256, a leading run of 79 kept features (514, 250), one converted last feature (514, 508)
CASES = {(259, 13): 175, (514, 13): 346, (514, 250): 424, (514, 508): 511}
PER_ENTRY = [(*c, p) for c in CASES for p in (F64, F32)] + [(514, 13, p) for p in (F32_EXACT, F64_EXACT)]


def u_store(precision):
    return pr.U32 if precision in (F32, F32_EXACT) else 0.0


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def report(what, n, dev, ref, tol, precision=F64):
    r, at = pr.worst_ratio(dev, ref, tol)
    print(f"\nconvert all: {what:12s} precision {precision} n {n:4d}: worst |dev - ref| / tol = {r:.3f} at {at}", end="")
    return r, at


def descriptors(N, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, DESC_BYTES), dtype=np.uint8)


def snapshot(e):
    """everything a map operation may touch, host mirrors and device arrays"""
    x, fp, P = e.get_state()
    desc, tp, tm = e.get_map_features()
    t, c = e.feature_layout()
    mp = e.map_points()
    return {"n": e.n, "N": e.N, "x": x, "fp": fp, "P": P, "desc": desc, "tp": tp, "tm": tm, "type": t.copy(), "covpos": c.copy(),
            "dev_type": mp["type"].copy(), "dev_covpos": mp["covpos"].copy(), "dev_tp": mp["times_predicted"].copy(),
            "dev_tm": mp["times_matched"].copy()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_unchanged(before, after, what):
    for k in before:
        if isinstance(before[k], np.ndarray):
            assert same_bits(before[k], after[k]), (what, k)
        else:
            assert before[k] == after[k], (what, k)


def check_layout(snap, types, covpos, what=""):
    for k in ("type", "dev_type"):
        np.testing.assert_array_equal(snap[k], types, err_msg=f"{what} {k}")
    for k in ("covpos", "dev_covpos"):
        np.testing.assert_array_equal(snap[k], covpos, err_msg=f"{what} {k}")


def check_batch(e, precision, what):
    """one ekf_convert_all_inverse_depth_to_depth on e as it stands (threshold above every index), per entry against
    convert_all_ref built from the state e returns -> (snapshot before, snapshot after, reference)"""
    b = snapshot(e)
    sel = np.nonzero(b["type"] == FEATURE_INVERSE_DEPTH)[0]
    ref = car.convert_all_ref(b["x"], b["fp"], b["type"], b["covpos"], b["P"], sel, u_store(precision))
    got = e.convert_all_inverse_depth_to_depth()
    a = snapshot(e)
    assert got.dtype == np.int32 and got.tolist() == sel.tolist(), what
    assert (a["n"], a["N"]) == (b["n"] - 3 * len(sel), b["N"]) and a["P"].shape == (ref["n"], ref["n"]), what
    bad = []
    for name, dev, (want, tol) in (("P", a["P"], ref["P"]), ("xyz", a["fp"][sel, 0:3], ref["xyz"])):
        r, at = report(name, b["n"], dev, want, tol, precision)
        if not (r <= 1.0):  # (a NaN is a failure)
            bad.append((name, r, at))
    assert not bad, (what, bad)
    kept, s = ref["kept"], ref["s"]
    assert same_bits(a["P"][np.ix_(kept, kept)], b["P"][np.ix_(s[kept], s[kept])]), what  # moved, bit for bit, both triangles
    assert (a["fp"][sel, 3:6] == 0).all(), what
    others = np.setdiff1d(np.arange(b["N"]), sel)
    assert same_bits(a["fp"][others], b["fp"][others]), what
    check_layout(a, ref["types"], ref["covpos"], what)
    np.testing.assert_array_equal(ref["covpos"], mr.layout(ref["types"])[0])
    for k in ("x", "desc", "tp", "tm", "dev_tp", "dev_tm"):
        assert same_bits(a[k], b[k]), (what, k)
    return b, a, ref


def scene_engine(eng_mod, n, pos, precision, P=None):
    s = mr.convert_scene(n, pos)
    e = eng_mod.EkfEngine(s.cam, mr.convert_params(), s.n_features, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(s.n_features, n + pos), s.P0 if P is None else P)
    return e, s


# ------------------------------------------------------------------------------------------------ 1. per entry
@pytest.mark.parametrize("n,pos,precision", PER_ENTRY)
def test_convert_all_per_entry(eng_mod, n, pos, precision):
    """set_state, predict (P is a predicted covariance, bitwise symmetric), the call: every entry of P' and of the new positions
    within its bound, P' bitwise symmetric, the new layout in the host mirrors and the device tables, x, descriptors and counters
    untouched.  (514, 508): one feature converts, and the result also passes the single conversion's check."""
    e, s = scene_engine(eng_mod, n, pos, precision)
    e.predict()
    b, a, ref = check_batch(e, precision, (n, pos, precision))
    assert a["n"] == CASES[(n, pos)]
    np.testing.assert_array_equal(a["P"], a["P"].T)
    if (n, pos) == (514, 508):
        fi = (pos - 13) // 3
        single = mr.convert_ref(b["x"], b["fp"], b["type"], b["covpos"], b["P"], fi, u_store(precision))
        mr.check_converted(lambda *args: report(*args, precision=precision), n, b["P"], a["P"], a["fp"], single, fi, b["fp"])


# ------------------------------------------------------------------------------------------------ 2. selection
@pytest.mark.parametrize("precision", [F64, F32])
def test_convert_all_selects_the_features_below_the_threshold(eng_mod, precision):
    """convert_all_ref.select_many_scene: four of six inverse-depth features a factor 4 below the threshold, on both sides of
    k_linearity's workgroup seam; 100 and 255 a factor 4 or more above it"""
    s, P, thr = car.select_many_scene()
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = thr
    N = car.SELECT_MANY_N
    e = eng_mod.EkfEngine(s.cam, par, N, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(N, N), P)
    b = snapshot(e)
    assert b["n"] == 931
    got = e.convert_all_inverse_depth_to_depth()
    assert got.tolist() == list(car.SELECT_MANY_CHOSEN) == [0, 254, 256, 299]
    a = snapshot(e)
    nt = b["type"].copy()
    nt[list(car.SELECT_MANY_CHOSEN)] = FEATURE_DEPTH
    check_layout(a, nt, mr.layout(nt)[0], f"selection, precision {precision}")
    assert a["n"] == 919 and (a["type"][[100, 255]] == FEATURE_INVERSE_DEPTH).all()
    ref = car.convert_all_ref(b["x"], b["fp"], b["type"], b["covpos"], b["P"], got, u_store(precision))
    r, at = report("P selected", b["n"], a["P"], *ref["P"], precision)
    assert r <= 1.0, (r, at)


def test_a_small_index_buffer_does_not_stop_the_conversion(eng_mod):
    s, P, thr = car.select_many_scene()
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = thr
    N = car.SELECT_MANY_N
    engines = []
    for _ in range(3):
        e = eng_mod.EkfEngine(s.cam, par, N, max_keypoints=64)
        e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(N, N), P)
        engines.append(e)
    full, two, none = engines
    want = full.convert_all_inverse_depth_to_depth()
    idx = np.full(4, -7, dtype=np.int32)
    count = C.c_int(-1)
    assert two.L.ekf_convert_all_inverse_depth_to_depth(two.h, idx.ctypes.data_as(C.c_void_p), 2, C.byref(count)) == 0
    assert count.value == 4 and idx.tolist() == [0, 254, -7, -7]
    count = C.c_int(-1)
    assert none.L.ekf_convert_all_inverse_depth_to_depth(none.h, None, 0, C.byref(count)) == 0 and count.value == 4
    a = snapshot(full)
    assert len(want) == 4 and a["n"] == 919
    for e in (two, none):
        assert_unchanged(a, snapshot(e), "index buffer")


@pytest.mark.parametrize("precision", [F64, F32])
def test_nothing_below_the_threshold_changes_nothing(eng_mod, precision):
    s, P, thr = mr.select_scene(300, None)
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = thr
    e = eng_mod.EkfEngine(s.cam, par, 300, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(300, 300), P)
    b = snapshot(e)
    assert len(e.convert_all_inverse_depth_to_depth()) == 0
    assert_unchanged(b, snapshot(e), ("no conversion", precision))
    empty = eng_mod.EkfEngine(s.cam, par, 8, max_keypoints=64, precision=precision)
    empty.reset()
    assert len(empty.convert_all_inverse_depth_to_depth()) == 0 and (empty.N, empty.n) == (0, 13)


# ------------------------------------------------------------------------------------------------ 3. asymmetric upload
@pytest.mark.parametrize("precision", [F64, F32])
def test_an_asymmetric_upload_is_read_in_its_upper_triangle(eng_mod, precision):
    """the strict lower triangle of the uploaded P perturbed by a quarter, no prediction behind it: kept x kept entries are moved
    bit for bit in both triangles (check_batch), every other entry is the reference's -- formed from the upper triangle and the
    diagonal blocks of the converted features as they are stored -- and equals its mirror"""
    s = mr.convert_scene(259, 13)
    Q = np.asarray(s.P0, dtype=np.float64) * (1.0 + 0.25 * np.tril(np.ones((259, 259)), -1))
    e, _ = scene_engine(eng_mod, 259, 13, precision, P=Q)
    b, a, ref = check_batch(e, precision, ("asymmetric", precision))
    assert not np.array_equal(b["P"], b["P"].T)
    kept = ref["kept"]
    moved = kept[:, None] & kept[None, :]
    assert same_bits(a["P"][~moved], a["P"].T[~moved])
    assert not np.array_equal(a["P"], a["P"].T)  # (the kept x kept entries keep the asymmetry they came with)


# ------------------------------------------------------------------------------------------------ 4. the single route's map
def test_the_map_is_the_one_the_single_conversions_leave(eng_mod):
    A, s = scene_engine(eng_mod, 514, 13, F64)
    B, _ = scene_engine(eng_mod, 514, 13, F64)
    for e in (A, B):
        e.predict()
    got = A.convert_all_inverse_depth_to_depth()
    singles = []
    while True:
        k = B.convert_inverse_depth_to_depth()
        if k < 0:
            break
        singles.append(k)
    assert got.tolist() == singles and len(singles) == 56
    a, b = snapshot(A), snapshot(B)
    for k in ("N", "n"):
        assert a[k] == b[k], k
    for k in ("type", "covpos", "dev_type", "dev_covpos", "fp", "x", "desc", "tp", "tm"):
        assert same_bits(a[k], b[k]), k
    scale = np.abs(b["P"]).max()
    print(f"\nconvert all vs 56 single conversions, fp64: max |P_A - P_B| / max|P| = {np.abs(a['P'] - b['P']).max() / scale:.3g}", end="")


# ------------------------------------------------------------------------------------------------ 5. history independence
@pytest.mark.parametrize("precision", [F32_EXACT, F64])
def test_steps_after_the_batch_conversion_do_not_depend_on_the_history(eng_mod, precision):
    """The protocol and the acceptance rule of test_gpu_map_stages.test_steps_after_map_operations_do_not_depend_on_the_history.
    Engine A: a step, the batch conversion (every feature: the threshold is 1e9), two steps.  Engine B: a fresh engine given A's
    state right behind the conversion, and the same two steps.  A's buffers hold what the wider map left beyond n (and its second
    covariance buffer the matrix before the conversion); B's hold zeros there."""
    seq = SyntheticSequence(100, 3)
    seq.par.inverseDepthLinearityIndexThreshold = 1e9
    mk = len(max((f[0] for f in seq.frames), key=len)) + 64

    def fresh():
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=mk, precision=precision)
        e.set_sweep_mode(4)
        return e

    def finish(e):
        infos = [e.step(*seq.frames[t]) for t in (1, 2)]
        assert all(i.status == 0 for i in infos) and infos[0].n_inliers > 0
        x, fp, P = e.get_state()
        return x, fp, P, np.array([(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos])

    A = fresh()
    A.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    A.step(*seq.frames[0])
    assert len(A.convert_all_inverse_depth_to_depth()) == 100
    mid = snapshot(A)
    assert (mid["N"], mid["n"]) == (100, 313) and (mid["type"] == FEATURE_DEPTH).all()
    got = finish(A)
    runs = []
    for _ in range(2):
        B = fresh()
        B.set_state(mid["x"], mid["fp"], mid["type"], mid["desc"], mid["P"])
        assert_unchanged({k: mid[k] for k in ("x", "fp", "P", "type", "covpos")}, snapshot(B), "state handed to B")
        runs.append(finish(B))
    exact = all(same_bits(u, v) for u, v in zip(runs[0], runs[1]))
    print(f"history independence, precision {precision}: control runs bit-identical: {exact}")
    for name, u, v in zip(("x", "feature_pos", "P", "counts"), got, runs[0]):
        if exact:
            assert same_bits(u, v), (name, float(np.max(np.abs(u - v))))
        else:
            assert np.max(np.abs(u - v)) <= 1e-12 * max(np.max(np.abs(v)), 1e-300), (name, float(np.max(np.abs(u - v))))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_sharded_engine_refuses(eng_mod, seq12):
    seq = seq12
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = 1e9
    grp = LocalShardGroup(seq.cam, par, seq.n_features, 2, max_keypoints=4 * seq.n_features + 64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, 0.5 * (seq.P0 + seq.P0.T))
    e = grp.engines[0]

    def view():
        x, fp, P = e.get_state()
        t, c = e.feature_layout()
        return {"n": e.n, "N": e.N, "x": x, "fp": fp, "P": P, "type": t.copy(), "covpos": c.copy()}

    before = view()
    with pytest.raises(eng_mod.EkfError) as ei:
        e.convert_all_inverse_depth_to_depth()
    assert ei.value.code == INVALID_ARG and "sharded" in str(ei.value)
    assert_unchanged(before, view(), "sharded")
    grp.close()


def indefinite_between_two_features(seq, i=5, j=6):
    """seq.P0 with the cross-covariance of features i and j set to 100 sigma_i sigma_j on its diagonal: every 2 x 2 innovation
    covariance (the gates, the 1-point hypotheses, the rescue) is the one P0 gives, the joint S of an update that holds both
    features is not positive definite.  On frame 0 of the sequence below one match is a low-innovation inlier (feature 0) and the
    other eleven are rescued, so it is the step's second and last update that fails (the oracle: status 3, 1 + 11 matches)."""
    P = seq.P0.copy()
    d = np.sqrt(np.diag(P))
    for k in range(6):
        a, b = 13 + 6 * i + k, 13 + 6 * j + k
        P[a, b] = P[b, a] = 100.0 * d[a] * d[b]
    return P


def test_a_pending_asynchronous_error_is_reported_and_nothing_converted(eng_mod):
    """ekf_set_async_errors: a step does not read the error flag of its last update back.  A covariance with which the step's last
    update fails: the control engine (errors read in the step) reports EKF_ERR_NOT_POSITIVE_DEFINITE from the step, the
    asynchronous one returns from the step and the batch conversion behind it reports that error, as ekf_update_external does,
    and converts nothing; asked again it converts the map."""
    seq = SyntheticSequence(12, 1, outlier_fraction=0.0, distractors_per_feature=0.0, max_bit_flips=0)
    seq.par.inverseDepthLinearityIndexThreshold = 1e9
    P = indefinite_between_two_features(seq)
    engines = []
    for on in (False, True):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=len(seq.frames[0][0]) + 64)
        e.set_async_errors(on)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P)
        engines.append(e)
    sync, asyn = engines
    with pytest.raises(eng_mod.EkfError) as ei:
        sync.step(*seq.frames[0])
    assert ei.value.code == NOT_POSITIVE_DEFINITE
    info = asyn.step(*seq.frames[0])
    assert info.status == 0 and (info.n_matches, info.n_inliers, info.n_rescued) == (12, 1, 11)
    with pytest.raises(eng_mod.EkfError) as ei:
        asyn.convert_all_inverse_depth_to_depth()
    assert ei.value.code == NOT_POSITIVE_DEFINITE and "positive definite" in str(ei.value)
    a = snapshot(asyn)  # (the error was reported and cleared by the call above)
    assert (a["N"], a["n"]) == (12, 85) and (a["type"] == FEATURE_INVERSE_DEPTH).all() and (a["dev_type"] == FEATURE_INVERSE_DEPTH).all()
    assert len(asyn.convert_all_inverse_depth_to_depth()) == 12 and asyn.n == 49


# ------------------------------------------------------------------------------------------------ 7. driver class and sample
def read_ply_flags(path):
    lines = open(path).read().splitlines()
    end = lines.index("end_header")
    return np.array([int(ln.split()[6]) for ln in lines[end + 1:] if ln], dtype=int)


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setConvertAll and EKF::convertAllMapFeaturesInverseDepthToDepth over the committed frames
    (tests/cpp/convert_all_check.cpp), and ekf_sequence with and without --convert-all on a configuration that manages the map on
    every step and puts every inverse-depth feature below the threshold: with the flag the last frame holds fewer inverse-depth
    features, every feature older than the last tick is XYZ in map.ply and log.txt counts the conversions of every tick; without
    it one feature converts per tick and log.txt has no such line"""
    import re

    import yaml

    from tests.test_gpu_map_points import s3_config_320

    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check_bin, sample = str(tmp_path / "convert_all_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check_bin, os.path.join(ROOT, "tests", "cpp", "convert_all_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    text = s3_config_320(40)
    old = 'InverseDepthLinearityIndexThreshold: "0.1"'
    assert old in text and 'MapManagementFrequency: "1"' in text
    cfg = tmp_path / "config.yml"
    cfg.write_text(text.replace(old, 'InverseDepthLinearityIndexThreshold: "1e9"'))
    r = subprocess.run([check_bin, str(cfg), FRAMES + "/", "1e10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("step")]) == 7 and "class features" in r.stdout
    runs = {}
    for name, flags in (("default", []), ("all", ["--convert-all"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([sample, str(cfg), FRAMES + "/", str(out) + "/", "0", "99999", "1e10"] + flags, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        doc = yaml.safe_load(re.sub(r"!!opencv-matrix", "", (out / "output.yml").read_text().split("\n", 1)[1]))
        frames = [doc[f"Frame {k}"] for k in range(1, 8)]
        runs[name] = {"inv": [f["MapFeaturesInvDepthCount"] for f in frames], "depth": [f["MapFeaturesDepthCount"] for f in frames],
                      "keys": [list(f) for f in frames], "log": (out / "log.txt").read_text(), "ply": read_ply_flags(str(out / "map.ply"))}
    d, a = runs["default"], runs["all"]
    assert a["inv"][-1] < d["inv"][-1]
    assert d["keys"] == a["keys"]  # output.yml keeps its schema
    assert "Converted to depth" not in d["log"] and all(0 < dk <= k for k, dk in enumerate(d["depth"], 1))  # one conversion per tick
    logged = [int(ln.split(":")[1]) for ln in a["log"].splitlines() if ln.startswith("Converted to depth:")]
    assert len(logged) == 7 and logged[0] > 1 and sum(logged) >= a["depth"][-1] > 7
    inv = a["ply"]
    assert inv.sum() == a["inv"][-1] and (np.diff(inv) >= 0).all()  # the inverse-depth features are the ones the last tick added
