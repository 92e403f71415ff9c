"""The external measurement update on the device (ekf_update_external and its two helpers, kernels_external.hip; DESIGN.md
section 4.13) against the engine's own visual update, against its numpy restatement (tests/external_update_ref.py), and through
the C++ driver class and the sample program.

Maps: seq12 (n = 85: one partial tile of the downdate, less than one 256-column block), seq50 (n = 313: two column blocks,
several tiles, a ragged edge), a mixed map of depth and inverse-depth features (n = 301: covpos is not 13 + 6 i) and a
200-feature sequence (n = 1213: many tile rows).

Tolerances.  fp64 storage: the project's fp64 gate, parity_metric.F64_TOL, on every block.  fp32 storage: the state is formed
in fp64 from the same widened P, so x and the features keep F64_TOL; an entry of P is the reference's fp64 value rounded once
to fp32, and two fp64 sums that differ in their last bits can straddle a rounding boundary, so it may sit on the neighbouring
fp32 value: |got - ref| <= 2^-23 |ref| + F64_TOL max|P|.  The entries of rows / columns 3..6 are formed by the normalisation
from entries that were already rounded once, each of which may sit on its neighbour: |ref| is replaced by sum |J| |P| + |ref|
(one factor J for a strip entry, J on both sides for the 4 x 4 block).  These bounds follow from rounding to nearest; they are
not measured.

Worst figures measured on an MI355X (printed by the tests before they assert): against ekf_update 3.0e-15 (w block), P 4.4e-16;
against the reference nis 6.0e-16, z 4.1e-16, feature parameters 5.7e-16 component-wise, P (fp64 storage) 3.3e-16 in the max
norm; fp32 storage: |err| / bound at most 7.9e-22 -- the entries that differ from the reference at all are cancellation
residues, 1e-16 of the terms they are the difference of, far below F64_TOL max|P|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import external_update_ref as xr
import map_points_ref as mp
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE, EkfExternalUpdate
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import F64_TOL, block_errs, over_tolerance, parity_report, rel_fro, rel_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
SWEEP_LAUNCHES = 4  # EKF_SWEEP_LAUNCHES: the run-to-run reproducible mode
MAPS = ["seq12", "seq50", "mixed", "seq200"]
NOT_POSITIVE_DEFINITE = 3


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


@pytest.fixture(scope="module")
def seqs(seq12, seq50):
    return {"seq12": seq12, "seq50": seq50, "seq200": SyntheticSequence(200, 2)}


def make(eng_mod, seqs, which, precision=0, steps=2, sweep_mode=None):
    """the engine after two steps (test_gpu_map_points.make); "mixed": the map of
    test_mixed_map_depth_features_are_copied_exactly, four depth features in front of 46 inverse-depth ones"""
    if which == "mixed":
        seq = SyntheticSequence(50, 4)
        seq.par.inverseDepthLinearityIndexThreshold = 1e9  # every call converts the first remaining inverse-depth feature
        e = eng_mod.EkfEngine(seq.cam, seq.par, 66, max_keypoints=264, precision=precision)
    else:
        seq = seqs[which]
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=4 * seq.n_features + 64, precision=precision)
    if sweep_mode is not None:
        e.set_sweep_mode(sweep_mode)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    if which == "mixed":
        for t, (kps, desc) in enumerate(seq.frames):
            e.step(kps, desc)
            assert e.convert_inverse_depth_to_depth() == t
        assert e.n == 301
    else:
        for kps, desc in seq.frames[:steps]:
            e.step(kps, desc)
    return e, seq


def snapshot(e):
    """everything an external update may change, and what it must not"""
    return e.get_state() + e.feature_layout() + e.get_map_features()


def assert_same_bits(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def storage_of(precision):
    return np.float32 if precision in (1, 2) else np.float64


def reference(e, rows, residual, R, gate_nis=0.0):
    x, fp, P = e.get_state()
    t, c = e.feature_layout()
    return xr.external_update_ref(x, fp, t, c, P, *rows, residual, R, gate_nis, storage_of(e.precision))


def check_against_reference(e, got, ref, label):
    """the engine after the call against the reference's outcome; prints every figure before it asserts"""
    assert got["applied"] == (ref["status"] == "applied") and got["rows"] == len(ref["z"])
    nis_err = abs(got["nis"] - ref["nis"]) / ref["nis"]
    z_err = np.abs(got["z"] - ref["z"]).max() / np.abs(ref["z"]).max()
    x, fp, P = e.get_state()
    be = block_errs(x, fp, ref["x13"], ref["feature_pos"])
    Pr = ref["P"]
    if storage_of(e.precision) is np.float64:
        p_fig = {"P_max": rel_max(P, Pr), "P_fro": rel_fro(P, Pr)}
        p_ok = p_fig["P_max"] <= F64_TOL and p_fig["P_fro"] <= F64_TOL
    else:
        scale = np.abs(Pr)
        strip = np.zeros(P.shape, dtype=bool)
        strip[3:7, :] = strip[:, 3:7] = True
        scale[strip] += ref["strip_bound"][strip]
        bound = 2.0 ** -23 * scale + F64_TOL * np.abs(Pr).max()
        ratio = np.abs(P - Pr) / bound
        p_fig = {"P worst |err| / bound": float(ratio.max()), "P entries off the reference": int((P != Pr).sum())}
        p_ok = bool(np.all(ratio <= 1.0))
    print(f"{label}: nis {nis_err:.1e} z {z_err:.1e}", {k: f"{v:.1e}" for k, v in be.items()}, p_fig)
    assert nis_err <= F64_TOL and z_err <= F64_TOL
    assert not over_tolerance(be, F64_TOL), be
    assert p_ok, p_fig
    np.testing.assert_array_equal(P, P.T)


# ---- the rows the tests feed
def distance_row(e, i, j):
    """(rows, h): u' Jw_i on feature i's columns, -u' Jw_j on feature j's, columns ascending"""
    _, fp, _ = e.get_state(want_P=False)
    t, c = e.feature_layout()
    Xi, Ji = mp.world_point(fp[i], t[i])
    Xj, Jj = mp.world_point(fp[j], t[j])
    h = np.linalg.norm(Xi - Xj)
    u = (Xi - Xj) / h
    parts = sorted([(int(c[i]), u @ Ji), (int(c[j]), -(u @ Jj))])
    col = np.concatenate([np.arange(pos, pos + len(v)) for pos, v in parts]).astype(np.int32)
    val = np.concatenate([v for _, v in parts])
    return (np.array([0, len(col)], dtype=np.int32), col, val), h


POSITION_ROWS = (np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.ones(3))
POSITION_R = 1e-4 * np.array([[2.0, 0.5, 0.2], [0.5, 1.5, -0.3], [0.2, -0.3, 1.0]])
POSITION_OFFSET = np.array([0.003, -0.002, 0.001])


def random_rows(n, seed):
    """16 rows of exactly 32 entries; row 0 touches column 0, row 1 column n - 1; R = A A' + I"""
    rng = np.random.default_rng(seed)
    cols = []
    for i in range(16):
        k = rng.choice(n, size=32, replace=False)
        if i == 0 and 0 not in k:
            k[0] = 0
        if i == 1 and n - 1 not in k:
            k[0] = n - 1
        cols.append(np.sort(k))
    assert all(len(set(k)) == 32 for k in cols) and cols[0][0] == 0 and cols[1][-1] == n - 1
    col = np.concatenate(cols).astype(np.int32)
    val = rng.standard_normal(len(col))
    A = 0.5 * rng.standard_normal((16, 16))
    return (np.arange(0, 16 * 32 + 1, 32, dtype=np.int32), col, val), 0.01 * rng.standard_normal(16), A @ A.T + np.eye(16)


def visual_matches(e):
    """<= 8 matches for the first predicted features, a fraction of a pixel off their predictions, with the engine's Jacobians"""
    preds, Hs, Hf = e.predict_measurements()
    k = min(8, len(preds))
    assert k >= 4
    m = np.zeros(k, dtype=MATCH_DTYPE)
    m["featureIndex"] = preds["featureIndex"][:k]
    m["keypointIndex"] = -1
    m["imagePos"] = preds["imagePos"][:k] + np.array([0.3, -0.2]) * (1 + np.arange(k))[:, None] / k
    return m, preds[:k], Hs[:k], Hf[:k]


# ------------------------------------------------------------------------------ 1. against the engine's own visual update
@pytest.mark.parametrize("which", ["seq12", "seq50", "mixed"])
def test_camera_rows_reproduce_the_visual_update(eng_mod, seqs, which):
    a, seq = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    b, _ = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    assert_same_bits(a.get_state(), b.get_state())
    m, preds, Hs, Hf = visual_matches(a)
    t, c = a.feature_layout()
    rows, residual = xr.visual_rows(preds, Hs, Hf, m, t, c)
    if which == "mixed":
        assert set(np.diff(rows[0])) == {16, 19}  # depth features among the matches
    else:
        assert np.all(np.diff(rows[0]) == 19)
    a.update(m)
    got = b.update_external(rows, residual, seq.cam.pixelErrorX * np.eye(len(residual)))
    assert got["applied"] and got["rows"] == 2 * len(m)
    be = parity_report(*b.get_state(), *a.get_state())
    print(f"{which}: update_external with the camera's rows against ekf_update:", {k: f"{v:.1e}" for k, v in be.items()})
    assert not over_tolerance(be, F64_TOL), be


# ------------------------------------------------------------------------------------------- 2. against the reference
@pytest.mark.parametrize("precision", [0, 1, 2, 3])
@pytest.mark.parametrize("which", MAPS)
def test_update_matches_reference(eng_mod, seqs, which, precision):
    e, _ = make(eng_mod, seqs, which, precision)
    n, N = e.n, e.N
    # m = 1: a distance between the first and the last feature, 5 % off
    rows, h = distance_row(e, 0, N - 1)
    residual, R = np.array([0.05 * h]), np.array([[(0.01 * h) ** 2]])
    ref = reference(e, rows, residual, R)
    check_against_reference(e, e.update_external(rows, residual, R), ref, f"{which} precision {precision} m = 1")
    # m = 3: a position fix with a full covariance
    ref = reference(e, POSITION_ROWS, POSITION_OFFSET, POSITION_R)
    check_against_reference(e, e.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R), ref, f"{which} precision {precision} m = 3")
    # m = 16: random rows of 32 entries
    rows, residual, R = random_rows(n, 100 + n)
    ref = reference(e, rows, residual, R)
    check_against_reference(e, e.update_external(rows, residual, R), ref, f"{which} precision {precision} m = 16")


def test_dense_rows_are_the_same_call(eng_mod, seqs):
    a, _ = make(eng_mod, seqs, "seq12", sweep_mode=SWEEP_LAUNCHES)
    b, _ = make(eng_mod, seqs, "seq12", sweep_mode=SWEEP_LAUNCHES)
    H = np.zeros((3, a.n))
    H[0, 0] = H[1, 1] = H[2, 2] = 1.0
    ra = a.update_external(H, POSITION_OFFSET, POSITION_R)
    rb = b.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R)
    assert ra["nis"] == rb["nis"] and ra["applied"] and rb["applied"]
    assert_same_bits(a.get_state(), b.get_state())


# ------------------------------------------------------------------------------------------- 3. symmetry and extent
@pytest.mark.parametrize("precision", [0, 1, 2, 3])
def test_uploaded_asymmetric_covariance_comes_out_symmetric(eng_mod, seq50, precision):
    seq = seq50
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=64, precision=precision)
    rng = np.random.default_rng(3)
    P0 = seq.P0 * (1.0 + 1e-3 * np.triu(rng.standard_normal(seq.P0.shape), 1))  # off by a part in a thousand above the diagonal
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P0)
    _, _, P = e.get_state()
    assert np.any(P != P.T)
    ref = reference(e, POSITION_ROWS, POSITION_OFFSET, POSITION_R)
    check_against_reference(e, e.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R), ref,
                            f"asymmetric P0, precision {precision}")


@pytest.mark.parametrize("precision", [0, 1, 2, 3])
def test_gated_out_update_leaves_the_next_step_alone(eng_mod, seqs, precision):
    plain, seq = make(eng_mod, seqs, "seq50", precision, sweep_mode=SWEEP_LAUNCHES)
    gated, _ = make(eng_mod, seqs, "seq50", precision, sweep_mode=SWEEP_LAUNCHES)
    got = gated.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R, gate_nis=1e-9)
    assert not got["applied"] and got["nis"] > 1e-9
    assert_same_bits(snapshot(plain), snapshot(gated))
    for kps, desc in seq.frames[2:4]:
        plain.step(kps, desc)
        gated.step(kps, desc)
    assert_same_bits(snapshot(plain), snapshot(gated))


# --------------------------------------------------------------------------------------------- 4. gate and failure
@pytest.mark.parametrize("precision", [0, 2])
def test_gate_on_either_side_of_the_nis(eng_mod, seqs, precision):
    e, _ = make(eng_mod, seqs, "seq50", precision)
    nis = reference(e, POSITION_ROWS, POSITION_OFFSET, POSITION_R)["nis"]
    before = snapshot(e)
    got = e.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R, gate_nis=nis * (1 - 1e-6))
    assert not got["applied"] and got["rows"] == 3 and abs(got["nis"] - nis) <= F64_TOL * nis
    assert_same_bits(before, snapshot(e))
    ref = reference(e, POSITION_ROWS, POSITION_OFFSET, POSITION_R, gate_nis=nis * (1 + 1e-6))
    got = e.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R, gate_nis=nis * (1 + 1e-6))
    assert got["applied"]
    check_against_reference(e, got, ref, f"gate above the NIS, precision {precision}")


@pytest.mark.parametrize("precision", [0, 2])
def test_not_positive_definite_changes_nothing(eng_mod, seqs, precision):
    plain, seq = make(eng_mod, seqs, "seq50", precision, sweep_mode=SWEEP_LAUNCHES)
    failed, _ = make(eng_mod, seqs, "seq50", precision, sweep_mode=SWEEP_LAUNCHES)
    before = snapshot(failed)
    with pytest.raises(eng_mod.EkfError) as ei:
        failed.update_external(POSITION_ROWS, POSITION_OFFSET, -1e6 * np.eye(3))
    assert ei.value.code == NOT_POSITIVE_DEFINITE and "positive definite" in str(ei.value)
    assert_same_bits(before, snapshot(failed))
    assert failed.update_external(POSITION_ROWS, POSITION_OFFSET, -1e6 * np.eye(3), allow_errors=(3,)) == {"code": 3}
    for kps, desc in seq.frames[2:4]:
        info_p, info_f = plain.step(kps, desc), failed.step(kps, desc)
        assert info_f.status == 0 and info_p.n_inliers == info_f.n_inliers
    assert_same_bits(snapshot(plain), snapshot(failed))


# ------------------------------------------------------------------------------------------------------ 5. helpers
@pytest.mark.parametrize("which", ["seq50", "mixed"])
def test_helpers_build_the_rows_the_test_builds(eng_mod, seqs, which):
    a, _ = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    b, _ = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    x, _, _ = a.get_state(want_P=False)
    r = x[:3] + POSITION_OFFSET
    ga = a.fuse_camera_position(r, POSITION_R, gate_nis=1e3)
    gb = b.update_external(POSITION_ROWS, r - x[:3], POSITION_R, gate_nis=1e3)
    assert ga["applied"] and ga["nis"] == gb["nis"] and np.array_equal(ga["z"], gb["z"])
    assert_same_bits(a.get_state(), b.get_state())
    # a distance between a (depth, in the mixed map) feature and the last one: the helper's host trigonometry against numpy's
    i, j = 1, a.N - 1
    rows, h = distance_row(b, i, j)
    d, sigma = 1.1 * h, 1e-3 * 1.1 * h
    ref = reference(b, rows, np.array([d - h]), np.array([[sigma * sigma]]))
    ga = a.fuse_feature_distance(i, j, d, sigma)
    gb = b.update_external(rows, np.array([d - h]), np.array([[sigma * sigma]]))
    assert ga["applied"] and ga["rows"] == 1 and abs(ga["nis"] - gb["nis"]) <= F64_TOL * gb["nis"]
    be = parity_report(*a.get_state(), *b.get_state())
    print(f"{which}: fuse_feature_distance against update_external with the test's row:", {k: f"{v:.1e}" for k, v in be.items()})
    assert not over_tolerance(be, F64_TOL), be
    # the map's scale moved: the exported points are closer to the measured distance, by what the reference says
    pts = a.map_points()
    after = np.linalg.norm(pts["xyz"][i] - pts["xyz"][j])
    t, _ = a.feature_layout()
    want = np.linalg.norm(mp.world_point(ref["feature_pos"][i], t[i])[0] - mp.world_point(ref["feature_pos"][j], t[j])[0])
    print(f"{which}: distance {h:.6f} -> {after:.6f}, measured {d:.6f}, reference {want:.6f}")
    assert abs(after - d) < abs(h - d)
    assert abs(after - want) <= F64_TOL * want


def test_distance_helper_refuses_bad_arguments(eng_mod, seqs):
    e, _ = make(eng_mod, seqs, "seq12")
    before = snapshot(e)
    for args in [(0, 0, 1.0, 0.1), (-1, 2, 1.0, 0.1), (0, e.N, 1.0, 0.1), (0, 1, 1.0, 0.0), (0, 1, 1.0, -1.0), (0, 1, 0.0, 0.1),
                 (0, 1, -2.0, 0.1), (0, 1, float("nan"), 0.1)]:
        with pytest.raises(eng_mod.EkfError) as ei:
            e.fuse_feature_distance(*args)
        assert ei.value.code == 1, args
    assert_same_bits(before, snapshot(e))
    # h = 0: two features at the same world point
    x, fp, P = e.get_state()
    fp[1] = fp[0]
    t, _ = e.feature_layout()
    e.set_state(x, fp, t, None, P)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.fuse_feature_distance(0, 1, 1.0, 0.1)
    assert ei.value.code == 1 and "coincide" in str(ei.value)


# -------------------------------------------------------------------------------------------------------- 6. edges
def raw_call(e, m, row_start, col, val, residual, R, gate=0.0, out=None):
    a = [np.ascontiguousarray(v, dtype=dt) for v, dt in ((row_start, np.int32), (col, np.int32), (val, np.float64),
                                                          (residual, np.float64), (R, np.float64))]
    return e.L.ekf_update_external(e.h, m, *[v.ctypes.data_as(C.c_void_p) for v in a], gate, out)


def test_invalid_arguments_change_nothing(eng_mod, seqs):
    e, seq = make(eng_mod, seqs, "seq12")
    n = e.n
    before = snapshot(e)
    ok = dict(m=1, row_start=[0, 2], col=[0, 5], val=[1.0, 0.5], residual=[0.01], R=[1e-4])
    cases = {
        "m = 0": dict(m=0, row_start=[0]),
        "m = 17": dict(m=17, row_start=list(range(18)), col=list(range(17)), val=[1.0] * 17, residual=[0.0] * 17, R=np.eye(17)),
        "an empty row": dict(row_start=[0, 0]),
        "33 entries in a row": dict(row_start=[0, 33], col=list(range(33)), val=[1.0] * 33),
        "an unsorted column": dict(col=[5, 0]),
        "a repeated column": dict(col=[5, 5]),
        "col = n": dict(col=[0, n]),
        "col = -1": dict(col=[-1, 5]),
        "a NaN value": dict(val=[1.0, float("nan")]),
        "an infinite residual": dict(residual=[float("inf")]),
        "a NaN in R": dict(R=[float("nan")]),
        "gate_nis < 0": dict(gate=-1.0),
        "gate_nis NaN": dict(gate=float("nan")),
    }
    for name, change in cases.items():
        assert raw_call(e, **{**ok, **change}) == 1, name
        assert b"ekf_update_external" in e.L.ekf_last_error(e.h), name
    assert_same_bits(before, snapshot(e))
    # out = NULL is accepted, and the lower triangle of R is not read
    ref = reference(e, ([0, 2], [0, 5], [1.0, 0.5]), [0.01], [[1e-4]])
    assert raw_call(e, **ok) == 0
    x, fp, P = e.get_state()
    assert rel_max(P, ref["P"]) <= F64_TOL and np.any(before[2] != P)
    R = POSITION_R.copy()
    R[np.tril_indices(3, -1)] = np.nan
    out = EkfExternalUpdate()
    assert raw_call(e, 3, *POSITION_ROWS, POSITION_OFFSET, R, 0.0, C.byref(out)) == 0 and out.applied == 1 and out.rows == 3
    assert all(v == 0.0 for v in out.z[3:])


def test_sharded_engine_refuses(eng_mod, seq12):
    seq = seq12
    grp = LocalShardGroup(seq.cam, seq.par, seq.n_features, 2, max_keypoints=4 * seq.n_features + 64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, 0.5 * (seq.P0 + seq.P0.T))
    for call in (lambda g: g.update_external(POSITION_ROWS, POSITION_OFFSET, POSITION_R),
                 lambda g: g.fuse_camera_position(np.zeros(3), POSITION_R), lambda g: g.fuse_feature_distance(0, 1, 1.0, 0.1)):
        with pytest.raises(eng_mod.EkfError) as ei:
            call(grp.engines[0])
        assert ei.value.code == 1 and "sharded" in str(ei.value)
    grp.close()


@pytest.mark.parametrize("precision", [0, 2])
def test_empty_map_takes_camera_rows(eng_mod, seq12, precision):
    e = eng_mod.EkfEngine(seq12.cam, seq12.par, 40, max_keypoints=64, precision=precision)
    e.reset()
    assert e.N == 0 and e.n == 13
    ref = reference(e, POSITION_ROWS, POSITION_OFFSET, POSITION_R)
    check_against_reference(e, e.fuse_camera_position(POSITION_OFFSET, POSITION_R), ref, f"empty map, precision {precision}")
    with pytest.raises(eng_mod.EkfError):
        e.update_external(([0, 1], [13], [1.0]), [0.0], [[1.0]])  # column 13 does not exist


# ----------------------------------------------------------------------------------------------- 7. C++ and sample
def test_driver_class_and_sample_program(tmp_path):
    from tests.test_gpu_map_points import s3_config_320

    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    sample, check = str(tmp_path / "ekf_sequence"), str(tmp_path / "external_update_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "external_update_check.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    threshold = "1e10"  # new-feature threshold on these frames (test_gpu_ncc.test_real_frames_engine_equals_oracle)
    # ImageEKF::fuseCameraPosition / fuseFeatureDistance / updateExternal on the eight committed frames against the C ABI
    r = subprocess.run([check, str(cfg), SEQ + "/", threshold], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "external update through the driver class: ok" in r.stdout, r.stdout
    # the sample: one "position fix:" line per listed frame, under that frame's step line
    outdir = tmp_path / "out"
    outdir.mkdir()
    fixes = tmp_path / "fixes.txt"
    fixes.write_text("# frame x y z sigma\n2 0.0 0.0 0.0 0.05\n\n5 0.001 -0.002 0.0005 0.02  # a comment behind a fix\n")
    r = subprocess.run([sample, str(cfg), SEQ + "/", str(outdir) + "/", "0", "99999", threshold, "--position-fixes", str(fixes)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [k for k, ln in enumerate(lines) if ln.startswith("        position fix: nis ")]
    assert len(at) == 2, r.stdout
    for k, frame in zip(at, (2, 5)):
        assert lines[k - 1].startswith(f"step {frame} ") or lines[k - 1].startswith(f"step {frame}:"), lines[k - 1]
        assert float(lines[k].split("nis")[1]) >= 0.0
    assert (outdir / "output.yml").exists()
