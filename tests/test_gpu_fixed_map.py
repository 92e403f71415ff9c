"""The fixed-map (Schmidt-Kalman) camera update on the device (ekf_update_fixed_map / ekf_set_fixed_map, kernels_fixedmap.hip;
DESIGN.md section 4.14) against its numpy restatement (tests/fixed_map_ref.py), against the engine's own full update, inside the
step functions, and through the C++ driver class and the sample program.

Maps and helpers follow tests/test_gpu_external_update.py: seq12 (n = 85: less than one 256-column block of the strip), seq50
(n = 313: a ragged second block), a mixed map of depth and inverse-depth features (n = 301: covpos is not 13 + 6 i) and a
200-feature sequence (n = 1213).  The reference is the Python-loop one up to 64 measurement rows and its vectorised path above
(stated where it is used): the two agree to 1e-13 (tests/test_fixed_map_cpu.py), far inside the tolerance.

Tolerances are that file's; they follow from rounding to nearest, they are not measured.  fp64 storage: parity_metric.F64_TOL on
x13 and on the strip (rows and columns 0..12 of P) in the max norm and the Frobenius norm.  fp32 storage: x13 keeps F64_TOL (formed
in fp64 from the same widened P); a strip entry is the reference's fp64 value rounded once, so it may sit on the neighbouring fp32
value: |err| <= 2^-23 (|ref| + strip_bound on rows / columns 3..6) + F64_TOL max|P|.  Everything outside the strip, and
feature_pos, must have the bits it had before the call.

Worst figures measured on an MI355X (printed by the tests before they assert): against the reference, camera blocks 2.7e-15
(w block, mixed map; 5.1e-14 at N = 1400 with 2800 rows), strip in fp64 storage 5.8e-14 in the max norm and 1.8e-14 in the
Frobenius norm over the row-count edges (n = 1033, up to 320 rows) and 2.2e-12 / 4.2e-13 at N = 1400; fp32 storage: |err| / bound
at most 3.6e-24 -- the entries that differ from the reference at all are cancellation residues far below F64_TOL max|P|.  Against
ekf_update: x13 3.5e-18, strip 7.7e-16, NIS equal.  Frame 1 of the mode against its stage sequence: equal."""
import os
import subprocess

import numpy as np
import pytest

import external_update_ref as xr
import fixed_map_ref as fm
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import F64_TOL, block_errs, rel_fro, rel_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
SEQ = os.path.join(ROOT, "tests", "golden", "s3_frames")
SWEEP_AUTO, SWEEP_LAUNCHES = 2, 4  # EKF_SWEEP_AUTO: one persistent launch where it applies; _LAUNCHES: the run-to-run reproducible mode
MAPS = ["seq12", "seq50", "mixed", "seq200"]
INVALID_ARG, NOT_POSITIVE_DEFINITE = 1, 3
CAMERA = ("r", "q", "v", "w")


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


@pytest.fixture(scope="module")
def seqs(seq12, seq50):
    return {"seq12": seq12, "seq50": seq50, "seq200": SyntheticSequence(200, 2)}


@pytest.fixture(scope="module")
def seq170():
    return SyntheticSequence(170, 1, outlier_fraction=0.0, distractors_per_feature=0.0, max_bit_flips=0)


def make(eng_mod, seqs, which, precision=0, steps=2, sweep_mode=None):
    """the engine after two steps (test_gpu_external_update.make)"""
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


def fresh(eng_mod, seq, precision=0, sweep_mode=None, P=None):
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=4 * seq.n_features + 64, precision=precision)
    if sweep_mode is not None:
        e.set_sweep_mode(sweep_mode)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0 if P is None else P)
    return e


def snapshot(e):
    return e.get_state() + e.feature_layout() + e.get_map_features()


def assert_same_bits(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def storage_of(precision):
    return np.float32 if precision in (1, 2) else np.float64


def matches_for(preds, k=None):
    """matches for the first k (default: ALL) predicted features, a fraction of a pixel off their predictions"""
    k = len(preds) if k is None else k
    assert 1 <= k <= len(preds)
    m = np.zeros(k, dtype=MATCH_DTYPE)
    m["featureIndex"] = preds["featureIndex"][:k]
    m["keypointIndex"] = -1
    m["imagePos"] = preds["imagePos"][:k] + np.array([0.3, -0.2]) * (1 + np.arange(k))[:, None] / k
    return m


def reference(e, seq, m, preds, Hs, Hf, state=None):
    """the reference's outcome for the matches m from the engine's exported state (or the state given)"""
    x, fp, P = e.get_state() if state is None else state
    t, c = e.feature_layout()
    k = len(m)
    rows, residual = xr.visual_rows(preds[:k], Hs[:k], Hf[:k], m, t, c)
    R = seq.cam.pixelErrorX * np.eye(len(residual))
    # the Python-loop Cholesky is O(m^3) interpreted operations: above 64 rows the reference's vectorised path
    return fm.fixed_map_update_ref(x, fp, t, c, P, rows, residual, R, storage_of(e.precision), vectorised=len(residual) > 64)


def check_against_reference(e, before, ref, label):
    """the engine after the call against the reference and against the state before the call; prints every figure first"""
    assert ref["status"] == "applied"
    x, fp, P = e.get_state()
    x0, fp0, P0 = before
    n = len(P)
    strip = fm.strip_mask(n)
    be = {k: v for k, v in block_errs(x, fp, ref["x13"], ref["feature_pos"]).items() if k in CAMERA}
    Pr = ref["P"]
    if storage_of(e.precision) is np.float64:
        p_fig = {"strip_max": rel_max(P[strip], Pr[strip]), "strip_fro": rel_fro(P[strip], Pr[strip])}
        p_ok = p_fig["strip_max"] <= F64_TOL and p_fig["strip_fro"] <= F64_TOL
    else:
        scale = np.abs(Pr)
        norm = np.zeros(P.shape, dtype=bool)
        norm[3:7, :] = norm[:, 3:7] = True
        scale[norm] += ref["strip_bound"][norm]
        bound = 2.0 ** -23 * scale + F64_TOL * np.abs(Pr).max()
        ratio = (np.abs(P - Pr) / bound)[strip]
        p_fig = {"strip worst |err| / bound": float(ratio.max()), "strip entries off the reference": int((P != Pr)[strip].sum())}
        p_ok = bool(np.all(ratio <= 1.0))
    print(f"{label}:", {k: f"{v:.1e}" for k, v in be.items()}, p_fig)
    assert all(v <= F64_TOL for v in be.values()), be
    assert p_ok, p_fig
    assert np.any(x != x0) and np.any(P[:13] != P0[:13])  # it did move the camera
    np.testing.assert_array_equal(P[:13], P[:, :13].T)  # the strip is bitwise symmetric
    np.testing.assert_array_equal(fp, fp0)
    np.testing.assert_array_equal(P[~strip], P0[~strip])


# ------------------------------------------------------------------------------------ 1. the stage against the reference
@pytest.mark.parametrize("precision", [0, 2, 3])
@pytest.mark.parametrize("which", MAPS)
def test_stage_matches_reference(eng_mod, seqs, which, precision):
    e, seq = make(eng_mod, seqs, which, precision)
    e.predict()
    preds, Hs, Hf = e.predict_measurements()
    m = matches_for(preds)
    before = e.get_state()
    layout, feats = e.feature_layout(), e.get_map_features()
    ref = reference(e, seq, m, preds, Hs, Hf, before)
    count0 = e.fixed_map()[1]
    assert e.update_fixed_map(m) == 0
    check_against_reference(e, before, ref, f"{which} precision {precision} m = {2 * len(m)}")
    assert_same_bits(layout + feats, e.feature_layout() + e.get_map_features())
    assert e.fixed_map() == (False, count0 + 1)  # the stage runs whatever the mode, and counts
    e.close()


# --------------------------------------------------------------------------------------------------- 2. row-count edges
_edge_refs = {}


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("sweep_mode", [SWEEP_AUTO, SWEEP_LAUNCHES])
@pytest.mark.parametrize("precision", [0, 2])
def test_row_count_edges(eng_mod, seq170, precision, sweep_mode, path):
    """M = 1 .. 160 matches: below, at and above a 32-row panel, the 32-row chunks and the 16 row slices of the strip kernel, with
    the rows of B from the sweep (path 1: Y = B[:, 0:13], X = B) and from the explicit inverse (path 2: Y = K_c', X = G -- the route
    of updates above 2048 rows, reached here through ekf_set_update_path).  The reference of (precision, M) is shared: the state
    before the update does not depend on the sweep mode or the path."""
    seq = seq170
    e = fresh(eng_mod, seq, precision, sweep_mode)
    e.set_update_path(path)
    start = e.get_state()
    for M in (1, 16, 17, 64, 65, 128, 129, 160):
        e.set_state(start[0], start[1], seq.feature_type, seq.feature_desc, start[2])
        e.predict()
        preds, Hs, Hf = e.predict_measurements()
        m = matches_for(preds, M)
        before = e.get_state()
        if (precision, M) not in _edge_refs:
            _edge_refs[(precision, M)] = (reference(e, seq, m, preds, Hs, Hf, before), before)
        ref, before0 = _edge_refs[(precision, M)]
        assert_same_bits(before, before0)
        assert e.update_fixed_map(m) == 0
        check_against_reference(e, before, ref, f"precision {precision} sweep {sweep_mode} path {path} M = {M}")
    e.close()


# ------------------------------------------------------------------------------------------- 3. against the engine itself
@pytest.mark.parametrize("which", ["seq12", "seq50", "mixed"])
def test_strip_is_the_full_updates_strip(eng_mod, seqs, which):
    a, seq = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    b, _ = make(eng_mod, seqs, which, sweep_mode=SWEEP_LAUNCHES)
    assert_same_bits(a.get_state(), b.get_state())
    for e in (a, b):
        e.set_consistency(True)
        e.predict()
    preds, _, _ = a.predict_measurements()
    b.predict_measurements()
    m = matches_for(preds)
    a.update(m)
    b.update_fixed_map(m)
    (xa, _, Pa), (xb, _, Pb) = a.get_state(), b.get_state()
    strip = fm.strip_mask(len(Pa))
    be = {k: v for k, v in block_errs(xb, np.zeros((0, 6)), xa, np.zeros((0, 6))).items() if k in CAMERA}
    fig = {"strip_max": rel_max(Pb[strip], Pa[strip]), "strip_fro": rel_fro(Pb[strip], Pa[strip])}
    ra, rb = a.consistency(), b.consistency()
    assert len(ra) == len(rb) == 1
    nis = abs(rb[0]["nis"] - ra[0]["nis"]) / ra[0]["nis"]
    print(f"{which}: update_fixed_map against ekf_update:", {k: f"{v:.1e}" for k, v in be.items()}, fig, f"nis {nis:.1e}")
    assert all(v <= F64_TOL for v in be.values()), be
    assert fig["strip_max"] <= F64_TOL and fig["strip_fro"] <= F64_TOL
    assert (rb[0]["stage"], rb[0]["matches"], rb[0]["rows"]) == (0, len(m), 2 * len(m)) == (ra[0]["stage"], ra[0]["matches"], ra[0]["rows"])
    assert nis <= F64_TOL
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. above 2048 rows
def test_above_2048_rows(eng_mod):
    """The map tests/test_gpu_exact_edge_cases.py uses for this boundary, EKF_PRECISION_F64_EXACT, every predicted feature matched:
    more than 2048 rows, so inv(L) is formed and the strip is K_c G with no m x m x n product.  The reference is computed with
    VECTORISED numpy (numpy's Cholesky and matrix products, not the Python-loop Cholesky: 2800^3 / 6 interpreted operations), and
    the comparison covers the strip only -- what lies outside it is compared with the state before the call, bit for bit."""
    seq = SyntheticSequence(1400, 1, width=1280, height=720)
    e = eng_mod.EkfEngine(seq.cam, seq.par, 1400, max_keypoints=64, precision=3)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.timing(True)
    e.timing_reset()
    e.predict()
    preds, Hs, Hf = e.predict_measurements()
    m = matches_for(preds)
    assert 2 * len(m) > 2048, len(m)
    x0, fp0, P0 = e.get_state()
    t, c = e.feature_layout()
    rows, residual = xr.visual_rows(preds, Hs, Hf, m, t, c)
    ref = fm.fixed_map_update_ref(x0, fp0, t, c, P0, rows, residual, seq.cam.pixelErrorX * np.eye(len(residual)), np.float64,
                                  vectorised=True, strip_only=True)
    assert ref["status"] == "applied"
    assert e.update_fixed_map(m) == 0
    x, fp, P = e.get_state()
    be = {k: v for k, v in block_errs(x, fp, ref["x13"], fp0).items() if k in CAMERA}
    fig = {"strip_max": rel_max(P[:13], ref["P"]), "strip_fro": rel_fro(P[:13], ref["P"])}
    print(f"N = 1400, m = {2 * len(m)}:", {k: f"{v:.1e}" for k, v in be.items()}, fig)
    assert all(v <= F64_TOL for v in be.values()), be
    assert fig["strip_max"] <= F64_TOL and fig["strip_fro"] <= F64_TOL, fig
    assert np.any(x != x0) and np.any(P[:13] != P0[:13])
    np.testing.assert_array_equal(P[:13], P[:, :13].T)
    np.testing.assert_array_equal(fp, fp0)
    np.testing.assert_array_equal(P[13:, 13:], P0[13:, 13:])
    assert e.timing_get().p_update_launches == 0 and len(e.p_update_launches()[0]) == 0  # no downdate ran
    e.close()


# ------------------------------------------------------------------------------------------------ 5. steps in the mode
def staged_frame(e, kps, desc, fixed):
    """the stage sequence of EKF::step (EKF.cpp:273-531; tests/cpp/compat_check.cpp shows the order) with update_fixed_map in place
    of update when `fixed`"""
    upd = e.update_fixed_map if fixed else e.update
    e.predict()
    e.predict_measurements()
    m = e.match(kps, desc)
    mask, _ = e.ransac(m)
    if mask.any():
        upd(m[mask])
    out = m[~mask]
    if len(out):
        e.predict_measurements(out["featureIndex"])
        rescued = out[e.rescue(out)]
        if len(rescued):
            upd(rescued)


@pytest.mark.parametrize("precision", [0, 2])
def test_steps_in_the_mode(eng_mod, seq50, precision):
    seq = seq50
    e = fresh(eng_mod, seq, precision)
    full = fresh(eng_mod, seq, precision)
    staged = fresh(eng_mod, seq, precision)
    e.set_fixed_map(True)
    assert e.fixed_map() == (True, 0) and full.fixed_map() == (False, 0)
    e.timing(True)
    e.timing_reset()
    _, fp0, P0 = e.get_state()
    n_updates = 0
    for t, (kps, desc) in enumerate(seq.frames):
        info = e.step(kps, desc)
        assert info.status == 0 and info.n_inliers > 0
        n_updates += (info.n_inliers > 0) + (info.n_rescued > 0)
        x, fp, P = e.get_state()
        np.testing.assert_array_equal(fp, fp0)
        np.testing.assert_array_equal(P[13:, 13:], P0[13:, 13:])
        np.testing.assert_array_equal(P, P.T)
        assert e.fixed_map() == (True, n_updates)
        if t == 0:
            # the inputs of matching and RANSAC are those of a full-mode step
            fi = full.step(kps, desc)
            assert (info.n_predicted, info.n_matches, info.n_hypotheses, info.n_inliers) == (fi.n_predicted, fi.n_matches, fi.n_hypotheses, fi.n_inliers)
            staged_frame(staged, kps, desc, fixed=True)
            xs, fps, Ps = staged.get_state()
            be = {k: v for k, v in block_errs(x, fp, xs, fps).items() if k in CAMERA}
            fig = {"P_max": rel_max(P, Ps), "P_fro": rel_fro(P, Ps)}
            print(f"precision {precision}: frame 1 of the mode against its stage sequence:", {k: f"{v:.1e}" for k, v in be.items()}, fig)
            if precision == 0:
                assert all(v <= F64_TOL for v in be.values()) and fig["P_max"] <= F64_TOL and fig["P_fro"] <= F64_TOL, (be, fig)
            np.testing.assert_array_equal(fps, fp0)
    assert e.timing_get().p_update_launches == 0 and n_updates >= len(seq.frames)
    # the features' bookkeeping did run: predicted and matched counts moved as in the full-mode step
    _, tp, tm = e.get_map_features()
    assert tp.sum() > 0 and tm.sum() > 0
    for eng in (e, full, staged):
        eng.close()


# ----------------------------------------------------------------------------------------------------------- 6. toggle
@pytest.mark.parametrize("precision", [0, 2])
def test_toggle(eng_mod, seq50, precision):
    seq = seq50
    a = fresh(eng_mod, seq, precision, SWEEP_LAUNCHES)
    a.set_fixed_map(True)
    for kps, desc in seq.frames[:2]:
        a.step(kps, desc)
    a.set_fixed_map(False)
    assert a.fixed_map()[0] is False
    x, fp, P = a.get_state()
    desc_a, _, _ = a.get_map_features()
    b = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=4 * seq.n_features + 64, precision=precision)
    b.set_sweep_mode(SWEEP_LAUNCHES)
    b.set_state(x, fp, seq.feature_type, desc_a, P)  # never had the mode on
    assert_same_bits(a.get_state(), b.get_state())
    for kps, desc in seq.frames[2:]:
        ia, ib = a.step(kps, desc), b.step(kps, desc)
        assert (ia.n_matches, ia.n_inliers, ia.n_rescued, ia.status) == (ib.n_matches, ib.n_inliers, ib.n_rescued, ib.status)
        assert_same_bits(a.get_state(), b.get_state())
    _, fp2, P2 = a.get_state()
    assert np.any(fp2 != fp) and np.any(P2[13:, 13:] != P[13:, 13:])  # mapping did resume
    assert b.fixed_map() == (False, 0) and a.fixed_map()[0] is False
    a.close()
    b.close()


def test_on_and_straight_off_changes_nothing(eng_mod, seq50):
    seq = seq50
    a, b = fresh(eng_mod, seq, 2, SWEEP_LAUNCHES), fresh(eng_mod, seq, 2, SWEEP_LAUNCHES)
    a.set_fixed_map(True)
    a.set_fixed_map(False)
    for kps, desc in seq.frames[:3]:
        a.step(kps, desc)
        b.step(kps, desc)
        assert_same_bits(snapshot(a), snapshot(b))
    assert a.fixed_map() == (False, 0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------- 7. failure and refusals
@pytest.mark.parametrize("precision", [0, 2])
def test_indefinite_covariance_is_reported_and_skipped(eng_mod, seq12, precision):
    """S = H P H' + R not positive definite (P made indefinite on purpose, tests/test_gpu_edge_cases.py): reported as ekf_update
    reports it, and x, P, the map and the counter stay as they were"""
    e = fresh(eng_mod, seq12, precision, P=-1e3 * np.eye(seq12.state_dim))
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = np.zeros(4, dtype=MATCH_DTYPE)
    m["featureIndex"] = preds["featureIndex"][:4]
    m["imagePos"] = preds["imagePos"][:4] + 0.5
    before = snapshot(e)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.update_fixed_map(m)
    assert ei.value.code == NOT_POSITIVE_DEFINITE and "positive definite" in str(ei.value)
    assert_same_bits(before, snapshot(e))
    assert e.update_fixed_map(m, allow_errors=(NOT_POSITIVE_DEFINITE,)) == NOT_POSITIVE_DEFINITE
    assert_same_bits(before, snapshot(e))
    assert e.fixed_map() == (False, 0)
    e.close()


def test_refusals_change_nothing(eng_mod, seq12):
    seq = seq12
    # a repeated featureIndex
    e = fresh(eng_mod, seq)
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = matches_for(preds, 4)
    m["featureIndex"][3] = m["featureIndex"][0]
    before = snapshot(e)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.update_fixed_map(m)
    assert ei.value.code == INVALID_ARG
    assert_same_bits(before, snapshot(e))
    assert e.fixed_map() == (False, 0)
    e.close()
    # the fast fp32 configuration
    e = fresh(eng_mod, seq, precision=1)
    e.predict()
    preds, _, _ = e.predict_measurements()
    before = snapshot(e)
    for call in (lambda: e.update_fixed_map(matches_for(preds, 4)), lambda: e.set_fixed_map(True)):
        with pytest.raises(eng_mod.EkfError) as ei:
            call()
        assert ei.value.code == INVALID_ARG and "EKF_PRECISION_F32" in str(ei.value)
    e.set_fixed_map(False)  # off is always accepted
    assert_same_bits(before, snapshot(e))
    assert e.fixed_map() == (False, 0)
    e.close()
    # a sharded engine
    grp = LocalShardGroup(seq.cam, seq.par, seq.n_features, 2, max_keypoints=4 * seq.n_features + 64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, 0.5 * (seq.P0 + seq.P0.T))
    g = grp.engines[0]
    for call in (lambda: g.update_fixed_map(matches_for(preds, 4)), lambda: g.set_fixed_map(True)):
        with pytest.raises(eng_mod.EkfError) as ei:
            call()
        assert ei.value.code == INVALID_ARG and "sharded" in str(ei.value)
    assert g.fixed_map() == (False, 0)
    grp.close()


# ----------------------------------------------------------------------------------------------- 8. C++ and sample
def test_driver_class_and_sample_program(tmp_path):
    """ImageEKF::setFixedMap over the committed frames (tests/cpp/fixed_map_check.cpp: mode on from frame 4 -- from there on the
    number of features and their parameters do not change, map management is skipped, the log carries the line) and
    ekf_sequence --fixed-map-from 4; built the way tests/test_gpu_external_update.py builds its programs"""
    from tests.test_gpu_map_points import s3_config_320

    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    sample, check = str(tmp_path / "ekf_sequence"), str(tmp_path / "fixed_map_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check, os.path.join(ROOT, "tests", "cpp", "fixed_map_check.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    threshold = "1e10"  # new-feature threshold on these frames (test_gpu_ncc.test_real_frames_engine_equals_oracle)
    chk_out = tmp_path / "chk"
    chk_out.mkdir()
    r = subprocess.run([check, str(cfg), SEQ + "/", threshold, "4", str(chk_out) + "/"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fixed map through the driver class: ok" in r.stdout, r.stdout
    assert "log.txt, step 4: Fixed map: on" in r.stdout, r.stdout
    outdir = tmp_path / "out"
    outdir.mkdir()
    r = subprocess.run([sample, str(cfg), SEQ + "/", str(outdir) + "/", "0", "99999", threshold, "--fixed-map-from", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [k for k, ln in enumerate(lines) if ln.startswith("        fixed map: on")]
    steps = [ln for ln in lines if ln.startswith("step ")]
    assert len(steps) == 7 and len(at) == 4, r.stdout  # steps 4..7 of the seven (eight frames: the first initialises)
    feats = [int(ln.split("features")[1].split()[0]) for ln in steps]
    assert len(set(feats[3:])) == 1, feats  # the number of features does not change from step 4 on
    assert lines[at[0] - 1].startswith("step 4 ") or lines[at[0] - 1].startswith("step 4:"), lines[at[0] - 1]
    assert (outdir / "output.yml").exists()
