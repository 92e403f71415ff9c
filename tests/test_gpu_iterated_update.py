"""The iterated EKF update on the device (ekf_update_iterated / ekf_set_update_iterations) against
tests/iterated_update_ref.py (the oracle's measurement prediction + tests/update_ref.py, fp64 / longdouble on the host).

Cases (tests/test_iterated_update_cpu.py shows on the CPU that they are usable): ("mixed", 85, 17) both feature types and one
partial 128-column tile, ("mixed", 259, 17) a tile edge, ("mixed", 85, 16) m = 32: exactly one panel -- matches 3 px off their
predictions -- and ("seq170", 1033, 33) at 0.3 px: three panels, the persistent sweep.  Engines are primed as
test_gpu_update_entries.fresh_engine primes them; every reference starts from what the engine holds after its predictions.

The last pass is checked per entry by the route through a twin engine: x^(K-1) from linearisation_point() is uploaded into a
second engine with the prior P, whose own predict_measurements gives the predictions and Jacobians the covariance pass used (the
upload forms R(q) from the stored quaternion as the state-only tail does)."""
import numpy as np
import pytest

import iterated_update_ref as ir
import update_ref as ur
import update_ref_fast as uf
from parity_metric import F32_TOL, F64_TOL, over_tolerance, parity_report
from test_gpu_update_entries import check, fresh_engine, storage_of
from openekfmonoslam_amd.ekftypes import ITER_STOP_COUNT, ITER_STOP_FAILED, ITER_STOP_FEATURE_LEFT, ITER_STOP_TOL
from openekfmonoslam_amd.synth import SyntheticSequence

pytestmark = pytest.mark.gpu
PRECISIONS = (0, 2, 3)  # fp64, F32_EXACT, F64_EXACT
CASES = [("mixed", 85, 17, 3.0), ("mixed", 259, 17, 3.0), ("mixed", 85, 16, 3.0), ("seq170", 1033, 33, 0.3)]
IDS = [f"{c[0]}-n{c[1]}-M{c[2]}" for c in CASES]
SINGLE = 1  # EKF_SWEEP_SINGLE
_RUNS = {}


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


def gate_of(precision):
    return F64_TOL if precision == 0 else F32_TOL


def start(eng_mod, case, precision, mode=None):
    """a primed engine after predict + predict_measurements -> (engine, cam, matches, (x, fp, t, c, P) as the engine holds them)"""
    kind, n, M, amp = case
    e, cam = fresh_engine(eng_mod, kind, n, precision, mode=mode)
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = ir.scaled_matches(preds, M, amp)
    x, fp, P = e.get_state()
    t, c = e.feature_layout()
    return e, cam, m, (x, fp, t, c, P)


def iterated(eng_mod, oracle_lib, case, precision, K=3, tol=0.0):
    """one run of update_iterated and its reference, shared by the tests of a case (read-only use)"""
    key = (case, precision, K, tol)
    if key not in _RUNS:
        e, cam, m, (x, fp, t, c, P) = start(eng_mod, case, precision)
        _, par, _, _, _, desc, _ = ur.case_map(case[0], case[1])
        o = oracle_lib.Oracle(cam, par, len(fp) + 8)
        exact = "sweep" if precision in (2, 3) else False
        ref = ir.iterated_update_ref(o, x, fp, t, desc, c, P, m, cam.pixelErrorX, K, tol, storage_of(precision), exact, uf.update_core)
        assert e.update_iterated(m, K, tol) == 0
        _RUNS[key] = dict(e=e, cam=cam, par=par, desc=desc, m=m, prior=(x, fp, t, c, P), ref=ref, state=e.get_state(),
                          recs=e.iteration_records(), lin=e.linearisation_point())
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. one pass is the engine as it is
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_pass_is_update_bit_for_bit(eng_mod, case, precision):
    a, _, m, _ = start(eng_mod, case, precision, mode=SINGLE)
    b, _, mb, _ = start(eng_mod, case, precision, mode=SINGLE)
    np.testing.assert_array_equal(m, mb)
    assert a.update(m) == 0 and b.update_iterated(m, 1) == 0
    for u, v in zip(a.get_state(), b.get_state()):
        np.testing.assert_array_equal(u, v)
    rec = b.iteration_records()
    assert len(rec) == 1 and (rec[0]["stage"], rec[0]["passes_run"], rec[0]["stop_reason"]) == (0, 1, ITER_STOP_COUNT)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_default_step_is_unchanged_by_the_mode_at_one_pass(eng_mod, precision):
    """step with the mode set to one pass against an engine that never called the new interface: the same bits"""
    seq = SyntheticSequence(170, 3)
    states = []
    for touch in (False, True):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        if touch:
            e.set_update_iterations(1)
            assert e.update_iterations() == (1, 0.0)
        infos = [e.step(kps, desc) for kps, desc in seq.frames]
        assert all(i.status == 0 for i in infos)
        assert len(e.iteration_records()) == 0
        states.append((e.get_state(), [(i.n_matches, i.n_inliers, i.n_rescued) for i in infos]))
    assert states[0][1] == states[1][1]
    for u, v in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------------------------------------ 2. three passes against the reference
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_passes_against_the_reference(eng_mod, oracle_lib, case, precision):
    r = iterated(eng_mod, oracle_lib, case, precision)
    x, fp, P = r["state"]
    f = r["ref"]["final"]
    be = parity_report(x, fp, P, f["x13"].astype(np.float64), f["feature_pos"].astype(np.float64), f["P"].astype(np.float64))
    print(f"{case} precision {precision}: K = 3 against the reference", {k: f"{v:.2e}" for k, v in be.items()})
    assert r["ref"]["passes_run"] == 3 and r["ref"]["all_predicted"]
    assert not over_tolerance(be, gate_of(precision)), over_tolerance(be, gate_of(precision))


# ------------------------------------------------------------------------------------------------ 3. the last pass, per entry
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_last_pass_per_entry(eng_mod, oracle_lib, case, precision):
    r = iterated(eng_mod, oracle_lib, case, precision)
    x, fp, t, c, P = r["prior"]
    m = r["m"]
    xl, fl = r["lin"]
    twin = eng_mod.EkfEngine(r["cam"], r["par"], len(fp) + 8, max_keypoints=64, precision=precision)
    twin.set_state(xl, fl, t, r["desc"], P)
    preds, Hs, Hf = twin.predict_measurements(np.asarray(m["featureIndex"], dtype=np.int32))
    assert len(preds) == len(m)
    lin = oracle_lib.align_to_matches(preds, Hs, Hf, m)
    n = len(P)
    rows, nu = ir.corrected_residual(lin, m, t, c, ir.stacked(x, fp, t, c, n), ir.stacked(xl, fl, t, c, n))
    core = uf.update_core(x, fp, P, rows, nu, r["cam"].pixelErrorX * np.eye(len(nu)))
    exact = "sweep" if precision in (2, 3) else False
    ref = ur.with_bounds(core, t, c, storage_of(precision), exact)
    margin = ref["deadband_margin"]
    band, _, tol_fp = ir.deadband_band(core, ref, t, c, exact)
    print(f"{case} precision {precision}: dead-band margin of the covariance pass {margin:.3g}, {int(band.sum())} components in the band")
    if precision == 0 or case[0] == "seq170":
        assert margin > 1.0, f"a component of dx lies within its tolerance of the dead-band: {margin}"
    else:
        # FINDING (tests/test_iterated_update_cpu.py): with the exact configurations' digit terms the margin is below 1
        # on the mixed cases at 3 px (0.39 - 0.69).  The components inside the band -- parameters of features, never the camera, with
        # a correction below 1e-12 -- are held to |dx_j| + tol_j, since either decision of the dead-band is a correct result there
        # (iterated_update_ref.deadband_band); every other component and every entry of P keeps its bound.
        assert band.any() and float(np.abs(ref["dx"])[band].max()) < 4 * ur.EKF_DELTA
        ref = dict(ref, tol_feature_pos=tol_fp)
    check(r["e"], ref, (x, fp, t, c, P), f"last pass of K = 3, {case}", precision, "iterated")


# ------------------------------------------------------------------------------------------------ 4. records
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_records(eng_mod, oracle_lib, case, precision):
    r = iterated(eng_mod, oracle_lib, case, precision)
    rec = r["recs"]
    assert len(rec) == 1 and (rec[0]["stage"], rec[0]["passes_run"], rec[0]["stop_reason"]) == (0, 3, ITER_STOP_COUNT)
    got, want = rec[0]["step"], np.array(r["ref"]["steps"])
    print(f"{case} precision {precision}: steps {got[:3]} reference {want}")
    assert np.all(got[3:] == 0)
    if precision == 0:
        np.testing.assert_allclose(got[:3], want, rtol=1e-6, atol=0)


def test_tolerance_ends_the_iteration(eng_mod, oracle_lib):
    case = CASES[0]
    r = iterated(eng_mod, oracle_lib, case, 0, K=8, tol=1e-2)
    rec, ref = r["recs"][0], r["ref"]
    print("tol = 1e-2: passes", rec["passes_run"], "steps", rec["step"], "reference", ref["passes_run"], ref["steps"])
    assert ref["stop_reason"] == ir.STOP_TOL and 1 < ref["passes_run"] < 8
    assert (rec["passes_run"], rec["stop_reason"]) == (ref["passes_run"], ITER_STOP_TOL)
    np.testing.assert_allclose(rec["step"][:ref["passes_run"]], ref["steps"], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 5. a feature leaves the image
@pytest.mark.parametrize("precision", PRECISIONS)
def test_feature_left(eng_mod, oracle_lib, precision):
    cam, par, x, fp, t, desc, P0 = ur.case_map("mixed", 85)
    o = oracle_lib.Oracle(cam, par, len(fp) + 8)
    o.set_state(x, fp, t, desc, P0)
    o.predict()
    cam2 = ir.border_camera(cam, o.predict_measurements()[0])
    states = []
    for K in (1, 3):
        e = eng_mod.EkfEngine(cam2, par, len(fp) + 8, max_keypoints=64, precision=precision)
        e.set_state(x, fp, t, desc, P0)
        assert e.fuse_camera_position(x[:3], 1e6 * np.eye(3))["applied"]
        e.predict()
        preds, _, _ = e.predict_measurements()
        m = ir.border_matches(preds, 17)
        assert e.update_iterated(m, K) == 0
        rec = e.iteration_records()[0]
        assert (rec["passes_run"], rec["stop_reason"]) == (1, ITER_STOP_FEATURE_LEFT if K == 3 else ITER_STOP_COUNT)
        states.append(e.get_state())
    be = parity_report(*states[1], *states[0])
    print(f"feature left, precision {precision}: K = 3 against K = 1", {k: f"{v:.2e}" for k, v in be.items()})
    assert not over_tolerance(be, gate_of(precision))


# ------------------------------------------------------------------------------------------------ 6. the rest of the map is untouched
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bookkeeping_of_the_map_is_untouched(eng_mod, precision):
    case = CASES[3]
    feats = []
    for K in (1, 3):
        e, _, m, _ = start(eng_mod, case, precision)
        assert e.update_iterated(m, K) == 0
        feats.append(e.get_map_features())
    for u, v in zip(*feats):
        np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(eng_mod):
    e, _, m, _ = start(eng_mod, CASES[0], 0)
    before = e.get_state()

    def refused(fn, *a, text):
        with pytest.raises(eng_mod.EkfError) as ei:
            fn(*a)
        assert ei.value.code == 1 and text in str(ei.value), str(ei.value)  # EKF_ERR_INVALID_ARG
        for u, v in zip(before, e.get_state()):
            np.testing.assert_array_equal(u, v)

    for k in (0, 9, -1):
        refused(e.update_iterated, m, k, text="iterations must be 1 .. 8")
        refused(e.set_update_iterations, k, text="iterations must be 1 .. 8")
    for tol in (-1.0, float("nan"), float("inf")):
        refused(e.update_iterated, m, 2, tol, text="tol must be finite and not negative")
        refused(e.set_update_iterations, 2, tol, text="tol must be finite and not negative")
    e.set_update_iterations(2, 1e-3)
    assert e.update_iterations() == (2, 1e-3)
    refused(e.set_fixed_map, True, text="more than one pass")
    e.set_update_iterations(1)
    e.set_fixed_map(True)
    refused(e.set_update_iterations, 2, text="fixed-map mode is on")
    refused(e.update_iterated, m, 2, text="fixed-map mode is on")
    assert e.update_iterations() == (1, 0.0)


def test_sharded_engine_is_refused(eng_mod):
    seq = SyntheticSequence(24, 1)
    e = eng_mod.EkfEngine(seq.cam, seq.par, 32, max_keypoints=64, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ei:
        e.set_update_iterations(2)
    assert ei.value.code == 1 and "sharded" in str(ei.value)
    assert e.update_iterations() == (1, 0.0)


def test_failed_pass_leaves_the_filter_alone(eng_mod):
    """S of the first pass is not positive definite (a legal set_state with an indefinite P): the call reports what update()
    reports, x and P keep their bits, the record says `failed`"""
    cam, par, x, fp, t, desc, P0 = ur.case_map("mixed", 85)
    e = eng_mod.EkfEngine(cam, par, len(fp) + 8, max_keypoints=64)
    e.set_state(x, fp, t, desc, -1e3 * np.eye(len(P0)))
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = ir.scaled_matches(preds, 17, 3.0)
    before = e.get_state()
    rc = e.update_iterated(m, 3, allow_errors=(3,))  # EKF_ERR_NOT_POSITIVE_DEFINITE
    assert rc == 3
    for u, v in zip(before, e.get_state()):
        np.testing.assert_array_equal(u, v)
    rec = e.iteration_records()
    assert len(rec) == 1 and rec[0]["stop_reason"] == ITER_STOP_FAILED


def test_retry_repeats_the_same_pass(eng_mod, oracle_lib):
    """the persistent sweep of the second pass runs without its chain (stall_sweep): the retry carries that pass's table"""
    case = CASES[3]
    r = iterated(eng_mod, oracle_lib, case, 0)
    e, _, m, _ = start(eng_mod, case, 0)
    e.stall_sweep(1)
    assert e.update_iterated(m, 3) == 0
    assert e.sweep_retries == 1
    be = parity_report(*e.get_state(), *r["state"])
    assert not over_tolerance(be, F64_TOL), be


# ------------------------------------------------------------------------------------------------ 8. the step functions
def step_reference(ol, seq, K):
    """EKF::step composed from the oracle's stages, the iterated update in place of its two updates -> (decisions, x, fp, P)"""
    o = ol.Oracle(seq.cam, seq.par, seq.n_features + 8)
    o.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    scratch = ol.Oracle(seq.cam, seq.par, seq.n_features + 8)
    t, desc = np.array(seq.feature_type), np.array(seq.feature_desc)
    decisions, n_updates = [], []

    def update(matches, kdesc):
        if len(matches) == 0:
            return 0
        r = ir.iterated_update_ref(scratch, o.x13(), o.feature_pos(), t, desc, o.feature_covpos(), o.P(), matches,
                                   seq.cam.pixelErrorX, K, core_fn=uf.update_core)
        assert r["passes_run"] == K
        desc[matches["featureIndex"]] = kdesc[matches["keypointIndex"]]
        f = r["final"]
        o.set_state(f["x13"].astype(np.float64), f["feature_pos"].astype(np.float64), t, desc, f["P"].astype(np.float64))
        return 1

    for kps, kdesc in seq.frames:
        o.predict()
        preds, Hs, Hf = o.predict_measurements()
        m = o.match(preds, kps, kdesc)
        mp, mHs, mHf = ol.align_to_matches(preds, Hs, Hf, m)
        mask, _ = o.ransac(mp, mHs, mHf, m)
        ran = update(m[mask], kdesc)
        out = m[~mask]
        rescued = out[:0]
        if len(out):
            po, _, _ = o.predict_measurements(np.asarray(out["featureIndex"], dtype=np.int32))
            seen = np.isin(out["featureIndex"], po["featureIndex"])
            keep = np.zeros(len(out), dtype=bool)
            if seen.any():
                keep[seen] = o.rescue(out[seen], ol.align_to_matches(po, po, po, out[seen])[0])
            rescued = out[keep]
        ran += update(rescued, kdesc)
        decisions.append((len(m), int(mask.sum()), len(rescued)))
        n_updates.append(ran)
    return decisions, n_updates, o.x13(), o.feature_pos(), o.P()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_step_with_two_passes(eng_mod, oracle_lib, precision):
    seq = SyntheticSequence(170, 3)
    if "step" not in _RUNS:
        _RUNS["step"] = step_reference(oracle_lib, seq, 2)
    decisions, n_updates, xo, fo, Po = _RUNS["step"]
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.set_update_iterations(2)
    got = []
    for (kps, kdesc), ran in zip(seq.frames, n_updates):
        info = e.step(kps, kdesc)
        assert info.status == 0
        got.append((info.n_matches, info.n_inliers, info.n_rescued))
        rec = e.iteration_records()
        assert len(rec) == ran and all(r["passes_run"] == 2 and r["stop_reason"] == ITER_STOP_COUNT for r in rec)
        assert [int(r["stage"]) for r in rec] == [1, 2][:ran] or (ran == 1 and int(rec[0]["stage"]) in (1, 2))
    assert got == decisions, (got, decisions)
    be = parity_report(*e.get_state(), xo, fo, Po)
    print(f"step, two passes, precision {precision}:", {k: f"{v:.2e}" for k, v in be.items()})
    assert not over_tolerance(be, F32_TOL), over_tolerance(be, F32_TOL)


# ------------------------------------------------------------------------------------------------ consistency records
def test_consistency_records_the_covariance_pass(eng_mod, oracle_lib):
    """with ekf_set_consistency only the covariance pass records, and its innovations are nu_(K-1)"""
    case = CASES[0]
    r = iterated(eng_mod, oracle_lib, case, 0)
    e, _, m, _ = start(eng_mod, case, 0)
    e.set_consistency(True)
    assert e.update_iterated(m, 3) == 0
    rec = e.consistency()
    assert len(rec) == 1 and (rec[0]["stage"], rec[0]["matches"]) == (0, len(m))
    inn = e.innovations(0)
    nu = np.asarray(r["ref"]["nu"]).reshape(-1, 2)
    np.testing.assert_array_equal(inn["featureIndex"], m["featureIndex"])
    np.testing.assert_allclose(inn["nu"], nu, rtol=0, atol=1e-9 * np.abs(nu).max())
    z = r["ref"]["final"]["z"].astype(np.float64)
    np.testing.assert_allclose(rec[0]["nis"], z @ z, rtol=1e-9)
    for u, v in zip(e.get_state(), r["state"]):  # the mode changes no result
        np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------------------------------------ the point and the map it was taken on
def test_linearisation_point_does_not_outlive_the_map(eng_mod):
    """the point is sized by the map as it is: once a feature is removed, or the map replaced, it is refused, not copied"""
    e, _, m, (x, fp, t, c, P) = start(eng_mod, CASES[0], 0)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.linearisation_point()
    assert ei.value.code == 1
    assert e.update_iterated(m, 2) == 0
    xl, fl = e.linearisation_point()
    assert xl.shape == (13,) and fl.shape == (e.N, 6)
    e.remove_features([int(m["featureIndex"][0])])
    assert e.N == len(fp) - 1
    with pytest.raises(eng_mod.EkfError) as ei:
        e.linearisation_point()
    assert ei.value.code == 1 and "on this map" in str(ei.value)
    e2, _, m2, _ = start(eng_mod, CASES[0], 0)
    assert e2.update_iterated(m2, 2) == 0
    _, _, _, _, _, desc, _ = ur.case_map(CASES[0][0], CASES[0][1])
    e2.set_state(x, fp[:5], t[:5], desc[:5], P[:int(c[5]), :int(c[5])])
    with pytest.raises(eng_mod.EkfError):
        e2.linearisation_point()


def test_sharded_engine_refuses_the_stage_call(eng_mod):
    seq = SyntheticSequence(24, 1)
    e = eng_mod.EkfEngine(seq.cam, seq.par, 32, max_keypoints=64, shard=(0, 2))
    m = np.zeros(1, dtype=eng_mod.MATCH_DTYPE)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.update_iterated(m, 2)
    assert ei.value.code == 1 and "sharded" in str(ei.value)
    assert len(e.iteration_records()) == 0


@pytest.mark.parametrize("K", [2, 3])
def test_failed_pass_inside_a_step(eng_mod, K):
    """tests/test_gpu_convert_all.indefinite_between_two_features: every 2 x 2 innovation covariance is the one P0 gives, the joint S of
    an update that holds features 5 and 6 is not positive definite.  One match is a low-innovation inlier, the others are rescued:
    the step's first update runs its K passes, the first pass of its second fails -- the step reports what a step with plain updates
    reports, the second record says `failed` with no pass run, and x and P are finite and those the first update left (a twin that
    stops after the first update cannot be built from the stage calls, so that is checked through the record and P = P')"""
    from test_gpu_convert_all import indefinite_between_two_features

    seq = SyntheticSequence(12, 1, outlier_fraction=0.0, distractors_per_feature=0.0, max_bit_flips=0)
    P = indefinite_between_two_features(seq)
    codes = []
    for k in (1, K):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=len(seq.frames[0][0]) + 64)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P)
        e.set_update_iterations(k)
        with pytest.raises(eng_mod.EkfError) as ei:
            e.step(*seq.frames[0])
        codes.append(ei.value.code)
    assert codes == [3, 3]  # EKF_ERR_NOT_POSITIVE_DEFINITE
    rec = e.iteration_records()
    print("records of the failing step:", rec)
    assert len(rec) == 2 and [int(r["stage"]) for r in rec] == [1, 2]
    assert (rec[0]["passes_run"], rec[0]["stop_reason"]) == (K, ITER_STOP_COUNT)
    assert (rec[1]["passes_run"], rec[1]["stop_reason"]) == (0, ITER_STOP_FAILED)
    x, fp, Pn = e.get_state()
    assert np.isfinite(x).all() and np.isfinite(fp).all() and np.isfinite(Pn).all()
    assert abs(np.sqrt(x[3:7] @ x[3:7]) - 1.0) <= 4 * ur.U64  # the first update's covariance pass normalised q; nothing moved it since


def test_sample_program_with_iterations(tmp_path):
    """ekf_sequence --iterations 2 --iteration-tol 1e-3 over the committed frames: ImageEKF::setUpdateIterations and
    iterationRecords through the sample (built the way tests/test_gpu_fixed_map.py builds it)"""
    import os
    import subprocess

    from tests.test_gpu_map_points import s3_config_320

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg, seqdir = os.path.join(root, "openekfmonoslam_amd"), os.path.join(root, "tests", "golden", "s3_frames")
    sample = str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(root, "samples", "ekf_sequence.cpp"),
                           "-L", pkg, "-lekf_engine", "-lz", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"])
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    outdir = tmp_path / "out"
    outdir.mkdir()
    r = subprocess.run([sample, str(cfg), seqdir + "/", str(outdir) + "/", "0", "99999", "1e10", "--iterations", "2", "--iteration-tol", "1e-3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    steps = [ln for ln in lines if ln.startswith("step ")]
    recs = [ln for ln in lines if ln.startswith("        iterated update ")]
    assert len(steps) == 7 and len(recs) >= 7, r.stdout
    assert all(int(ln.split("passes")[1].split()[0]) in (1, 2) for ln in recs), recs
    r = subprocess.run([sample, str(cfg), seqdir + "/", str(outdir) + "/", "0", "99999", "1e10", "--iterations", "9"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "iterations must be 1 .. 8" in r.stdout + r.stderr
