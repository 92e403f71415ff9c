"""Filter consistency on the device (ekf_set_consistency, k_consistency) against its numpy
restatement (tests/consistency_ref.py): the NIS, the innovations (bit for bit), the conditional shares and the marginal
distances of staged updates in every precision, on both ways of forming B and in every sweep mode; the records of full
steps and their running totals; the untouched mode-off path; a failed update; the refusals, the capacity errors, an image
step through the NCC matcher and the C++ seam.

The reference works from the covariance get_state() returned before the update, so fp32 storage is not counted as error.

Tolerances: |device - reference| / reference, the worst value per quantity and precision over CASES as measured on an
MI355X (written into DESIGN.md 4.11), times ten; see TOL."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as cr
from openekfmonoslam_amd.ekftypes import CONSISTENCY_DTYPE, INNOVATION_DTYPE
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_map_points import s3_config_320
from tests.test_gpu_ncc import _with_templates
from tests.test_gpu_parity import eng_mod  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
FRAMES = os.path.join(ROOT, "tests", "golden", "s3_frames")

PATH_SWEEP, PATH_GEMM = 1, 2
SWEEP_PAIRS, SWEEP_SINGLE, SWEEP_PERSISTENT = 0, 1, 3

# ten times the worst |device - reference| / reference measured over CASES per precision:
# precision -> (nis, nis_conditional, d2_marginal)
TOL = {
    0: (7.0e-15, 3.9e-12, 5.5e-15),
    1: (3.2e-7, 1.1e-4, 6.6e-15),
    2: (1.4e-14, 3.5e-12, 6.6e-15),
    3: (7.0e-15, 3.9e-12, 5.5e-15),
}

_SEQS = {}


def sequence(nfeat):
    if nfeat not in _SEQS:
        _SEQS[nfeat] = SyntheticSequence(nfeat, 3)
    return _SEQS[nfeat]


def _cases():
    out = []
    for prec in (0, 1, 2, 3):
        for nfeat in (12, 50, 200):  # N = 200: the whole list, the largest M the frame gives (below 256 rows of matches)
            out.append(pytest.param(nfeat, prec, 0, 2, None, id=f"n{nfeat}-p{prec}"))
        # an odd M: 2 M = 74 rows is no multiple of 64 (nor of the 32-row panel); and the smallest update, one match
        out.append(pytest.param(50, prec, 0, 2, 37, id=f"n50-p{prec}-odd"))
        out.append(pytest.param(12, prec, 0, 2, 1, id=f"n12-p{prec}-one"))
        for path, name in ((PATH_SWEEP, "sweep"), (PATH_GEMM, "gemm")):
            out.append(pytest.param(50, prec, path, 2, None, id=f"n50-p{prec}-{name}"))
        for mode, name in ((SWEEP_SINGLE, "single"), (SWEEP_PAIRS, "pairs"), (SWEEP_PERSISTENT, "persistent")):
            out.append(pytest.param(50, prec, 0, mode, None, id=f"n50-p{prec}-{name}"))
    return out


CASES = _cases()


def staged_update(eng_mod, nfeat, precision, path, sweep, cut):
    """predict -> predict_measurements -> match -> update with the mode on -> (record, innovations, reference, M)"""
    seq = sequence(nfeat)
    e = eng_mod.EkfEngine(seq.cam, seq.par, nfeat + 8, max_keypoints=4 * nfeat + 64, precision=precision)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.set_update_path(path)
    e.set_sweep_mode(sweep)
    e.set_consistency(True)
    e.predict()
    preds, Hs, Hf = e.predict_measurements()
    m = e.match(*seq.frames[0])
    if cut is not None:
        M = min(cut, len(m))
        M -= 1 - M % 2  # odd
        assert M >= 1
        m = m[:M]
    _, _, P = e.get_state()
    ftype, covpos = e.feature_layout()
    ref = cr.reference(P, ftype, covpos, preds, Hs, Hf, m, seq.cam.pixelErrorX)
    e.update(m)
    recs = e.consistency()
    assert len(recs) == 1
    inn = e.innovations(0)
    totals = e.consistency_totals()
    e.close()
    return recs[0], inn, ref, m, totals


def relative_errors(rec, inn, ref):
    """(nis, worst nis_conditional, worst d2_marginal): |device - reference| / reference"""
    return (abs(rec["nis"] - ref["nis"]) / ref["nis"], float(np.max(np.abs(inn["nis_conditional"] - ref["c"]) / ref["c"])),
            float(np.max(np.abs(inn["d2_marginal"] - ref["d2"]) / ref["d2"])))


@pytest.mark.parametrize("nfeat,precision,path,sweep,cut", CASES)
def test_staged_update_against_the_reference(eng_mod, nfeat, precision, path, sweep, cut):
    rec, inn, ref, m, totals = staged_update(eng_mod, nfeat, precision, path, sweep, cut)
    M = len(m)
    assert M == cut or (cut is None and M >= 6)
    assert (rec["stage"], rec["matches"], rec["rows"]) == (0, M, 2 * M) and len(inn) == M
    np.testing.assert_array_equal(inn["featureIndex"], m["featureIndex"])
    assert (inn["stage"] == 0).all() and (inn["_reserved"] == 0).all()
    np.testing.assert_array_equal(inn["nu"], ref["nu"])  # exact: one subtraction and the dead band
    errs = relative_errors(rec, inn, ref)
    print(f"N {nfeat} precision {precision} path {path} sweep {sweep} M {M}: nis {rec['nis']:.6f} rel err nis {errs[0]:.3e} "
          f"conditional {errs[1]:.3e} marginal {errs[2]:.3e}")
    for name, err, tol in zip(("nis", "nis_conditional", "d2_marginal"), errs, TOL[precision]):
        assert err <= tol, (name, err, tol)
    assert rec["nis"] > 0 and abs(inn["nis_conditional"].sum() - rec["nis"]) <= 1e-12 * rec["nis"]
    if M == 1:
        assert inn["nis_conditional"][0] == rec["nis"]
    assert totals == (rec["nis"], 2 * M, 1)


def _stepped(eng_mod, on, sweep=None):
    seq = sequence(50)
    e = eng_mod.EkfEngine(seq.cam, seq.par, 58, max_keypoints=264)
    if sweep is not None:
        e.set_sweep_mode(sweep)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    if on:
        e.set_consistency(True)
    return e, seq


def test_full_steps_leave_their_records_and_totals(eng_mod):
    """Three frames at N = 50.  The first update of a step runs on the inliers; its second update runs on the list the rescue
    partition leaves in d.msel, the rescued matches (step.cpp: high_innovation_update behind launch_rescue_partition, d.mout ->
    d.msel), so stage 2 has n_rescued matches."""
    e, seq = _stepped(eng_mod, True)
    nis_sum, rows_sum, updates, stage2 = 0.0, 0, 0, 0
    for t in range(3):
        info = e.step(*seq.frames[t])
        recs = e.consistency()
        assert 1 <= len(recs) <= 2 and recs[0]["stage"] == 1 and recs[0]["matches"] == info.n_inliers > 0
        assert len(recs) == 1 + (info.n_rescued > 0)
        if len(recs) == 2:
            assert recs[1]["stage"] == 2 and recs[1]["matches"] == info.n_rescued
            stage2 += 1
        for k, r in enumerate(recs):
            inn = e.innovations(k)
            assert r["rows"] == 2 * r["matches"] == 2 * len(inn) and (inn["stage"] == r["stage"]).all()
            assert len(set(inn["featureIndex"].tolist())) == len(inn)
            assert r["nis"] > 0 and abs(inn["nis_conditional"].sum() - r["nis"]) <= 1e-12 * r["nis"]
            assert (inn["d2_marginal"] >= 0).all() and (inn["d2_marginal"] < 1e300).all()
            nis_sum += float(r["nis"])  # the order the device added them in
            rows_sum += int(r["rows"])
            updates += 1
        assert e.consistency_totals() == (nis_sum, rows_sum, updates)  # bit for bit
    assert stage2 > 0
    e.reset_consistency_totals()
    assert e.consistency_totals() == (0.0, 0, 0)
    assert len(e.consistency()) >= 1  # the records of the last step are not totals
    with pytest.raises(eng_mod.EkfError) as ex:
        e.innovations(2)
    assert ex.value.code == 1


def test_off_is_off(eng_mod):
    """the same three frames with the mode on and off (launch-per-panel sweep: the run-to-run reproducible one): the filter is
    the same to the bit, and the engine with the mode off has nothing to report"""
    states = []
    for on in (False, True):
        e, seq = _stepped(eng_mod, on, sweep=4)
        infos = [e.step(*seq.frames[t]) for t in range(3)]
        states.append((e.get_state(), [(i.n_matches, i.n_hypotheses, i.n_inliers, i.n_rescued) for i in infos]))
        assert len(e.consistency()) == (0 if not on else 1 + (infos[-1].n_rescued > 0))
        if not on:
            assert e.consistency_totals() == (0.0, 0, 0)
            with pytest.raises(eng_mod.EkfError):
                e.innovations(0)
    assert states[0][1] == states[1][1]
    for a, b in zip(states[0][0], states[1][0]):
        np.testing.assert_array_equal(a, b)


def test_failed_update_leaves_no_record(eng_mod, seq12):
    """S not positive definite (tests/test_gpu_edge_cases.py, the indefinite covariance): the update is reported and skipped,
    and so is its record -- the kernel honours the error flag"""
    from openekfmonoslam_amd.ekftypes import MATCH_DTYPE

    e = eng_mod.EkfEngine(seq12.cam, seq12.par, 16, max_keypoints=128)
    e.set_consistency(True)
    e.set_state(seq12.x13, seq12.feature_pos, seq12.feature_type, seq12.feature_desc, seq12.P0)
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = np.zeros(4, dtype=MATCH_DTYPE)
    m["featureIndex"] = preds["featureIndex"][:4]
    m["imagePos"] = preds["imagePos"][:4] + 0.5
    e.update(m)  # a good update first: the totals are not trivially zero
    before = e.consistency_totals()
    assert len(e.consistency()) == 1 and before[1:] == (8, 1) and before[0] > 0
    e.set_state(seq12.x13, seq12.feature_pos, seq12.feature_type, seq12.feature_desc, -1e3 * np.eye(seq12.state_dim))
    e.predict()
    preds, _, _ = e.predict_measurements()
    m["featureIndex"] = preds["featureIndex"][:4]
    m["imagePos"] = preds["imagePos"][:4] + 0.5
    with pytest.raises(eng_mod.EkfError) as ex:
        e.update(m)
    assert ex.value.code == 3  # EKF_ERR_NOT_POSITIVE_DEFINITE
    assert len(e.consistency()) == 0
    assert e.consistency_totals() == before


def test_refusals_and_capacity(eng_mod, seq12):
    s = eng_mod.EkfEngine(seq12.cam, seq12.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_consistency(True)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.close()
    e, seq = _stepped(eng_mod, True)
    e.step(*seq.frames[0])
    info = e.step(*seq.frames[1])
    need = (info.n_inliers > 0) + (info.n_rescued > 0)  # an update without matches leaves no record
    assert need >= 1
    n = C.c_int(-1)
    assert e.L.ekf_get_consistency(e.h, None, 0, C.byref(n)) == 0 and n.value == need  # count only
    buf = np.zeros(2, dtype=CONSISTENCY_DTYPE)
    n = C.c_int(-1)
    assert e.L.ekf_get_consistency(e.h, buf.ctypes.data_as(C.c_void_p), need - 1, C.byref(n)) == 2  # EKF_ERR_CAPACITY
    assert n.value == need
    recs = e.consistency()
    k = int(np.argmax(recs["matches"]))  # the larger of the step's updates
    Mk = int(recs[k]["matches"])
    assert Mk == max(info.n_inliers, info.n_rescued) and Mk > 1
    inn = np.zeros(Mk, dtype=INNOVATION_DTYPE)
    n = C.c_int(-1)
    assert e.L.ekf_get_innovations(e.h, k, None, 0, C.byref(n)) == 0 and n.value == Mk
    n = C.c_int(-1)
    assert e.L.ekf_get_innovations(e.h, k, inn.ctypes.data_as(C.c_void_p), Mk - 1, C.byref(n)) == 2
    assert n.value == Mk and (inn["featureIndex"] == 0).all() and (inn["nis_conditional"] == 0).all()
    assert e.L.ekf_get_innovations(e.h, k, inn.ctypes.data_as(C.c_void_p), Mk, C.byref(n)) == 0
    assert (inn["nis_conditional"] > 0).any()
    # off: nothing to report, and on again does not bring the old records back
    e.set_consistency(False)
    assert len(e.consistency()) == 0
    e.set_consistency(True)
    assert len(e.consistency()) == 0
    # update_only_state is not covered
    e.predict()
    e.predict_measurements()
    m = e.match(*seq.frames[2])
    e.update_only_state(m)
    assert len(e.consistency()) == 0


def test_image_step_through_the_ncc_matcher(eng_mod, oracle_lib):
    """the mode composes with the image front end: one ekf_step_image on the fixture of tests/test_gpu_ncc.py; its records list
    the matches in the updates' order -- the order the staged calls (predict, NCC match, RANSAC, update, re-prediction of the
    outliers, rescue) give on a twin engine"""
    seq = SyntheticSequence(50, 2)
    e, _ = _with_templates(eng_mod, oracle_lib, seq)
    twin, _ = _with_templates(eng_mod, oracle_lib, seq)
    e.set_consistency(True)
    img = seq.render_image(1)
    info = e.step_image(img)
    recs = e.consistency()
    assert info.n_inliers >= 1 and info.n_inliers + info.n_rescued > 25 and len(recs) == 1 + (info.n_rescued > 0)
    assert (recs[0]["stage"], recs[0]["matches"]) == (1, info.n_inliers)
    twin.predict()
    preds, _, _ = twin.predict_measurements()
    twin.upload_image(img)
    m = twin.match_ncc()
    mask, _ = twin.ransac(m)
    assert len(m) == info.n_matches and mask.sum() == info.n_inliers
    inn = e.innovations(0)
    np.testing.assert_array_equal(inn["featureIndex"], m["featureIndex"][mask])
    lut = {int(p["featureIndex"]): p["imagePos"] for p in preds}
    nu = np.array([cr.innovation(mt["imagePos"], lut[int(mt["featureIndex"])]) for mt in m[mask]])
    np.testing.assert_array_equal(inn["nu"], nu)
    assert recs[0]["nis"] > 0 and abs(inn["nis_conditional"].sum() - recs[0]["nis"]) <= 1e-12 * recs[0]["nis"]
    if len(recs) == 2:
        assert (recs[1]["stage"], recs[1]["matches"]) == (2, info.n_rescued)
        out = m[~mask]
        twin.update(m[mask])
        twin.predict_measurements(out["featureIndex"])
        rescued = out[twin.rescue(out)]
        inn2 = e.innovations(1)
        np.testing.assert_array_equal(inn2["featureIndex"], rescued["featureIndex"])
        assert recs[1]["nis"] > 0 and abs(inn2["nis_conditional"].sum() - recs[1]["nis"]) <= 1e-12 * recs[1]["nis"]


def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setConsistency / consistency() over the committed frames (tests/cpp/consistency_check.cpp: at least one record
    per frame that has inliers), and ekf_sequence --consistency: one line of consistency.csv per record"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check_bin, sample = str(tmp_path / "consistency_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check_bin, os.path.join(ROOT, "tests", "cpp", "consistency_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check_bin, str(cfg), FRAMES + "/", "1e10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 7
    for s in steps:
        assert int(s[9]) >= 1 if int(s[5]) > 0 else int(s[9]) <= 1, s
    assert sum(int(s[5]) > 0 for s in steps) >= 6
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sample, str(cfg), FRAMES + "/", str(out) + "/", "--consistency"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    printed = [ln.split() for ln in r.stdout.splitlines() if ln.strip().startswith("update stage")]
    rows = [ln.split(",") for ln in (out / "consistency.csv").read_text().splitlines()]
    assert len(rows) == len(printed) >= 6 and all(len(row) == 5 for row in rows)
    assert [int(row[1]) for row in rows] == [int(p[2].rstrip(":")) for p in printed]
    # (NIS = 0 is a legitimate record: a match that lands on the pixel its feature was initialised at is inside the dead band)
    assert all(int(row[3]) == 2 * int(row[2]) > 0 and float(row[4]) >= 0 for row in rows) and any(float(row[4]) > 0 for row in rows), rows
    assert set(int(row[0]) for row in rows) <= set(range(1, 8))
    total = [ln for ln in r.stdout.splitlines() if ln.startswith("consistency:")]
    assert len(total) == 1 and f"{len(rows)} updates" in total[0]
    nis = sum(float(row[4]) for row in rows)
    assert abs(float(total[0].split("=")[-1]) - nis / sum(int(row[3]) for row in rows)) < 1e-5
    assert (out / "output.yml").exists()
