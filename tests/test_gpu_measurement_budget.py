"""Measurement budget on the device (ekf_set_measurement_budget, k_budget_score / k_budget_rank) against
its numpy restatement (tests/measurement_budget_ref.py): the untouched paths with the budget off or not binding, the keys, gains,
ranks and selections of one prediction on maps at the kernels' edges, budgeted steps against the oracle's stages, the bookkeeping
of what describes the whole prediction, an image sequence through the NCC matcher, the refusals and the C++ seam.

Keys and gains: |device - reference| / reference, the reference computed from the covariance get_state() returns after predict()
(fp32 storage is not counted as error) and the Jacobians of ekf_predict_measurements.  TOL is ten times the worst figure measured
on an MI355X per precision over RANK_MAPS (written into DESIGN.md 4.12); the arithmetic is fp64 in every precision, so all of them
stay below 1e-9.

Measured on an MI355X (worst over the maps of each precision):
    precision 0: key 3.42e-13, gain 5.67e-14    (the map with five depth features, whose converted rows of P cancel in the sums;
                                                 the seven maps without them: key 5.70e-16, gain 1.58e-16)
    precision 1: key 5.57e-16, gain 1.58e-16    precision 2: key 5.10e-16, gain 1.58e-16    precision 3: key 3.67e-16, gain 1.55e-16
The S_i of the selector and the S_i of k_hp_rows' chunk 0 are equal bit for bit in every precision (asserted)."""
import os
import subprocess

import ctypes as C
import numpy as np
import pytest

import measurement_budget_ref as mb
from openekfmonoslam_amd.ekftypes import MEASUREMENT_RANK_DTYPE
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_map_points import s3_config_320
from tests.test_gpu_ncc import _with_templates
from tests.test_gpu_parity import F32_TOL, assert_state_close, block_errs, eng_mod, rel_fro, rel_max  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openekfmonoslam_amd")
FRAMES = os.path.join(ROOT, "tests", "golden", "s3_frames")

# ten times the worst relative error measured per precision (see above): precision -> (key, gain)
TOL = {0: (3.42e-12, 5.67e-13), 1: (5.57e-15, 1.58e-15), 2: (5.10e-15, 1.58e-15), 3: (3.67e-15, 1.55e-15)}

_SEQS = {}


def sequence(nfeat, frames=3):
    if (nfeat, frames) not in _SEQS:
        _SEQS[(nfeat, frames)] = SyntheticSequence(nfeat, frames)
    return _SEQS[(nfeat, frames)]


def engine(eng_mod, seq, precision=0, sweep=None):
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision)
    if sweep is not None:
        e.set_sweep_mode(sweep)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    return e


def info_tuple(i):
    return (i.n_predicted, i.n_matches, i.n_hypotheses, i.n_inliers, i.n_outliers, i.n_rescued, i.status)


# ------------------------------------------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("precision", [0, 2])
def test_off_is_off(eng_mod, precision):
    """three frames at N = 50 (launch-per-panel sweep: the run-to-run reproducible one): an engine never touched, one set to K and
    back to 0, and one with K >= N give the same filter, map tables and step records to the bit, and have nothing to report"""
    seq = sequence(50)
    runs = []
    for mode in ("never", "back", "n", "n+5"):
        e = engine(eng_mod, seq, precision, sweep=4)
        if mode == "back":
            e.set_measurement_budget(7)
            e.set_measurement_budget(0)
        elif mode != "never":
            e.set_measurement_budget(50 if mode == "n" else 55)
        infos = [info_tuple(e.step(*seq.frames[t])) for t in range(3)]
        assert len(e.measurement_ranks()) == 0
        assert e.measurement_budget_counts() == (infos[-1][0], infos[-1][0])
        runs.append((infos, e.get_state(), e.get_map_features()))
        e.close()
    for infos, state, feats in runs[1:]:
        assert infos == runs[0][0]
        for a, b in zip(state + feats, runs[0][1] + runs[0][2]):
            np.testing.assert_array_equal(a, b)
    assert runs[0][0][0][3] > 0


# ------------------------------------------------------------------------------------------ 2. ranks against the reference
_RANK_RUNS = {}


def rank_run(eng_mod, nfeat, precision, ndepth):
    """one map: the reference from the stage calls of one engine, then one budgeted step per usable K on a second engine
    (keep_step_predictions on: the selector's S_i of every predicted feature) -> dict, computed once per map and shared by the
    three tests below"""
    key = (nfeat, precision, ndepth)
    if key in _RANK_RUNS:
        return _RANK_RUNS[key]
    seq = sequence(nfeat, 1)
    if ndepth:
        seq = SyntheticSequence(nfeat, 1)
        seq.par.inverseDepthLinearityIndexThreshold = 1e9  # every call converts the first remaining inverse-depth feature

    def fresh():
        e = engine(eng_mod, seq, precision)
        for _ in range(ndepth):
            assert e.convert_inverse_depth_to_depth() >= 0
        return e

    a = fresh()
    x0, fp0, P0 = a.get_state()
    ftype, covpos = (v.copy() for v in a.feature_layout())
    assert (ftype == 1).sum() == ndepth
    a.predict()
    preds, Hs, Hf = a.predict_measurements()
    _, _, P = a.get_state()
    a.close()
    S_ref, key_ref, gain_ref = mb.scores(P, preds["featureIndex"], ftype, covpos, Hs, Hf, seq.cam.pixelErrorX)
    n_pred = len(preds)
    budgets = mb.usable_budgets(key_ref, preds["featureIndex"], mb.budget_candidates(n_pred))
    b = fresh()
    b.keep_step_predictions(True)
    steps = {}
    for K in budgets:
        if steps:
            b.set_state(x0, fp0, ftype, seq.feature_desc, P0)
        b.set_measurement_budget(K)
        info = b.step(*seq.frames[0])
        steps[K] = (info_tuple(info), b.measurement_ranks(), b.step_predictions(), b.measurement_budget_counts(),
                    b.get_map_features()[1].copy())
    b.close()
    out = {"preds": preds, "S_ref": S_ref, "key": key_ref, "gain": gain_ref, "budgets": budgets, "steps": steps, "seq": seq}
    _RANK_RUNS[key] = out
    return out


@pytest.mark.parametrize("nfeat,precision,ndepth", mb.RANK_MAPS)
def test_keys_and_gains_against_the_reference(eng_mod, nfeat, precision, ndepth):
    r = rank_run(eng_mod, nfeat, precision, ndepth)
    assert len(r["preds"]) == nfeat and len(r["budgets"]) >= 3
    worst = [0.0, 0.0]
    for K, (_, recs, sp, _, _) in r["steps"].items():
        assert recs.dtype == MEASUREMENT_RANK_DTYPE and len(recs) == nfeat
        np.testing.assert_array_equal(recs["featureIndex"], r["preds"]["featureIndex"])  # feature order
        assert (recs["_pad"] == 0).all() and (recs["key"] > 0).all()
        worst[0] = max(worst[0], float(np.max(np.abs(recs["key"] - r["key"]) / r["key"])))
        worst[1] = max(worst[1], float(np.max(np.abs(recs["gain"] - r["gain"]) / r["gain"])))
        # the key is the determinant of the S_i the selector wrote, R = pixelErrorX I
        S = sp["covarianceMatrix"].reshape(-1, 2, 2)
        pe = r["seq"].cam.pixelErrorX
        np.testing.assert_array_equal(recs["key"], (S[:, 0, 0] - 1.0 + pe) * (S[:, 1, 1] - 1.0 + pe) - S[:, 0, 1] * S[:, 1, 0])
    print(f"N {nfeat} precision {precision} depth {ndepth}: rel err key {worst[0]:.3e} gain {worst[1]:.3e}")
    assert worst[0] <= TOL[precision][0] and worst[1] <= TOL[precision][1], (worst, TOL[precision])
    assert max(worst) < 1e-9


@pytest.mark.parametrize("nfeat,precision,ndepth", mb.RANK_MAPS)
def test_selector_s_equals_the_hp_pass_s(eng_mod, nfeat, precision, ndepth):
    """the S_i the selector forms for every predicted feature (read through the kept step predictions, packed before the H P
    pass) and the S_i k_hp_rows forms from the same P and Jacobians (the stage call's predictions): bit equality, hence also
    for the selected features whose table entries the H P pass rewrites"""
    r = rank_run(eng_mod, nfeat, precision, ndepth)
    for K, (_, recs, sp, _, _) in r["steps"].items():
        assert len(sp) == nfeat
        np.testing.assert_array_equal(sp["featureIndex"], r["preds"]["featureIndex"])
        np.testing.assert_array_equal(sp["imagePos"], r["preds"]["imagePos"])
        np.testing.assert_array_equal(sp["covarianceMatrix"], r["preds"]["covarianceMatrix"])


@pytest.mark.parametrize("nfeat,precision,ndepth", mb.RANK_MAPS)
def test_ranks_and_selection_against_the_reference(eng_mod, nfeat, precision, ndepth):
    r = rank_run(eng_mod, nfeat, precision, ndepth)
    assert len(r["budgets"]) >= 3
    fidx = r["preds"]["featureIndex"]
    for K, (info, recs, _, counts, tp) in r["steps"].items():
        rank, sel = mb.rank_and_select(r["key"], fidx, K)
        np.testing.assert_array_equal(recs["rank"], rank)
        np.testing.assert_array_equal(recs["selected"], sel.astype(np.int32))
        assert info[0] == K == sel.sum() and counts == (nfeat, K) and info[1] <= K
        # timesPredicted moved for the selected only
        np.testing.assert_array_equal(np.flatnonzero(tp), fidx[sel])


def test_non_positive_keys_tie_and_rank_by_feature_index(eng_mod):
    """N = 600 (three tiles of the rank kernel), the own 6 x 6 block of every odd feature NaN: their keys are -1, they tie, and
    among them the lower feature index ranks first -- across tiles in front of, behind and inside a workgroup's own; the valid
    features rank ahead of all of them.  No keypoints: the step measures nothing, P is not updated."""
    from openekfmonoslam_amd.ekftypes import DESC_BYTES, KEYPOINT_DTYPE

    seq = sequence(600, 1)
    P0 = seq.P0.copy()
    for i in range(1, 600, 2):
        P0[13 + 6 * i:19 + 6 * i, 13 + 6 * i:19 + 6 * i] = np.nan
    e = eng_mod.EkfEngine(seq.cam, seq.par, 608, max_keypoints=64)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P0)
    K = 100
    e.set_measurement_budget(K)
    info = e.step(np.zeros(0, dtype=KEYPOINT_DTYPE), np.zeros((0, DESC_BYTES), dtype=np.uint8))
    assert info_tuple(info) == (K, 0, 0, 0, 0, 0, 0)
    recs = e.measurement_ranks()
    assert len(recs) == 600 and recs["featureIndex"].tolist() == list(range(600))
    odd = recs["featureIndex"] % 2 == 1
    assert (recs["key"][odd] == -1.0).all() and (recs["gain"][odd] == 0.0).all() and (recs["key"][~odd] > 0).all()
    rank, sel = mb.rank_and_select(recs["key"], recs["featureIndex"], K)
    np.testing.assert_array_equal(recs["rank"], rank)
    np.testing.assert_array_equal(recs["selected"], sel.astype(np.int32))
    assert recs["rank"][odd].tolist() == list(range(300, 600)) and recs["selected"][odd].sum() == 0
    e.close()


# ----------------------------------------------------------------------------------- 3. a budgeted step against the oracle
@pytest.mark.parametrize("nfeat,precision", [(50, 0), (50, 2), (200, 0), (200, 2)])
def test_budgeted_steps_against_the_oracle(eng_mod, oracle_lib, nfeat, precision):
    seq = sequence(nfeat)
    K = nfeat // 4
    e = engine(eng_mod, seq, precision)
    o = oracle_lib.Oracle(seq.cam, seq.par, nfeat + 8)
    o.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.set_measurement_budget(K)
    e.set_consistency(True)
    variant = oracle_lib.LITERAL if nfeat <= 50 else oracle_lib.ALGORITHMIC
    for t, (kps, desc) in enumerate(seq.frames):
        ie = e.step(kps, desc)
        io, predicted, selected, matches = mb.budgeted_oracle_step(o, kps, desc, K, variant)
        assert info_tuple(ie) == info_tuple(io), (t, info_tuple(ie), info_tuple(io))
        assert ie.n_predicted == K and ie.n_matches > 0
        recs = e.measurement_ranks()
        np.testing.assert_array_equal(recs["featureIndex"], predicted)
        np.testing.assert_array_equal(recs["featureIndex"][recs["selected"] == 1], selected)
        # the match lists: the updates' matches in their order (inliers, then rescued)
        mask = np.isin(matches["featureIndex"], e.innovations(0)["featureIndex"])
        np.testing.assert_array_equal(e.innovations(0)["featureIndex"], matches["featureIndex"][mask])
        assert mask.sum() == ie.n_inliers
        de, tpe, tme = e.get_map_features()
        do, tpo, tmo = o.map_features()
        np.testing.assert_array_equal(tpe, tpo)
        np.testing.assert_array_equal(tme, tmo)
        np.testing.assert_array_equal(de, do)
        if precision == 0:
            assert_state_close(e, o, 1e-8, f"budgeted step {t}")
        else:
            x, fp, P = e.get_state()
            assert rel_fro(P, o.P()) <= F32_TOL and rel_max(P, o.P()) <= F32_TOL, (t, rel_fro(P, o.P()), rel_max(P, o.P()))
            be = block_errs(x, fp, o.x13(), o.feature_pos())
            assert all(be[k] <= F32_TOL for k in ("r", "q", "v", "w", "features_blockwise", "features_componentwise")), (t, be)
    assert tmo.sum() > 0 and (tpo <= 3).all() and tpo.sum() == 3 * K


# ------------------------------------------------------------------------------------------------------- 4. bookkeeping
def test_what_describes_the_whole_prediction_is_unchanged(eng_mod, oracle_lib):
    """an image step at N = 50 with K = 12: the unseen list is the un-budgeted engine's, the kept step predictions cover every
    predicted feature, and the new-feature detector keeps out of the gates of the unselected features -- on a scene where it
    does return pixels inside those gates once the unselected features are removed from the map"""
    seq = SyntheticSequence(50, 2)
    fp = seq.feature_pos.copy()
    gone = [3, 17, 30]
    fp[gone, 3] += 1.2  # three features turned out of the field of view: the unseen list is not empty
    K = 12
    img = seq.render_image(1)

    def with_templates():
        e, _ = _with_templates(eng_mod, oracle_lib, seq)
        e.set_state(seq.x13, fp, seq.feature_type, seq.feature_desc, seq.P0)
        e.upload_image(seq.render_image(0))
        e.capture_templates(np.arange(50), seq.pixel_positions(0).astype(np.float64))
        return e

    engines = []
    for budget in (K, 0):
        e = with_templates()
        e.keep_step_predictions(True)
        e.set_measurement_budget(budget)
        engines.append(e)
    e, plain = engines
    ie, ip = e.step_image(img), plain.step_image(img)
    unseen = e.unseen_features()
    np.testing.assert_array_equal(unseen, plain.unseen_features())
    assert unseen.tolist() == gone
    sp, recs = e.step_predictions(), e.measurement_ranks()
    n_pred = 50 - len(unseen)
    assert len(sp) == len(recs) == n_pred == ip.n_predicted and ie.n_predicted == K
    assert e.measurement_budget_counts() == (n_pred, K) and plain.measurement_budget_counts() == (n_pred, n_pred)
    np.testing.assert_array_equal(sp["featureIndex"], recs["featureIndex"])
    np.testing.assert_array_equal(sp["featureIndex"], plain.step_predictions()["featureIndex"])
    np.testing.assert_array_equal(sp["imagePos"], plain.step_predictions()["imagePos"])
    np.testing.assert_array_equal(sp["covarianceMatrix"], plain.step_predictions()["covarianceMatrix"])
    unselected = sp[recs["selected"] == 0]
    assert len(unselected) == n_pred - K
    o = oracle_lib.Oracle(seq.cam, seq.par, 8)

    def inside_unselected(uv):
        hits = 0
        for p in unselected:
            ax, ang = o.ellipse(p["covarianceMatrix"])
            cx, cy = np.float32(p["imagePos"][0]), np.float32(p["imagePos"][1])
            hits += sum(o.point_in_ellipse(np.float32(u), np.float32(v), cx, cy, int(np.rint(ax[0])), int(np.rint(ax[1])), ang) for u, v in uv)
        return hits

    uv = e.detect_new_features(500)
    assert len(uv) > 0 and inside_unselected(uv) == 0
    # the same scene without the unselected features in the map: the detector does pick pixels there
    twin = with_templates()
    twin.remove_features(np.sort(unselected["featureIndex"]).astype(np.int32))
    twin.step_image(img)
    assert inside_unselected(twin.detect_new_features(500)) > 0


# ---------------------------------------------------------------------------------------------------- 5. NCC image steps
def test_real_frames_through_the_ncc_matcher(eng_mod):
    """tests/golden/s3_frames (320 x 240), 40 features initialised on frame 0, K = 10: seven image steps return EKF_OK, measure
    ten features each, match only selected ones, and the consistency records have at most 2 K rows"""
    from PIL import Image

    from openekfmonoslam_amd.ekftypes import s3_camera, s3_params

    frames = [np.asarray(Image.open(os.path.join(FRAMES, f"{k:05d}.png"))) for k in range(8)]
    K = 10
    e = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), 96)
    e.reset()
    e.upload_image(frames[0])
    uv = e.detect_new_features(40, min_response=1e10)
    assert len(uv) == 40
    e.add_features(uv)
    e.capture_templates(np.arange(40), uv)
    e.set_measurement_budget(K)
    e.set_consistency(True)
    matched = 0
    for t in range(1, 8):
        info = e.step_image(frames[t])
        assert info.status == 0 and info.n_predicted == K and info.n_matches <= K
        recs = e.measurement_ranks()
        assert len(recs) == e.measurement_budget_counts()[0] > K and recs["selected"].sum() == K
        selected = set(recs["featureIndex"][recs["selected"] == 1].tolist())
        cons = e.consistency()
        assert len(cons) == (info.n_inliers > 0) + (info.n_rescued > 0)
        for k, c in enumerate(cons):
            assert c["rows"] <= 2 * K
            assert set(e.innovations(k)["featureIndex"].tolist()) <= selected
        matched += info.n_inliers + info.n_rescued
    assert matched >= 7  # the selected features are tracked
    _, tp, tm = e.get_map_features()
    assert tp.sum() == 7 * K and tm.sum() == matched


def test_keypoint_image_matcher(eng_mod):
    """the other image matcher (detector + BRIEF-32 on the device): the keypoints come from the gates of every predicted feature,
    the matches from the selected ones"""
    seq = SyntheticSequence(50, 2)
    K = 12
    e = engine(eng_mod, seq)
    e.set_image_matcher(eng_mod.IMAGE_MATCHER_KEYPOINTS, 1e9)
    e.upload_image(seq.render_image(0))
    e.set_measurement_budget(K)
    info = e.step_image(seq.render_image(1))
    recs = e.measurement_ranks()
    assert info.status == 0 and info.n_predicted == K and info.n_matches <= K and len(recs) == 50 and recs["selected"].sum() == K
    _, tp, _ = e.get_map_features()
    np.testing.assert_array_equal(np.flatnonzero(tp), recs["featureIndex"][recs["selected"] == 1])


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_and_capacity(eng_mod, seq12):
    s = eng_mod.EkfEngine(seq12.cam, seq12.par, 12, shard=(0, 2))
    with pytest.raises(eng_mod.EkfError) as ex:
        s.set_measurement_budget(4)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    s.set_measurement_budget(0)  # off is not refused
    s.close()
    e = engine(eng_mod, seq12)
    n = C.c_int(-1)
    assert e.L.ekf_get_measurement_ranks(e.h, None, 0, C.byref(n)) == 0 and n.value == 0  # before any budgeted prediction
    e.set_measurement_budget(5)
    assert len(e.measurement_ranks()) == 0
    with pytest.raises(eng_mod.EkfError) as ex:
        e.set_measurement_budget(-1)
    assert ex.value.code == 1
    # ... and nothing changed: the step is budgeted with K = 5; the stage call before it ignores the budget
    e.predict()
    preds, _, _ = e.predict_measurements()
    assert len(preds) == 12 and len(e.measurement_ranks()) == 0
    e.set_state(seq12.x13, seq12.feature_pos, seq12.feature_type, seq12.feature_desc, seq12.P0)
    info = e.step(*seq12.frames[0])
    assert info.n_predicted == 5 and e.measurement_budget_counts() == (12, 5)
    assert e.L.ekf_get_measurement_ranks(e.h, None, 0, C.byref(n)) == 0 and n.value == 12  # count only
    buf = np.zeros(12, dtype=MEASUREMENT_RANK_DTYPE)
    n = C.c_int(-1)
    assert e.L.ekf_get_measurement_ranks(e.h, buf.ctypes.data_as(C.c_void_p), 11, C.byref(n)) == 2  # EKF_ERR_CAPACITY
    assert n.value == 12 and (buf["key"] == 0).all()
    assert e.L.ekf_get_measurement_ranks(e.h, buf.ctypes.data_as(C.c_void_p), 12, C.byref(n)) == 0 and n.value == 12
    assert sorted(buf["rank"].tolist()) == list(range(12)) and buf["selected"].sum() == 5
    # a step in which the budget does not bind, and the budget off: nothing to report
    e.set_measurement_budget(12)
    e.step(*seq12.frames[1])
    assert len(e.measurement_ranks()) == 0
    e.set_measurement_budget(5)
    e.step(*seq12.frames[2])
    assert len(e.measurement_ranks()) == 12
    e.set_measurement_budget(0)
    assert len(e.measurement_ranks()) == 0


# --------------------------------------------------------------------------------------------------------------- 7. C++
def test_driver_class_and_sample(tmp_path):
    """ImageEKF::setMeasurementBudget / measurementRanks over the committed frames (tests/cpp/measurement_budget_check.cpp), and
    ekf_sequence --budget 10: log.txt carries the predicted and the selected count of every frame"""
    link = ["-L", PKG, "-lekf_engine", "-lz", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    check_bin, sample = str(tmp_path / "measurement_budget_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check_bin, os.path.join(ROOT, "tests", "cpp", "measurement_budget_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check_bin, str(cfg), FRAMES + "/", "1e10", "10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 7 and all(int(s[7]) == 10 and int(s[5]) > 10 and int(s[11]) == int(s[5]) for s in steps), steps
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sample, str(cfg), FRAMES + "/", str(out) + "/", "--budget", "10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    printed = [ln.split() for ln in r.stdout.splitlines() if ln.strip().startswith("measurement budget:")]
    logged = [ln.split() for ln in (out / "log.txt").read_text().splitlines() if ln.startswith("Measurement budget:")]
    assert len(printed) == len(logged) == 7
    assert [(p[3], p[5]) for p in printed] == [(g[3], g[5]) for g in logged]
    assert all(int(g[5]) == 10 and int(g[3]) > 10 for g in logged), logged
    step_lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(step_lines) == 7 and all(int(s[3]) == 10 for s in step_lines)
    assert (out / "output.yml").exists() and (out / "map.ply").exists()
