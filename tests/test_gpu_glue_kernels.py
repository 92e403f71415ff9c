"""GPU: the frame's glue kernels at the sizes where their launches change shape -- the 1-point RANSAC's support pass
(k_ransac_hyp over the per-match records k_match_index / k_match_compact write; k_ransac_select) and the pixel predictions with
their Jacobians (k_predict_features, k_predict_cov_features) -- through the stage calls and through EKF::step.

RANSAC.  The scenes are tests/predict_ref.py's (a general pose, both feature types, every feature in view, P0 symmetric positive
definite with distinct entries), the match lists the predicted pixels displaced by 0 .. 2 thresholds in a seeded direction.  The
reference restates ONE hypothesis in numpy from the tables the device itself holds (state after the prediction, predicted pixel
and S of the hypothesis' feature, its two H P rows read back with ekf_debug_get_hp_rows -- so the reference is the same in every
storage precision) and re-projects every matched feature with predict_ref.visibility_ref (np.longdouble); the hypothesis loop is
tests/ransac_ref.py's sequential_loop.  A decision closer than MARGIN pixels to its threshold would be decided by rounding: the
tests assert that the evaluated hypotheses hold none (the reference's own error is ~1e-9 px: fp64 products of gains ~1e-2 and
weights ~1, a projection of slope ~1e2 px per unit).  Per-hypothesis support masks are read with ransacAllInliersProbability = 1e-9
on the list rotated by h, as tests/test_gpu_gating_stages.py does.

Prediction tables: against the CPU oracle with the bounds tests/test_gpu_parity.py holds the same tables to (imagePos rtol 1e-12 /
atol 1e-9, Hs and Hf 1e-11 of the largest entry); EKF::step's fused launch against the stage calls bit for bit, on maps with both
feature types."""
import math

import numpy as np
import pytest

import predict_ref as pr
import ransac_ref as rr
from openekfmonoslam_amd.ekftypes import DESC_BYTES, KEYPOINT_DTYPE, MATCH_DTYPE
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import rel_max, state_err
from test_ransac_ref_cpu import TINY_PROBABILITY, with_probability

pytestmark = pytest.mark.gpu

F64, F32_EXACT = 0, 2
MARGIN = 1e-6  # pixels
RANSAC_SIZES = [1, 63, 64, 65, 256, 257, 513, 1025]
INFO_FIELDS = ("n_predicted", "n_matches", "n_hypotheses", "n_inliers", "n_outliers", "n_rescued", "status")


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def mixed_types(N):
    """every third feature inverse depth, the others XYZ"""
    return np.where(np.arange(N) % 3 == 0, pr.FEATURE_INVERSE_DEPTH, pr.FEATURE_DEPTH).astype(np.int32)


_SCENES = {}


def all_visible_scene(N):
    if N not in _SCENES:
        _SCENES[N] = pr.make_scene(mixed_types(N), vis=np.ones(N, dtype=bool))
    return _SCENES[N]


class Tables:
    """an engine on a scene, predicted, and what the device holds for the reference of a hypothesis"""

    def __init__(self, eng_mod, s, precision, prob=None, feature_pos=None):
        self.s = s
        self.par = s.par if prob is None else with_probability(s.par, prob)
        self.e = eng_mod.EkfEngine(s.cam, self.par, s.n_features + 8, max_keypoints=64, precision=precision)
        self.e.set_state(s.x13, s.feature_pos if feature_pos is None else feature_pos, s.feature_type, s.desc, s.P0)
        self.e.predict()
        self.preds, _, _ = self.e.predict_measurements()
        self.x13, self.fpos, _ = self.e.get_state(want_P=False)
        self.types, self.covpos = self.e.feature_layout()
        self.row_of = {int(f): k for k, f in enumerate(self.preds["featureIndex"])}
        self._hp = {}

    def hp(self, f):
        if f not in self._hp:
            self._hp[f] = self.e.hp_rows([f])[0][0].copy()
        return self._hp[f]

    def matches(self, seed, keep=None):
        """the predicted features (or those of them in `keep`), displaced by 0 .. 2 thresholds"""
        p = self.preds if keep is None else self.preds[keep]
        rng = np.random.default_rng(seed)
        m = np.zeros(len(p), dtype=MATCH_DTYPE)
        m["featureIndex"] = p["featureIndex"]
        m["keypointIndex"] = -1
        r = rng.uniform(0.0, 2.0 * self.par.ransacThresholdPredictDistance, len(p))
        a = rng.uniform(0.0, 2.0 * np.pi, len(p))
        m["imagePos"] = p["imagePos"] + np.stack([r * np.cos(a), r * np.sin(a)], -1)
        return m

    def distances(self, m, h):
        """(D [M], margin [M]) of hypothesis h of the list m: pixel distance of every match to its feature's re-projection (NaN:
        not predicted) and how far the decision is from flipping"""
        cam, thr = self.s.cam, self.par.ransacThresholdPredictDistance
        fi = int(m["featureIndex"][h])
        k = self.row_of[fi]
        g = self.hp(fi)
        S = self.preds["covarianceMatrix"][k].reshape(2, 2) - np.eye(2) + cam.pixelErrorX * np.eye(2)
        nu = m["imagePos"][h] - self.preds["imagePos"][k]
        nu = np.where(np.abs(nu) > rr.EKF_DELTA, nu, 0.0)
        det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
        w = np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]]) / det @ nu
        dx = g[0] * w[0] + g[1] * w[1]
        dx = np.where(np.abs(dx) > rr.EKF_DELTA, dx, 0.0)
        x = self.x13 + dx[:13]
        fp = self.fpos.copy()
        for a in range(6):
            sel = a < np.where(self.types == pr.FEATURE_INVERSE_DEPTH, 6, 3)
            fp[sel, a] += dx[self.covpos[sel] + a]
        ok, vmargin, uv = pr.visibility_ref(cam, x, fp, self.types)
        f = m["featureIndex"]
        d = np.hypot(m["imagePos"][:, 0] - uv[f, 0], m["imagePos"][:, 1] - uv[f, 1])
        D = np.where(ok[f], d, np.nan)
        margin = np.where(ok[f], np.minimum(np.abs(d - thr), vmargin[f]), vmargin[f])
        return D, margin

    def reference_loop(self, m, prob):
        """ransac_ref.sequential_loop with the hypotheses' rows formed as the loop reaches them -> (mask, hypotheses, supports)"""
        M, thr = len(m), self.par.ransacThresholdPredictDistance
        best, nhyp, i = 0, rr.INITIAL_HYPOTHESES, 0
        mask, counts = np.zeros(M, dtype=bool), []
        while i < nhyp and i < M:
            D, margin = self.distances(m, i)
            assert margin.min() >= MARGIN, ("a decision of the reference is within its own error", i, float(margin.min()))
            with np.errstate(invalid="ignore"):
                row = D < thr
            counts.append(int(row.sum()))
            if counts[-1] > best:
                best, mask = counts[-1], row
                nhyp = hypothesis_bound(best, M, prob)
            i += 1
        return mask, i, counts


def hypothesis_bound(ns, M, prob):
    """ransac_ref.hypothesis_bound, and the case it leaves out: every match supports the hypothesis (ns = M), e = 0 and log(0) = -inf
    make the bound (int)(-0.0) = 0 (1PointRansac.cpp:170-176, k_ransac_select)"""
    return 0 if ns == M else rr.hypothesis_bound(ns, M, prob)


def assert_loop_equal(t, m, what):
    mask, nh, counts = t.reference_loop(m, t.par.ransacAllInliersProbability)
    mask_e, nh_e = t.e.ransac(m)
    assert nh_e == nh, (what, nh_e, nh, counts)
    np.testing.assert_array_equal(mask_e, mask, err_msg=str(what))
    return mask, nh, counts


# ------------------------------------------------------------------------------------------------------ RANSAC
@pytest.mark.parametrize("precision", [F64, F32_EXACT])
@pytest.mark.parametrize("N", RANSAC_SIZES)
def test_ransac_full_loop_by_match_count(eng_mod, N, precision):
    """every feature matched (M = N: one lane, the wavefront seams, the 256 -> 512-thread launch, more than two matches per thread),
    about a third of the features unmatched, one match, none: inlier mask (the winner's support), its size and n_hypotheses"""
    t = Tables(eng_mod, all_visible_scene(N), precision)
    assert len(t.preds) == N
    mask_e, nh_e = t.e.ransac(np.zeros(0, dtype=MATCH_DTYPE))
    assert len(mask_e) == 0 and nh_e == 0
    full = t.matches(N)
    mask, nh, counts = assert_loop_equal(t, full, ("all matched", N))
    assert nh >= 1 and max(counts) == mask.sum() >= 1
    if N >= 63:
        assert not mask.all() and nh >= 2, (counts, nh)  # (supports that differ: the loop went on past the first hypothesis)
        keep = np.arange(N) % 3 != 1
        assert_loop_equal(t, t.matches(N + 1, keep), ("a third unmatched", N))
        assert_loop_equal(t, np.roll(full, -(N // 2)), ("rotated", N))
    one = full[N // 2 : N // 2 + 1]
    mask, nh, _ = assert_loop_equal(t, one, ("one match", N))
    assert nh == 1 and mask.tolist() == [True]  # a hypothesis moves its own feature onto its match
    t.e.close()


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
@pytest.mark.parametrize("N", [65, 257, 1025])
def test_ransac_support_mask_and_count_per_hypothesis(eng_mod, N, precision):
    """with the bound collapsing behind the first supported hypothesis, RANSAC on the list rotated by h returns hypothesis h's own
    support mask and count"""
    t = Tables(eng_mod, all_visible_scene(N), precision, prob=TINY_PROBABILITY)
    m = t.matches(7 * N)
    single = 0
    for h in (0, 1, 63, 64, N // 2, N - 1):
        mr = np.roll(m, -h)
        mask, nh, counts = assert_loop_equal(t, mr, ("hypothesis", N, h))
        single += nh == 1
        if nh == 1:
            D, _ = t.distances(m, h)
            with np.errstate(invalid="ignore"):
                np.testing.assert_array_equal(np.roll(mask, h), D < t.par.ransacThresholdPredictDistance)
    assert single >= 4
    t.e.close()


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
def test_ransac_feature_behind_the_camera(eng_mod, precision):
    """a matched XYZ feature behind the camera is re-projected by no hypothesis: its flag is 0 in every mask, whatever its match says"""
    N = 257
    s = all_visible_scene(N)
    hidden = 100
    assert s.feature_type[hidden] == pr.FEATURE_DEPTH
    R = pr._quat_to_rot(s.x_pred[3:7].astype(pr.LD)).astype(np.float64)
    fpos = s.feature_pos.copy()
    fpos[hidden, 0:3] = s.x_pred[0:3] - 5.0 * R[:, 2]  # five metres along -z of the camera
    for prob in (None, TINY_PROBABILITY):
        t = Tables(eng_mod, s, precision, prob=prob, feature_pos=fpos)
        assert len(t.preds) == N - 1 and hidden not in t.row_of
        m = t.matches(3)
        extra = np.zeros(1, dtype=MATCH_DTYPE)
        extra["featureIndex"], extra["keypointIndex"], extra["imagePos"] = hidden, -1, [s.cam.cx, s.cam.cy]
        m = np.concatenate([m[:200], extra, m[200:]])  # (behind every hypothesis the loops below evaluate)
        for h in ((0, 5, 130) if prob else (0,)):
            mr = np.roll(m, -h)
            mask, nh, _ = assert_loop_equal(t, mr, ("hidden", prob, h))
            assert nh < 200 - h and mask.sum() > 1 and not mask[(200 - h) % len(m)]
        t.e.close()


def test_ransac_hypotheses_divided_between_two_shards(eng_mod):
    """EKF::step on two emulated shards evaluates the hypotheses [h_lo, h_hi) of its own features on each rank and gathers counts and
    masks: the same control flow and the same filter as the unsharded step"""
    N, frames = 257, 2
    seq = SyntheticSequence(N, frames)
    P0 = 0.5 * (seq.P0 + seq.P0.T)
    grp = LocalShardGroup(seq.cam, seq.par, N, 2, max_keypoints=4 * N + 64, precision=F64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P0)
    infos = grp.run(lambda rank, e: [e.step(*seq.frames[i]) for i in range(frames)])
    ref = eng_mod.EkfEngine(seq.cam, seq.par, N, max_keypoints=4 * N + 64, precision=F64)
    ref.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, P0)
    ref_infos = [ref.step(*seq.frames[i]) for i in range(frames)]
    for r in range(2):
        for i in range(frames):
            for f in INFO_FIELDS:
                assert getattr(infos[r][i], f) == getattr(ref_infos[i], f), (r, i, f)
    assert all(i.n_hypotheses >= 1 and i.n_inliers >= 1 for i in ref_infos)
    x, fp, P = grp.get_state()
    xr, fpr, Pr = ref.get_state()
    assert state_err(x, fp, xr, fpr) <= 1e-12 and rel_max(P, Pr) <= 1e-12
    grp.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------ prediction tables
_PRED_SCENES = {}


def prediction_scene(N):
    """both feature types, predict_ref's visibility pattern, no covariance (the tables compared do not depend on it)"""
    if N not in _PRED_SCENES:
        s = pr.make_scene(mixed_types(N), with_P0=False)
        o_args = (s.x13, s.feature_pos, s.feature_type, s.desc, np.zeros((s.n, s.n)))
        _PRED_SCENES[N] = (s, o_args)
    return _PRED_SCENES[N]


def assert_tables_close(got, want, what):
    pe, Hse, Hfe = got
    po, Hso, Hfo = want
    assert len(pe) == len(po), what
    np.testing.assert_array_equal(pe["featureIndex"], po["featureIndex"], err_msg=str(what))
    if len(po) == 0:
        return
    np.testing.assert_allclose(pe["imagePos"], po["imagePos"], rtol=1e-12, atol=1e-9, err_msg=str(what))
    assert rel_max(Hse, Hso) <= 1e-11 and rel_max(Hfe, Hfo) <= 1e-11, what


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_full_prediction_tables_per_entry(eng_mod, oracle_lib, N, precision):
    s, args = prediction_scene(N)
    e = eng_mod.EkfEngine(s.cam, s.par, N + 8, max_keypoints=64, precision=precision)
    o = oracle_lib.Oracle(s.cam, s.par, N + 8)
    e.set_state(*args)
    o.set_state(*args)
    e.predict()
    o.predict()
    want = o.predict_measurements()
    np.testing.assert_array_equal(want[0]["featureIndex"], np.nonzero(s.vis)[0])
    assert_tables_close(e.predict_measurements(), want, ("full", N))
    np.testing.assert_array_equal(e.unseen_features(), np.nonzero(~s.vis)[0])  # pred_vis of the full prediction
    e.close()


@pytest.mark.parametrize("count", [1, 63, 65, 256])
def test_sublist_prediction_tables_per_entry(eng_mod, oracle_lib, count):
    """the outlier re-prediction (one workgroup with its own compaction) on a permuted list of `count` features of a map of 300"""
    N = 300
    s, args = prediction_scene(N)
    e = eng_mod.EkfEngine(s.cam, s.par, N + 8, max_keypoints=64, precision=F64)
    o = oracle_lib.Oracle(s.cam, s.par, N + 8)
    e.set_state(*args)
    o.set_state(*args)
    e.predict()
    o.predict()
    full = e.predict_measurements()
    idx = np.random.default_rng(count).permutation(N)[:count].astype(np.int32)
    if count == 1:
        idx = np.nonzero(s.vis)[0][:1].astype(np.int32)
    want = o.predict_measurements(idx)
    np.testing.assert_array_equal(want[0]["featureIndex"], idx[s.vis[idx]])
    got = e.predict_measurements(idx)
    assert_tables_close(got, want, ("sub-list", count))
    # the same kernel body as the full prediction: the same bits
    row = {int(f): k for k, f in enumerate(full[0]["featureIndex"])}
    sel = [row[int(f)] for f in got[0]["featureIndex"]]
    np.testing.assert_array_equal(got[0]["imagePos"], full[0]["imagePos"][sel])
    np.testing.assert_array_equal(got[1], full[1][sel])
    np.testing.assert_array_equal(got[2], full[2][sel])
    np.testing.assert_array_equal(e.unseen_features(), np.nonzero(~s.vis)[0])  # (the sub-list leaves the full prediction's list)
    e.close()


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
@pytest.mark.parametrize("N", [255, 1000])
def test_step_prediction_equals_stage_calls_mixed_map(eng_mod, N, precision):
    """EKF::step's fused prediction (counts on the device) against ekf_predict + ekf_predict_measurements on the same frame, bit for
    bit: the state, P, the H P rows (formed from Hs and Hf) and the unseen list; with ekf_keep_step_predictions the predicted pixels
    and S.  The frame has no keypoints: nothing is matched or updated."""
    s = pr.make_scene(mixed_types(N))
    kps, desc = np.zeros(0, dtype=KEYPOINT_DTYPE), np.zeros((0, DESC_BYTES), dtype=np.uint8)

    def engine():
        e = eng_mod.EkfEngine(s.cam, s.par, N + 8, max_keypoints=64, precision=precision)
        e.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
        return e

    fused, kept, staged = engine(), engine(), engine()
    kept.keep_step_predictions(True)
    infos = [fused.step(kps, desc), kept.step(kps, desc)]
    staged.predict()
    want, _, _ = staged.predict_measurements()
    np.testing.assert_array_equal(want["featureIndex"], np.nonzero(s.vis)[0])
    every = np.arange(N, dtype=np.int32)
    xs, fs, Ps = staged.get_state()
    HPs, HPcs = staged.hp_rows(every)
    for name, e, info in (("fused", fused, infos[0]), ("kept", kept, infos[1])):
        assert (info.n_predicted, info.n_matches, info.status) == (len(want), 0, 0), name
        x, f, P = e.get_state()
        np.testing.assert_array_equal(x, xs, err_msg=name)
        np.testing.assert_array_equal(f, fs, err_msg=name)
        np.testing.assert_array_equal(P, Ps, err_msg=name)
        np.testing.assert_array_equal(e.unseen_features(), staged.unseen_features(), err_msg=name)
        HP, HPc = e.hp_rows(every)
        np.testing.assert_array_equal(HP, HPs, err_msg=name)
        np.testing.assert_array_equal(HPc, HPcs, err_msg=name)
    got = kept.step_predictions()
    np.testing.assert_array_equal(got["featureIndex"], want["featureIndex"])
    np.testing.assert_array_equal(got["imagePos"], want["imagePos"])
    np.testing.assert_array_equal(got["covarianceMatrix"], want["covarianceMatrix"])
    for e in (fused, kept, staged):
        e.close()


def test_step_with_matches_equals_stage_calls(eng_mod):
    """one frame with keypoints through EKF::step (records written by k_match_compact, counts on the device) and through the stage
    calls predict / predict_measurements / match / ransac (records written by k_match_index): the same matches, the same number
    of hypotheses and inliers"""
    N = 300
    seq = SyntheticSequence(N, 1)

    def engine():
        e = eng_mod.EkfEngine(seq.cam, seq.par, N + 8, max_keypoints=4 * N + 64, precision=F64)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        return e

    stepped, staged = engine(), engine()
    info = stepped.step(*seq.frames[0])
    staged.predict()
    staged.predict_measurements()
    m = staged.match(*seq.frames[0])
    mask, nh = staged.ransac(m)
    assert (info.n_matches, info.n_hypotheses, info.n_inliers) == (len(m), nh, int(mask.sum()))
    assert nh >= 1 and mask.sum() >= 1 and math.isfinite(stepped.get_state(want_P=False)[0].sum())
    stepped.close()
    staged.close()
