"""GPU: the update's glue kernels in the exact configurations -- dx = B'z from the digit planes (k_dx_planes: every element's digit
word converted with digit_planes.h's px_word_value) and the state update with the quaternion normalisation of P behind the downdate
(k_apply_normalize) -- through the stage calls predict / predict_measurements / update, against the fp64 oracle.

Scenes are tests/predict_ref.py's with every feature inverse depth and in view (n = 13 + 6 N).  Shapes, where k_dx_planes can go wrong
(its grid is (n / 256 column blocks) x 16 k-splits over the m16 = round_up(2 M, 32) / 16 groups of 16 rows):
  N = 12,  M = 1, 12   n = 85: one partial column block; M = 1: m16 = 2, fourteen of the sixteen k-splits are empty
  N = 272, M = 1       n = 1645 = 6 x 256 + 109 columns: the last column block ragged
  N = 272, M = 16, 17  32 -> 64 rows of the planes (m16 = 2 -> 4)
  N = 272, M = 257     m16 = 34: three groups per split, the last splits partial or empty
Tolerances: EKF_PRECISION_F32_EXACT parity_metric.F32_TOL on every block and every feature parameter; EKF_PRECISION_F64_EXACT the
1e-7 the suite holds that precision to (tests/test_gpu_exact_edge_cases.py: 38-bit digits of B under a-priori column scales, no
storage rounding), far inside parity_metric's figure.  The oracle's update of a shape is computed once and shared by both precisions.

Full steps (the partition of the matches enqueued behind the first batch of hypotheses, before the host has seen the batch's outcome):
a stepped engine against a second engine driven through the stage calls, bit for bit."""
import numpy as np
import pytest

import predict_ref as pr
from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import F32_TOL, over_tolerance, parity_report
from tests.oracle_lib import ALGORITHMIC, align_to_matches
from tests.test_gpu_edge_cases import _matches_from_predictions

pytestmark = pytest.mark.gpu

F32_EXACT, F64_EXACT = 2, 3
TOL = {F32_EXACT: F32_TOL, F64_EXACT: 1e-7}
SHAPES = [(12, 1), (12, 12), (272, 1), (272, 16), (272, 17), (272, 257)]


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


_SCENES, _REFERENCES = {}, {}


def scene(N):
    if N not in _SCENES:
        _SCENES[N] = pr.make_scene(np.full(N, pr.FEATURE_INVERSE_DEPTH, dtype=np.int32), vis=np.ones(N, dtype=bool))
    return _SCENES[N]


def reference(oracle_lib, N, M):
    """(matches, x, feature parameters, P) of the oracle's update with the first M predictions matched (read-only, shared)"""
    if (N, M) not in _REFERENCES:
        s = scene(N)
        o = oracle_lib.Oracle(s.cam, s.par, N + 8)
        o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
        o.predict()
        preds, Hs, Hf = o.predict_measurements()
        assert len(preds) == N
        mo = _matches_from_predictions(preds, M)
        mp, mHs, mHf = align_to_matches(preds, Hs, Hf, mo)
        assert o.update(mo, mp, mHs, mHf, ALGORITHMIC) == 0
        out = (mo, o.x13().copy(), o.feature_pos().copy(), o.P().copy())
        for a in out:
            a.setflags(write=False)
        _REFERENCES[(N, M)] = out
    return _REFERENCES[(N, M)]


@pytest.mark.parametrize("precision", [pytest.param(F32_EXACT, id="f32x"), pytest.param(F64_EXACT, id="f64x")])
@pytest.mark.parametrize("N,M", SHAPES)
def test_update_state_and_covariance_at_the_dx_kernel_edges(eng_mod, oracle_lib, N, M, precision):
    s = scene(N)
    assert s.n == 13 + 6 * N
    mo, xo, fpo, Po = reference(oracle_lib, N, M)
    e = eng_mod.EkfEngine(s.cam, s.par, N + 8, max_keypoints=64, precision=precision)
    try:
        assert e.precision == precision
        e.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
        assert e.n == s.n
        e.predict()
        preds, _, _ = e.predict_measurements()
        assert len(preds) == N
        e.update(mo)
        x, fp, P = e.get_state()
    finally:
        e.close()
    be = parity_report(x, fp, P, xo, fpo, Po)
    print(f"\nupdate glue: N {N:4d} M {M:4d} precision {precision}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(be.items())), end="")
    bad = over_tolerance(be, TOL[precision], N, componentwise=True)
    assert not bad, (N, M, precision, bad)
    # the update moved the state (dx is not lost), and the exact downdate with the normalisation behind it leaves P bitwise symmetric
    assert np.abs(x - s.x_pred).max() > 0.0
    assert np.array_equal(P, P.T)
    assert abs(np.linalg.norm(x[3:7]) - 1.0) <= 1e-12


# ------------------------------------------------------------------------------ the low-innovation partition behind the first batch
STEP_FIELDS = ("n_predicted", "n_matches", "n_hypotheses", "n_inliers", "n_outliers", "n_rescued", "status")


@pytest.fixture(scope="module")
def seq200():
    return SyntheticSequence(200, 3)


def staged_step(e, kps, desc):
    """EKF::step through the stage calls -> its counters"""
    e.predict()
    preds, _, _ = e.predict_measurements()
    m = e.match(kps, desc)
    mask, nh = e.ransac(m)
    inl, out = m[mask], m[~mask]
    if len(inl):
        e.update(inl)
    nr = 0
    if len(out):
        e.predict_measurements(out["featureIndex"])
        resc = out[e.rescue(out)]
        nr = len(resc)
        if nr:
            e.update(resc)
    return dict(n_predicted=len(preds), n_matches=len(m), n_hypotheses=nh, n_inliers=len(inl), n_outliers=len(out), n_rescued=nr, status=0)


@pytest.mark.parametrize("precision", [pytest.param(0, id="f64"), pytest.param(F32_EXACT, id="f32x")])
@pytest.mark.parametrize("ransac_batch", [pytest.param(0, id="one_batch"), pytest.param(1, id="second_batch")])
def test_step_partition_behind_the_first_batch_equals_stage_calls(eng_mod, seq200, ransac_batch, precision):
    """A device-count step enqueues the partition of the matches behind its FIRST batch of hypotheses, before the host has seen the
    batch's outcome; the launch works only if that batch ended the loop.  With the default batch it does (one_batch); with
    ransac_batch = 1 the loop needs further batches, the early launch must leave every list alone and the launch behind the loop
    does the work (second_batch).  Either way: the counters of every frame, then x, the feature parameters and P, equal bit for bit
    to a second engine driven through predict / predict_measurements / match / ransac / update / rescue / update (launch-per-panel
    sweep on both: the persistent sweep's sums go in arrival order)."""
    seq = seq200

    def engine(batch):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision,
                              ransac_batch=batch)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        e.set_sweep_mode(4)
        return e

    stepped, staged = engine(ransac_batch), engine(0)
    try:
        rescued = 0
        for t, (kps, desc) in enumerate(seq.frames):
            info = stepped.step(kps, desc)
            want = staged_step(staged, kps, desc)
            got = {f: getattr(info, f) for f in STEP_FIELDS}
            assert got == want, (t, got, want)
            if ransac_batch == 1:
                assert info.n_hypotheses > 1, "the frame must need a second batch"
            rescued += info.n_rescued
        assert rescued > 0, "the scene must exercise both updates"
        for u, v in zip(stepped.get_state(), staged.get_state()):
            np.testing.assert_array_equal(u, v)
    finally:
        stepped.close()
        staged.close()
