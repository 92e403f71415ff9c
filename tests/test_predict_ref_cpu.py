"""CPU only: tests/predict_ref.py against the oracle within the reference's own bounds, and the input conditions that
tests/test_gpu_prediction_stages.py relies on (no case is excused: the scenes are built so that every condition holds).

Reference against oracle: the oracle is fp64 and sums in another order than the device, but with the same number of terms per
sum, so it has to meet the tolerances the device is held to (u_store = 0).
"""
import numpy as np
import pytest

import predict_ref as pr
from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH, FEATURE_INVERSE_DEPTH

LD = pr.LD


def _oracle_on(ol, s):
    o = ol.Oracle(s.cam, s.par, s.n_features + 8)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    return o


@pytest.mark.parametrize("n,omega_zero", [(13 + 3, False), (13 + 258, False), (13 + 258, True), (13 + 513, False), (13 + 768, False)])
def test_covariance_reference_equals_oracle(oracle_lib, n, omega_zero):
    s = pr.scene_for_n(n, omega_zero)
    o = _oracle_on(oracle_lib, s)
    o.predict()  # (twice, as the device test: F from a state a prediction produced)
    x1, P1 = o.x13(), o.P()
    Fo, GQGo = o.predict(want_F=True)
    F, Fabs, GQG, GQGabs, xp = pr.predict_F(x1, s.par)
    assert (np.abs(Fo - F) <= pr.K_F * pr.U64 * Fabs).all(), pr.worst_ratio(Fo, F, pr.K_F * pr.U64 * Fabs)
    assert (np.abs(GQGo - GQG) <= (8 + 2 * pr.K_F) * pr.U64 * GQGabs).all()
    if omega_zero:  # the |w| < eps branch: no quaternion-by-omega block, the omega diagonal of F zeroed
        assert (F[3:7, 10:13] == 0).all() and (np.diag(F)[10:13] == 0).all() and (np.diag(Fo)[10:13] == 0).all()
    else:
        assert (F[3:7, 10:13] != 0).all()
    assert np.abs(o.x13() - xp).max() <= 16 * pr.U64
    P2 = o.P()
    ref = pr.predict_cov_ref(x1, P1, s.par)
    for name, got in (("corner", P2[:13, :13]), ("row strip", P2[:13, 13:]), ("column strip", P2[13:, :13])):
        r, at = pr.worst_ratio(got, *ref[name])
        print(f"oracle / reference {name} n={n}: worst |oracle - ref| / tol = {r:.3f} at {at}")
        assert r <= 1.0, (name, r, at)
    np.testing.assert_array_equal(P2[13:, 13:], P1[13:, 13:])


@pytest.mark.parametrize("n", [13 + 258, 514])
def test_row_pair_reference_equals_oracle(oracle_lib, n):
    s = pr.scene_for_n(n)
    o = _oracle_on(oracle_lib, s)
    o.predict()
    np.testing.assert_allclose(o.x13(), s.x_pred, rtol=0, atol=1e-15)
    P1 = o.P()
    preds, Hs, Hf, HPo = o.predict_measurements(want_HP=True)
    idx = preds["featureIndex"]
    np.testing.assert_array_equal(idx, np.nonzero(s.vis)[0])
    (HP, tHP), (HPc, tHPc), (S, tS) = pr.hp_ref(P1, Hs, Hf, idx, s.feature_type, s.covpos)
    for name, got, ref, tol in (("HP", HPo, HP, tHP), ("S", preds["covarianceMatrix"], S, tS)):
        r, at = pr.worst_ratio(got, ref, tol)
        print(f"oracle / reference {name} n={n}: worst |oracle - ref| / tol = {r:.3f} at {at}")
        assert r <= 1.0, (name, r, at)
    # a subset prediction of the oracle follows the same decisions, in list order
    sub = np.array(idx[::3][::-1], dtype=np.int32)
    np.testing.assert_array_equal(o.predict_measurements(sub)[0]["featureIndex"], sub)


def _check_map(s, n, both_types):
    assert s.n == n == 13 + sum(pr.dim(t) for t in s.feature_type)
    kinds = set(int(t) for t in s.feature_type)
    if both_types:
        assert kinds == {FEATURE_DEPTH, FEATURE_INVERSE_DEPTH}
    assert int(s.covpos[-1]) + pr.dim(s.feature_type[-1]) - 1 == n - 1  # one feature's block ends at the last column
    assert (np.diff(s.covpos) == [pr.dim(t) for t in s.feature_type[:-1]]).all()


def _check_visibility(s):
    """the pattern is what the reference decides, with 1 px to spare at every threshold; the poison pose sees every unseen feature"""
    ok, margin, _ = pr.visibility_ref(s.cam, s.x_pred, s.feature_pos, s.feature_type)
    np.testing.assert_array_equal(ok, s.vis)
    assert margin.min() >= 1.0, (int(margin.argmin()), margin.min())
    okp, marginp, _ = pr.visibility_ref(s.cam, s.x_poison, s.feature_pos, s.feature_type)
    if (~s.vis).any():
        assert okp[~s.vis].all() and marginp[~s.vis].min() >= 1.0
    return margin.min()


def _check_pattern(vis):
    """predicted and unpredicted items within two of either side of every multiple of 64 (256 and 1024 among them) -- except on the
    sides that belong to the all-unpredicted wavefront 1 and the all-predicted wavefront 2"""
    N = len(vis)
    if N >= 128:
        assert not vis[64:128].any()
    if N >= 192:
        assert vis[128:192].all()
    for b in range(64, N, 64):
        for lo, hi, wf in ((b - 2, b, b // 64 - 1), (b, b + 2, b // 64)):
            if wf in (1, 2) or hi > N:
                continue
            assert set(vis[lo:hi].tolist()) == {True, False}, (b, lo)
    for b in (256, 1024):
        if N > b + 1:
            assert set(vis[b - 2:b].tolist()) == set(vis[b:b + 2].tolist()) == {True, False}


@pytest.mark.parametrize("m", pr.COV_SIZES)
def test_conditions_covariance_sizes(m):
    n = 13 + m
    s = pr.scene_for_n(n)
    _check_map(s, n, both_types=m >= 9)
    # threads of the strip workgroups: 255 fills the first but for one thread, 258 puts two into the second, 513 one into the third,
    # 768 fills the third to its last thread
    assert {3: (1, 3), 255: (1, 255), 258: (2, 2), 510: (2, 254), 513: (3, 1), 768: (3, 256)}[m] == ((m + 255) // 256, m - 256 * ((m - 1) // 256))


@pytest.mark.parametrize("n", sorted(set(pr.HP_SIZES_F64 + pr.HP_SIZES_F32)))
def test_conditions_row_pair_sizes(n):
    s = pr.scene_for_n(n)
    _check_map(s, n, both_types=True)
    _check_pattern(s.vis)
    m = _check_visibility(s)
    print(f"n={n}: N={s.n_features}, {int(s.vis.sum())} predicted, smallest visibility margin {m:.1f} px")
    assert n % 3 == 1
    # chunks and tails (fp64: 2 columns per lane, 512 per chunk; fp32: 4 and 1024)
    if n in pr.HP_SIZES_F64:
        assert {511: (1, 1), 514: (2, 0), 1021: (2, 1), 1024: (2, 0)}[n] == ((n + 511) // 512, n % 2)
    if n in pr.HP_SIZES_F32:
        assert {1021: (1, 1), 1024: (1, 0), 1027: (2, 3), 1030: (2, 2)}[n] == ((n + 1023) // 1024, n % 4)
    # an inverse-depth and an XYZ feature among the predicted ones, and one of the predicted blocks ends in the last chunk
    kinds = set(int(t) for t in s.feature_type[s.vis])
    assert kinds == {FEATURE_DEPTH, FEATURE_INVERSE_DEPTH}


@pytest.mark.parametrize("N", sorted(set(pr.LIST_SIZES + pr.FUSED_SIZES + [300])))
def test_conditions_list_sizes(N):
    s = pr.xyz_scene(N, with_P0=False)
    _check_map(s, 13 + 3 * N, both_types=False)
    _check_pattern(s.vis)
    _check_visibility(s)
    assert 0 < s.vis.sum() < N


def test_pattern_boundaries():
    vis = pr.vis_pattern(1025)
    _check_pattern(vis)
    assert vis[1024] and not vis[1023] and vis[256] and not vis[255]  # the last item of N = 1025 / 257 is a predicted one ...
    assert not pr.vis_pattern(1024)[1023] and not pr.vis_pattern(256)[255]  # ... and the last one of 1024 / 256 is not


@pytest.mark.parametrize("n", sorted(set([13 + m for m in pr.COV_SIZES] + pr.HP_SIZES_F64 + pr.HP_SIZES_F32)))
def test_P0_is_spd_with_distinct_entries(n):
    P = pr.make_P0(n)
    np.testing.assert_array_equal(P, P.T)
    off = P - np.diag(np.diag(P))
    assert np.abs(off).max() <= 1e-6
    assert (np.diag(P) - np.abs(off).sum(axis=1) > 0.2 * n * 1e-6).all()  # Gershgorin, with room for the fp32 rounding of the entries
    iu = np.triu_indices(n)
    assert len(np.unique(P[iu])) == len(iu[0])
    # stored in fp32: entries one to three lanes, one workgroup (255 / 256) or one chunk (512 / 1024) apart in a row stay distinct
    Pf = P.astype(np.float32)
    for k in (1, 2, 3, 255, 256, 512, 1024):
        if k < n:
            assert (Pf[:, k:] != Pf[:, :-k]).all(), k
    Pf64 = Pf.astype(np.float64)
    offf = Pf64 - np.diag(np.diag(Pf64))
    assert (np.diag(Pf64) - np.abs(offf).sum(axis=1) > 0).all()
