"""tests/map_ref.py (the longdouble reference of the map-management stage tests) held to the oracle, and the input conditions that
tests/test_gpu_map_stages.py assumes.  No GPU.

The oracle is an fp64 implementation of the same formulas (oracle/ekf_oracle.c:380-617: features added one at a time, convertToDepth,
computeLinearityIndex, removeFeaturesFromStateAndCovariance); that it stays inside the derived bounds with u_store = 0, at every
scene the device tests use, is what shows the bounds are not too tight for a correct implementation."""
import numpy as np
import pytest

import map_ref as mr
import predict_ref as pr
from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH, FEATURE_INVERSE_DEPTH


def report(what, n, dev, ref, tol):
    r, at = pr.worst_ratio(dev, ref, tol)
    print(f"map reference vs oracle: {what:12s} n {n:4d}: worst |oracle - ref| / tol = {r:.3f} at {at}")
    return r, at


def oracle_before_add(ol, n_old, cap):
    if n_old == 13:
        cam, par = pr.s3_camera(), pr.s3_params()
        o = ol.Oracle(cam, par, cap)
        o.reset()
    else:
        s = pr.scene_for_n(n_old)
        cam, par = s.cam, s.par
        o = ol.Oracle(cam, par, s.n_features + cap)
        o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    o.predict()
    return o, cam, par


@pytest.mark.parametrize("n_old", mr.ADD_N_OLD + [mr.ADD_FULL_WORKGROUPS[0]])
def test_batched_add_formulas_equal_the_oracle_adding_one_at_a_time(oracle_lib, n_old):
    count = max(mr.ADD_COUNTS)
    o, cam, par = oracle_before_add(oracle_lib, n_old, count)
    x0, P0, N_old = o.x13(), o.P(), o.N
    uv = mr.add_pixels(count)
    ref = mr.add_ref(x0, P0, cam, par, uv)
    # the oracle forms the new columns from P[0:n, 0:7], and its predicted P is symmetric only to rounding: the same formula on P'
    ref_t = ref if np.array_equal(P0, P0.T) else mr.add_ref(x0, P0.T, cam, par, uv)
    g = ref["g"]
    assert (g[:, 0] ** 2 + g[:, 2] ** 2 >= 0.25).all()  # no ray near the singularity of atan2 / of dth, dph
    for k in range(count):
        assert o.add_feature(uv[k]) == N_old + k
    P = o.P()
    m = 6 * count
    assert o.n == n_old + m
    bad = []
    for name, got, (want, tol) in (("feature_pos", o.feature_pos()[N_old:], ref["feature_pos"]),
                                   ("rows", P[n_old:, :n_old].reshape(count, 6, n_old), ref["rows"]),
                                   ("columns", P[:n_old, n_old:].T.reshape(count, 6, n_old), ref_t["rows"]),
                                   ("corner", P[n_old:, n_old:], ref["corner"])):
        r, at = report(name, n_old, got, want, tol)
        if not (r <= 1.0):
            bad.append((name, r, at))
    assert not bad, bad
    np.testing.assert_array_equal(P[:n_old, :n_old], P0)
    # the tolerances mean something: non-zero wherever a value is computed, zero where it is copied
    computed = ref["rows"][0][:, (3, 4), :] != 0  # (after a reset most of P[0:7] is zero: a zero product has tolerance 0)
    assert (ref["rows"][1][:, (3, 4), :][computed] > 0).all() and (ref["rows"][1][:, mr.EXACT_ROWS, :] == 0).all()
    assert (ref["feature_pos"][1][:, 3:5] > 0).all() and (ref["feature_pos"][1][:, 3:5] < 1e-12).all()
    rel = ref["rows"][1][:, (3, 4), :] / np.maximum(np.abs(ref["rows"][0][:, (3, 4), :]), 1e-300)
    print(f"  rows: median tol / |ref| = {float(np.median(rel)):.2e}")


def test_off_diagonal_corner_blocks_carry_no_noise():
    """the reference itself: block (j, i), i != j, is Jpo_j P77 Jpo_i' alone; the noise (1 px^2, rho SD^2 = 1) would show"""
    s = pr.scene_for_n(259)
    ref = mr.add_ref(s.x_pred, s.P0, s.cam, s.par, mr.add_pixels(5))
    corner = np.asarray(ref["corner"][0], dtype=np.float64)
    pre = mr.add_prepare(s.x_pred, s.cam, mr.add_pixels(5))
    J = np.asarray(pre["Jpo"][0], dtype=np.float64)
    for j in range(5):
        for i in range(5):
            plain = J[j] @ s.P0[:7, :7] @ J[i].T
            d = corner[6 * j:6 * j + 6, 6 * i:6 * i + 6] - plain
            if i == j:
                assert abs(d[5, 5] - 1.0) < 1e-12 and d[3, 3] > 1e-9
            else:
                assert np.abs(d).max() < 1e-18


@pytest.mark.parametrize("n,pos", mr.CONVERT_CASES)
def test_convert_and_linearity_equal_the_oracle(oracle_lib, n, pos):
    s = mr.convert_scene(n, pos)
    assert s.n == n
    fi = int(np.nonzero(s.feature_type == FEATURE_INVERSE_DEPTH)[0][0])
    assert s.covpos[fi] == pos and (pos + 6 == n) == (fi == s.n_features - 1)
    o = oracle_lib.Oracle(s.cam, mr.convert_params(), s.n_features)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    ref = mr.convert_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, s.P0, fi)
    L, Ltol = ref["linearity"]
    inv = np.nonzero(s.feature_type == FEATURE_INVERSE_DEPTH)[0]
    Lo = np.array([o.linearity_index(f) for f in inv])
    r, at = report("linearity", n, Lo, L[inv], Ltol[inv])
    assert r <= 1.0 and (L[inv] > 0).all() and (L[inv] < 1e9).all()
    assert o.convert_inverse_depth_to_depth() == fi
    P = o.P()
    mr.check_converted(report, n, s.P0, P, o.feature_pos(), ref, fi, s.feature_pos)
    _, nt, nc = mr.compact_index(s.feature_type, s.covpos, [])
    nt[fi] = FEATURE_DEPTH
    np.testing.assert_array_equal(o.feature_type(), nt)
    np.testing.assert_array_equal(o.feature_covpos(), mr.layout(nt)[0])


@pytest.mark.parametrize("n_new,kind", mr.REMOVE_CASES)
def test_compact_index_equals_the_oracle(oracle_lib, n_new, kind):
    types, drop = mr.remove_case(n_new, kind)
    covpos, n0 = mr.layout(types)
    assert 300 < n0 <= 650
    if kind == "straddle":
        assert covpos[drop[0]] <= 250 and covpos[drop[-1]] + mr.dim(types[drop[-1]]) > 257 and (np.diff(drop) == 1).all()
    s = pr.scene_for_n(n0)
    np.testing.assert_array_equal(s.feature_type, types)
    o = oracle_lib.Oracle(s.cam, s.par, s.n_features)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
    o.remove_features(drop)
    new2old, nt, nc = mr.compact_index(types, covpos, drop)
    assert o.n == n_new == len(new2old)
    np.testing.assert_array_equal(o.P(), s.P0[np.ix_(new2old, new2old)])
    np.testing.assert_array_equal(o.feature_type(), nt)
    np.testing.assert_array_equal(o.feature_covpos(), nc)
    np.testing.assert_array_equal(o.feature_pos(), np.delete(s.feature_pos, drop, axis=0))


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("n", [259, 514, 520, 649, 1024])
def test_P0_rounded_to_fp32_has_distinct_entries(n):
    """a gather from a wrong row or column, or a stale value, changes a bit: no two entries of the upper triangle are equal"""
    P = pr.make_P0(n).astype(np.float32)
    tri = P[np.triu_indices(n)]
    assert len(np.unique(tri)) == len(tri)


def test_every_start_map_of_the_removal_cases_has_distinct_fp32_entries():
    for n_new, kind in mr.REMOVE_CASES:
        n0 = mr.layout(mr.remove_case(n_new, kind)[0])[1]
        tri = pr.make_P0(n0).astype(np.float32)[np.triu_indices(n0)]
        assert len(np.unique(tri)) == len(tri), (n_new, kind, n0)


@pytest.mark.parametrize("N,fstar", mr.SELECT_CASES)
def test_selection_scenes_have_one_feature_below_the_threshold_by_a_factor(oracle_lib, N, fstar):
    s, P, thr = mr.select_scene(N, fstar)
    assert s.n_features == N
    L, tol = mr.linearity_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, P)
    inv = np.nonzero(s.feature_type == FEATURE_INVERSE_DEPTH)[0]
    assert (L[inv] > 0).all() and np.isinf(L[s.feature_type != FEATURE_INVERSE_DEPTH]).all()
    below = inv[L[inv] < thr]
    np.testing.assert_array_equal(below, [] if fstar is None else [fstar])
    ratio = np.maximum(L[inv] / thr, thr / L[inv])
    print(f"selection N {N} f* {fstar}: threshold {thr:.4f}, indices {float(L[inv].min()):.4f} .. {float(L[inv].max()):.4f}, "
          f"nearest factor {float(ratio.min()):.2f}")
    assert (ratio >= 2.0).all()
    assert np.array_equal(P, P.T)
    for Pq in (P, P.astype(np.float32).astype(np.float64)):  # the fp32-stored matrix selects the same feature by the same factor
        Lq = mr.linearity_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, Pq)[0][inv]
        assert (np.maximum(Lq / thr, thr / Lq) >= 2.0).all() and np.array_equal(inv[Lq < thr], below)
    par = mr.convert_params()
    par.inverseDepthLinearityIndexThreshold = thr
    o = oracle_lib.Oracle(s.cam, par, N)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, P)
    Lo = np.array([o.linearity_index(f) for f in inv])
    r, at = pr.worst_ratio(Lo, L[inv], tol[inv])
    assert r <= 1.0, (r, at)
    assert o.convert_inverse_depth_to_depth() == (-1 if fstar is None else fstar)


def test_linearity_indices_of_the_mixed_scene_are_positive():
    s = pr.make_scene(pr.types_for_n(514))
    L = mr.linearity_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, s.P0)[0]
    inv = s.feature_type == FEATURE_INVERSE_DEPTH
    print(f"linearity indices at n = 514: {float(L[inv].min()):.3f} .. {float(L[inv].max()):.3f}")
    assert (L[inv] > 0.1).all()
