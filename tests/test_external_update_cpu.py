"""CPU-only checks of the numpy restatement of the external measurement update (tests/external_update_ref.py): fed the camera's
own Jacobian rows it reproduces the oracle's update, and its NIS, symmetry, gate and failure report are what DESIGN.md section
4.13 says."""
import numpy as np
import pytest

import external_update_ref as xr
from parity_metric import F64_TOL, over_tolerance, parity_report


def oracle_with_matches(ol, seq, n_matches=8):
    o = ol.Oracle(seq.cam, seq.par, seq.n_features + 8)
    o.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    o.predict()
    po, Hs, Hf = o.predict_measurements()
    mo = o.match(po, *seq.frames[0])[:n_matches]
    assert len(mo) == n_matches
    return (o, mo) + ol.align_to_matches(po, Hs, Hf, mo)


def state_of(o):
    return o.x13(), o.feature_pos(), o.feature_type(), o.feature_covpos(), o.P()


@pytest.mark.parametrize("which", ["seq12", "seq50"])
def test_reference_reproduces_the_oracle_update(oracle_lib, seq12, seq50, which):
    seq = seq12 if which == "seq12" else seq50
    o, mo, mp, mHs, mHf = oracle_with_matches(oracle_lib, seq)
    x, fp, t, c, P = state_of(o)
    (rs, col, val), res = xr.visual_rows(mp, mHs, mHf, mo, t, c)
    assert len(res) == 16 and np.all(np.diff(rs) == 19)
    R = seq.cam.pixelErrorX * np.eye(len(res))
    ref = xr.external_update_ref(x, fp, t, c, P, rs, col, val, res, R)
    assert ref["status"] == "applied"
    assert o.update(mo, mp, mHs, mHf, oracle_lib.ALGORITHMIC) == 0
    be = parity_report(ref["x13"], ref["feature_pos"], ref["P"], o.x13(), o.feature_pos(), o.P())
    print(f"{which}: reference against oracle_lib update(ALGORITHMIC):", {k: f"{v:.1e}" for k, v in be.items()})
    assert not over_tolerance(be, F64_TOL), be
    # nis = nu' inv(S) nu
    H = np.zeros((len(res), len(P)))
    for i in range(len(res)):
        H[i, col[rs[i]:rs[i + 1]]] = val[rs[i]:rs[i + 1]]
    S = H @ P @ H.T + R
    nis = res @ np.linalg.solve(S, res)
    assert abs(ref["nis"] - nis) <= F64_TOL * nis
    assert abs(ref["z"] @ ref["z"] - ref["nis"]) <= 1e-15 * ref["nis"]
    # P comes out exactly symmetric and its diagonal does not grow
    np.testing.assert_array_equal(ref["P"], ref["P"].T)
    P6 = xr.external_update_ref(x, fp, t, c, P, rs, col, val, res, R)["P"]
    np.testing.assert_array_equal(P6, ref["P"])  # the inputs were not modified by the first call
    assert np.all(np.diag(ref["P_downdated"]) <= np.diag(P))
    keep = np.r_[0:3, 7:len(P)]  # (the normalisation rescales the quaternion's four variances and nothing else on the diagonal)
    np.testing.assert_array_equal(np.diag(ref["P"])[keep], np.diag(ref["P_downdated"])[keep])


def test_gate_and_failure_leave_the_inputs_untouched(oracle_lib, seq12):
    o, mo, mp, mHs, mHf = oracle_with_matches(oracle_lib, seq12, 3)
    x, fp, t, c, P = state_of(o)
    (rs, col, val), res = xr.visual_rows(mp, mHs, mHf, mo, t, c)
    R = seq12.cam.pixelErrorX * np.eye(len(res))
    free = xr.external_update_ref(x, fp, t, c, P, rs, col, val, res, R)
    assert free["status"] == "applied" and free["nis"] > 0
    keep = [a.copy() for a in (x, fp, P)]
    gated = xr.external_update_ref(x, fp, t, c, P, rs, col, val, res, R, gate_nis=free["nis"] * (1 - 1e-9))
    assert gated["status"] == "gated" and gated["nis"] == free["nis"]
    for a, b, g in zip((x, fp, P), keep, (gated["x13"], gated["feature_pos"], gated["P"])):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(g, b)
    passed = xr.external_update_ref(x, fp, t, c, P, rs, col, val, res, R, gate_nis=free["nis"] * (1 + 1e-9))
    assert passed["status"] == "applied"
    np.testing.assert_array_equal(passed["P"], free["P"])


def test_not_positive_definite_is_reported():
    x = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    P = 1e-3 * np.eye(13)
    rs, col, val = xr.csr_of(np.eye(3, 13))
    ref = xr.external_update_ref(x, np.zeros((0, 6)), [], [], P, rs, col, val, np.ones(3), -np.eye(3))
    assert ref["status"] == "not_pd"
    np.testing.assert_array_equal(ref["P"], P)
    np.testing.assert_array_equal(ref["x13"], x)


def test_fp32_storage_rounds_twice():
    rng = np.random.default_rng(5)
    M = rng.standard_normal((13, 13))
    P = (M @ M.T).astype(np.float32).astype(np.float64)
    P = np.triu(P) + np.triu(P, 1).T
    x = np.array([0.1, 0.2, 0.3, 0.9, 0.1, -0.2, 0.3, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    rs, col, val = xr.csr_of(np.eye(3, 13))
    a = xr.external_update_ref(x, np.zeros((0, 6)), [], [], P, rs, col, val, [0.1, -0.1, 0.2], np.eye(3), storage=np.float32)
    b = xr.external_update_ref(x, np.zeros((0, 6)), [], [], P, rs, col, val, [0.1, -0.1, 0.2], np.eye(3))
    np.testing.assert_array_equal(a["P"], a["P"].astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(a["P"], a["P"].T)
    assert 0 < np.abs(a["P"] - b["P"]).max() <= 2.0 ** -22 * np.abs(b["P"]).max()
    np.testing.assert_array_equal(a["x13"], b["x13"])  # the state is formed in fp64 from the same P
