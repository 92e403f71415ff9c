"""CPU-only checks of the filter-consistency records: identities of the numpy restatement
(tests/consistency_ref.py), the dead band, the record layouts and the symbols of the built library."""
import ctypes as C

import numpy as np

import consistency_ref as cr
from openekfmonoslam_amd import ekftypes


def _spd_case(M, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(2 * M, 2 * M + 5))
    return A @ A.T + np.eye(2 * M), rng.normal(0.0, 1.5, 2 * M)


def test_conditional_shares_sum_to_the_nis_and_nis_is_the_quadratic_form():
    for M, seed in ((1, 1), (7, 2), (33, 3)):
        S, nu = _spd_case(M, seed)
        nis, c, d2 = cr.from_S(S, nu)
        assert abs(c.sum() - nis) <= 1e-13 * nis
        direct = float(nu @ np.linalg.solve(S, nu))
        assert abs(direct - nis) <= 1e-11 * nis, (M, direct, nis)
        assert len(c) == len(d2) == M and (c >= 0).all() and (d2 >= 0).all()


def test_single_match_marginal_equals_conditional_equals_nis():
    S, nu = _spd_case(1, 5)
    nis, c, d2 = cr.from_S(S, nu)
    assert abs(c[0] - nis) <= 1e-15 * nis and abs(d2[0] - nis) <= 1e-13 * nis
    # the first match of a longer list is conditional on nothing: its share is its marginal distance
    S, nu = _spd_case(6, 6)
    _, c, d2 = cr.from_S(S, nu)
    assert abs(c[0] - d2[0]) <= 1e-12 * d2[0]


def test_dead_band():
    nu = cr.innovation([100.0 + 5e-13, 50.0 + 1e-9], [100.0, 50.0])
    assert nu[0] == 0.0 and nu[1] == (50.0 + 1e-9) - 50.0 and nu[1] != 0.0
    assert cr.innovation([1e-12], [0.0])[0] == 0.0  # |a| <= EKF_DELTA is inside the band
    # through the whole reference: one inverse-depth feature, identity Jacobian blocks
    preds = np.zeros(1, dtype=ekftypes.PREDICTION_DTYPE)
    preds["featureIndex"] = 0
    preds["imagePos"] = [[320.0, 240.0]]
    m = np.zeros(1, dtype=ekftypes.MATCH_DTYPE)
    m["imagePos"] = [[320.0 + 5e-13, 240.0 + 0.25]]
    Hs = np.zeros((1, 2, 13))
    Hf = np.zeros((1, 2, 6))
    Hf[0, 0, 0] = Hf[0, 1, 1] = 1.0
    r = cr.reference(np.eye(19), [2], [13], preds, Hs, Hf, m, 1.0)
    assert r["nu"][0, 0] == 0.0 and r["nu"][0, 1] == 0.25
    assert abs(r["nis"] - 0.25 * 0.25 / 2.0) <= 1e-16 and abs(r["d2"][0] - r["nis"]) <= 1e-16


def test_depth_feature_uses_three_columns_of_hf():
    preds = np.zeros(1, dtype=ekftypes.PREDICTION_DTYPE)
    m = np.zeros(1, dtype=ekftypes.MATCH_DTYPE)
    m["imagePos"] = [[1.0, 2.0]]
    Hf = np.ones((1, 2, 6))
    H, _ = cr.build_H(16, [1], [13], preds, np.zeros((1, 2, 13)), Hf, m)
    assert H.shape == (2, 16) and (H[:, 13:16] == 1.0).all() and (H[:, :13] == 0.0).all()


def test_struct_sizes():
    assert C.sizeof(ekftypes.EkfUpdateConsistency) == 24 and ekftypes.CONSISTENCY_DTYPE.itemsize == 24
    assert C.sizeof(ekftypes.EkfInnovation) == 48 and ekftypes.INNOVATION_DTYPE.itemsize == 48
    assert ekftypes.EkfUpdateConsistency.nis.offset == 16
    assert [getattr(ekftypes.EkfInnovation, f).offset for f in ("featureIndex", "stage", "nu", "d2_marginal", "nis_conditional", "_reserved")] == [
        0, 4, 8, 24, 32, 40]
    assert [ekftypes.INNOVATION_DTYPE.fields[f][1] for f in ("featureIndex", "stage", "nu", "d2_marginal", "nis_conditional", "_reserved")] == [
        0, 4, 8, 24, 32, 40]


def test_library_exports_the_consistency_calls():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    names = ("ekf_set_consistency", "ekf_get_consistency", "ekf_get_innovations", "ekf_get_consistency_totals",
             "ekf_reset_consistency_totals")
    for name in names:
        assert hasattr(lib, name) and name in engine.ABI, name
    n = C.c_int(-1)
    assert lib.ekf_set_consistency(None, 1) == 1  # EKF_ERR_INVALID_ARG: no engine
    assert lib.ekf_get_consistency(None, None, 0, C.byref(n)) == 1
    assert lib.ekf_get_innovations(None, 0, None, 0, C.byref(n)) == 1
    assert lib.ekf_get_consistency_totals(None, None, None, None) == 1
    assert lib.ekf_reset_consistency_totals(None) == 1
    for name in ("set_consistency", "consistency", "innovations", "consistency_totals", "reset_consistency_totals"):
        assert callable(getattr(engine.EkfEngine, name)), name
