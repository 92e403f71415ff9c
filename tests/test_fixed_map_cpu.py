"""The fixed-map (Schmidt-Kalman) update's numpy reference (tests/fixed_map_ref.py) against the reference
of the full update it is a restriction of, and against the properties that define it.  CPU only.

Inputs, per (N, M) = (12, 8), (50, 35), (170, 160) -- n = 85, 313, 1033 state columns and m = 16, 70, 320 measurement rows --
from default_rng(N): P = (I + A) diag(d^2) (I + A)' with A = 0.05 N(0, 1) and d^2 = |diag SyntheticSequence(N, 1).P0| + 1e-12
(the scales of a real map: 1e-12 velocities beside unit inverse depths); feature i < M measured by rows 2i, 2i + 1 of 19 entries
50 N(0, 1) on the 13 camera columns and the feature's 6; residual 0.5 N(0, 1); R = I.

  (a) the strip and x13 are those of external_update_ref EXACTLY (same operations in the same order); the rest of P and
      feature_pos are the input
  (b) the result is the Joseph form (I - K~ H) P (I - K~ H)' + K~ R K~' with the map rows of the optimal gain zeroed
  (c) it is never smaller than the full update's result: lambda_min(P_fixed - P_full) >= 0
  (d) an asymmetric map block keeps its bits
(b) and (c) to parity_metric.F64_TOL max|P|: both sides are fp64 evaluations of the same quantity in different orders."""
import numpy as np
import pytest

import external_update_ref as xr
import fixed_map_ref as fm
from openekfmonoslam_amd.synth import SyntheticSequence
from parity_metric import F64_TOL

CASES = [(12, 8), (50, 35), (170, 160)]


def make_inputs(N, M):
    rng = np.random.default_rng(N)
    seq = SyntheticSequence(N, 1)
    n = 13 + 6 * N
    A = 0.05 * rng.standard_normal((n, n))
    d2 = np.abs(np.diag(seq.P0)) + 1e-12
    IA = np.eye(n) + A
    P = (IA * d2) @ IA.T
    covpos = 13 + 6 * np.arange(N)
    row_start, col, val = [0], [], []
    for i in range(M):
        for _ in range(2):
            col += list(range(13)) + list(range(covpos[i], covpos[i] + 6))
            val += list(50.0 * rng.standard_normal(19))
            row_start.append(len(col))
    rows = (np.array(row_start, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val))
    residual = 0.5 * rng.standard_normal(2 * M)
    return dict(x=seq.x13, fp=seq.feature_pos, t=seq.feature_type, c=covpos, P=P, rows=rows, residual=residual, R=np.eye(2 * M), rng=rng)


@pytest.fixture(scope="module", params=CASES, ids=[f"N{N}-M{M}" for N, M in CASES])
def case(request):
    N, M = request.param
    i = make_inputs(N, M)
    fixed = fm.fixed_map_update_ref(i["x"], i["fp"], i["t"], i["c"], i["P"], i["rows"], i["residual"], i["R"], np.float64)
    full = xr.external_update_ref(i["x"], i["fp"], i["t"], i["c"], i["P"], *i["rows"], i["residual"], i["R"], 0.0, np.float64)
    assert fixed["status"] == full["status"] == "applied"
    return i, fixed, full


def test_strip_and_camera_state_are_the_full_updates(case):
    i, fixed, full = case
    n = len(i["P"])
    strip = fm.strip_mask(n)
    np.testing.assert_array_equal(fixed["P"][strip], full["P"][strip])
    np.testing.assert_array_equal(fixed["P_downdated"][strip], full["P_downdated"][strip])
    np.testing.assert_array_equal(fixed["x13"], full["x13"])
    np.testing.assert_array_equal(fixed["strip_bound"][3:7], full["strip_bound"][3:7])
    assert fixed["nis"] == full["nis"] and np.array_equal(fixed["z"], full["z"])
    np.testing.assert_array_equal(fixed["P"][~strip], i["P"][~strip])
    np.testing.assert_array_equal(fixed["feature_pos"], np.asarray(i["fp"]).reshape(-1, 6))
    assert np.any(full["feature_pos"] != fixed["feature_pos"])  # (the full update does move the map)
    np.testing.assert_array_equal(fixed["P"][:13, :13], fixed["P"][:13, :13].T)
    np.testing.assert_array_equal(fixed["P"][:13], fixed["P"][:, :13].T)


def dense_H(rows, n):
    row_start, col, val = rows
    H = np.zeros((len(row_start) - 1, n))
    for r in range(len(H)):
        H[r, col[row_start[r]:row_start[r + 1]]] = val[row_start[r]:row_start[r + 1]]
    return H


def test_result_is_the_joseph_form_with_the_map_gain_zeroed(case):
    i, fixed, _ = case
    n = len(i["P"])
    Ps = 0.5 * i["P"] + 0.5 * i["P"].T
    H = dense_H(i["rows"], n)
    S = H @ Ps @ H.T + i["R"]
    K = np.linalg.solve(S, H @ Ps).T
    K[13:] = 0.0
    IKH = np.eye(n) - K @ H
    joseph = IKH @ Ps @ IKH.T + K @ i["R"] @ K.T
    err = np.abs(fixed["P_downdated"] - joseph).max() / np.abs(Ps).max()
    print(f"n = {n}, m = {len(H)}: |P_fixed - Joseph| / max|P| = {err:.2e}")
    assert err <= F64_TOL


def test_never_smaller_than_the_full_update(case):
    i, fixed, full = case
    Ps = 0.5 * i["P"] + 0.5 * i["P"].T
    D = fixed["P_downdated"] - full["P_downdated"]
    lam = np.linalg.eigvalsh(0.5 * (D + D.T)).min() / np.abs(Ps).max()
    print(f"n = {len(Ps)}: lambda_min(P_fixed - P_full) / max|P| = {lam:.2e}")
    assert lam >= -F64_TOL
    assert np.linalg.eigvalsh(0.5 * (D + D.T)).max() > 0.0  # (and it is larger somewhere: the map was not updated)


def test_asymmetric_map_block_keeps_its_bits(case):
    i, _, _ = case
    rng = np.random.default_rng(7)
    # off by a part in 1e9 above the diagonal: S = (H P) H' + R is formed from the rows of P as stored and stays positive definite
    P = i["P"] * (1.0 + 1e-9 * np.triu(rng.standard_normal(i["P"].shape), 1))
    assert np.any(P[13:, 13:] != P[13:, 13:].T)
    got = fm.fixed_map_update_ref(i["x"], i["fp"], i["t"], i["c"], P, i["rows"], i["residual"], i["R"], np.float32)
    assert got["status"] == "applied"
    np.testing.assert_array_equal(got["P"][13:, 13:], P[13:, 13:])
    np.testing.assert_array_equal(got["P"][:13], got["P"][:, :13].T)  # the strip comes out symmetric all the same
    assert np.all(got["P"][:13] == got["P"][:13].astype(np.float32))  # ... and rounded to the storage type


def test_vectorised_path_agrees_with_the_loops(case):
    i, fixed, _ = case
    got = fm.fixed_map_update_ref(i["x"], i["fp"], i["t"], i["c"], i["P"], i["rows"], i["residual"], i["R"], np.float64, vectorised=True)
    scale = np.abs(i["P"]).max()
    assert np.abs(got["P"] - fixed["P"]).max() <= F64_TOL * scale
    assert np.abs(got["x13"] - fixed["x13"]).max() <= F64_TOL * max(1.0, np.abs(fixed["x13"]).max())
    assert abs(got["nis"] - fixed["nis"]) <= F64_TOL * fixed["nis"]
    # ... and the 13-row form of the result is the same numbers
    rows13 = fm.fixed_map_update_ref(i["x"], i["fp"], i["t"], i["c"], i["P"], i["rows"], i["residual"], i["R"], np.float64, strip_only=True)
    np.testing.assert_array_equal(rows13["P_downdated"], fixed["P_downdated"][:13])
    assert np.abs(rows13["P"] - fixed["P"][:13]).max() <= 1e-15 * scale
    assert np.abs(rows13["strip_bound"][3:7] - fixed["strip_bound"][3:7]).max() <= 1e-15 * scale
    np.testing.assert_array_equal(rows13["x13"], fixed["x13"])
