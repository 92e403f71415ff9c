"""The dt-parametrised prediction reference (tests/predict_dt_ref.py) without a GPU: at dt = 1 it is predict_ref value for value; its
F(dt) is the derivative of the state transition (central finite differences in longdouble, so the reference is not only a
restatement of the kernel: a dropped factor of dt shows at 1e-3 or more); the two small-angle tests act each on its own in the two
combinations a dt != 1 makes reachable; and the frame-interval calls are declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import predict_dt_ref as pdr
import predict_ref as pr

LD = pr.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ekf_set_frame_interval", "ekf_get_frame_interval", "ekf_predict_dt", "ekf_set_staged_intervals", "ekf_predict_camera_ahead")


@pytest.mark.parametrize("omega_zero", [False, True])
def test_dt_one_is_predict_ref(omega_zero):
    s = pr.scene_for_n(13 + 258, omega_zero=omega_zero)
    old, new = pr.predict_F(s.x13, s.par), pdr.predict_F(s.x13, s.par, 1.0)
    for name, a, b in zip(("F", "Fabs", "GQG", "GQGabs", "x"), old, new):
        assert a.dtype == b.dtype == LD, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    old, new = pr.predict_cov_ref(s.x13, s.P0, s.par), pdr.predict_cov_ref(s.x13, s.P0, s.par, 1.0)
    assert sorted(old) == sorted(new)
    for name in old:
        np.testing.assert_array_equal(old[name][0], new[name][0], err_msg=name)
        # the same abs-evaluated sums behind the tolerances: only the recounted K differs
        k_old, k_new = (pr.K_CORNER, pdr.K_CORNER) if name == "corner" else (pr.K_STRIP, pdr.K_STRIP)
        np.testing.assert_allclose((old[name][1] / k_old).astype(np.float64), (new[name][1] / k_new).astype(np.float64), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(pdr.state_ref(s.x13, 1.0)[0], old_x := pr.predict_F(s.x13, s.par)[4])
    assert old_x.dtype == LD


@pytest.mark.parametrize("dt", [0.37, 1.0, 2.5])
def test_F_is_the_derivative_of_the_transition(dt):
    s = pr.scene_for_n(16)
    F = pdr.predict_F(s.x13, s.par, dt)[0]
    x = np.asarray(s.x13, dtype=np.float64).astype(LD)
    h = LD(1e-6)
    FD = np.zeros((13, 13), LD)
    for j in range(13):
        e = np.zeros(13, LD)
        e[j] = h
        FD[:, j] = (pdr.transition(x + e, dt) - pdr.transition(x - e, dt)) / (2 * h)
    err = float(np.abs(F - FD).max())
    print(f"prediction over dt: F against finite differences, dt {dt}: max |F - FD| = {err:.3g}")
    assert err <= 1e-11
    # (what the bound is to catch: the same F with the dt of its position block dropped is off by |dt - 1|, of its quaternion block by more than 1e-3)
    assert dt == 1.0 or np.abs(pdr.predict_F(s.x13, s.par, 1.0)[0] - FD).max() >= 1e-3


def _x_with_omega(w):
    x = np.array(pr.scene_for_n(16).x13, dtype=np.float64)
    x[10:13] = w
    return x


def test_small_w_dt_with_w_above_the_threshold():
    """w = (3e-16, 0, 0), dt = 0.5: |w dt| = 1.5e-16 < eps <= |w_x|.  The first test alone acts: the rotation quaternion is the
    identity (q is carried over, the quaternion block of F is I), and the second does not: the angular-velocity diagonal of F
    stays 1 and the quaternion-by-omega block of F and G is Qm D(dt)."""
    s = pr.scene_for_n(16)
    x = _x_with_omega([3e-16, 0.0, 0.0])
    dt = 0.5
    assert abs(x[10]) * dt < pr.EKF_EPSILON <= abs(x[10])
    F, _, GQG, _, xp = pdr.predict_F(x, s.par, dt)
    np.testing.assert_array_equal(F[3:7, 3:7], np.eye(4))
    np.testing.assert_array_equal(xp[3:7], x[3:7].astype(LD))
    np.testing.assert_array_equal(xp[0:3], x[0:3].astype(LD) + x[7:10].astype(LD) * LD(dt))
    np.testing.assert_array_equal(np.diag(F)[10:13], np.ones(3))
    assert np.abs(F[3:7, 10:13]).max() > 0.1  # d q / d w ~ (dt / 2) Qm[:, 1:]
    q = x[3:7].astype(LD)
    Qm = np.array([[q[0], -q[1], -q[2], -q[3]], [q[1], q[0], -q[3], q[2]], [q[2], q[3], q[0], -q[1]], [q[3], -q[2], q[1], q[0]]], LD)
    np.testing.assert_allclose((F[3:7, 10:13] / LD(dt / 2)).astype(np.float64), Qm[:, 1:].astype(np.float64), rtol=0, atol=1e-15)
    an = LD(s.par.angularAccelSD) ** 2 * LD(dt) ** 2
    assert (np.diag(GQG)[3:7] > 0).all() and abs(float(np.trace(GQG[3:7, 3:7]) / (3 * an * LD(dt / 2) ** 2)) - 1) < 1e-12


def test_w_below_the_threshold_with_w_dt_above_it():
    """w = (1.5e-16, 0, 0), dt = 2.5: every |w_i| < eps <= |w dt| = 3.75e-16.  The second test alone acts: F[10+i][10+i] = 0 and the
    quaternion blocks of F's omega columns and of G are zero, and the first does not: the rotation quaternion is quat(w dt), not the
    identity."""
    s = pr.scene_for_n(16)
    x = _x_with_omega([1.5e-16, 0.0, 0.0])
    dt = 2.5
    assert abs(x[10]) < pr.EKF_EPSILON <= abs(x[10]) * dt
    F, _, GQG, _, xp = pdr.predict_F(x, s.par, dt)
    np.testing.assert_array_equal(np.diag(F)[10:13], np.zeros(3))
    np.testing.assert_array_equal(F[3:7, 10:13], np.zeros((4, 3)))
    np.testing.assert_array_equal(GQG[3:7, :], np.zeros((4, 13)))
    half = LD(x[10]) * LD(dt) / 2
    assert abs(F[4, 3] / np.sin(half) - 1) < 1e-18 and F[3, 3] == np.cos(half)  # quat(w dt): sin(|w dt| / 2) on the x axis
    assert np.abs(xp[3:7] - x[3:7].astype(LD)).max() > 0
    ln, an = (LD(sd) ** 2 * LD(dt) ** 2 for sd in (s.par.linearAccelSD, s.par.angularAccelSD))
    np.testing.assert_allclose(np.diag(GQG)[7:13].astype(np.float64), np.array([ln] * 3 + [an] * 3, dtype=np.float64), rtol=1e-15)


def test_exact_zero_w_over_a_long_interval():
    s = pr.scene_for_n(16)
    x = _x_with_omega([0.0, 0.0, 0.0])
    F, _, GQG, _, xp = pdr.predict_F(x, s.par, 2.5)
    np.testing.assert_array_equal(F[3:7, 3:7], np.eye(4))
    np.testing.assert_array_equal(np.diag(F)[10:13], np.zeros(3))
    np.testing.assert_array_equal(F[0:3, 7:10], 2.5 * np.eye(3))
    np.testing.assert_array_equal(xp[3:7], x[3:7].astype(LD))
    ln = LD(s.par.linearAccelSD) ** 2 * LD(2.5) ** 2
    np.testing.assert_allclose(np.diag(GQG)[0:3].astype(np.float64), float(ln * LD(2.5) ** 2), rtol=1e-15)  # G[r, .] = dt I


def test_one_step_of_two_is_not_two_steps_of_one():
    """the velocity impulse is drawn once per prediction: two unit steps add 5 SD^2 to the position variance, one step over 2 adds
    16 SD^2 -- while the state and the product of the two F agree with the long step's (the model is linear in r and v)"""
    s = pr.scene_for_n(16)
    x = _x_with_omega([0.0, 0.0, 0.0])
    F1, _, Q1, _, x1 = pdr.predict_F(x, s.par, 1.0)
    F1b, _, Q1b, _, x2 = pdr.predict_F(x1.astype(np.float64), s.par, 1.0)
    F2, _, Q2, _, x2d = pdr.predict_F(x, s.par, 2.0)
    np.testing.assert_allclose(x2.astype(np.float64), x2d.astype(np.float64), rtol=0, atol=1e-15)
    np.testing.assert_allclose((F1b @ F1)[:3, :].astype(np.float64), F2[:3, :].astype(np.float64), rtol=0, atol=1e-15)
    two = F1b @ Q1 @ F1b.T + Q1b
    ln = float(s.par.linearAccelSD) ** 2
    assert abs(float(two[0, 0]) / (5 * ln) - 1) < 1e-12 and abs(float(Q2[0, 0]) / (16 * ln) - 1) < 1e-12


def test_header_abi_and_binding_carry_the_interval_calls():
    from openekfmonoslam_amd import engine

    header = open(os.path.join(ROOT, "include", "ekf_engine.h")).read()
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    d = C.c_double(-1.0)
    for rc in (lib.ekf_set_frame_interval(None, 1.0), lib.ekf_get_frame_interval(None, C.byref(d)), lib.ekf_predict_dt(None, 1.0),
               lib.ekf_set_staged_intervals(None, 0, None), lib.ekf_predict_camera_ahead(None, 1.0, None, None)):
        assert rc == 1  # EKF_ERR_INVALID_ARG: no engine
    for name in ("set_frame_interval", "frame_interval", "predict", "set_staged_intervals", "camera_ahead"):
        assert callable(getattr(engine.EkfEngine, name)), name
