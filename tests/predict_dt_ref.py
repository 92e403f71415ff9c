"""TEST INFRASTRUCTURE ONLY: tests/predict_ref.py's predict_F and predict_cov_ref restated in np.longdouble with the interval dt as a
parameter (k_predict_prepare / motion_model in csrc/kernels_predict.hip), the look-ahead's camera corner
(k_camera_ahead), the state transition itself (for finite differences: the reference is then more than a restatement of the kernel),
and the per-entry tolerances for a general dt.  Scenes, worst_ratio and the sizes come from predict_ref.

At dt = 1 every value returned here is equal to predict_ref's (tests/test_predict_dt_ref_cpu.py); the tolerances are not: an output's
tolerance keeps predict_ref's form

    u_store |ref| + K u64 sum|terms|

with the same "abs" evaluation beside every sum, but K is recounted below as a worst-case first-order bound, rounding by rounding,
for the operations the kernel performs when dt is a run-time number.  Derived, not measured.  u = 2^-53; "n u" below means a
relative error of at most n u against the abs-evaluated expression.

  assumption   |w| dt / 2 <= pi / 4 (asserted): there a relative error e of the argument of sin / cos changes the value by at most e
               relative (x cot x <= 1, x tan x <= 1).  The device's sin / cos are within 2 ulp = 4 u.
  dt / 2, -dt / 2                exact (a halving)
  om = sqrt(w.w)                 3 roundings under the root (one product and two additions on the longest path, all terms >= 0),
                                 halved by the root, + 1: 2.5;  om om: 6;  1 / om, w_a / om: 3.5
  w dt (per component)           1 -- NEW with a general dt;  nw = |w dt|: 1 + 2.5 = 3.5
  arguments nw / 2, om dt / 2    3.5 (om dt: the NEW product; the halving is exact) -- so sin, cos: 4 + 3.5 = 7.5
  quat(w dt), vector part        s w_i / nw: 7.5 + 1 (w_i = w dt) + 1 + 3.5 + 1 = 14;  scalar part cos: 7.5
  D, first row                   (-dt/2) (w_a / om) sh: 3.5 + 1 (NEW: the product with dt / 2 is no longer a halving) + 7.5 + 1 = 13
  D, diagonal                    t1 = (dt/2) w_a w_a / (om om) ch: 2 products (the first NEW) + 6 + 1 + 7.5 + 1 = 17.5
                                 t2 = (1 / om) (1 - c) sh, c = w_a w_a / (om om) (8, and c <= 1): 1 - c against 1 + c: 8 c / (1 + c) + 1
                                 <= 5; 3.5 + 5 + 1 + 7.5 + 1 = 18;  t1 + t2: 18 + 1 = 19
  D, off the diagonal            w_a w_b / (om om): 8;  (dt/2) ch: 8.5 (NEW product);  (1 / om) sh: 12;  their difference against the
                                 sum of the absolute values: 13;  the product: 8 + 13 + 1 = 22
  Qm D                           a 4-term sum of products: + 4
  K_F = 26       an entry of F or G: 22 + 4 (every other entry -- 1, dt, the quaternion block at <= 14 -- is below that)
  K_X = 18       the predicted camera state: q (x) quat(w dt) is a 4-term sum of products with entries at <= 14; r + v dt: 2
  K_STRIP = 40   P[a][j] = sum_b F[a][b] P[b][j]: 13 products + 12 additions (<= 13 u, with or without FMA) + K_F for the entries of
                 F + 1 final rounding
  K_CORNER = 80  (F C) F' + G Q G': two nested 13-term sums, each 13 + K_F, + 1 addition + 1 final rounding.  G Q G' alone: Q =
                 (SD SD dt) dt is 3 roundings (two of them NEW), a 6-term sum of two products each 6 + 1, two entries of G: 10 + 2 K_F
                 = 62, below the 78 of the nested sums.  The look-ahead's corner stores fp64 (u_store = 0): the final rounding is
                 then the addition's, and the same K holds.
"""
import numpy as np

import predict_ref as pr
from predict_ref import EKF_EPSILON, LD, U32, U64  # noqa: F401  (the tests take them from here)

K_F, K_X, K_STRIP, K_CORNER = 26, 18, 40, 80
assert K_STRIP == 13 + K_F + 1 and K_CORNER == 2 * (13 + K_F) + 2 and 10 + 2 * K_F + 1 < K_CORNER


# ------------------------------------------------------------------------------------------------ the state transition
def _rot_quat(w, dt):
    """quat(w dt) with the kernel's first small-angle test: |w dt| < eps -> the identity"""
    wd = w * dt
    nw = np.sqrt(wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2])
    if nw < EKF_EPSILON:
        return np.array([1, 0, 0, 0], LD)
    s = np.sin(nw / LD(2))
    return np.array([np.cos(nw / LD(2)), s * wd[0] / nw, s * wd[1] / nw, s * wd[2] / nw], LD)


def transition(x13, dt):
    """f(x, dt) in longdouble: r + v dt, q (x) quat(w dt), v, w  (StateAndCovariancePrediction.cpp:43-65 with its dt = 1 a parameter)"""
    x = np.asarray(x13).astype(LD)
    dt = LD(dt)
    qw, qx, qy, qz = _rot_quat(x[10:13], dt)
    xp = x.copy()
    xp[0:3] = x[0:3] + x[7:10] * dt
    w1, x1, y1, z1 = x[3:7]
    xp[3] = w1 * qw - x1 * qx - y1 * qy - z1 * qz
    xp[4] = w1 * qx + x1 * qw + y1 * qz - z1 * qy
    xp[5] = w1 * qy - x1 * qz + y1 * qw + z1 * qx
    xp[6] = w1 * qz + x1 * qy - y1 * qx + z1 * qw
    return xp


def state_ref(x13, dt):
    """-> (predicted camera state, tolerance), longdouble [13]"""
    x = np.asarray(x13, dtype=np.float64).astype(LD)
    xp = transition(x, dt)
    qr = np.abs(_rot_quat(x[10:13], LD(dt)))
    a = np.abs(x)
    mag = a.copy()
    mag[0:3] = a[0:3] + a[7:10] * LD(dt)
    mag[3:7] = np.array([a[3] * qr[0] + a[4] * qr[1] + a[5] * qr[2] + a[6] * qr[3], a[3] * qr[1] + a[4] * qr[0] + a[5] * qr[3] + a[6] * qr[2],
                         a[3] * qr[2] + a[4] * qr[3] + a[5] * qr[0] + a[6] * qr[1], a[3] * qr[3] + a[4] * qr[2] + a[5] * qr[1] + a[6] * qr[0]], LD)
    return xp, K_X * U64 * mag


# ------------------------------------------------------------------------------------------------ F, G Q G', predicted state
def predict_F(x13, par, dt):
    """-> F, Fabs, GQG, GQGabs (13 x 13, longdouble) and the predicted camera state x (13, longdouble) over the interval dt.
    The two small-angle tests act each on its own: |w dt| < eps makes the rotation quaternion the identity; every |w_i| < eps zeroes
    F[10+i][10+i] and the quaternion block of G."""
    x = np.asarray(x13, dtype=np.float64).astype(LD)
    dt = LD(dt)
    two = LD(2)
    F = np.zeros((13, 13), LD)
    for i in range(13):
        F[i, i] = 1
    for i in range(3):
        F[i, i + 7] = dt
    qw, qx, qy, qz = _rot_quat(x[10:13], dt)
    F[3:7, 3:7] = np.array([[qw, -qx, -qy, -qz], [qx, qw, qz, -qy], [qy, -qz, qw, qx], [qz, qy, -qx, qw]], LD)
    Fabs = np.abs(F)
    G = np.zeros((13, 6), LD)
    Gabs = np.zeros((13, 6), LD)
    if all(abs(x[10 + i]) < EKF_EPSILON for i in range(3)):
        for i in range(3):
            F[10 + i, 10 + i] = 0
            Fabs[10 + i, 10 + i] = 0
    else:
        om = np.sqrt(x[10] * x[10] + x[11] * x[11] + x[12] * x[12])
        assert om * dt / two <= np.arctan(LD(1)), "the tolerance count assumes |w| dt / 2 <= pi / 4"
        q = x[3:7]
        Qm = np.array([[q[0], -q[1], -q[2], -q[3]], [q[1], q[0], -q[3], q[2]], [q[2], q[3], q[0], -q[1]], [q[3], -q[2], q[1], q[0]]], LD)
        sh, ch = np.sin(om * dt / two), np.cos(om * dt / two)
        D = np.zeros((4, 3), LD)
        Dabs = np.zeros((4, 3), LD)
        for a in range(3):
            wa = x[10 + a]
            D[0, a] = (-dt / two) * (wa / om) * sh
            Dabs[0, a] = abs(D[0, a])
            for b in range(3):
                wb = x[10 + b]
                if a == b:
                    t1 = (dt / two) * wa * wa / (om * om) * ch
                    c = wa * wa / (om * om)
                    D[1 + a, b] = t1 + (1 / om) * (1 - c) * sh
                    Dabs[1 + a, b] = abs(t1) + (1 / om) * (1 + c) * abs(sh)
                else:
                    D[1 + a, b] = (wa * wb / (om * om)) * ((dt / two) * ch - (1 / om) * sh)
                    Dabs[1 + a, b] = abs(wa * wb / (om * om)) * (abs((dt / two) * ch) + abs((1 / om) * sh))
        QD, QDabs = Qm @ D, np.abs(Qm) @ Dabs
        F[3:7, 10:13] = QD
        Fabs[3:7, 10:13] = QDabs
        G[3:7, 3:6] = QD
        Gabs[3:7, 3:6] = QDabs
    for i in range(3):
        G[i + 7, i] = G[i + 10, i + 3] = 1
        G[i, i] = dt
    Gabs = np.maximum(Gabs, np.abs(G))
    ln = LD(par.linearAccelSD) * LD(par.linearAccelSD) * dt * dt
    an = LD(par.angularAccelSD) * LD(par.angularAccelSD) * dt * dt
    Q = np.diag(np.array([ln, ln, ln, an, an, an], LD))
    GQG, GQGabs = G @ Q @ G.T, Gabs @ Q @ Gabs.T
    return F, Fabs, GQG, GQGabs, transition(x, dt)


def predict_cov_ref(x13, P, par, dt, u_store=0.0):
    """P before the prediction (as stored) -> dict of (ref, tol) longdouble pairs for the corner [13, 13], the row strip
    [13, n - 13] and the column strip [n - 13, 13] of the covariance predicted over dt."""
    F, Fabs, GQG, GQGabs, _ = predict_F(x13, par, dt)
    P = np.asarray(P, dtype=np.float64)
    C = P[:13, :13].astype(LD)
    top = P[:13, 13:].astype(LD)
    left = P[13:, :13].astype(LD)
    out = {}
    ref = F @ C @ F.T + GQG
    out["corner"] = (ref, u_store * np.abs(ref) + K_CORNER * U64 * (Fabs @ np.abs(C) @ Fabs.T + GQGabs))
    ref = F @ top
    out["row strip"] = (ref, u_store * np.abs(ref) + K_STRIP * U64 * (Fabs @ np.abs(top)))
    ref = left @ F.T
    out["column strip"] = (ref, u_store * np.abs(ref) + K_STRIP * U64 * (np.abs(left) @ Fabs.T))
    return out


def camera_ahead_ref(x13, P_corner, par, tau):
    """the look-ahead: (x_ref, x_tol) [13] and (corner_ref, corner_tol) [13, 13] at horizon tau from the state and the camera corner
    of P as stored; the device answers in fp64, so u_store = 0"""
    C = np.zeros((13, 13))
    C[:, :] = np.asarray(P_corner, dtype=np.float64)[:13, :13]
    return state_ref(x13, tau), predict_cov_ref(x13, C, par, tau, 0.0)["corner"]


worst_ratio = pr.worst_ratio
