"""numpy restatement of the map export (ekf_get_map_points) from what the engine already
exports: (x13, feature_pos, feature_type, covpos, P).

With r = x[0:3], q = x[3:7], R(q), m(theta, phi), a feature's parameters y (6 for inverse depth, 3 for depth),
pos = covpos, d = 6 or 3:

  X       = y[0:3] + m(y[3], y[4]) / y[5]          (inverse depth)      X = y[0:3]  (depth)
  cov     = Jw P[pos:pos+d, pos:pos+d] Jw'         Jw = dX/dy (3 x d), the identity for a depth feature
  cam     = R(q)' (X - r)
  cov_cam = Jc Z Jc'                               Z = P on rows/columns {0..6} u {pos..pos+d-1},
                                                   Jc = [ -R' | d(R(q)'a)/dq at a = X - r | R' Jw ]   (3 x (7+d))
  linearity = computeLinearityIndex (EKF/MapManagement.cpp:312-341); 1e300 for a depth feature

Besides each value the reference returns what a tolerance is scaled by: for a covariance the bound matrix
B = |J| |Z| |J|' (entrywise absolute values), for a point the same expression with every term replaced by its
absolute value (a sum of n products evaluated in floating point is off by at most ~n u times that).
"""
import numpy as np

FEATURE_DEPTH = 1
FEATURE_INVERSE_DEPTH = 2


def quat_to_rot(q):
    r, x, y, z = q
    return np.array([
        [r * r + x * x - y * y - z * z, 2 * (x * y - r * z), 2 * (z * x + r * y)],
        [2 * (x * y + r * z), r * r - x * x + y * y - z * z, 2 * (y * z - r * x)],
        [2 * (z * x - r * y), 2 * (y * z + r * x), r * r - x * x - y * y + z * z]])


def quat_to_rot_abs(q):
    """quat_to_rot with every term replaced by its absolute value"""
    r, x, y, z = np.abs(q)
    s = r * r + x * x + y * y + z * z
    return np.array([[s, 2 * (x * y + r * z), 2 * (z * x + r * y)],
                     [2 * (x * y + r * z), s, 2 * (y * z + r * x)],
                     [2 * (z * x + r * y), 2 * (y * z + r * x), s]])


def dir_vec(theta, phi):
    return np.array([np.cos(phi) * np.sin(theta), -np.sin(phi), np.cos(phi) * np.cos(theta)])


def jac_rot_by_quat(q, a):
    """d(R(q) a)/dq, 3 x 4, the four components of q independent (EKF/CommonFunctions.cpp:87-145)"""
    q0, qx, qy, qz = 2 * np.asarray(q, dtype=np.float64)
    x, y, z = a
    return np.array([
        [q0 * x - qz * y + qy * z, qx * x + qy * y + qz * z, -qy * x + qx * y + q0 * z, -qz * x - q0 * y + qx * z],
        [qz * x + q0 * y - qx * z, qy * x - qx * y - q0 * z, qx * x + qy * y + qz * z, q0 * x - qz * y + qy * z],
        [-qy * x + qx * y + q0 * z, qz * x + q0 * y - qx * z, -q0 * x + qz * y - qy * z, qx * x + qy * y + qz * z]])


def world_point(y, ftype):
    """X(y) and Jw = dX/dy (3 x d)"""
    y = np.asarray(y, dtype=np.float64)
    if ftype != FEATURE_INVERSE_DEPTH:
        return y[:3].copy(), np.eye(3)
    theta, phi, rho = y[3], y[4], y[5]
    m = dir_vec(theta, phi)
    J = np.zeros((3, 6))
    J[:, :3] = np.eye(3)
    J[:, 3] = [np.cos(phi) * np.cos(theta) / rho, 0.0, -np.cos(phi) * np.sin(theta) / rho]
    J[:, 4] = [-np.sin(phi) * np.sin(theta) / rho, -np.cos(phi) / rho, -np.sin(phi) * np.cos(theta) / rho]
    J[:, 5] = -m / (rho * rho)
    return y[:3] + m / rho, J


def camera_point(r, q, y, ftype):
    """cam(r, q, y) and Jc = d cam / d(r, q, y) (3 x (7+d))"""
    X, Jw = world_point(y, ftype)
    R = quat_to_rot(q)
    a = X - np.asarray(r, dtype=np.float64)
    qc = np.array([q[0], -q[1], -q[2], -q[3]])
    Jq = jac_rot_by_quat(qc, a)  # R(q)' = R(conj q); chain rule through the conjugate: vector columns negated
    Jq[:, 1:] = -Jq[:, 1:]
    return R.T @ a, np.hstack([-R.T, Jq, R.T @ Jw])


def linearity_index(r, y, var_rho):
    sigma = np.sqrt(var_rho) / (y[5] * y[5])
    X = y[:3] + dir_vec(y[3], y[4]) / y[5]
    tc, tf = X - r, X - y[:3]
    df, dc = np.sqrt(tf @ tf), np.sqrt(tc @ tc)
    return 4.0 * sigma * ((tc @ tf) / (df * dc)) / dc


def map_points_ref(x13, feature_pos, feature_type, covpos, P):
    """dict of arrays over the N features: xyz, xyz_bound, cov, B, cam, cam_bound, cov_cam, B_cam, linearity, and the
    Jacobians as lists (Jw, Jc)."""
    x13 = np.asarray(x13, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    r, q = x13[:3], x13[3:7]
    N = len(feature_type)
    out = {k: np.zeros((N, 3)) for k in ("xyz", "xyz_bound", "cam", "cam_bound")}
    out.update({k: np.zeros((N, 3, 3)) for k in ("cov", "B", "cov_cam", "B_cam")})
    out["linearity"] = np.full(N, 1e300)
    out["Jw"], out["Jc"] = [], []
    R_abs = quat_to_rot_abs(q)
    for i in range(N):
        t, pos = int(feature_type[i]), int(covpos[i])
        d = 6 if t == FEATURE_INVERSE_DEPTH else 3
        y = np.asarray(feature_pos[i], dtype=np.float64)[:d]
        X, Jw = world_point(y, t)
        cam, Jc = camera_point(r, q, y, t)
        idx = np.r_[0:7, pos:pos + d]
        Z = P[np.ix_(idx, idx)]
        Pf = P[pos:pos + d, pos:pos + d]
        out["xyz"][i] = X
        out["xyz_bound"][i] = np.abs(y[:3]) + (np.abs(dir_vec(y[3], y[4]) / y[5]) if d == 6 else 0.0)
        out["cov"][i] = Jw @ Pf @ Jw.T if d == 6 else Pf
        out["B"][i] = np.abs(Jw) @ np.abs(Pf) @ np.abs(Jw).T
        out["cam"][i] = cam
        out["cam_bound"][i] = R_abs.T @ (out["xyz_bound"][i] + np.abs(r))
        out["cov_cam"][i] = Jc @ Z @ Jc.T
        out["B_cam"][i] = np.abs(Jc) @ np.abs(Z) @ np.abs(Jc).T
        if d == 6:
            out["linearity"][i] = linearity_index(r, y, P[pos + 5, pos + 5])
        out["Jw"].append(Jw)
        out["Jc"].append(Jc)
    return out
