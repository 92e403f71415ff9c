"""numpy restatement of the fixed-map (Schmidt-Kalman) camera update (ekf_update_fixed_map) from what the
engine exports: (x13, feature_pos, feature_type, covpos, P) and the measurement as sparse rows.  TEST INFRASTRUCTURE (numpy only).

It is external_update_ref.external_update_ref restricted to the camera's strip -- the same helpers, the same order of
operations and the same rounding points, everything in fp64:

  A = H P, S = A H' + R, L, z = inv(L) residual, B = inv(L) A                      exactly as there
  dx_c = sum_k B[k, 0:13] z[k], k ascending;  x13 += dx_c where |dx_c| > EKF_DELTA;  J from the un-normalised q;  q /= |q|
  strip: P[i, j] <- (0.5 P + 0.5 P')[i, j] - sum_k B[k, i] B[k, j] for i < 13, i <= j, mirrored to P[j, i]   -> rounded to `storage`
  P <- D P D', D = diag(I3, J, I): rows / columns 3..6 only, all of them inside the strip                    -> rounded to `storage`
  P[13:, 13:] and the feature parameters are the inputs' (not symmetrised, not rounded again)

`vectorised=True` forms S, L, z and B with numpy's matrix routines instead of the Python loops (updates of thousands of rows: the
loop Cholesky is O(m^3) interpreted operations); the results then agree with the loops to rounding, not bit for bit."""
import numpy as np

import external_update_ref as xr


def fixed_map_update_ref(x13, feature_pos, feature_type, covpos, P, rows, residual, R, storage=np.float64, vectorised=False,
                         strip_only=False):
    """rows = (row_start, col, val) as external_update_ref takes them.  -> dict(status = "applied" | "not_pd", nis, z, x13,
    feature_pos, P, P_downdated, strip_bound); the inputs are not modified.  strip_only (maps of thousands of features: no n x n
    temporaries): P, P_downdated and strip_bound hold the camera's 13 rows [13, n] instead of the whole matrix"""
    x = np.array(x13, dtype=np.float64)
    fp = np.array(feature_pos, dtype=np.float64).reshape(-1, 6)
    P = np.asarray(P, dtype=np.float64) if strip_only else np.array(P, dtype=np.float64)
    n = len(P)
    row_start, col, val = rows
    row_start = np.asarray(row_start, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    residual = np.atleast_1d(np.asarray(residual, dtype=np.float64))
    m = len(row_start) - 1
    R = np.asarray(R, dtype=np.float64).reshape(m, m)
    out = {"status": "applied", "nis": 0.0, "z": np.zeros(m), "x13": x, "feature_pos": fp, "P": P, "P_downdated": P,
           "strip_bound": np.abs(P)}
    if vectorised:
        H = np.zeros((m, n))
        for i in range(m):
            H[i, col[row_start[i]:row_start[i + 1]]] = val[row_start[i]:row_start[i + 1]]
        A = H @ P
        S = xr.mirror_upper(A @ H.T + R)
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            out["status"] = "not_pd"
            return out
        V = np.linalg.solve(L, np.eye(m))
        z = V @ residual
        B = V @ A
    else:
        A = np.zeros((m, n))
        for i in range(m):
            for k in range(row_start[i], row_start[i + 1]):
                A[i] += val[k] * P[col[k]]
        S = np.zeros((m, m))
        for i in range(m):
            for j in range(i, m):
                s = 0.0
                for k in range(row_start[j], row_start[j + 1]):
                    s += A[i, col[k]] * val[k]
                S[i, j] = S[j, i] = s + R[i, j]
        L = xr.cholesky_lower(S)
        if L is None:
            out["status"] = "not_pd"
            return out
        z = np.zeros(m)
        B = np.zeros((m, n))
        for i in range(m):
            zi = residual[i]
            b = A[i].copy()
            for k in range(i):
                zi -= L[i, k] * z[k]
                b -= L[i, k] * B[k]
            z[i] = zi / L[i, i]
            B[i] = b * (1.0 / L[i, i])
    nis = 0.0
    for i in range(m):
        nis += z[i] * z[i]
    out["nis"], out["z"] = nis, z
    dx = np.zeros(13)
    for k in range(m):
        dx += B[k, :13] * z[k]
    dx = np.where(np.abs(dx) > xr.EKF_DELTA, dx, 0.0)
    x = x + dx
    nrm, J = xr.quat_norm_jacobian(x[3:7])
    x[3:7] = x[3:7] / nrm
    # the camera's rows of 0.5 (P + P') - B'B: every pair i <= j once, the 13 x 13 block mirrored from its upper triangle
    strip = 0.5 * P[:13] + 0.5 * P[:, :13].T
    BB = np.zeros((13, n))
    for k in range(m):
        BB += np.outer(B[k, :13], B[k])
    strip = strip - BB
    strip[:, :13] = xr.mirror_upper(strip[:, :13])
    strip = strip.astype(storage).astype(np.float64)
    if strip_only:
        # normalizeCovariance on the 13 rows: the 13 x 13 block by the helper, the columns behind it by J alone
        bound = np.abs(strip)
        bound[:, :13] = xr.normalize_bound(strip[:, :13], J)
        bound[3:7, 13:] = np.abs(J) @ np.abs(strip[3:7, 13:])
        Pn = strip.copy()
        Pn[:, :13] = xr.normalize_covariance(strip[:, :13], J)
        Pn[3:7, 13:] = J @ strip[3:7, 13:]
        out["P_downdated"], out["strip_bound"], out["P"] = strip, bound, Pn.astype(storage).astype(np.float64)
        out["x13"] = x
        return out
    P6 = P.copy()
    P6[:13] = strip
    P6[:, :13] = strip.T
    out["P_downdated"] = P6
    out["strip_bound"] = xr.normalize_bound(P6, J)
    # normalizeCovariance touches rows / columns 3..6 alone: the map block passes through it unread
    Pn = xr.normalize_covariance(P6, J).astype(storage).astype(np.float64)
    Pn[13:, 13:] = P[13:, 13:]
    out["P"] = Pn
    out["x13"] = x
    return out


def strip_mask(n):
    """True on rows and columns 0..12"""
    s = np.zeros((n, n), dtype=bool)
    s[:13, :] = s[:, :13] = True
    return s
