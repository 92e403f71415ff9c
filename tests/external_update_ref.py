"""numpy restatement of the external measurement update (ekf_update_external) from what the engine
exports: (x13, feature_pos, feature_type, covpos, P) and the call's own arguments.  TEST INFRASTRUCTURE (numpy only).

It is the oracle's update_algorithmic followed by the tail of orc_update (oracle/ekf_oracle.c) with a general H given by
sparse rows over state indices, everything in fp64:

  A = H P                     A[i, :] = sum_k val_k P[col_k, :], k in CSR order, from the rows of P as stored
  S = A H' + R                S[i, j] = sum_k A[i, col_jk] val_jk + R[i, j] for i <= j, mirrored; lower Cholesky factor L by columns;
                              a pivot that is not > 0: "not_pd", nothing changes
  z = inv(L) residual, nis = z'z, B = inv(L) A, dx = B'z       (gate_nis > 0 and not nis <= gate_nis: "gated", nothing changes)
  x += dx where |dx| > EKF_DELTA; J = normalizeQuaternionJacobian(q) from the un-normalised q; q /= |q|
  P <- (0.5 P + 0.5 P') - sum_k B[k, :]' B[k, :], k ascending, once per pair i <= j, mirrored      -> rounded to `storage`
  P <- D P D', D = diag(I3, J, I) (normalizeCovariance on rows / columns 3..6)                      -> rounded to `storage`

`storage` (np.float64 / np.float32) rounds where the engine rounds an fp32-stored covariance."""
import numpy as np

EKF_DELTA = 1.0e-12
FEATURE_INVERSE_DEPTH = 2


def csr_of(H):
    """(row_start, col, val) of the non-zeros of a dense [m, n] matrix"""
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    nz = [np.flatnonzero(r) for r in H]
    row_start = np.cumsum([0] + [len(k) for k in nz]).astype(np.int32)
    return row_start, np.concatenate(nz).astype(np.int32), np.concatenate([r[k] for r, k in zip(H, nz)])


def quat_norm_jacobian(q):
    r, x, y, z = q
    nrm = np.sqrt(r * r + x * x + y * y + z * z)
    a = 1.0 / (nrm * nrm * nrm)
    M = np.array([[x * x + y * y + z * z, -r * x, -r * y, -r * z],
                  [-x * r, r * r + y * y + z * z, -x * y, -x * z],
                  [-y * r, -y * x, r * r + x * x + z * z, -y * z],
                  [-z * r, -z * x, -z * y, r * r + x * x + y * y]])
    return nrm, M * a


def cholesky_lower(S):
    """L by columns in the oracle's order, or None when a pivot is not > 0"""
    m = len(S)
    L = np.zeros((m, m))
    for j in range(m):
        d = S[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            s = S[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    return L


def mirror_upper(M):
    return np.triu(M) + np.triu(M, 1).T


def normalize_covariance(P, J):
    """D P D' on rows / columns 3..6, the five disjoint blocks of EKF/Update.cpp:64-85"""
    out = P.copy()
    out[0:3, 3:7] = P[0:3, 3:7] @ J.T
    out[3:7, 0:3] = J @ P[3:7, 0:3]
    out[3:7, 3:7] = mirror_upper((J @ P[3:7, 3:7]) @ J.T)
    out[3:7, 7:] = J @ P[3:7, 7:]
    out[7:, 3:7] = P[7:, 3:7] @ J.T
    return out


def normalize_bound(P, J):
    """the same products with every term replaced by its absolute value: what an error of the rounded inputs of the strip
    entries is scaled by (entries outside rows / columns 3..6: |P|)"""
    out = np.abs(P)
    out[3:7, :] = np.abs(J) @ out[3:7, :]
    out[:, 3:7] = out[:, 3:7] @ np.abs(J).T
    return out


def external_update_ref(x13, feature_pos, feature_type, covpos, P, row_start, col, val, residual, R, gate_nis=0.0,
                        storage=np.float64):
    """-> dict(status = "applied" | "gated" | "not_pd", nis, z, x13, feature_pos, P, P_downdated, strip_bound); the inputs are not
    modified"""
    x = np.array(x13, dtype=np.float64)
    fp = np.array(feature_pos, dtype=np.float64).reshape(-1, 6)
    P = np.array(P, dtype=np.float64)
    n = len(P)
    row_start = np.asarray(row_start, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    residual = np.atleast_1d(np.asarray(residual, dtype=np.float64))
    m = len(row_start) - 1
    R = np.asarray(R, dtype=np.float64).reshape(m, m)
    out = {"status": "applied", "nis": 0.0, "z": np.zeros(m), "x13": x, "feature_pos": fp, "P": P, "P_downdated": P,
           "strip_bound": np.abs(P)}
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
    L = cholesky_lower(S)
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
    if gate_nis > 0.0 and not nis <= gate_nis:
        out["status"] = "gated"
        return out
    dx = np.zeros(n)
    for k in range(m):
        dx += B[k] * z[k]
    dx = np.where(np.abs(dx) > EKF_DELTA, dx, 0.0)
    x = x + dx[:13]
    fp = fp.copy()
    for f in range(len(fp)):
        d = 6 if int(feature_type[f]) == FEATURE_INVERSE_DEPTH else 3
        fp[f, :d] += dx[covpos[f]:covpos[f] + d]
    nrm, J = quat_norm_jacobian(x[3:7])
    x[3:7] = x[3:7] / nrm
    P6 = 0.5 * P + 0.5 * P.T
    BB = np.zeros((n, n))
    for k in range(m):
        BB += np.outer(B[k], B[k])
    P6 = mirror_upper(P6 - BB).astype(storage).astype(np.float64)
    out["P_downdated"] = P6  # before the normalisation: what "the diagonal does not grow" is a statement about
    out["strip_bound"] = normalize_bound(P6, J)
    out["P"] = normalize_covariance(P6, J).astype(storage).astype(np.float64)
    out["x13"], out["feature_pos"] = x, fp
    return out


def visual_rows(preds, Hs, Hf, matches, feature_type, covpos):
    """The engine's own camera measurement as external rows: for match i (predictions and Jacobians aligned to the matches)
    rows 2i, 2i + 1 hold Hs on columns 0..12 and Hf on the feature's columns (13 + d entries, zeros included), and the
    residual is the innovation with the reference's dead-band (EKF/Update.cpp:125-135).  -> (row_start, col, val), residual"""
    row_start, col, val, res = [0], [], [], []
    for i, (p, m) in enumerate(zip(preds, matches)):
        f = int(m["featureIndex"])
        assert f == int(p["featureIndex"])
        d = 6 if int(feature_type[f]) == FEATURE_INVERSE_DEPTH else 3
        for r in range(2):
            col += list(range(13)) + list(range(int(covpos[f]), int(covpos[f]) + d))
            val += list(Hs[i][r][:13]) + list(Hf[i][r][:d])
            row_start.append(len(col))
            nu = float(m["imagePos"][r]) - float(p["imagePos"][r])
            res.append(nu if abs(nu) > EKF_DELTA else 0.0)
    return (np.array(row_start, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val)), np.array(res)
