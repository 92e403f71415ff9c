"""numpy restatement (fp64) of the filter-consistency records (ekf_set_consistency, k_consistency).

For one covariance update with M matches in the update's order and m = 2 M rows:
    nu   the dead-banded innovation: imagePos - predicted distorted pixel, 0 where |.| <= EKF_DELTA (gather_body)
    S    H P H' + pixelErrorX I with P the covariance the update starts from, L its Cholesky factor, z = inv(L) nu
    nis  sum of z_k^2
    c_i  z_2i^2 + z_2i+1^2: conditional on the matches before i in the list; their sum is nis
    d2_i nu_i' inv(S_i) nu_i with S_i the match's own 2 x 2 diagonal block of S (closed-form inverse; 1e300 when det <= 0)

The inputs are what the engine returns: get_state() before the update, feature_layout(), predict_measurements() and the match
list."""
import numpy as np

EKF_DELTA = 1.0e-12
FEATURE_INVERSE_DEPTH = 2


def innovation(image_pos, predicted):
    a = np.asarray(image_pos, dtype=np.float64) - np.asarray(predicted, dtype=np.float64)
    return np.where(np.abs(a) > EKF_DELTA, a, 0.0)


def build_H(n, ftype, covpos, preds, Hs, Hf, matches):
    """H (2M x n) and nu (2M) in match order; preds / Hs (k, 2, 13) / Hf (k, 2, 6) in prediction order.  A depth feature uses
    the first three columns of its Hf."""
    lut = {int(p["featureIndex"]): k for k, p in enumerate(preds)}
    M = len(matches)
    H = np.zeros((2 * M, n))
    nu = np.zeros(2 * M)
    for i, mt in enumerate(matches):
        fi = int(mt["featureIndex"])
        k = lut[fi]
        dim = 6 if int(ftype[fi]) == FEATURE_INVERSE_DEPTH else 3
        H[2 * i : 2 * i + 2, :13] = Hs[k]
        H[2 * i : 2 * i + 2, int(covpos[fi]) : int(covpos[fi]) + dim] = Hf[k][:, :dim]
        nu[2 * i : 2 * i + 2] = innovation(mt["imagePos"], preds[k]["imagePos"])
    return H, nu


def from_S(S, nu):
    """(nis, c [M], d2 [M]) of an SPD S (2M x 2M) and nu (2M)"""
    S = np.asarray(S, dtype=np.float64)
    nu = np.asarray(nu, dtype=np.float64)
    M = len(nu) // 2
    L = np.linalg.cholesky(S)
    z = np.linalg.solve(L, nu)  # (a general solve of a triangular system: forward substitution to rounding)
    z2 = z * z
    c = z2[0::2] + z2[1::2]
    d2 = np.zeros(M)
    for i in range(M):
        s00, s01, s10, s11 = S[2 * i, 2 * i], S[2 * i, 2 * i + 1], S[2 * i + 1, 2 * i], S[2 * i + 1, 2 * i + 1]
        det = s00 * s11 - s01 * s10
        n0, n1 = nu[2 * i], nu[2 * i + 1]
        d2[i] = (n0 * (s11 * n0 - s01 * n1) + n1 * (s00 * n1 - s10 * n0)) / det if det > 0.0 else 1e300
    return float(z2.sum()), c, d2


def reference(P, ftype, covpos, preds, Hs, Hf, matches, pixel_error):
    """-> dict(nis, nu [M, 2], c [M], d2 [M], S) of the update of `matches` from the covariance P"""
    P = np.asarray(P, dtype=np.float64)
    H, nu = build_H(P.shape[0], ftype, covpos, preds, Hs, Hf, matches)
    S = H @ P @ H.T + pixel_error * np.eye(len(nu))
    nis, c, d2 = from_S(S, nu)
    return {"nis": nis, "nu": nu.reshape(-1, 2), "c": c, "d2": d2, "S": S}
