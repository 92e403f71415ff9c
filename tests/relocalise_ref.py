"""Reference of the relocalisation (ekf_relocalise): global descriptor match, counter-based triples, P3P,
scoring and selection, in numpy.  This file is the contract of kernels_reloc.hip: the device runs the same steps in the same
order in fp64.  Every floating-point routine takes the dtype it computes in (np.float64, or np.longdouble to measure the
reference's own rounding error).

Conventions: R(q) maps camera axes to world axes (quat_to_rot), r is the camera position, a bearing is the unit vector of an
undistorted pixel in camera axes, and every feature takes part as its world point X.
"""
import math

import numpy as np

MASK64 = (1 << 64) - 1
MAX_HYPOTHESES = 4096
NO_SECOND = 2 ** 31 - 1  # d2 of a feature that saw one keypoint only
BEARING_TOL = 1e-6       # a solution must reproduce its three bearings to this (largest component)
COS_MAX = 1.0 - 1e-12    # two bearings of a triple closer than 1.4e-6 rad count as one: the triple has no solution
CUBIC_POLISH, QUARTIC_POLISH = 3, 4  # Newton steps: fixed counts, no data-dependent loop
FEATURE_DEPTH, FEATURE_INVERSE_DEPTH = 1, 2

DEFAULT_PARAMS = dict(hypotheses=256, min_inliers=6, seed=1, max_distance=48.0, second_best_coef=0.8, inlier_px=3.0,
                      max_rel_depth_sd=0.0, sigma_position=0.05, sigma_angle=0.02, install=0)


# ------------------------------------------------------------------------------------------------------ sampling
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample_triple(seed, h, C):
    """Three distinct candidate indices of hypothesis h (C >= 3): index k is splitmix64(seed + 3 h + k) mod C; an index already
    taken steps to the next one mod C, tested twice against both earlier indices (two steps always suffice)."""
    idx = []
    for k in range(3):
        i = splitmix64((seed + 3 * h + k) & MASK64) % C
        for _ in range(2):
            if i in idx:
                i = (i + 1) % C
        idx.append(i)
    return idx


# ---------------------------------------------------------------------------------------------------- world points
def dir_vec(theta, phi):
    return np.array([math.cos(phi) * math.sin(theta), -math.sin(phi), math.cos(phi) * math.cos(theta)])


def world_points(feature_pos, feature_type, covpos, P, max_rel_depth_sd):
    """X [N,3] and the mask of the features that take part: every depth feature; an inverse-depth feature with rho > 0 and
    (max_rel_depth_sd == 0 or sqrt(P[rho,rho]) / rho <= max_rel_depth_sd)."""
    N = len(feature_type)
    X = np.zeros((N, 3))
    used = np.zeros(N, dtype=bool)
    for f in range(N):
        y = feature_pos[f]
        if feature_type[f] == FEATURE_INVERSE_DEPTH:
            rho = y[5]
            ii = covpos[f] + 5
            with np.errstate(all="ignore"):
                X[f] = y[0:3] + dir_vec(y[3], y[4]) / rho
                used[f] = rho > 0 and (max_rel_depth_sd == 0 or math.sqrt(P[ii, ii]) / rho <= max_rel_depth_sd)
        else:
            X[f] = y[0:3]
            used[f] = True
    return X, used


# --------------------------------------------------------------------------------------------------- global match
_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def hamming_table(feat_desc, kp_desc):
    """[N, K] Hamming distances of 32-byte descriptors."""
    out = np.zeros((len(feat_desc), len(kp_desc)), dtype=np.int32)
    for f in range(len(feat_desc)):
        out[f] = _POP[np.bitwise_xor(kp_desc, feat_desc[f][None, :])].sum(axis=1) if len(kp_desc) else 0
    return out


def global_match(feat_desc, used, kps_xy, kp_desc, max_distance, second_best_coef):
    """Candidate list in ascending feature order: (feature, keypoint, (x, y) as doubles, distance).  d1 = the smallest distance
    over all keypoints (ties to the lower keypoint index), d2 = the smallest over the other keypoints."""
    K = len(kp_desc)
    cands = []
    if K == 0:
        return cands
    D = hamming_table(feat_desc, kp_desc)
    for f in range(len(feat_desc)):
        if not used[f]:
            continue
        k1 = int(np.argmin(D[f]))  # first occurrence of the minimum
        d1 = int(D[f, k1])
        d2 = int(np.delete(D[f], k1).min()) if K > 1 else NO_SECOND
        if d1 <= max_distance and (second_best_coef == 0 or d2 == NO_SECOND or float(d1) < second_best_coef * float(d2)):
            cands.append((f, k1, (float(kps_xy[k1][0]), float(kps_xy[k1][1])), d1))
    return cands


# -------------------------------------------------------------------------------------------------------- bearings
def undistort(cam, u, v, dt=np.float64):
    mx, my = dt(u) - dt(cam.cx), dt(v) - dt(cam.cy)
    dxm, dym = dt(cam.dx) * mx, dt(cam.dy) * my
    rd2 = dxm * dxm + dym * dym
    dist = 1 + dt(cam.k1) * rd2 + dt(cam.k2) * rd2 * rd2
    return dt(cam.cx) + mx * dist, dt(cam.cy) + my * dist


def bearing(cam, u, v, dt=np.float64):
    uu, vu = undistort(cam, u, v, dt)
    b = np.array([(uu - dt(cam.cx)) / dt(cam.fx), (vu - dt(cam.cy)) / dt(cam.fy), dt(1)], dtype=dt)
    return b / np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])


# ------------------------------------------------------------------------------------------------------------ P3P
def _polymul(a, b, dt):
    out = np.zeros(len(a) + len(b) - 1, dtype=dt)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] = out[i + j] + ai * bj
    return out


def quartic_coefficients(a, b, c, ca, cb, cg, dt=np.float64):
    """Ascending coefficients k0..k4 of b (D^2 + N^2 - 2 cg N D) - c q D^2 in v (see the module docstring of DESIGN.md 4.17):
    q = 1 - 2 cb v + v^2, N = (a - c) q + b (1 - v^2), D = 2 b (cg - ca v)."""
    one, two = dt(1), dt(2)
    q = np.array([one, -two * cb, one], dtype=dt)
    Np = np.array([(a - c) + b, -two * cb * (a - c), (a - c) - b], dtype=dt)
    Dp = np.array([two * b * cg, -two * b * ca], dtype=dt)
    D2 = _polymul(Dp, Dp, dt)          # degree 2
    N2 = _polymul(Np, Np, dt)          # degree 4
    ND = _polymul(Np, Dp, dt)          # degree 3
    qD2 = _polymul(q, D2, dt)          # degree 4
    k = np.zeros(5, dtype=dt)
    for i in range(5):
        d2 = D2[i] if i < 3 else dt(0)
        nd = ND[i] if i < 4 else dt(0)
        k[i] = b * (d2 + N2[i] - two * cg * nd) - c * qD2[i]
    return k, q, Np, Dp


def _largest_cubic_root(a2, a1, a0, dt):
    """Largest real root of z^3 + a2 z^2 + a1 z + a0: closed form, then CUBIC_POLISH Newton steps."""
    three, nine = dt(3), dt(9)
    Q = (a2 * a2 - three * a1) / nine
    R = (dt(2) * a2 * a2 * a2 - nine * a2 * a1 + dt(27) * a0) / dt(54)
    Q3 = Q * Q * Q
    if R * R < Q3:
        th = np.arccos(R / np.sqrt(Q3))
        z = -dt(2) * np.sqrt(Q) * np.cos((th + dt(2) * np.arccos(dt(-1))) / three) - a2 / three
    else:
        A = -np.copysign(dt(1), R) * np.cbrt(np.abs(R) + np.sqrt(R * R - Q3))
        B = Q / A if A != 0 else dt(0)
        z = A + B - a2 / three
    for _ in range(CUBIC_POLISH):
        f = ((z + a2) * z + a1) * z + a0
        fp = (three * z + dt(2) * a2) * z + a1
        if fp != 0:
            z = z - f / fp
    return z


def quartic_real_roots(k, dt=np.float64):
    """Real roots of k0 + k1 v + .. + k4 v^4, ascending: Ferrari's factorisation into two quadratics through the largest root of
    the resolvent cubic, then QUARTIC_POLISH Newton steps per root on the monic quartic.  A non-finite anything: no roots."""
    with np.errstate(all="ignore"):
        if not (np.all(np.isfinite(k)) and k[4] != 0):
            return []
        A, B, C, D = k[3] / k[4], k[2] / k[4], k[1] / k[4], k[0] / k[4]
        A2 = A * A
        p = B - dt(3) * A2 / dt(8)
        q = C - A * B / dt(2) + A2 * A / dt(8)
        r = D - A * C / dt(4) + A2 * B / dt(16) - dt(3) * A2 * A2 / dt(256)
        z = _largest_cubic_root(dt(2) * p, p * p - dt(4) * r, -q * q, dt)
        if not np.isfinite(z):
            return []
        if z > 0:
            s = np.sqrt(z)
            qs = q / s
        else:  # biquadratic: y^4 + p y^2 + r
            z = dt(0)
            s = dt(0)
            disc = p * p - dt(4) * r
            if not disc >= 0:
                return []
            qs = np.sqrt(disc)
        t = [(p + z - qs) / dt(2), (p + z + qs) / dt(2)]  # (y^2 + s y + t0)(y^2 - s y + t1)
        lin = [s, -s]
        roots = []
        for m in range(2):
            disc = lin[m] * lin[m] - dt(4) * t[m]
            if not disc >= 0:
                continue
            sq = np.sqrt(disc)
            w = -(lin[m] + np.copysign(sq, lin[m])) / dt(2)  # the root of larger magnitude first, the other from the product
            y0 = w
            y1 = t[m] / w if w != 0 else dt(0)
            roots += [y0 - A / dt(4), y1 - A / dt(4)]
        out = []
        for v in roots:
            for _ in range(QUARTIC_POLISH):
                f = (((v + A) * v + B) * v + C) * v + D
                fp = ((dt(4) * v + dt(3) * A) * v + dt(2) * B) * v + C
                if fp != 0:
                    v = v - f / fp
            if np.isfinite(v):
                out.append(v)
        # insertion sort, stable (the device's fixed network gives the same order)
        for i in range(1, len(out)):
            j = i
            while j > 0 and out[j] < out[j - 1]:
                out[j], out[j - 1] = out[j - 1], out[j]
                j -= 1
        return out


def quat_to_rot(q, dt=np.float64):
    r, x, y, z = q
    return np.array([[r * r + x * x - y * y - z * z, 2 * (x * y - r * z), 2 * (z * x + r * y)],
                     [2 * (x * y + r * z), r * r - x * x + y * y - z * z, 2 * (y * z - r * x)],
                     [2 * (z * x - r * y), 2 * (y * z + r * x), r * r - x * x - y * y + z * z]], dtype=dt)


def rot_to_quat(R, dt=np.float64):
    """q (w x y z) with R(q) = R, normalised, w >= 0: the branch of the largest of (trace, R00, R11, R22), first on ties."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    one, two, quarter = dt(1), dt(2), dt(0.25)
    best, val = 0, tr
    for i in range(3):
        if R[i, i] > val:
            best, val = i + 1, R[i, i]
    if best == 0:
        s = np.sqrt(one + tr) * two
        q = [quarter * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif best == 1:
        s = np.sqrt(one + R[0, 0] - R[1, 1] - R[2, 2]) * two
        q = [(R[2, 1] - R[1, 2]) / s, quarter * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif best == 2:
        s = np.sqrt(one + R[1, 1] - R[0, 0] - R[2, 2]) * two
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, quarter * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(one + R[2, 2] - R[0, 0] - R[1, 1]) * two
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, quarter * s]
    q = np.array(q, dtype=dt)
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return -q if q[0] < 0 else q


def _cross(a, b, dt):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=dt)


def _unit(a):
    return a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _mv(M, v):
    """M v and (below) M' v of a 3 x 3 matrix, summed left to right as the device does."""
    return np.array([M[i, 0] * v[0] + M[i, 1] * v[1] + M[i, 2] * v[2] for i in range(3)], dtype=M.dtype)


def _mtv(M, v):
    return np.array([M[0, i] * v[0] + M[1, i] * v[1] + M[2, i] * v[2] for i in range(3)], dtype=M.dtype)


def _triad(P1, P2, P3, dt):
    """Rows: e1 = unit(P2 - P1), e2 = e3 x e1, e3 = unit(e1 x (P3 - P1))."""
    e1 = _unit(P2 - P1)
    e3 = _unit(_cross(e1, P3 - P1, dt))
    e2 = _cross(e3, e1, dt)
    return np.stack([e1, e2, e3])


def p3p(X, f, dt=np.float64):
    """All poses (r, q) that see world points X[0..2] along unit bearings f[0..2], ordered by ascending v = d3 / d1; at most 4.
    Degenerate or non-finite input returns fewer, never a NaN."""
    X = np.asarray(X, dtype=dt)
    f = np.asarray(f, dtype=dt)
    sols = []
    with np.errstate(all="ignore"):
        d23, d13, d12 = X[1] - X[2], X[0] - X[2], X[0] - X[1]
        a = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2]
        b = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2]
        c = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2]
        ca = f[1, 0] * f[2, 0] + f[1, 1] * f[2, 1] + f[1, 2] * f[2, 2]
        cb = f[0, 0] * f[2, 0] + f[0, 1] * f[2, 1] + f[0, 2] * f[2, 2]
        cg = f[0, 0] * f[1, 0] + f[0, 1] * f[1, 1] + f[0, 2] * f[1, 2]
        if not (ca < COS_MAX and cb < COS_MAX and cg < COS_MAX):  # two bearings coincide (two features on one keypoint), or a NaN
            return sols
        k, qp, Np, Dp = quartic_coefficients(a, b, c, ca, cb, cg, dt)
        G = _triad(X[0], X[1], X[2], dt)
        for v in quartic_real_roots(k, dt):
            qv = (v + qp[1]) * v + qp[0]
            Nv = (Np[2] * v + Np[1]) * v + Np[0]
            Dv = Dp[1] * v + Dp[0]
            u = Nv / Dv
            if not (v > 0 and u > 0 and qv > 0):
                continue
            d1 = np.sqrt(b / qv)
            Y = np.stack([d1 * f[0], (u * d1) * f[1], (v * d1) * f[2]])
            E = _triad(Y[0], Y[1], Y[2], dt)
            # R = sum_k g_k e_k': R e_k = g_k
            R = np.array([[G[0, i] * E[0, j] + G[1, i] * E[1, j] + G[2, i] * E[2, j] for j in range(3)] for i in range(3)], dtype=dt)
            if not np.all(np.isfinite(R)):
                continue
            q = rot_to_quat(R, dt)
            Rq = quat_to_rot(q, dt)
            r = X[0] - _mv(Rq, Y[0])
            if not (np.all(np.isfinite(q)) and np.all(np.isfinite(r))):
                continue
            ok = True
            for i in range(3):
                ci = _mtv(Rq, X[i] - r)
                ci = _unit(ci)
                dev = np.max(np.abs(ci - f[i]))
                if not dev <= BEARING_TOL:
                    ok = False
            if ok:
                sols.append((r, q))
    return sols


# ---------------------------------------------------------------------------------------------------------- score
def inv3(S, dt=np.float64):
    """The adjugate inverse of device_math.h (zeros when the determinant is 0)."""
    S = np.asarray(S, dtype=dt).reshape(9)
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0:
        return np.zeros((3, 3), dtype=dt)
    d = 1 / d
    return np.array([(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
                     (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
                     (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d],
                    dtype=dt).reshape(3, 3)


EKF_PI = 3.14159265


def predict_pixel(cam, r, q, X, dt=np.float64):
    """predict_pixel of device_math.h for world points X [C, 3] (depth features) seen from (r, q): (predicted? [C], distorted
    pixel [C, 2]; the pixel of a point that is not predicted means nothing).  Element by element the operations and their order are
    the device's."""
    X = np.asarray(X, dtype=dt).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Ri = inv3(quat_to_rot(q, dt), dt)
        t = X - np.asarray(r, dtype=dt)[None, :]
        h = [Ri[i, 0] * t[:, 0] + Ri[i, 1] * t[:, 1] + Ri[i, 2] * t[:, 2] for i in range(3)]
        ax = np.arctan2(h[0], h[2]) * dt(180.0) / dt(EKF_PI)
        ay = np.arctan2(h[1], h[2]) * dt(180.0) / dt(EKF_PI)
        avx, avy = dt(cam.angularVisionX), dt(cam.angularVisionY)  # (the filter compares with the whole angle)
        ok = (-avx < ax) & (ax < avx) & (-avy < ay) & (ay < avy)
        u = dt(cam.cx) + (dt(cam.fx) * h[0] / h[2])
        v = dt(cam.cy) + (dt(cam.fy) * h[1] / h[2])
        pdx, pdy = u - dt(cam.cx), v - dt(cam.cy)
        mx, my = dt(cam.dx) * pdx, dt(cam.dy) * pdy
        d2 = mx * mx + my * my
        ru = np.sqrt(d2)
        k1, k2 = dt(cam.k1), dt(cam.k2)
        rd = ru / (1 + k1 * d2 + k2 * d2 * d2)
        for _ in range(10):
            r2 = rd * rd
            r3, r4 = r2 * rd, r2 * r2
            r5 = r4 * rd
            fv = rd + k1 * r3 + k2 * r5 - ru
            fp = 1 + 3 * k1 * r2 + 5 * k2 * r4
            rd = rd - fv / fp
        rd2 = rd * rd
        d = 1 + k1 * rd2 + k2 * rd2 * rd2
        uv = np.stack([dt(cam.cx) + pdx / d, dt(cam.cy) + pdy / d], axis=-1)
        ok = ok & (uv[:, 0] > 0) & (uv[:, 0] < cam.pixelsX) & (uv[:, 1] > 0) & (uv[:, 1] < cam.pixelsY)
        return ok, uv


def score_pose(cam, r, q, Xc, pix, inlier_px, dt=np.float64):
    """(inliers, sum of squared inlier errors added in candidate order, the squared error of every candidate -- inf when it is
    not predicted)."""
    thr2 = dt(inlier_px) * dt(inlier_px)
    ok, uv = predict_pixel(cam, r, q, Xc, dt)
    pix = np.asarray(pix, dtype=dt).reshape(-1, 2)
    with np.errstate(all="ignore"):
        du, dv = pix[:, 0] - uv[:, 0], pix[:, 1] - uv[:, 1]
        e2 = np.where(ok, du * du + dv * dv, dt(np.inf))
    n, sse = 0, dt(0)
    for j in np.flatnonzero(e2 <= thr2):
        n += 1
        sse = sse + e2[j]
    return n, sse, e2


def better(n_a, sse_a, n_b, sse_b):
    """The order of solutions and of hypotheses: more inliers, then the smaller sum; equal keeps the earlier one."""
    return n_a > n_b or (n_a == n_b and sse_a < sse_b)


# ------------------------------------------------------------------------------------------------------- the whole
def relocalise(cam, feature_pos, feature_type, covpos, P, feat_desc, kps_xy, kp_desc, params, dt=np.float64, triples=None):
    """The whole call.  Returns a dict: candidates, hypotheses (one dict per h: cand, n_solutions, inliers, sse, r, q, errs) and
    the result fields of EkfRelocResult (without `installed`)."""
    p = dict(DEFAULT_PARAMS)
    p.update(params)
    X, used = world_points(feature_pos, feature_type, covpos, P, p["max_rel_depth_sd"])
    cands = global_match(feat_desc, used, kps_xy, kp_desc, p["max_distance"], p["second_best_coef"])
    C, H = len(cands), int(p["hypotheses"])
    res = dict(found=0, n_features_used=int(used.sum()), n_candidates=C, n_hypotheses=H, n_valid_hypotheses=0,
               best_hypothesis=-1, n_inliers=0, rms_px=0.0, r=np.zeros(3), q=np.zeros(4), candidates=cands, hypotheses=[],
               inlier_mask=np.zeros(C, dtype=np.uint8))
    if C < 3:
        return res
    Xc = np.array([X[c[0]] for c in cands], dtype=dt)
    pix = [c[2] for c in cands]
    fb = np.stack([bearing(cam, px[0], px[1], dt) for px in pix])
    best = None
    for h in range(H):
        tri = sample_triple(int(p["seed"]), h, C) if triples is None else triples[h]
        sols = p3p(Xc[tri], fb[tri], dt)
        rec = dict(cand=tri, n_solutions=len(sols), inliers=0, sse=dt(0), r=np.zeros(3, dtype=dt), q=np.zeros(4, dtype=dt), errs=None)
        for si, (r, q) in enumerate(sols):
            n, sse, errs = score_pose(cam, r, q, Xc, pix, p["inlier_px"], dt)
            if si == 0 or better(n, sse, rec["inliers"], rec["sse"]):
                rec.update(inliers=n, sse=sse, r=r, q=q, errs=errs)
        res["hypotheses"].append(rec)
        if rec["n_solutions"] > 0:
            res["n_valid_hypotheses"] += 1
            if best is None or better(rec["inliers"], rec["sse"], res["hypotheses"][best]["inliers"], res["hypotheses"][best]["sse"]):
                best = h
    if best is not None:
        b = res["hypotheses"][best]
        res.update(best_hypothesis=best, n_inliers=b["inliers"], r=b["r"], q=b["q"],
                   rms_px=float(np.sqrt(b["sse"] / b["inliers"])) if b["inliers"] > 0 else 0.0,
                   found=int(b["inliers"] >= p["min_inliers"]))
        thr2 = float(p["inlier_px"]) ** 2
        res["inlier_mask"] = (b["errs"] <= thr2).astype(np.uint8)
    return res


def install_covariance(P, par, sigma_position, sigma_angle, storage=np.float64):
    """P after an installed relocalisation: the camera's rows and columns replaced, everything else as it was."""
    P2 = np.array(P, dtype=np.float64, copy=True)
    P2[0:13, :] = 0.0
    P2[:, 0:13] = 0.0
    diag = [sigma_position ** 2] * 3 + [0.25 * sigma_angle ** 2] * 4 + [par.initLinearAccelSD ** 2] * 3 + [par.initAngularAccelSD ** 2] * 3
    for i, d in enumerate(diag):
        P2[i, i] = float(storage(d))
    return P2
