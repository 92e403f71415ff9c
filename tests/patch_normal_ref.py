"""numpy fp64 restatement of the patch-normal estimator and of the warp that uses its estimate (DESIGN.md section 4.9,
k_ncc_normal / k_ncc_warp).  This file is the definition; the kernel follows it operation by operation, the constants
are those of openekfmonoslam_amd/csrc/patch_normal.h.

A feature's patch is a small plane through its world point X.  Its normal is kept as a slope (p, q) in the axes of the camera
that captured the feature, n = R(q0) (p, q, -1) / |(p, q, -1)|, with a symmetric 2 x 2 information matrix (l00, l01, l11).
The rule of section 4.6 (the plane faces the capturing camera) is the point p = -h0/h2, q = -h1/h2, h = R(q0)' (X - r0).

One estimator step aligns the stored source patches to the current frame around an anchor pixel: every sum below runs in
pixel order (np.cumsum is sequential), then over the levels 0, 1, 2."""
import numpy as np

import template_warp_ref as tw
from openekfmonoslam_amd.synth import quat_to_rot

T, R, S, SR = tw.T, tw.R, tw.S, tw.SR
# ---- the constants of patch_normal.h ----------------------------------------------------------------------------------
FD_STEP = 2.0 ** -10   # central-difference step in p and q
S_MIN = 2.0 ** -8      # floor of the residual's standard deviation per pixel (normalised vectors: unit norm over 121 pixels)
STEP_MAX = 0.25        # longest step in (p, q) per update
PRIOR_INFO = 1.0       # information of the first update's prior: identity times this
MIN_SS = 0.5           # a vector whose sum of squared deviations is not above this is constant (bytes: exactly constant)
SLOPES = ((0.0, 0.0), (FD_STEP, 0.0), (-FD_STEP, 0.0), (0.0, FD_STEP), (0.0, -FD_STEP))


def seqsum(v):
    """sum over the last axis, strictly left to right"""
    return np.cumsum(np.asarray(v, dtype=np.float64), axis=-1)[..., -1]


def rule_pq(r0, q0, X):
    """the slope of section 4.6's rule: the plane through X that faces the capturing camera"""
    R0 = quat_to_rot(np.asarray(q0, dtype=np.float64))
    w = np.asarray(X, dtype=np.float64) - np.asarray(r0, dtype=np.float64)
    h = [R0[0, i] * w[0] + R0[1, i] * w[1] + R0[2, i] * w[2] for i in range(3)]
    return np.array([-h[0] / h[2], -h[1] / h[2]])


def normal_of(q0, pq):
    """unit normal in world axes of the slope pq"""
    R0 = quat_to_rot(np.asarray(q0, dtype=np.float64))
    p, q = float(pq[0]), float(pq[1])
    nrm = np.sqrt(p * p + q * q + 1.0)
    return np.array([(R0[i, 0] * p + R0[i, 1] * q - R0[i, 2]) / nrm for i in range(3)])


def _distort(cam, u, v):
    """device_math.h's distort, operation by operation"""
    pdx, pdy = u - cam.cx, v - cam.cy
    mx, my = cam.dx * pdx, cam.dy * pdy
    d2 = mx * mx + my * my
    ru = np.sqrt(d2)
    rd = ru / (1.0 + cam.k1 * d2 + cam.k2 * d2 * d2)
    for _ in range(10):
        r2 = rd * rd
        r3 = r2 * rd
        r4 = r2 * r2
        r5 = r4 * rd
        f = rd + cam.k1 * r3 + cam.k2 * r5 - ru
        fp = 1 + 3 * cam.k1 * r2 + 5 * cam.k2 * r4
        rd = rd - f / fp
    rd2 = rd * rd
    d = 1.0 + cam.k1 * rd2 + cam.k2 * (rd2 * rd2)
    return np.stack([cam.cx + pdx / d, cam.cy + pdy / d], axis=-1)


def _to_source(cam, r, Rq, r0, R0, n, nXr, px, py):
    """steps 2-4 of section 4.6 for level-0 positions (px, py): the level-0 position in the capture frame and the validity.
    Sums of three products run left to right, as in the kernel."""
    pdx, pdy = px - cam.cx, py - cam.cy
    mx, my = cam.dx * pdx, cam.dy * pdy
    rd2 = mx * mx + my * my
    f = 1.0 + cam.k1 * rd2 + cam.k2 * rd2 * rd2
    hx, hy = pdx * f / cam.fx, pdy * f / cam.fy
    d = [Rq[i, 0] * hx + Rq[i, 1] * hy + Rq[i, 2] * 1.0 for i in range(3)]
    nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = nXr / nd
        w = [r[i] + lam * d[i] - r0[i] for i in range(3)]
        h = [R0[0, i] * w[0] + R0[1, i] * w[1] + R0[2, i] * w[2] for i in range(3)]
        s = _distort(cam, cam.cx + cam.fx * h[0] / h[2], cam.cy + cam.fy * h[1] / h[2])
    return s, (nd < 0) & (lam > 0) & (h[2] > 0)


def _bilinear(src_l, sx, sy):
    x0 = np.minimum(np.floor(sx).astype(np.int64), S - 2)
    y0 = np.minimum(np.floor(sy).astype(np.int64), S - 2)
    ax, ay = sx - x0, sy - y0
    p = src_l.astype(np.float64)
    top = (1.0 - ax) * p[y0, x0] + ax * p[y0, x0 + 1]
    bot = (1.0 - ax) * p[y0 + 1, x0] + ax * p[y0 + 1, x0 + 1]
    return (1.0 - ay) * top + ay * bot


def warp_templates(cam, x13, fp, ftype, r0, q0, uv0, src, pred_uv, stored=None, pq=None):
    """tw.warp_templates with the normal of the slope pq in steps 3-4 (pq None: no estimate, the rule's own arithmetic).
    Same return values."""
    if pq is None or src is None:
        return tw.warp_templates(cam, x13, fp, ftype, r0, q0, uv0, src, pred_uv, stored)
    out = np.zeros((3, T, T), dtype=np.uint8) if stored is None else np.array(stored, dtype=np.uint8).reshape(3, T, T)
    fb, dist, coords = np.ones(3, dtype=bool), np.full((3, T, T), np.inf), np.full((3, T, T, 2), np.nan)
    x13 = np.asarray(x13, dtype=np.float64)
    r, Rq = x13[0:3], quat_to_rot(x13[3:7])
    r0 = np.asarray(r0, dtype=np.float64)
    R0 = quat_to_rot(np.asarray(q0, dtype=np.float64))
    X = tw.feature_xyz(fp, ftype)
    n = normal_of(q0, pq)
    nXr = float(n[0] * (X[0] - r[0]) + n[1] * (X[1] - r[1]) + n[2] * (X[2] - r[2]))
    dy, dx = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    for l in range(3):
        sc = float(1 << l)
        px = (tw.to_level(pred_uv[0], l) + dx + 0.5) * sc - 0.5
        py = (tw.to_level(pred_uv[1], l) + dy + 0.5) * sc - 0.5
        s, ok = _to_source(cam, r, Rq, r0, R0, n, nXr, px, py)
        sx = (s[..., 0] + 0.5) / sc - 0.5 - (tw.to_level(uv0[0], l) - SR)
        sy = (s[..., 1] + 0.5) / sc - 0.5 - (tw.to_level(uv0[1], l) - SR)
        coords[l] = np.stack([sx, sy], axis=-1)
        ok = ok & (sx >= 0) & (sx <= S - 1) & (sy >= 0) & (sy <= S - 1)
        if not ok.all():
            continue
        b = _bilinear(src[l], sx, sy)
        out[l] = np.clip(np.floor(b + 0.5), 0, 255).astype(np.uint8)
        dist[l] = np.abs(b - np.floor(b) - 0.5)
        fb[l] = False
    return out, fb, dist, coords


def _normalised(v):
    """zero mean, unit norm over the last axis; None when the vector is constant"""
    mean = seqsum(v) / float(T * T)
    dev = v - mean
    ss = seqsum(dev * dev)
    if not ss > MIN_SS:
        return None
    return dev / np.sqrt(ss)


def refine(cam, x13, fp, ftype, r0, q0, uv0, src, pyr, anchor, est=None):
    """One estimator step for one feature.  x13: the current camera state; r0, q0, uv0, src: the capture record and the
    uint8 [3, 41, 41] source patches; pyr: the current frame's pyramid; anchor: the match's level-0 pixel, integers;
    est: (pq, info) or None (first update: the rule's slope and PRIOR_INFO times the identity).
    Returns (pq, info, levels used) or None when nothing is written (no level remains or the solve is not finite)."""
    x13 = np.asarray(x13, dtype=np.float64)
    r, Rq = x13[0:3], quat_to_rot(x13[3:7])
    r0 = np.asarray(r0, dtype=np.float64)
    R0 = quat_to_rot(np.asarray(q0, dtype=np.float64))
    X = tw.feature_xyz(fp, ftype)
    if est is None:
        pq, info = rule_pq(r0, q0, X), np.array([PRIOR_INFO, 0.0, PRIOR_INFO])
    else:
        pq, info = np.asarray(est[0], dtype=np.float64), np.asarray(est[1], dtype=np.float64)
    ax, ay = int(anchor[0]), int(anchor[1])
    normals = [normal_of(q0, (pq[0] + dp, pq[1] + dq)) for dp, dq in SLOPES]
    nXrs = [float(n[0] * (X[0] - r[0]) + n[1] * (X[1] - r[1]) + n[2] * (X[2] - r[2])) for n in normals]
    # where the anchor itself lands, per slope (level-0 position in the capture frame)
    anc = [_to_source(cam, r, Rq, r0, R0, n, k, np.array(float(ax)), np.array(float(ay))) for n, k in zip(normals, nXrs)]
    dy, dx = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    dx, dy = dx.ravel(), dy.ravel()
    App = Apq = Aqq = gp = gq = rr = 0.0
    used = []
    for l in range(3):
        sc = float(1 << l)
        cxl, cyl = tw.to_level(ax, l), tw.to_level(ay, l)
        px, py = (cxl + dx + 0.5) * sc - 0.5, (cyl + dy + 0.5) * sc - 0.5
        offx, offy = float(tw.to_level(uv0[0], l) - SR), float(tw.to_level(uv0[1], l) - SR)
        # the source's centre pixel (level 0) in this level's source coordinates: 20 at level 0
        ctrx = (float(tw.to_level(uv0[0], 0)) + 0.5) / sc - 0.5 - offx
        ctry = (float(tw.to_level(uv0[1], 0)) + 0.5) / sc - 0.5 - offy
        hats, good = [], True
        for j in range(5):
            s, ok = _to_source(cam, r, Rq, r0, R0, normals[j], nXrs[j], px, py)
            sa, oka = anc[j]
            sx = ((s[..., 0] + 0.5) / sc - 0.5 - offx) - (((sa[0] + 0.5) / sc - 0.5 - offx) - ctrx)
            sy = ((s[..., 1] + 0.5) / sc - 0.5 - offy) - (((sa[1] + 0.5) / sc - 0.5 - offy) - ctry)
            ok = ok & bool(oka) & (sx >= 0) & (sx <= S - 1) & (sy >= 0) & (sy <= S - 1)
            if not ok.all():
                good = False
                break
            hat = _normalised(_bilinear(src[l], sx, sy))
            if hat is None:
                good = False
                break
            hats.append(hat)
        if not good:
            continue
        meas = _normalised(tw.window(pyr[l], cxl, cyl, R).astype(np.float64).ravel())
        if meas is None:
            continue
        res = meas - hats[0]
        Jp = (hats[1] - hats[2]) * (0.5 / FD_STEP)
        Jq = (hats[3] - hats[4]) * (0.5 / FD_STEP)
        App, Apq, Aqq = App + seqsum(Jp * Jp), Apq + seqsum(Jp * Jq), Aqq + seqsum(Jq * Jq)
        gp, gq, rr = gp + seqsum(Jp * res), gq + seqsum(Jq * res), rr + seqsum(res * res)
        used.append(l)
    if not used:
        return None
    m = float(T * T * len(used))
    s2 = max(rr / (m - 2.0), S_MIN * S_MIN)
    l00, l01, l11 = info[0] + App / s2, info[1] + Apq / s2, info[2] + Aqq / s2
    b0, b1 = gp / s2, gq / s2
    det = l00 * l11 - l01 * l01
    with np.errstate(divide="ignore", invalid="ignore"):
        d0, d1 = np.float64(l11 * b0 - l01 * b1) / det, np.float64(l00 * b1 - l01 * b0) / det
    length = np.sqrt(d0 * d0 + d1 * d1)
    if length > STEP_MAX:
        f = STEP_MAX / length
        d0, d1 = d0 * f, d1 * f
    out = np.array([pq[0] + d0, pq[1] + d1, l00, l01, l11])
    if not (det > 0.0 and np.isfinite(out).all()):
        return None
    return out[:2], out[2:], used


def angle_deg(a, b):
    c = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))
