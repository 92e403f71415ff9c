"""numpy fp64 restatement of the template warp (k_ncc_warp / k_ncc_warp_capture): the source
patches a capture keeps, and the 11 x 11 template of every pyramid level re-rendered from the current pose.  One
feature per call, vectorised over the 3 x 121 template pixels.  Also the pyramid and ZNCC helpers the tests share."""
import numpy as np

from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH
from openekfmonoslam_amd.synth import distort, quat_to_rot

T, R, S, SR = 11, 5, 41, 20  # template side / radius, source side / radius


def to_level(u, l):
    return int(np.floor((u + 0.5) / (1 << l)))


def pyramid(gray):
    """3-level pyramid of a gray uint8 frame: 2 x 2 means, rounded (k_ncc_down)"""
    out = [np.ascontiguousarray(gray, dtype=np.uint8)]
    for _ in range(2):
        a = out[-1].astype(np.int32)
        h, w = a.shape[0] // 2, a.shape[1] // 2
        a = a[: 2 * h, : 2 * w]
        out.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def window(level, cx, cy, radius):
    """(2 radius + 1)^2 pixels of one pyramid level around (cx, cy), reads clamped to the frame (pyr_at)"""
    h, w = level.shape
    ys = np.clip(np.arange(cy - radius, cy + radius + 1), 0, h - 1)
    xs = np.clip(np.arange(cx - radius, cx + radius + 1), 0, w - 1)
    return level[np.ix_(ys, xs)]


def source_patches(pyr, uv):
    """what a capture at pixel uv keeps with the mode on: uint8 [3, 41, 41]"""
    return np.stack([window(pyr[l], to_level(uv[0], l), to_level(uv[1], l), SR) for l in range(3)])


def stored_templates(pyr, uv):
    """what k_ncc_capture keeps: uint8 [3, 11, 11]"""
    return np.stack([window(pyr[l], to_level(uv[0], l), to_level(uv[1], l), R) for l in range(3)])


def feature_xyz(fp, ftype):
    """world point of a feature (`xyz` of DESIGN.md 9.1)"""
    fp = np.asarray(fp, dtype=np.float64)
    if ftype != FEATURE_INVERSE_DEPTH:
        return fp[:3].copy()
    theta, phi, rho = fp[3], fp[4], fp[5]
    m = np.array([np.cos(phi) * np.sin(theta), -np.sin(phi), np.cos(phi) * np.cos(theta)])
    return fp[:3] + m / rho


def zncc(a, b):
    a = a.astype(np.float64).ravel() - a.mean()
    b = b.astype(np.float64).ravel() - b.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / den) if den > 0 else -1.0


def warp_templates(cam, x13, fp, ftype, r0, q0, uv0, src, pred_uv, stored=None):
    """The warp of one feature.  cam: EkfCamera; x13: current camera state; fp / ftype: the feature's parameters and
    kind; r0, q0, uv0: capture pose and pixel; src: uint8 [3, 41, 41] or None (no source patch); pred_uv: the
    prediction; stored: uint8 [3, 11, 11] used by levels that fall back (zeros when not given).
    Returns (bytes uint8 [3, 11, 11], fall-back flags bool [3], |b - nearest (k + 1/2)| float [3, 11, 11] of the
    unrounded bilinear values, +inf on levels that fell back, source coordinates float [3, 11, 11, 2])."""
    out = np.zeros((3, T, T), dtype=np.uint8) if stored is None else np.array(stored, dtype=np.uint8).reshape(3, T, T)
    fb = np.ones(3, dtype=bool)
    dist = np.full((3, T, T), np.inf)
    coords = np.full((3, T, T, 2), np.nan)
    if src is None:
        return out, fb, dist, coords
    x13 = np.asarray(x13, dtype=np.float64)
    r, Rq = x13[0:3], quat_to_rot(x13[3:7])
    r0 = np.asarray(r0, dtype=np.float64)
    R0 = quat_to_rot(np.asarray(q0, dtype=np.float64))
    X = feature_xyz(fp, ftype)
    n = (r0 - X) / np.linalg.norm(r0 - X)
    nXr = float(n @ (X - r))
    dy, dx = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    for l in range(3):
        sc = float(1 << l)
        px = (to_level(pred_uv[0], l) + dx + 0.5) * sc - 0.5
        py = (to_level(pred_uv[1], l) + dy + 0.5) * sc - 0.5
        pdx, pdy = px - cam.cx, py - cam.cy
        mx, my = cam.dx * pdx, cam.dy * pdy
        rd2 = mx * mx + my * my
        f = 1.0 + cam.k1 * rd2 + cam.k2 * rd2 * rd2
        hc = np.stack([pdx * f / cam.fx, pdy * f / cam.fy, np.ones_like(px)], axis=-1)
        d = hc @ Rq.T
        nd = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = nXr / nd
            Y = r + lam[..., None] * d
            h = (Y - r0) @ R0  # R0' (Y - r0)
            s = distort(cam, np.stack([cam.cx + cam.fx * h[..., 0] / h[..., 2], cam.cy + cam.fy * h[..., 1] / h[..., 2]], axis=-1))
        sx = (s[..., 0] + 0.5) / sc - 0.5 - (to_level(uv0[0], l) - SR)
        sy = (s[..., 1] + 0.5) / sc - 0.5 - (to_level(uv0[1], l) - SR)
        coords[l] = np.stack([sx, sy], axis=-1)
        ok = (nd < 0) & (lam > 0) & (h[..., 2] > 0) & (sx >= 0) & (sx <= S - 1) & (sy >= 0) & (sy <= S - 1)
        if not ok.all():
            continue
        x0 = np.minimum(np.floor(sx).astype(np.int64), S - 2)
        y0 = np.minimum(np.floor(sy).astype(np.int64), S - 2)
        ax, ay = sx - x0, sy - y0
        p = src[l].astype(np.float64)
        top = (1.0 - ax) * p[y0, x0] + ax * p[y0, x0 + 1]
        bot = (1.0 - ax) * p[y0 + 1, x0] + ax * p[y0 + 1, x0 + 1]
        b = (1.0 - ay) * top + ay * bot
        out[l] = np.clip(np.floor(b + 0.5), 0, 255).astype(np.uint8)
        dist[l] = np.abs(b - np.floor(b) - 0.5)
        fb[l] = False
    return out, fb, dist, coords
