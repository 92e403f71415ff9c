"""numpy restatement of the keypoint detector and the BRIEF-32 descriptor of the image-in descriptor matcher
(kernels_detect.hip: k_kp_detect, k_kp_compact, k_brief).  Integer arithmetic throughout, so the
device must agree bit for bit.  `gray` is the engine's gray level 0 (the image itself for 1-channel frames; the
pyramid's level 0 otherwise, e.g. Oracle.image_level(0))."""
import os
import re

import numpy as np

from openekfmonoslam_amd.ekftypes import KEYPOINT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_H = os.path.join(ROOT, "openekfmonoslam_amd", "csrc", "brief_pattern.h")
BORDER = 16  # DBORDER of kernels_detect.hip
INT64_MAX = np.iinfo(np.int64).max


def brief_pattern(path=PATTERN_H):
    """the (ax, ay, bx, by) pairs of the header the kernel compiles, [256, 4] int"""
    text = open(path).read()
    body = text[text.index("#define EKF_BRIEF_PATTERN"):]
    pairs = re.findall(r"\{\s*(-?\d+),\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\s*\}", body)
    return np.array(pairs, dtype=np.int64)


def threshold(min_response):
    """the integer threshold ekf_detect_new_features / ekf_detect_keypoints derive from the double of the ABI"""
    if min_response >= 9.2e18:
        return INT64_MAX
    return 0 if min_response <= 0 else int(min_response)


def _box(a, k):
    """sums over every k x k window of a (valid windows only), exact integers"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), axis=0), axis=1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def response(gray):
    """R = 16 (Sxx Syy - Sxy^2) - (Sxx + Syy)^2 at every pixel: 3x3 Sobel gradients of the clamped gray level, their
    products summed over the 5x5 window centred on the pixel (int64 [h, w])"""
    p = np.pad(np.asarray(gray, dtype=np.int64), 3, mode="edge")  # clamped reads
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, hh, k = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    ix = (c + 2 * f + k) - (a + 2 * d + g)  # at pixels -2 .. w + 1
    iy = (g + 2 * hh + k) - (a + 2 * b + c)
    sxx, syy, sxy = _box(ix * ix, 5), _box(iy * iy, 5), _box(ix * iy, 5)
    tr = sxx + syy
    return 16 * (sxx * syy - sxy * sxy) - tr * tr


def keypoint_flags(gray, min_response, R=None):
    """bool [h, w]: border, threshold and 5x5 non-maximum suppression (strictly above the earlier pixels of the window in
    raster order, >= the later ones)"""
    R = response(gray) if R is None else R
    h, w = R.shape
    ok = R >= threshold(min_response)
    ok[:BORDER, :] = False
    ok[h - BORDER :, :] = False
    ok[:, :BORDER] = False
    ok[:, w - BORDER :] = False
    Rp = np.pad(R, 2, mode="constant", constant_values=np.iinfo(np.int64).min)
    for dy in range(5):
        for dx in range(5):
            if dy == 2 and dx == 2:
                continue
            q = Rp[dy : dy + h, dx : dx + w]
            ok &= (R > q) if (dy, dx) < (2, 2) else (R >= q)
    return ok


def keypoints(gray, min_response):
    """the whole frame's keypoints in raster order (y, then x) as KEYPOINT_DTYPE"""
    ys, xs = np.nonzero(keypoint_flags(gray, min_response))
    out = np.zeros(len(xs), dtype=KEYPOINT_DTYPE)
    out["x"], out["y"] = xs, ys
    return out


def describe(gray, uv, pattern=None):
    """BRIEF-32 at pixel positions uv [k, 2] (centre floor(u + 0.5), floor(v + 0.5)) -> uint8 [k, 32].  S = 9x9 box sum
    of the gray level with clamped reads; test i sets bit 7 - i % 8 of byte i / 8 when S(c + a_i) < S(c + b_i)."""
    pattern = brief_pattern() if pattern is None else pattern
    gray = np.asarray(gray)
    h, w = gray.shape
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    if len(uv) == 0:
        return np.zeros((0, 32), dtype=np.uint8)
    cx = np.floor(uv[:, 0] + 0.5).astype(np.int64)
    cy = np.floor(uv[:, 1] + 0.5).astype(np.int64)
    reach = int(np.abs(pattern).max()) + 4
    out_x = int(max(0, -cx.min(), cx.max() - (w - 1)))
    out_y = int(max(0, -cy.min(), cy.max() - (h - 1)))
    pad = reach + max(out_x, out_y) + 1
    S = _box(np.pad(gray.astype(np.int64), pad, mode="edge"), 9)  # S[y, x] = box centred on padded pixel (y + 4, x + 4)
    off = pad - 4

    def s_at(x, y):
        return S[y + off, x + off]

    sa = s_at(cx[:, None] + pattern[None, :, 0], cy[:, None] + pattern[None, :, 1])
    sb = s_at(cx[:, None] + pattern[None, :, 2], cy[:, None] + pattern[None, :, 3])
    return np.packbits(sa < sb, axis=1)  # bitorder "big": test 8 b is the most significant bit of byte b


def keypoints_and_descriptors(gray, min_response):
    kps = keypoints(gray, min_response)
    uv = np.stack([kps["x"], kps["y"]], axis=1).astype(np.float64)
    return kps, describe(gray, uv)


def cell_maxima(gray, min_response, cell=16):
    """the detector of ekf_detect_new_features without a mask: best pixel (R, ties: raster order) of every 16x16 cell
    inside the border with R >= max(threshold, 0), in cell order -> [k, 2] float (x, y)"""
    R = response(gray)
    h, w = R.shape
    Rm = np.full_like(R, -1)
    Rm[BORDER : h - BORDER, BORDER : w - BORDER] = R[BORDER : h - BORDER, BORDER : w - BORDER]
    thr = threshold(min_response)
    out = []
    for cy in range(h // cell):
        for cx in range(w // cell):
            blk = Rm[cy * cell : (cy + 1) * cell, cx * cell : (cx + 1) * cell]
            i = int(np.argmax(blk))
            r = blk.flat[i]
            if r >= 0 and r >= thr:
                out.append((cx * cell + i % cell, cy * cell + i // cell))
    return np.array(out, dtype=np.float64).reshape(-1, 2)
