"""numpy restatement of the whole NCC search of matcher mode B (k_ncc_match, and with max_rad=None the wide search of
DESIGN.md section 4.8: k_ncc_wide_classify / k_ncc_wide_coarse / k_ncc_wide_finish).

Inputs are what the public API returns: the three image_level() arrays, a prediction's imagePos and covarianceMatrix,
and the 3 x 11 x 11 template bytes the match compared (match_templates(); the oracle's templates() on the CPU).  The gate
is Oracle.ellipse / Oracle.point_in_ellipse, the key ncc_subpixel_ref.key, the optional fit ncc_subpixel_ref.refine.

max_rad=16 is the default path (the oracle's orc_match_ncc, which test_ncc_wide_cpu.py pins it to); max_rad=None removes
the cap on the coarse radius and is otherwise the same code: the wide search is defined as exactly that."""
import numpy as np

import ncc_subpixel_ref as sp
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE
from template_warp_ref import R, to_level, window

MAXRAD, TILE = 16, 32


class Gate:
    """the integer-axes ellipse of a prediction, as ncc_match_one forms it"""

    def __init__(self, orc, pos, S):
        ax, self.angle = orc.ellipse(S)
        self.orc = orc
        self.aw, self.ah = int(np.rint(ax[0])), int(np.rint(ax[1]))  # lrintf of the float axes
        self.cx, self.cy = float(np.float32(pos[0])), float(np.float32(pos[1]))
        self.major = max(self.aw, self.ah)

    def contains(self, x, y):
        return self.orc.point_in_ellipse(float(np.float32(x)), float(np.float32(y)), self.cx, self.cy, self.aw, self.ah, self.angle)


def match_one(orc, levels, pos, S, tmpl3, max_rad=MAXRAD, subpixel=False):
    """One prediction -> dict: valid, x, y (float32 as the match carries them), bx, by (integer best pixel), key, distance
    (float32), wide (the uncapped coarse radius exceeds 16), ncand (coarse candidates evaluated), best (every coarse
    candidate (x, y) that has the best key), tiles (their 32 x 32 tiles of the candidate box), fitted (axes, bool [2])"""
    g = Gate(orc, pos, S)
    h2, w2 = levels[2].shape
    c2x, c2y = to_level(pos[0], 2), to_level(pos[1], 2)
    rad = (g.major >> 2) + 1
    wide = rad > MAXRAD
    if max_rad is not None:
        rad = min(rad, max_rad)
    rad = min(rad, max(w2, h2))
    x_lo, x_hi = max(c2x - rad, 0), min(c2x + rad, w2 - 1)
    y_lo, y_hi = max(c2y - rad, 0), min(c2y + rad, h2 - 1)
    bx, by, bkey, ncand, best = c2x, c2y, -3.0, 0, []
    for y in range(y_lo, y_hi + 1):  # raster order, strict '>': the first maximum
        for x in range(x_lo, x_hi + 1):
            if not (x == c2x and y == c2y) and not g.contains((x + 0.5) * 4 - 0.5, (y + 0.5) * 4 - 0.5):
                continue
            k = sp.key(window(levels[2], x, y, R), tmpl3[2])
            ncand += 1
            if k > bkey:
                bkey, bx, by, best = k, x, y, [(x, y)]
            elif k == bkey:
                best.append((x, y))
    tiles = sorted({((x - x_lo) // TILE, (y - y_lo) // TILE) for x, y in best})
    for l in (1, 0):  # the 4 x 4 children of the best parent, no gate
        h, w = levels[l].shape
        px, py, bkey = bx, by, -3.0
        for y in range(2 * py - 1, 2 * py + 3):
            for x in range(2 * px - 1, 2 * px + 3):
                if x < 0 or y < 0 or x >= w or y >= h:
                    continue
                k = sp.key(window(levels[l], x, y, R), tmpl3[l])
                if k > bkey:
                    bkey, bx, by = k, x, y
    valid = bool(bkey >= 0.64 and g.contains(bx, by))
    fx, fy, fitted = np.float32(bx), np.float32(by), np.zeros(2, dtype=bool)
    if subpixel:
        fx, fy, fitted[0], fitted[1] = sp.refine(levels[0], tmpl3[0], bx, by)
    dist = np.float32(1.0 - np.sqrt(np.float64(bkey))) if valid else np.float32(0.0)
    return dict(valid=valid, x=fx, y=fy, bx=bx, by=by, key=bkey, distance=dist, wide=wide, ncand=ncand, best=best, tiles=tiles,
                fitted=fitted, major=g.major, minor=min(g.aw, g.ah))


def match_all(orc, levels, preds, tmpl, max_rad=MAXRAD, subpixel=False):
    """Every prediction (PREDICTION_DTYPE records, in slot order); tmpl: uint8 [k, 3, 11, 11], row j for preds[j].
    -> (matches MATCH_DTYPE in prediction order, per-slot dicts, (wide slots, coarse candidates of the wide slots),
    (axes fitted, axes left at the integer) over the matches)"""
    slots = [match_one(orc, levels, p["imagePos"], p["covarianceMatrix"], tmpl[j], max_rad, subpixel) for j, p in enumerate(preds)]
    out = np.zeros(len(preds), dtype=MATCH_DTYPE)
    n = fit = 0
    for p, s in zip(preds, slots):
        if s["valid"]:
            out[n]["featureIndex"], out[n]["keypointIndex"] = p["featureIndex"], -1
            out[n]["imagePos"] = (s["x"], s["y"])
            out[n]["distance"] = s["distance"]
            fit += int(s["fitted"].sum())
            n += 1
    counted = [s for s in slots if s["wide"]] if max_rad is None else []
    return out[:n].copy(), slots, (len(counted), sum(s["ncand"] for s in counted)), (fit, 2 * n - fit) if subpixel else (0, 0)


def assert_matches_equal(got, want, label=""):
    """which features match, the pixel and the float distance: identical"""
    assert len(got) == len(want), (label, len(got), len(want), got["featureIndex"], want["featureIndex"])
    for f in ("featureIndex", "keypointIndex", "imagePos", "distance"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{label}: {f}")


def blurred_noise(h, w, seed):
    """random values, 3 x 3 box-blurred so that windows one pixel apart correlate"""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    return np.rint(sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0).astype(np.uint8)
