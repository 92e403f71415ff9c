"""numpy restatement of the NCC matcher's distinctiveness test (ekf_set_ncc_distinct,
k_ncc_match<.., true>, k_ncc_wide_coarse<true>, k_ncc_wide_finish<.., true>), on top of the restatement of the search
itself (tests/ncc_wide_ref.py, which stays the definition of the best place, the acceptance test and the distance).

For one prediction, after the search as it is:
  1. coarse rival: the slot's level-2 candidates (coarse_scan: the candidate rule of ncc_wide_ref.match_one) without those
     within EXCL = 2 pixels (Chebyshev) of the coarse best B2; the largest key, first in raster order; none if nothing is
     left or the key is negative;
  2. refined rival: levels 1 and 0 from that pixel by the 4 x 4 children rule against the same templates; none if its
     level-0 key is negative or its pixel lies outside the gate;
  3. test: d1 = float32(1 - sqrt(k0)), d2 = float32(1 - sqrt(r0)); an accepted match with a rival is kept when
     float64(d1) < float64(d2) * coef, strictly.
States: 0 = no valid match, 1 = valid and no rival, 2 = rival and kept, 3 = rival and rejected (leaves the match list)."""
import numpy as np

import ncc_subpixel_ref as sp
import ncc_wide_ref as wr
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE, NCC_RIVAL_DTYPE
from template_warp_ref import R, to_level, window

EXCL = 2  # coarse pixels around the coarse best that belong to its own lobe: a 5 x 5 block


def coarse_scan(g, levels, pos, tmpl3, max_rad=wr.MAXRAD):
    """the slot's level-2 candidates [(x, y, key)] in raster order and the predicted coarse pixel"""
    h2, w2 = levels[2].shape
    c2x, c2y = to_level(pos[0], 2), to_level(pos[1], 2)
    rad = (g.major >> 2) + 1
    if max_rad is not None:
        rad = min(rad, max_rad)
    rad = min(rad, max(w2, h2))
    out = []
    for y in range(max(c2y - rad, 0), min(c2y + rad, h2 - 1) + 1):
        for x in range(max(c2x - rad, 0), min(c2x + rad, w2 - 1) + 1):
            if not (x == c2x and y == c2y) and not g.contains((x + 0.5) * 4 - 0.5, (y + 0.5) * 4 - 0.5):
                continue
            out.append((x, y, sp.key(window(levels[2], x, y, R), tmpl3[2])))
    return out, (c2x, c2y)


def first_max(cands):
    """(x, y, key) of the largest key, the first in raster order among equals; None for an empty list"""
    best = None
    for c in cands:
        if best is None or c[2] > best[2]:
            best = c
    return best


def coarse_rival(cands, centre):
    """step 1: (B2, rival) -- B2 the coarse best pixel (the prediction's where there is no candidate), rival (x, y, key)
    or None"""
    b = first_max(cands)
    b2 = (b[0], b[1]) if b is not None else centre
    r = first_max([c for c in cands if max(abs(c[0] - b2[0]), abs(c[1] - b2[1])) > EXCL])
    return b2, (r if r is not None and r[2] >= 0.0 else None)


def refine(levels, tmpl3, bx, by):
    """levels 1 and 0 from the coarse pixel (bx, by): the 4 x 4 children of the best parent, no gate -> (x, y, key);
    key -3 and the position carried over where a level has no candidate"""
    bkey = -3.0
    for l in (1, 0):
        h, w = levels[l].shape
        px, py, bkey = bx, by, -3.0
        for y in range(2 * py - 1, 2 * py + 3):
            for x in range(2 * px - 1, 2 * px + 3):
                if x < 0 or y < 0 or x >= w or y >= h:
                    continue
                k = sp.key(window(levels[l], x, y, R), tmpl3[l])
                if k > bkey:
                    bkey, bx, by = k, x, y
    return bx, by, bkey


def dist(key):
    return np.float32(1.0 - np.sqrt(np.float64(key)))


def judge(ok, k0, rival, in_gate, coef):
    """steps 2 (what is left of it) and 3.  ok, k0: the search's acceptance and level-0 key; rival: None or the refined
    (x, y, r0); in_gate: whether gate_contains holds at the rival's pixel -> (state, rx, ry, d1, d2)"""
    zero = np.float32(0.0)
    if not ok:
        return 0, 0, 0, zero, zero
    d1 = dist(k0)
    if rival is None or rival[2] < 0.0 or not in_gate:
        return 1, 0, 0, d1, zero
    d2 = dist(rival[2])
    keep = bool(np.float64(d1) < np.float64(d2) * np.float64(coef))
    return (2 if keep else 3), int(rival[0]), int(rival[1]), d1, d2


def match_one(orc, levels, pos, S, tmpl3, max_rad=wr.MAXRAD, subpixel=False, coef=0.0):
    """ncc_wide_ref.match_one's dict, and with coef > 0: state, rival (refined (x, y, key) or None, before the gate test),
    rx, ry, d1, d2, b2 (coarse best), coarse_rival (x, y, key) or None; `valid` is then the match's final validity"""
    s = wr.match_one(orc, levels, pos, S, tmpl3, max_rad, subpixel)
    if coef == 0.0:
        return s
    g = wr.Gate(orc, pos, S)
    cands, centre = coarse_scan(g, levels, pos, tmpl3, max_rad)
    assert len(cands) == s["ncand"]
    b2, cr = coarse_rival(cands, centre)
    assert refine(levels, tmpl3, *b2) == (s["bx"], s["by"], s["key"]), "the two restatements of the search disagree"
    rv = refine(levels, tmpl3, cr[0], cr[1]) if cr is not None else None
    in_gate = rv is not None and g.contains(rv[0], rv[1])
    state, rx, ry, d1, d2 = judge(s["valid"], s["key"], rv, in_gate, coef)
    s.update(state=state, rival=rv, rx=rx, ry=ry, d1=d1, d2=d2, b2=b2, coarse_rival=cr, accepted=s["valid"])
    s["valid"] = state in (1, 2)
    if not s["valid"]:
        s["distance"] = np.float32(0.0)
    return s


def match_all(orc, levels, preds, tmpl, max_rad=wr.MAXRAD, subpixel=False, coef=0.0):
    """ncc_wide_ref.match_all with the test: -> (matches, per-slot dicts, wide counts, sub-pixel counts over the kept
    matches, rival records NCC_RIVAL_DTYPE per slot (none with coef 0), (accepted matches with a rival, rejected))"""
    slots = [match_one(orc, levels, p["imagePos"], p["covarianceMatrix"], tmpl[j], max_rad, subpixel, coef) for j, p in enumerate(preds)]
    out = np.zeros(len(preds), dtype=MATCH_DTYPE)
    riv = np.zeros(len(preds) if coef != 0.0 else 0, dtype=NCC_RIVAL_DTYPE)
    n = fit = 0
    for j, (p, s) in enumerate(zip(preds, slots)):
        if coef != 0.0:
            riv[j] = (p["featureIndex"], s["state"], (np.float32(s["rx"]), np.float32(s["ry"])), s["d1"], s["d2"])
        if s["valid"]:
            out[n]["featureIndex"], out[n]["keypointIndex"] = p["featureIndex"], -1
            out[n]["imagePos"] = (s["x"], s["y"])
            out[n]["distance"] = s["distance"]
            fit += int(s["fitted"].sum())
            n += 1
    counted = [s for s in slots if s["wide"]] if max_rad is None else []
    with_rival = sum(1 for s in slots if s.get("state", 0) >= 2)
    rejected = sum(1 for s in slots if s.get("state", 0) == 3)
    return (out[:n].copy(), slots, (len(counted), sum(s["ncand"] for s in counted)), (fit, 2 * n - fit) if subpixel else (0, 0), riv,
            (with_rival, rejected))


def assert_rivals_equal(got, want, label=""):
    """every field of every record: identical (the floats by their bits)"""
    assert len(got) == len(want), (label, len(got), len(want))
    for f in ("featureIndex", "state", "rivalPos", "distance", "rivalDistance"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{label}: {f}")
