"""numpy fp64 restatement of the sub-pixel NCC fit (k_ncc_match<true>): the integer ZNCC^2 key of
ncc_key and, per axis, the vertex of the parabola through the keys of the best level-0 pixel and its two neighbours.
The integer position is an input: the coarse-to-fine search that finds it is defined by the oracle and by the mode-off
engine, and is not restated here.  Every step of the fit is one correctly rounded fp64 operation in the kernel's
order, so the device has to return the same float32 bits."""
import numpy as np

from template_warp_ref import R, window

N = 121


def key(window11, template11):
    """ncc_key: zncc^2 = num^2 / den from integer sums, -1.0 where the correlation is not positive or a variance is zero"""
    w = np.asarray(window11).astype(np.int64).ravel()
    t = np.asarray(template11).astype(np.int64).ravel()
    assert w.size == N and t.size == N
    s, ss, sx, st, stt = int(w.sum()), int((w * w).sum()), int((w * t).sum()), int(t.sum()), int((t * t).sum())
    num = N * sx - s * st
    den = (N * ss - s * s) * (N * stt - st * st)
    if num <= 0 or den <= 0:
        return -1.0
    dn = np.float64(num)
    return float(dn * dn / np.float64(den))


def offset(km, k0, kp):
    """(offset, fitted) of one axis from the keys at -1, 0, +1; a neighbour outside the frame is passed as a negative key"""
    km, k0, kp = np.float64(km), np.float64(k0), np.float64(kp)
    if km < 0.0 or kp < 0.0 or km > k0 or kp > k0:
        return np.float64(0.0), False
    a = km - kp
    b = (km - np.float64(2.0) * k0) + kp
    if b >= 0.0:
        return np.float64(0.0), False
    d = (np.float64(0.5) * a) / b
    return np.float64(min(max(d, -0.5), 0.5)), True


def neighbour_key(level0, template0, x, y):
    """key of the candidate centred on (x, y), reads clamped to the frame; -2.0 for a centre outside it (the candidate
    loop's own rule: such a pixel is never a candidate)"""
    h, w = level0.shape
    if x < 0 or y < 0 or x >= w or y >= h:
        return -2.0
    return key(window(level0, x, y, R), template0)


def refine(level0, template0, bx, by):
    """(x, y, refined_x, refined_y) of the match whose integer best pixel is (bx, by); x, y are float32"""
    bx, by = int(bx), int(by)
    k0 = key(window(level0, bx, by, R), template0)
    dx, fx, dy, fy = np.float64(0.0), False, np.float64(0.0), False
    if k0 >= 0.0:  # (a best pixel without a score is never a valid match; the kernel leaves it alone too)
        dx, fx = offset(neighbour_key(level0, template0, bx - 1, by), k0, neighbour_key(level0, template0, bx + 1, by))
        dy, fy = offset(neighbour_key(level0, template0, bx, by - 1), k0, neighbour_key(level0, template0, bx, by + 1))
    return np.float32(np.float64(bx) + dx), np.float32(np.float64(by) + dy), fx, fy
