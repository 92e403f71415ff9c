"""CPU-only checks of the sub-pixel NCC fit: what the rule of tests/ncc_subpixel_ref.py gains on the
textured-plane scene of tests/warp_scene.py, its branches on hand-made inputs, and the exported symbols."""
import ctypes as C

import numpy as np

import ncc_subpixel_ref as sp
import template_warp_ref as tw
import warp_scene as ws
from openekfmonoslam_amd import build, engine

N_FEAT, FRAMES, SIDEWAYS = 64, 8, 0.0213  # 0.0213 world units in 8 frames: ~0.35 px of image motion per frame
SEARCH = 3


def test_the_fit_earns_its_keep():
    """64 templates cut from frame 0 at the integer seed pixels, searched at level 0 within +-3 px of the rounded true pixel
    in frames 1..8 of the sideways trajectory (512 matches), against PlaneScene.true_pixels.  Required: the RMS error of the
    refined positions is at most half that of the integer ones (the parabola itself gives ~0.28; half leaves room for the
    rounding of the uint8 frames), and no refined axis is further than 0.5 px from its integer."""
    scene = ws.PlaneScene()
    uv0, pts, _, _, _, _ = scene.seed_features(N_FEAT)
    poses = ws.trajectory("sideways", FRAMES, SIDEWAYS)
    f0 = scene.render(poses[0], 0)
    tmpl = [tw.window(f0, int(u), int(v), tw.R) for u, v in uv0]
    err_int, err_sub, moved, fitted = [], [], [], 0
    for t in range(1, FRAMES + 1):
        img = scene.render(poses[t], t)
        uv, _ = scene.true_pixels(poses[t], pts)
        for i in range(N_FEAT):
            cx, cy = int(round(uv[i, 0])), int(round(uv[i, 1]))
            best, bx, by = -3.0, cx, cy
            for y in range(cy - SEARCH, cy + SEARCH + 1):  # raster order, strict '>': the first maximum, as the search keeps it
                for x in range(cx - SEARCH, cx + SEARCH + 1):
                    k = sp.key(tw.window(img, x, y, tw.R), tmpl[i])
                    if k > best:
                        best, bx, by = k, x, y
            x, y, fx, fy = sp.refine(img, tmpl[i], bx, by)
            fitted += int(fx) + int(fy)
            err_int.append([bx - uv[i, 0], by - uv[i, 1]])
            err_sub.append([x - uv[i, 0], y - uv[i, 1]])
            moved.append([float(x) - bx, float(y) - by])
    err_int, err_sub, moved = np.array(err_int), np.array(err_sub), np.array(moved)
    rms_int, rms_sub = np.sqrt((err_int ** 2).mean()), np.sqrt((err_sub ** 2).mean())
    print(f"{len(err_int)} matches, {fitted} axes fitted; RMS error integer {rms_int:.4f} px, refined {rms_sub:.4f} px "
          f"(ratio {rms_sub / rms_int:.3f}); worst axis error integer {np.abs(err_int).max():.3f}, refined {np.abs(err_sub).max():.3f}")
    assert len(err_int) == N_FEAT * FRAMES
    assert rms_sub <= 0.5 * rms_int, (rms_sub, rms_int)
    assert np.abs(moved).max() <= 0.5


def test_offset_branches():
    k0 = 0.8125
    d, fit = sp.offset(k0, k0, 0.5)  # km == k0: a = k0 - kp, b = -(k0 - kp), exactly
    assert fit and d == -0.5
    d, fit = sp.offset(0.5, k0, k0)
    assert fit and d == 0.5
    d, fit = sp.offset(0.7, k0, 0.7)  # symmetric: fitted, and the vertex is the integer
    assert fit and d == 0.0
    assert sp.offset(0.9, k0, 0.5) == (0.0, False)  # a neighbour above the centre
    assert sp.offset(0.5, k0, 0.9) == (0.0, False)
    assert sp.offset(-1.0, k0, 0.5) == (0.0, False)  # a neighbour without a score
    assert sp.offset(0.5, k0, -2.0) == (0.0, False)  # ... or outside the frame
    assert sp.offset(k0, k0, k0) == (0.0, False)  # b == 0
    assert sp.offset(0.0, 0.0, 0.0) == (0.0, False)
    # order of operations: b = (km - 2 k0) + kp, not km + kp - 2 k0
    km, kp = 0.1 + 2.0 ** -55, 0.3
    d, _ = sp.offset(km, 0.9, kp)
    assert d == (0.5 * (np.float64(km) - kp)) / ((np.float64(km) - 2.0 * 0.9) + kp)


def textured(h=40, w=48, seed=5):
    """random values, 3 x 3 box-blurred so that windows one pixel apart correlate"""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    return np.rint(sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0).astype(np.uint8)


def test_refine_on_a_shifted_copy():
    """a template that lies between two pixels of the frame: the fit moves towards the better neighbour, by less than 0.5"""
    frame = textured()
    f = frame.astype(np.float64)
    shifted = np.rint(0.7 * f[:, :-1] + 0.3 * f[:, 1:]).astype(np.uint8)  # the frame's content 0.3 px to the left
    t = tw.window(shifted, 20, 20, tw.R)
    x, y, fx, fy = sp.refine(frame, t, 20, 20)
    assert fx and fy
    assert x.dtype == np.float32 and y.dtype == np.float32
    assert 20.0 < x < 20.5 and abs(float(y) - 20.0) < 0.2, (x, y)


def test_refine_a_neighbour_key_above_the_centre():
    img = textured()
    t = tw.window(img, 20, 20, tw.R)  # the exact match is at (20, 20)
    assert sp.refine(img, t, 21, 20)[::2] == (np.float32(21.0), False)
    assert sp.refine(img, t, 20, 19)[1::2] == (np.float32(19.0), False)


def test_refine_constant_window_has_no_score():
    """the frame is constant left of column 30: the window of (24, y) is constant, that of (25, y) ends on column 30"""
    img = textured()
    img[:, :30] = 100
    assert sp.key(tw.window(img, 24, 20, tw.R), tw.window(img, 25, 20, tw.R)) == -1.0
    t = tw.window(img, 25, 20, tw.R)
    assert sp.key(tw.window(img, 25, 20, tw.R), t) == 1.0
    x, y, fx, fy = sp.refine(img, t, 25, 20)
    assert (x, fx) == (np.float32(25.0), False)
    # a best pixel without a score of its own stays where it is on both axes
    assert sp.refine(img, t, 10, 20) == (np.float32(10.0), np.float32(20.0), False, False)


def test_refine_at_the_border():
    img = textured()
    h, w = img.shape
    t = tw.window(img, 0, 20, tw.R)  # reads clamped to the frame
    x, y, fx, fy = sp.refine(img, t, 0, 20)
    assert (x, fx) == (np.float32(0.0), False) and fy  # (-1, 20) is outside the frame
    ky = [sp.key(tw.window(img, 0, 20 + d, tw.R), t) for d in (-1, 0, 1)]
    assert y == np.float32(20.0 + sp.offset(*ky)[0])
    t = tw.window(img, 30, h - 1, tw.R)
    x, y, fx, fy = sp.refine(img, t, 30, h - 1)
    assert (y, fy) == (np.float32(h - 1), False) and fx
    x, y, fx, fy = sp.refine(img, tw.window(img, w - 1, 0, tw.R), w - 1, 0)
    assert (float(x), float(y), fx, fy) == (w - 1, 0.0, False, False)


def test_refine_three_equal_keys():
    """a frame that varies along y only: every horizontal neighbour has the centre's key, b == 0"""
    img = np.repeat(np.random.default_rng(3).integers(0, 256, (40, 1)).astype(np.uint8), 48, axis=1)
    t = tw.window(img, 20, 20, tw.R)
    x, y, fx, fy = sp.refine(img, t, 20, 20)
    assert (x, fx) == (np.float32(20.0), False)
    assert fy and abs(float(y) - 20.0) <= 0.5


def test_refine_equal_key_on_one_side():
    """columns up to 25 repeat one column, the rest is texture: the windows of (19, y) and (20, y) are equal, that of
    (21, y) is not -> exactly -0.5"""
    img = textured()
    img[:, :26] = img[:, 25:26]
    t = tw.window(img, 20, 20, tw.R)
    assert sp.key(tw.window(img, 19, 20, tw.R), t) == 1.0 and sp.key(tw.window(img, 21, 20, tw.R), t) < 1.0
    x, _, fx, _ = sp.refine(img, t, 20, 20)
    assert fx and x == np.float32(19.5)


def test_library_exports_the_subpixel_calls():
    build.build_engine()
    lib = engine.load_library()
    for name in ("ekf_set_subpixel_matches", "ekf_get_subpixel_counts"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    assert lib.ekf_set_subpixel_matches(None, 1) == 1  # EKF_ERR_INVALID_ARG: no engine
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_get_subpixel_counts(None, C.byref(a), C.byref(b)) == 1
    assert hasattr(engine.EkfEngine, "set_subpixel_matches") and hasattr(engine.EkfEngine, "subpixel_counts")
