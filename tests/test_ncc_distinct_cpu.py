"""CPU-only checks of the NCC matcher's distinctiveness test on its numpy restatement
(tests/ncc_distinct_ref.py): with coef 0 it is the search of tests/ncc_wide_ref.py; a periodic frame is rejected; the
displaced targets and the real frames keep their matches at coef 0.5; the branches of the rule one by one; the exported
symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import ncc_distinct_ref as dr
import ncc_wide_ref as wr
import wide_scene as wsn
from openekfmonoslam_amd import build, engine
from openekfmonoslam_amd.ekftypes import NCC_RIVAL_DTYPE, s3_camera, s3_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3_frames")
PERIOD = 32


def snapshot(o, preds):
    """(oracle, levels, predictions, templates): what a match reads, copied (the oracle library keeps one image for all)"""
    return o, [o.image_level(l).copy() for l in range(3)], preds.copy(), o.templates()[preds["featureIndex"]].copy()


def run(snap, max_rad, coef):
    o, levels, preds, tm = snap
    return dr.match_all(o, levels, preds, tm, max_rad, False, coef)


def plain(snap, max_rad):
    o, levels, preds, tm = snap
    return wr.match_all(o, levels, preds, tm, max_rad)


def seeded_oracle(oracle_lib, uv, P, frame0, frame1):
    cam, par = s3_camera(wsn.W, wsn.H), s3_params()
    o = oracle_lib.Oracle(cam, par, len(uv) + 8)
    x13, fpos, ftype = wsn.seeded(cam, par, uv)
    o.set_state(x13, fpos, ftype, None, P)
    o.set_image(frame0)
    o.capture_templates(np.arange(len(uv)), uv)
    o.set_image(frame1)
    preds, _, _ = o.predict_measurements()
    assert len(preds) == len(uv)
    return snapshot(o, preds)


@pytest.fixture(scope="module")
def displaced(oracle_lib):
    sc = wsn.DisplacedScene()
    o = oracle_lib.Oracle(sc.cam, sc.par, 16)
    sc.load(o)
    preds, _, _ = o.predict_measurements()
    return sc, snapshot(o, preds)


@pytest.fixture(scope="module")
def real_frames(oracle_lib):
    """tests/golden/s3_frames through the pipeline of test_ncc_wide_cpu.test_restatement_equals_the_oracle_on_real_frames:
    {frame: (levels, predictions, templates)} of what the steps of frames 1 and 4 are about to match"""
    from PIL import Image

    frames = [np.asarray(Image.open(os.path.join(GOLDEN, f"{k:05d}.png"))) for k in range(6)]
    o = oracle_lib.Oracle(s3_camera(320, 240), s3_params(), 96)
    o.reset()
    o.set_image(frames[0])
    uv = o.detect_new_features(np.zeros(0, dtype=oracle_lib.PREDICTION_DTYPE), 40, min_response=1e10)
    assert len(uv) == 40
    for p in uv:
        o.add_feature(p)
    o.capture_templates(np.arange(40), uv)
    seen = {}
    for t in (1, 2, 3, 4):
        if t in (1, 4):
            x, fp, ft, P = o.x13(), o.feature_pos(), o.feature_type(), o.P()
            o.predict()
            preds, _, _ = o.predict_measurements()
            o.set_image(frames[t])
            seen[t] = snapshot(o, preds)
            o.set_state(x, fp, ft, None, P)
        assert o.step_image(frames[t], oracle_lib.ALGORITHMIC).status == 0
    return seen


@pytest.mark.parametrize("max_rad", [wr.MAXRAD, None])
def test_coef_zero_is_the_search(displaced, real_frames, max_rad):
    sc, snap = displaced
    got = run(snap, max_rad, 0.0)
    want = plain(snap, max_rad)
    wr.assert_matches_equal(got[0], want[0], "displaced scene")
    assert got[2:4] == want[2:4] and len(got[4]) == 0 and got[5] == (0, 0)
    got = run(real_frames[1], max_rad, 0.0)
    want = plain(real_frames[1], max_rad)
    assert len(want[0]) >= 30
    wr.assert_matches_equal(got[0], want[0], "real frame 1")
    assert len(got[4]) == 0 and got[5] == (0, 0)


@pytest.mark.parametrize("max_rad", [wr.MAXRAD, None])
@pytest.mark.parametrize("gate", [40.0, 150.0])
def test_periodic_frame_is_rejected(oracle_lib, gate, max_rad):
    frame = wsn.periodic_frame(PERIOD)
    uv = np.array([[160.0, 120.0]])
    snap = seeded_oracle(oracle_lib, uv, wsn.diag_P(s3_camera(wsn.W, wsn.H), 1, gate, gate), frame, frame)
    m, slots, _, _, riv, counts = run(snap, max_rad, 0.5)
    s = slots[0]
    print(f"gate {gate} max_rad {max_rad}: best {(s['bx'], s['by'])} d1 {s['d1']}, rival {(s['rx'], s['ry'])} d2 {s['d2']}")
    assert s["accepted"] and s["state"] == 3 and len(m) == 0 and counts == (1, 1)
    assert (s["rx"] - s["bx"]) % PERIOD == 0 and (s["ry"] - s["by"]) % PERIOD == 0 and (s["rx"], s["ry"]) != (s["bx"], s["by"])
    assert s["d1"] == 0.0 and s["d2"] == 0.0
    assert riv.dtype == NCC_RIVAL_DTYPE and riv[0]["state"] == 3 and riv[0]["featureIndex"] == 0
    for coef in (1.0, 1e-3):  # 0 < 0 * coef never holds
        assert run(snap, max_rad, coef)[1][0]["state"] == 3


def test_displaced_targets_are_kept(displaced):
    sc, snap = displaced
    m, slots, _, _, riv, counts = run(snap, None, 0.5)
    print("rival distances:", [float(s["d2"]) for s in slots])
    wr.assert_matches_equal(m, plain(snap, None)[0], "coef 0.5 against the search alone")
    assert len(m) == sc.n and counts == (sc.n, 0)
    assert all(s["state"] == 2 and s["d1"] == 0.0 and s["d2"] > 0.5 for s in slots)
    np.testing.assert_array_equal(riv["featureIndex"], snap[2]["featureIndex"])


def test_real_frames_lose_few_matches(real_frames):
    for t, snap in real_frames.items():
        base = plain(snap, wr.MAXRAD)[0]
        m, slots, _, _, riv, (with_rival, rejected) = run(snap, wr.MAXRAD, 0.5)
        pairs = sorted((float(s["d1"]), float(s["d2"])) for s in slots if s["state"] >= 2)
        print(f"real frame {t}: {len(base)} valid, {with_rival} with a rival, {rejected} rejected; (d1, d2): {pairs}")
        assert len(base) >= 30 and len(m) == len(base) - rejected
        assert rejected <= 0.10 * len(base)
        kept = np.isin(base["featureIndex"], m["featureIndex"])
        wr.assert_matches_equal(m, base[kept], f"real frame {t}: the matches that stay")


def test_nothing_outside_the_block(oracle_lib):
    """gates under 8 px: the coarse box is 5 x 5 around the prediction, the best is the prediction, nothing is left"""
    sc = wsn.DisplacedScene()
    snap = seeded_oracle(oracle_lib, sc.UV, wsn.diag_P(sc.cam, sc.n, 1.0, 1.0), sc.frame0, sc.frame0)
    m, slots, _, _, riv, counts = run(snap, wr.MAXRAD, 0.5)
    assert all(s["major"] < 8 and s["ncand"] <= 25 for s in slots), [(s["major"], s["ncand"]) for s in slots]
    assert all(s["state"] == 1 and s["coarse_rival"] is None and s["d1"] == 0.0 for s in slots) and counts == (0, 0) and len(m) == sc.n
    assert (riv["rivalDistance"] == 0).all() and (riv["rivalPos"] == 0).all()


def test_branches_of_the_rule():
    # coarse: the block around the best is left out, the first of equal keys wins, a negative key is no rival
    cands = [(3, 1, 0.5), (9, 1, 0.7), (10, 3, 0.9), (12, 5, 0.8), (13, 3, 0.7), (2, 6, 0.7)]
    b2, r = dr.coarse_rival(cands, (0, 0))
    assert b2 == (10, 3) and r == (13, 3, 0.7)  # (9, 1) and (12, 5) are within 2; (13, 3) precedes (2, 6)
    assert dr.coarse_rival([(10, 3, 0.9), (13, 3, -1.0)], (0, 0)) == ((10, 3), None)
    assert dr.coarse_rival([(10, 3, 0.9), (12, 1, 0.9)], (0, 0)) == ((10, 3), None)
    assert dr.coarse_rival([], (7, 8)) == ((7, 8), None)
    assert dr.coarse_rival([(10, 3, 0.9), (13, 3, 0.0)], (0, 0))[1] == (13, 3, 0.0)
    # refined: a rival outside the gate or without a score is none; the match stays and carries its distance
    d1 = dr.dist(0.81)
    assert dr.judge(True, 0.81, (50, 60, 0.95), False, 0.5) == (1, 0, 0, d1, np.float32(0))
    assert dr.judge(True, 0.81, (50, 60, -1.0), True, 0.5) == (1, 0, 0, d1, np.float32(0))
    assert dr.judge(True, 0.81, None, False, 0.5) == (1, 0, 0, d1, np.float32(0))
    assert dr.judge(False, 0.5, (50, 60, 0.95), True, 0.5) == (0, 0, 0, np.float32(0), np.float32(0))
    # a rival that scores above the best: rejected for every coef <= 1
    for coef in (0.01, 0.5, 1.0):
        assert dr.judge(True, 0.81, (50, 60, 0.9), True, coef)[0] == 3
    # the comparison: strict, in double, of the two floats
    d2 = dr.dist(0.25)
    assert dr.judge(True, 0.81, (50, 60, 0.25), True, 0.5) == (2, 50, 60, d1, d2)  # 0.1 < 0.25
    assert dr.judge(True, 0.81, (50, 60, 0.25), True, 0.2)[0] == 3                 # 0.1 < 0.1: the rounded floats decide
    assert dr.judge(True, 1.0, (50, 60, 1.0), True, 1.0)[0] == 3                   # 0 < 0 does not hold
    assert dr.judge(True, 0.81, (50, 60, 0.81), True, 1.0)[0] == 3                 # equal distances


def test_library_exports_the_distinct_calls():
    build.build_engine()
    lib = engine.load_library()
    for name in ("ekf_set_ncc_distinct", "ekf_get_ncc_distinct_counts", "ekf_get_ncc_rivals"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    assert lib.ekf_set_ncc_distinct(None, 0.5) == 1  # EKF_ERR_INVALID_ARG: no engine
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_get_ncc_distinct_counts(None, C.byref(a), C.byref(b)) == 1
    assert lib.ekf_get_ncc_rivals(None, None, 0, C.byref(a)) == 1
    for name in ("set_ncc_distinct", "ncc_distinct_counts", "ncc_rivals"):
        assert hasattr(engine.EkfEngine, name)
    assert NCC_RIVAL_DTYPE.itemsize == 24
