"""CPU-only checks of the wide search: the numpy restatement of the whole NCC search
(tests/ncc_wide_ref.py) equals the oracle's orc_match_ncc with the coarse radius capped at 16, so that its uncapped
variant differs from a trusted definition in one line; what the cap costs on the displaced-target scene; the exported
symbols."""
import ctypes as C
import os

import numpy as np

import ncc_wide_ref as wr
import wide_scene as wsn
from openekfmonoslam_amd import build, engine
from openekfmonoslam_amd.ekftypes import s3_camera, s3_params
from openekfmonoslam_amd.synth import SyntheticSequence

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3_frames")


def reference_of(o, preds, max_rad=wr.MAXRAD):
    levels = [o.image_level(l) for l in range(3)]
    return wr.match_all(o, levels, preds, o.templates()[preds["featureIndex"]], max_rad)


def test_restatement_equals_the_oracle_on_synthetic_frames(oracle_lib):
    """the frames of test_gpu_ncc.test_match_ncc_identical: which features match, the pixel and the float distance"""
    seq = SyntheticSequence(50, 3)
    o = oracle_lib.Oracle(seq.cam, seq.par, 50)
    o.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    o.set_image(seq.render_image(0))
    o.capture_templates(np.arange(50), seq.pixel_positions(0).astype(np.float64))
    for t in (1, 2):
        o.predict()
        preds, _, _ = o.predict_measurements()
        o.set_image(seq.render_image(t))
        want = o.match_ncc(preds)
        got, slots, wide, _ = reference_of(o, preds)
        assert len(want) > 30
        wr.assert_matches_equal(got, want, f"synthetic frame {t}")
        assert wide == (0, 0)  # (nothing is counted with the cap in place)
        print(f"synthetic frame {t}: {len(want)} matches, {sum(s['wide'] for s in slots)} gates beyond the cap")


def test_restatement_equals_the_oracle_on_real_frames(oracle_lib):
    """tests/golden/s3_frames through the pipeline of test_gpu_ncc.test_real_frames_engine_equals_oracle: the first frame
    after the initialisation (fresh inverse-depth features, the widest gates) and one after three image steps"""
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
    for t in (1, 2, 3, 4):
        if t in (1, 4):  # what the step about to run will match: its prediction, this frame
            x, fp, ft, P = o.x13(), o.feature_pos(), o.feature_type(), o.P()
            o.predict()
            preds, _, _ = o.predict_measurements()
            o.set_image(frames[t])
            want = o.match_ncc(preds)
            got, slots, _, _ = reference_of(o, preds)
            assert len(want) >= 30
            wr.assert_matches_equal(got, want, f"real frame {t}")
            print(f"real frame {t}: {len(want)} matches, gates' major semi-axes up to {max(s['major'] for s in slots)} px")
            o.set_state(x, fp, ft, None, P)  # undo the prediction: the step makes its own
        assert o.step_image(frames[t], oracle_lib.ALGORITHMIC).status == 0


def test_the_cap_loses_displaced_targets(oracle_lib):
    """DisplacedScene: every target lies 100 px from its prediction inside a gate of about 150 px.  With the cap at most
    one of the eight features may match at its true pixel (here none: the oracle agrees), without it all eight do, with
    a score of exactly 1."""
    sc = wsn.DisplacedScene()
    o = oracle_lib.Oracle(sc.cam, sc.par, 16)
    sc.load(o)
    preds, _, _ = o.predict_measurements()
    assert len(preds) == sc.n
    np.testing.assert_allclose(preds["imagePos"], sc.UV, atol=1e-6)
    capped, slots, wide, _ = reference_of(o, preds)
    wr.assert_matches_equal(capped, o.match_ncc(preds), "displaced targets, capped")
    assert wide == (0, 0) and all(s["wide"] and 140 <= s["major"] <= 200 for s in slots), [s["major"] for s in slots]
    at_truth = sum(1 for m in capped if np.array_equal(m["imagePos"], sc.target[m["featureIndex"]]))
    assert at_truth <= 1
    whole, slots, wide, _ = reference_of(o, preds, None)
    np.testing.assert_array_equal(whole["featureIndex"], np.arange(sc.n))
    np.testing.assert_array_equal(whole["imagePos"], sc.target)
    np.testing.assert_array_equal(whole["distance"], np.zeros(sc.n, dtype=np.float32))
    assert wide[0] == sc.n and wide[1] == sum(s["ncand"] for s in slots) > sc.n * 33 * 33 / 2


def test_library_exports_the_wide_search_calls():
    build.build_engine()
    lib = engine.load_library()
    for name in ("ekf_set_ncc_wide_search", "ekf_get_ncc_wide_counts"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1
    assert lib.ekf_set_ncc_wide_search(None, 1) == 1  # EKF_ERR_INVALID_ARG: no engine
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_get_ncc_wide_counts(None, C.byref(a), C.byref(b)) == 1
    assert hasattr(engine.EkfEngine, "set_ncc_wide_search") and hasattr(engine.EkfEngine, "ncc_wide_counts")
