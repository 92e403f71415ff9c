"""Tables that are freed and allocated again on one engine (csrc/device_buffers.h owns them): the image pyramid, the raw staging
buffer and the wide-search tables when the frame size changes 160 x 120 -> 320 x 240 -> 160 x 120 (the coarse level's 32 x 32
tiles go 2 -> 6 -> 2), the second partial table of the distinctiveness test, and the staged keypoint frames when they are
uploaded again.  Every other test keeps one frame size and uploads its frames once.

The pyramid is compared with the oracle's, the matches with the numpy restatements the wide-search and distinctiveness tests
compare with (fed the engine's own pyramid, predictions and templates), the staged steps with ekf_step on a twin engine."""
import numpy as np
import pytest

import ncc_wide_ref as wr
import wide_scene as wsn
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_ncc_distinct import check as check_distinct
from tests.test_gpu_ncc_wide import device, reference
from tests.test_gpu_parity import eng_mod  # noqa: F401
from tests.test_gpu_step_counts import INFO_FIELDS

pytestmark = pytest.mark.gpu
N_FEAT = 12
SIZES = [(160, 120), (320, 240), (160, 120)]
AXES = np.where(np.arange(N_FEAT) % 3 == 0, 72.0, 30.0)  # gate semi-axes in pixels: every third beyond the 63 px of the coarse window


def sized_scene(w, h):
    """two frames of a 12-feature scene rendered at w x h, and the pixels its features are seeded at"""
    seq = SyntheticSequence(N_FEAT, 1, width=w, height=h)
    return seq.render_image(0), seq.render_image(1), seq.pixel_positions(0).astype(np.float64)


def wide_slots(o, preds):
    return sum(((int(np.rint(o.ellipse(p["covarianceMatrix"])[0].max())) >> 2) + 1) > wr.MAXRAD for p in preds)


def assert_pyramid(e, o, img, label):
    o.set_image(img)
    for l in range(3):
        got, want = e.image_level(l), o.image_level(l)
        assert got.shape == want.shape == (img.shape[0] >> l, img.shape[1] >> l), (label, l, got.shape, want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f"{label}: level {l}")


def regrow_images(eng_mod, oracle_lib):
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()  # one camera for every size: the small frames are its upper left corner
    o = oracle_lib.Oracle(cam, par, N_FEAT)
    e = eng_mod.EkfEngine(cam, par, N_FEAT + 8)
    P = wsn.diag_P(cam, N_FEAT, AXES, AXES)
    tiles = []
    for k, (w, h) in enumerate(SIZES):
        label = f"upload {k}, {w} x {h}"
        img0, img1, uv = sized_scene(w, h)
        state = wsn.seeded(cam, par, uv)
        o.set_state(*state, None, P)
        assert wide_slots(o, o.predict_measurements()[0]) >= 1, label  # on the CPU: the size exercises the wide tables
        e.set_state(*state, None, P)
        e.upload_image(img0)
        assert_pyramid(e, o, img0, label + ", frame 0")
        e.capture_templates(np.arange(N_FEAT), uv)
        e.upload_image(img1)
        assert_pyramid(e, o, img1, label + ", frame 1")
        tiles.append(-(-(w >> 2) // wr.TILE) * -(-(h >> 2) // wr.TILE))
        preds, _, _ = e.predict_measurements()
        assert len(preds) == N_FEAT
        on, counts = device(e, True)
        want, _, want_counts, _ = reference(e, oracle_lib, preds, None)
        print(f"{label}: {len(on)} matches, wide counts {counts}; reference {len(want)} matches, {want_counts}")
        wr.assert_matches_equal(on, want, label)
        assert counts == want_counts and counts[0] >= 1 and len(want) >= N_FEAT // 2, label
    assert tiles == [2, 6, 2]
    # the distinctiveness test brings the second partial table: the wide tables are allocated once more
    m, _, riv = check_distinct(e, oracle_lib, preds, 0.5, True, "second partial table")
    assert len(riv) == N_FEAT and len(m) >= 1
    e.close()


def reupload_frames(eng_mod):
    seq = SyntheticSequence(N_FEAT, 3, seed=1)  # (the default seed's scene has no inliers in its second frame)
    e, twin = (eng_mod.EkfEngine(seq.cam, seq.par, 16, max_keypoints=128) for _ in range(2))
    for f in (e, twin):
        f.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        f.set_sweep_mode(4)  # bitwise run-to-run comparisons need the launch-per-panel sweep
    second = [seq.frames[0], (seq.frames[1][0][:-5], seq.frames[1][1][:-5])]
    assert sum(len(k) for k, _ in second) not in (sum(len(k) for k, _ in seq.frames), 0)
    e.upload_frames(seq.frames)
    e.upload_frames(second)
    for t, (kps, desc) in enumerate(second):
        a, b = e.step_frame(t), twin.step(kps, desc)
        for f in INFO_FIELDS:
            assert getattr(a, f) == getattr(b, f), (t, f, getattr(a, f), getattr(b, f))
        assert a.n_inliers > 0 and a.n_rescued > 0, "the scene must exercise both updates"
    for u, v in zip(e.get_state(), twin.get_state()):
        np.testing.assert_array_equal(u, v)
    with pytest.raises(eng_mod.EkfError) as ex:  # the third frame went with the first upload
        e.step_frame(2)
    assert ex.value.code == 1  # EKF_ERR_INVALID_ARG
    e.upload_frames([])
    with pytest.raises(eng_mod.EkfError) as ex:
        e.step_frame(0)
    assert ex.value.code == 1
    e.close()
    twin.close()


def test_tables_are_replaced_on_one_engine(eng_mod, oracle_lib):
    regrow_images(eng_mod, oracle_lib)
    reupload_frames(eng_mod)
