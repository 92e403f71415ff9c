"""The map blob (ekf_save_map / ekf_load_map / ekf_map_blob_info; csrc/map_blob.h, csrc/kernels_mapblob.hip) through
the Python binding, against tests/map_blob_ref.py: the bytes a save writes, what the optional sections hold, the round trip into
another engine, bit-identical continuation, loads across storage types, refusals that change nothing, a save that changes nothing,
and pending asynchronous errors.  No tolerance anywhere: bytes and bits are compared; the one stated exception is the single
rounding of an fp64 blob into an fp32-stored engine."""
import os

import numpy as np
import pytest

import map_blob_ref as mb
import map_ref as mr
import template_warp_ref as tw
from openekfmonoslam_amd.ekftypes import DESC_BYTES, s3_camera, s3_params
from openekfmonoslam_amd.shard import LocalShardGroup
from openekfmonoslam_amd.synth import SyntheticSequence
from tests.test_gpu_convert_all import indefinite_between_two_features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = os.path.join(ROOT, "tests", "golden", "s3_frames")
F64, F32, F32_EXACT, F64_EXACT = 0, 1, 2, 3
PRECISIONS = [F64, F32, F32_EXACT, F64_EXACT]
INVALID_ARG, CAPACITY, NOT_POSITIVE_DEFINITE, NON_FINITE = 1, 2, 3, 4
SWEEP_LAUNCHES = 4  # EKF_SWEEP_LAUNCHES: the run-to-run reproducible mode
# the empty map; 8 and 9 inverse-depth features (n on both sides of the 64-tile seam); map_ref.convert_scene's mixed maps after one
# conversion, so that 3-row and 6-row features straddle the seams at 64, 128, ... and 256, 512
SIZES = ["empty", "n61", "n67", "scene259", "scene514"]


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1, "no MI355X visible"
    return engine


def elem_bytes(precision):
    return 4 if precision in (F32, F32_EXACT) else 8


def descriptors(N, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, DESC_BYTES), dtype=np.uint8)


def sized_engine(eng_mod, size, precision, extra=0):
    """an engine holding the map of `size` (set_state: P as uploaded, not known symmetric)"""
    if size == "empty":
        e = eng_mod.EkfEngine(s3_camera(), s3_params(), 4 + extra, precision=precision)
        e.reset()
        e.cam = s3_camera()
        return e
    if size in ("n61", "n67"):
        s = mr.make_scene(np.full(8 if size == "n61" else 9, 2, dtype=np.int32))
        par = s3_params()
    else:
        s = mr.convert_scene(259 if size == "scene259" else 514, 13 if size == "scene259" else 250)
        par = mr.convert_params()
    e = eng_mod.EkfEngine(s.cam, par, s.n_features + extra, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(s.n_features, s.n_features), s.P0)
    e.cam = s.cam
    if size.startswith("scene"):
        assert e.convert_inverse_depth_to_depth() >= 0  # a partial conversion: one feature
    return e


def camera_bytes(e_cam):
    return bytes(e_cam)


def reference_blob(e, cam, layout, **tables):
    """the blob map_blob_ref builds from what the getters return"""
    x, fp, P = e.get_state()
    t, _ = e.feature_layout()
    desc, tp, tm = e.get_map_features()
    N = e.N
    return mb.build(x, fp[:N], t[:N], desc[:N], tp[:N], tm[:N], P, elem_bytes(e.precision), layout, 0, camera_bytes(cam), **tables)


def snapshot(e, with_blob=True):
    """everything a load or a save may touch: the getters, and the engine's own blob (save is read-only: test 7)"""
    x, fp, P = e.get_state()
    desc, tp, tm = e.get_map_features()
    t, c = e.feature_layout()
    mp = e.map_points()
    s = {"n": e.n, "N": e.N, "x": x, "fp": fp, "P": P, "desc": desc[: e.N], "tp": tp[: e.N], "tm": tm[: e.N], "type": t.copy(), "covpos": c.copy(),
         "points": mp.copy(), "unseen": np.asarray(e.unseen_features()).copy()}
    if with_blob:
        s["blob"] = e.save_map()
    return s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert same_bits(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def info_tuple(i):
    return tuple(getattr(i, f) for f, _ in type(i)._fields_)


# ------------------------------------------------------------------------------------------------ 1. bytes
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("size", SIZES)
def test_saved_bytes_equal_the_reference(eng_mod, size, precision):
    e = sized_engine(eng_mod, size, precision)
    cam = e.cam
    # after a prediction P is bitwise symmetric: the packed triangle in the storage type
    e.predict()
    blob = e.save_map(eng_mod.MAP_TEMPLATES)
    want = reference_blob(e, cam, mb.TRIANGLE, templates=np.zeros((e.N, 363), np.uint8))
    assert blob.tobytes() == want.tobytes()
    p = mb.parse(blob)
    n = e.n
    assert len(p["sections"][mb.P]) == n * (n + 1) // 2 * elem_bytes(precision) and p["p_layout"] == mb.TRIANGLE
    info = eng_mod.map_blob_info(blob)
    assert (info["version"], info["N"], info["n"], info["p_elem_bytes"], info["p_layout"], info["total_bytes"]) == \
        (1, e.N, n, elem_bytes(precision), 0, blob.size)
    assert info["desc_bytes"] == DESC_BYTES and info["desc_flags"] == 0 and info["section_mask"] == eng_mod.MAP_TEMPLATES
    assert info["cam"]["fx"] == cam.fx and info["cam"]["pixelsX"] == cam.pixelsX
    bare = mb.parse(e.save_map(0))  # without the templates
    assert bare["section_mask"] == 0 and bare["sections"][mb.P] == p["sections"][mb.P]
    # as uploaded, made asymmetric on purpose: the full square, both triangles in the bytes
    x, fp, P = e.get_state()
    t, _ = e.feature_layout()
    desc, _, _ = e.get_map_features()
    Pa = np.float32(P).astype(np.float64) if elem_bytes(precision) == 4 else P.copy()
    Pa[0, e.n - 1] += 0.5
    Pa[e.n // 2, 1] += np.float64(np.float32(0.25))
    assert not np.array_equal(Pa, Pa.T)
    e.set_state(x, fp, t, desc[: e.N], Pa)
    blob = e.save_map()
    assert blob.dtype == np.uint8 and blob.size == e.map_blob_bytes()
    want = reference_blob(e, cam, mb.FULL, templates=np.zeros((e.N, 363), np.uint8))
    assert blob.tobytes() == want.tobytes()
    p = mb.parse(blob)
    assert (p["p_layout"], p["p_elem_bytes"], p["n"]) == (mb.FULL, elem_bytes(precision), e.n)
    back = mb.P_of(p).astype(np.float64)
    assert same_bits(back, e.get_state()[2]) and back[0, e.n - 1] != back[e.n - 1, 0]


# ------------------------------------------------------------------------------------- 2. templates and warp tables
def golden_frames():
    from PIL import Image

    return [np.asarray(Image.open(os.path.join(FRAMES, f"{k:05d}.png"))) for k in range(8)]


NF = 12  # captured features of the golden-frame engines


def golden_engine(eng_mod, frames, steps, cap=96, modes=True, precision=F64, desc=None):
    e = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), cap, precision=precision)
    e.set_sweep_mode(SWEEP_LAUNCHES)
    if modes:
        e.set_template_warp(True)
        e.set_patch_normals(True)
    e.reset()
    e.upload_image(frames[0])
    uv = e.detect_new_features(NF, min_response=1e10)
    assert len(uv) == NF
    e.add_features(uv, desc)
    e.capture_templates(np.arange(NF), uv)
    for t in range(1, 1 + steps):
        assert e.step_image(frames[t]).status == 0
    return e, uv


def test_optional_sections_hold_the_tables(eng_mod):
    frames = golden_frames()
    e, uv = golden_engine(eng_mod, frames, 0)
    x0 = e.get_state(want_P=False)[0]
    pyr = [e.image_level(l) for l in range(3)]
    p = mb.parse(e.save_map())
    assert p["section_mask"] == 7
    tm = np.frombuffer(p["sections"][mb.TEMPLATES], np.uint8).reshape(NF, 3, 11, 11)
    ws = np.frombuffer(p["sections"][mb.WARP_SOURCES], np.uint8).reshape(NF, 3, 41, 41)
    wp = np.frombuffer(p["sections"][mb.WARP_POSES], "<f8").reshape(NF, 9)
    for i in range(NF):
        assert np.array_equal(tm[i], tw.stored_templates(pyr, uv[i])), i
        assert np.array_equal(ws[i], tw.source_patches(pyr, uv[i])), i
        assert same_bits(wp[i], np.concatenate([x0[:7], uv[i]])), i  # capture state and pixel
    assert p["sections"][mb.PATCH_NORMALS] == bytes(48 * NF)  # no estimate yet
    for t in range(1, 4):
        assert e.step_image(frames[t]).status == 0
    e.set_patch_normal(3, [0.25, -0.125], (2.0, 0.5, 3.0))
    p = mb.parse(e.save_map())
    rec = np.frombuffer(p["sections"][mb.PATCH_NORMALS], np.dtype([("pq", "<f8", 2), ("info", "<f8", 3), ("updates", "<i4"), ("pad", "<i4")]))
    got = e.patch_normals()
    est = rec["updates"] > 0
    assert est[3] and est.sum() >= 2
    np.testing.assert_array_equal(rec["updates"], got["updates"])
    assert same_bits(rec["pq"][est], got["pq"][est]) and same_bits(rec["info"][est], got["info"][est])
    assert same_bits(rec["pq"][3], np.array([0.25, -0.125]))
    _, tp, tmm = e.get_map_features()
    assert p["sections"][mb.TIMES_PREDICTED] == tp[:NF].tobytes() and p["sections"][mb.TIMES_MATCHED] == tmm[:NF].tobytes() and tp.sum() > 0
    # a section whose table was never allocated is simply absent
    plain, _ = golden_engine(eng_mod, frames, 0, modes=False)
    q = mb.parse(plain.save_map())
    assert q["section_mask"] == 1 and mb.WARP_SOURCES not in q["sections"] and mb.PATCH_NORMALS not in q["sections"]


# ------------------------------------------------------------------------------ 3. round trip into a different engine
def test_round_trip_into_a_larger_engine(eng_mod):
    frames = golden_frames()
    src, _ = golden_engine(eng_mod, frames, 4)
    src.set_patch_normal(1, [0.5, 0.25])
    blob = src.save_map()
    dst = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), 160)
    dst.set_sweep_mode(SWEEP_LAUNCHES)
    info = dst.load_map(blob)
    assert (info["N"], info["n"], info["section_mask"], info["total_bytes"]) == (src.N, src.n, 7, blob.size)
    a, b = snapshot(src, False), snapshot(dst, False)
    assert_same(a, b, "getters after the load", skip=("unseen",))
    assert same_bits(a["P"], b["P"]) and same_bits(a["P"].T.copy(), b["P"].T.copy())  # both triangles
    assert same_bits(src.patch_normals(), dst.patch_normals())
    assert dst.save_map().tobytes() == blob.tobytes()
    # one match on the same frame compares the same (warped) templates: the modes are settings and are set by the caller
    dst.set_template_warp(True)
    dst.set_patch_normals(True)
    res = []
    for e in (src, dst):
        e.predict()
        preds, _, _ = e.predict_measurements()
        e.upload_image(frames[5])
        m = e.match_ncc()
        res.append((preds.copy(), m.copy(), e.match_templates(np.arange(e.N)).copy(), e.template_warp_counts()))
    assert len(res[0][0]) > 0 and len(res[0][1]) > 0 and res[0][3][0] > 0
    for u, v in zip(res[0][:3], res[1][:3]):
        assert same_bits(u, v)
    assert res[0][3] == res[1][3]


# ------------------------------------------------------------------------------------------------ 4. continuation
def assert_step_equal(a, b, ia, ib, what):
    assert info_tuple(ia) == info_tuple(ib), what
    sa, sb = snapshot(a, False), snapshot(b, False)
    assert_same(sa, sb, what)


def test_continuation_on_images_is_bit_identical(eng_mod):
    frames = golden_frames()
    src, _ = golden_engine(eng_mod, frames, 4)
    dst = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), 128)
    dst.set_sweep_mode(SWEEP_LAUNCHES)
    dst.set_template_warp(True)
    dst.set_patch_normals(True)
    dst.load_map(src.save_map())
    matched = 0
    for t in (5, 6, 7):
        ia, ib = src.step_image(frames[t]), dst.step_image(frames[t])
        assert_step_equal(src, dst, ia, ib, f"frame {t}")
        assert same_bits(src.patch_normals(), dst.patch_normals())
        matched += ia.n_inliers + ia.n_rescued
    assert matched > 0
    assert src.save_map().tobytes() == dst.save_map().tobytes()


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
def test_continuation_on_keypoints_is_bit_identical(eng_mod, precision):
    seq = SyntheticSequence(50, 5)
    mk = lambda cap: eng_mod.EkfEngine(seq.cam, seq.par, cap, max_keypoints=4 * seq.n_features + 64, precision=precision)  # noqa: E731
    src, dst = mk(seq.n_features), mk(seq.n_features + 40)
    for e in (src, dst):
        e.set_sweep_mode(SWEEP_LAUNCHES)
    src.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for kps, desc in seq.frames[:2]:
        src.step(kps, desc)
    blob = src.save_map()
    assert mb.parse(blob)["p_layout"] == mb.TRIANGLE
    dst.load_map(blob)
    for t in (2, 3, 4):
        ia, ib = src.step(*seq.frames[t]), dst.step(*seq.frames[t])
        assert ia.n_inliers > 0
        assert_step_equal(src, dst, ia, ib, f"frame {t}")


# ------------------------------------------------------------------------------------------------ 5. across precisions
@pytest.mark.parametrize("layout", ["triangle", "full"])
@pytest.mark.parametrize("size", ["n67", "scene259"])
def test_across_storage_types(eng_mod, size, layout):
    blobs, snaps = {}, {}
    for prec in (F64, F32_EXACT):
        e = sized_engine(eng_mod, size, prec)
        if layout == "triangle":
            e.predict()
        else:  # an uploaded covariance that is not symmetric
            x, fp, P = e.get_state()
            P[0, e.n - 1] += 0.5
            e.set_state(x, fp, e.feature_layout()[0], e.get_map_features()[0], P)
        blobs[prec], snaps[prec] = e.save_map(), snapshot(e, False)
        assert mb.parse(blobs[prec])["p_layout"] == (mb.TRIANGLE if layout == "triangle" else mb.FULL)
    for frm, to in ((F64, F32_EXACT), (F32_EXACT, F64)):
        d = sized_engine(eng_mod, "empty", to, extra=snaps[frm]["N"] + 3)
        info = d.load_map(blobs[frm])
        assert info["p_elem_bytes"] == elem_bytes(frm)
        got = snapshot(d, False)
        P_src = snaps[frm]["P"]
        want = np.float32(P_src).astype(np.float64) if to == F32_EXACT else P_src  # rounded once to nearest / widened exactly
        assert same_bits(got["P"], want), (frm, to)
        if frm == F64:
            assert not np.array_equal(want, P_src)
        assert_same(snaps[frm], got, (frm, to), skip=("P", "points", "unseen"))
        assert mb.parse(d.save_map())["p_elem_bytes"] == elem_bytes(to)


# ----------------------------------------------------------------------------------- 6. refusals leave nothing changed
def flip(blob, at, bit=0x10):
    b = blob.copy()
    b[at] ^= bit
    return b


def section_offset(blob, sid):
    return int(np.frombuffer(blob[64 + 32 * sid + 8: 64 + 32 * sid + 16].tobytes(), "<u8")[0])


def refusal_cases(blob):
    """(label, blob, status, word the message must hold)"""
    p = mb.parse(blob)
    n = p["n"]
    out = [("truncated by one byte", blob[:-1], INVALID_ARG, "total_bytes"), ("truncated by half", blob[: blob.size // 2], INVALID_ARG, "total_bytes"),
           ("bad magic", flip(blob, 3), INVALID_ARG, "magic"),
           ("version 2", mb.refresh_header_checksum(np.concatenate([blob[:8], np.array([2, 0, 0, 0], np.uint8), blob[12:]])), INVALID_ARG, "version")]
    for sid, sec in p["sections"].items():
        if len(sec):
            out.append((f"flipped bit in {mb.NAMES[sid]}", flip(blob, section_offset(blob, sid) + len(sec) // 2), INVALID_ARG, mb.NAMES[sid]))
    ft = np.frombuffer(p["sections"][mb.FEAT_TYPE], "<i4").copy()
    bad = ft.copy()
    bad[2] = 7
    out.append(("a FEAT_TYPE of 7", mb.reassemble(p, {mb.FEAT_TYPE: bad.tobytes()}), INVALID_ARG, "FEAT_TYPE"))
    bad = ft.copy()
    bad[2] = 1  # an inverse-depth feature declared XYZ: the types sum to n - 3
    out.append(("n inconsistent with the types", mb.reassemble(p, {mb.FEAT_TYPE: bad.tobytes()}), INVALID_ARG, "n = "))
    dt = "<f4" if p["p_elem_bytes"] == 4 else "<f8"
    sec = np.frombuffer(p["sections"][mb.P], dt).copy()
    bad = sec.copy()
    bad[mb.tri_row(n // 2, n) + 3] = np.nan
    out.append(("one NaN in P, checksums right", mb.reassemble(p, {mb.P: bad.tobytes()}), NON_FINITE, "not finite"))
    bad = sec.copy()
    bad[mb.tri_row(n - 2, n)] = 0.0
    out.append(("a zero diagonal entry, checksums right", mb.reassemble(p, {mb.P: bad.tobytes()}), NON_FINITE, "diagonal"))
    return out


@pytest.mark.parametrize("precision", [F64, F32_EXACT])
def test_refusals_leave_the_engine_unchanged(eng_mod, precision):
    frames = golden_frames()
    src, _ = golden_engine(eng_mod, frames, 2)
    blob = src.save_map()
    assert mb.parse(blob)["p_layout"] == mb.TRIANGLE
    if precision != F64:  # the same map in the other storage type, through the reference
        p = mb.parse(blob)
        blob = mb.reassemble(p, {mb.P: mb.pack_P(mb.P_of(p), 4, mb.TRIANGLE).tobytes()}, p_elem_bytes=4)
    e = sized_engine(eng_mod, "n61", precision, extra=20)
    e.set_template_warp(True)  # (the tables a load would allocate exist already: the engine's own blob has the same sections throughout)
    e.set_patch_normals(True)
    e.predict()
    before = snapshot(e)
    cases = refusal_cases(blob)
    assert len(cases) >= 4 + 12 + 4
    for label, bad, status, word in cases:
        with pytest.raises(eng_mod.EkfError) as ei:
            e.load_map(bad)
        assert ei.value.code == status and word in str(ei.value), (label, str(ei.value))
        assert_same(before, snapshot(e), label)
        if status == INVALID_ARG:  # the host-only check refuses them too, P's checksum included
            with pytest.raises(eng_mod.EkfError):
                eng_mod.map_blob_info(bad)
    with pytest.raises(eng_mod.EkfError):
        eng_mod.map_blob_info(flip(blob, section_offset(blob, mb.P) + 5))  # the host-only check covers P's checksum too
    e.load_map(blob)  # and the blob itself is fine
    assert e.N == NF


def test_refusals_by_the_engine_itself(eng_mod):
    src = sized_engine(eng_mod, "n67", F64)
    src.predict()
    blob = src.save_map()
    small = sized_engine(eng_mod, "empty", F64)  # max_features 4 < 9
    before = snapshot(small)
    with pytest.raises(eng_mod.EkfError) as ei:
        small.load_map(blob)
    assert ei.value.code == CAPACITY and "max_features" in str(ei.value)
    assert_same(before, snapshot(small), "capacity")
    l2 = eng_mod.EkfEngine(s3_camera(), s3_params(), 16, descriptor_cols_f32=8)
    l2.reset()
    before = snapshot(l2)
    with pytest.raises(eng_mod.EkfError) as ei:
        l2.load_map(blob)
    assert ei.value.code == INVALID_ARG and "desc" in str(ei.value)
    assert_same(before, snapshot(l2), "descriptor format")
    seq = SyntheticSequence(12, 1)
    grp = LocalShardGroup(seq.cam, seq.par, seq.n_features, 2, max_keypoints=4 * seq.n_features + 64)
    grp.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, 0.5 * (seq.P0 + seq.P0.T))
    sh = grp.engines[0]
    view = lambda: (sh.n, sh.N, sh.get_state()[0].tobytes(), sh.get_state()[2].tobytes())  # noqa: E731
    before = view()
    for call in (lambda: sh.load_map(blob), sh.save_map, sh.map_blob_bytes):
        with pytest.raises(eng_mod.EkfError) as ei:
            call()
        assert ei.value.code == INVALID_ARG and "sharded" in str(ei.value)
    assert view() == before
    grp.close()
    # a save into a buffer that is too small: the size needed, nothing written
    import ctypes as C

    need, buf = C.c_size_t(0), np.full(blob.size - 1, 0xAB, np.uint8)
    rc = src.L.ekf_save_map(src.h, 7, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(need))
    assert rc == CAPACITY and need.value == blob.size and (buf == 0xAB).all()


# ------------------------------------------------------------------------------ 7. save is read-only, and off is off
def test_save_changes_nothing(eng_mod):
    seq = SyntheticSequence(50, 5)
    engines = []
    for _ in range(2):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=F32_EXACT)
        e.set_sweep_mode(SWEEP_LAUNCHES)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        for kps, desc in seq.frames[:2]:
            e.step(kps, desc)
        engines.append(e)
    saver, plain = engines
    before = snapshot(saver, False)
    first = saver.save_map()
    assert_same(before, snapshot(saver, False), "after a save")
    assert saver.save_map().tobytes() == first.tobytes()
    for t in (2, 3, 4):
        ia, ib = saver.step(*seq.frames[t]), plain.step(*seq.frames[t])
        assert_step_equal(saver, plain, ia, ib, f"frame {t}")
        saver.save_map()


# ------------------------------------------------------------------------------------------------ 8. pending errors
def test_a_pending_asynchronous_error_is_reported_first(eng_mod):
    seq = SyntheticSequence(12, 1, outlier_fraction=0.0, distractors_per_feature=0.0, max_bit_flips=0)
    good = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=len(seq.frames[0][0]) + 64)
    good.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    good.predict()
    blob = good.save_map()
    for call in ("save", "load"):
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=len(seq.frames[0][0]) + 64)
        e.set_async_errors(True)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, indefinite_between_two_features(seq))
        assert e.step(*seq.frames[0]).status == 0  # the failure of its last update is not read back
        with pytest.raises(eng_mod.EkfError) as ei:
            e.save_map() if call == "save" else e.load_map(blob)
        assert ei.value.code == NOT_POSITIVE_DEFINITE and "positive definite" in str(ei.value)
        a = snapshot(e, False)  # (reported and cleared above) nothing else was done
        assert a["N"] == seq.n_features and not same_bits(a["P"], good.get_state()[2])
        e.load_map(blob)  # asked again, it loads
        assert_same(snapshot(good, False), snapshot(e, False), call, skip=("unseen",))


def test_a_load_leaves_no_update_to_retry(eng_mod):
    """A persistent sweep that timed out unread (ekf_set_async_errors, the stall hook) is run again by the call that finds it: the
    load, on the map the update belongs to.  The steps behind the load retry nothing and equal those of a fresh engine."""
    seq = SyntheticSequence(170, 4, seed=5)
    mk = lambda: eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=4 * seq.n_features + 64, precision=F32_EXACT)  # noqa: E731
    donor = mk()
    donor.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    donor.step(*seq.frames[0])
    blob = donor.save_map()
    e, fresh = mk(), mk()
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.upload_frames(seq.frames)
    e.set_async_errors(True)
    e.stall_sweep(1)  # the second update of frame 0: the step returns with the time-out unread
    assert e.step_frame(0).status == 0
    e.load_map(blob)
    retries = e.sweep_retries
    assert retries == 1
    fresh.load_map(blob)
    for g in (e, fresh):
        g.set_sweep_mode(SWEEP_LAUNCHES)  # (the time-out's back-off would otherwise choose another sweep for e than for fresh)
    for t in (1, 2):
        ia, ib = e.step(*seq.frames[t]), fresh.step(*seq.frames[t])
        e.synchronize()
        assert e.sweep_retries == retries
        assert (ia.n_predicted, ia.n_matches, ia.n_inliers, ia.n_rescued) == (ib.n_predicted, ib.n_matches, ib.n_inliers, ib.n_rescued)
        assert_same(snapshot(e, False), snapshot(fresh, False), f"frame {t}")


def test_set_state_disarms_the_retry_of_an_unread_update(eng_mod):
    """The same unread time-out, then ekf_set_state: the map has changed under the update, so the call that finds the time-out
    reports it (EKF_ERR_TIMEOUT, once) and does not run the update again on the new map; the engine then steps like a fresh one."""
    seq = SyntheticSequence(170, 2, seed=5)
    mk = lambda: eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=4 * seq.n_features + 64, precision=F32_EXACT)  # noqa: E731
    e, fresh = mk(), mk()
    for g in (e, fresh):
        g.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.upload_frames(seq.frames)
    e.set_async_errors(True)
    e.stall_sweep(1)
    assert e.step_frame(0).status == 0
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    with pytest.raises(eng_mod.EkfError) as ei:
        e.synchronize()
    assert ei.value.code == 8 and e.sweep_retries == 0  # EKF_ERR_TIMEOUT, reported and not retried
    e.synchronize()  # once
    assert_same(snapshot(fresh, False), snapshot(e, False), "after set_state", skip=("unseen",))
    for g in (e, fresh):
        g.set_sweep_mode(SWEEP_LAUNCHES)
    ia, ib = e.step(*seq.frames[0]), fresh.step(*seq.frames[0])
    e.synchronize()
    assert e.sweep_retries == 0
    assert (ia.n_predicted, ia.n_matches, ia.n_inliers, ia.n_rescued) == (ib.n_predicted, ib.n_matches, ib.n_inliers, ib.n_rescued)
    assert_same(snapshot(e, False), snapshot(fresh, False), "the step behind it")


# ------------------------------------------------------------------------------------------- 9. the seam and the sample
def read_output_frames(path):
    import re

    import yaml

    doc = yaml.safe_load(re.sub(r"!!opencv-matrix", "", open(path).read().split("\n", 1)[1]))
    return [doc[k] for k in sorted((k for k in doc if k.startswith("Frame ")), key=lambda s: int(s.split()[1]))]


def test_driver_class_and_sample(eng_mod, tmp_path):
    """ImageEKF::saveMap / loadMap (tests/cpp/map_blob_seam_check.cpp), then ekf_sequence twice: frames 0..4 with --save-map, and
    frames 5..7 with --load-map and --fixed-map-from 0 -- that process captures no template, yet its first step predicts and
    matches, and the poses in its output.yml are those of one Python engine that loaded the same file and stepped the same frames."""
    import subprocess

    from tests.test_gpu_map_points import s3_config_320

    pkg = os.path.join(ROOT, "openekfmonoslam_amd")
    link = ["-L", pkg, "-lekf_engine", "-lz", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"]
    check_bin, sample = str(tmp_path / "map_blob_seam_check"), str(tmp_path / "ekf_sequence")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", check_bin, os.path.join(ROOT, "tests", "cpp", "map_blob_seam_check.cpp")] + link)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-o", sample, os.path.join(ROOT, "samples", "ekf_sequence.cpp")] + link)
    cfg = tmp_path / "config.yml"
    cfg.write_text(s3_config_320(40))
    r = subprocess.run([check_bin, str(cfg), FRAMES + "/", "1e10", str(tmp_path / "seam.map")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "truncated file refused" in r.stdout and len([ln for ln in r.stdout.splitlines() if ln.startswith("step") and "same 1" in ln]) == 3
    out1, out2, mapfile = tmp_path / "first", tmp_path / "second", tmp_path / "run.map"
    out1.mkdir()
    out2.mkdir()
    r = subprocess.run([sample, str(cfg), FRAMES + "/", str(out1) + "/", "0", "4", "1e10", "--warp-templates", "--save-map", str(mapfile)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "saved map" in r.stdout, r.stdout + r.stderr
    blob = np.fromfile(str(mapfile), dtype=np.uint8)
    info = eng_mod.map_blob_info(blob)
    assert info["N"] > 0 and info["section_mask"] & eng_mod.MAP_WARP_SOURCES
    r = subprocess.run([sample, str(cfg), FRAMES + "/", str(out2) + "/", "5", "7", "1e10", "--warp-templates", "--load-map", str(mapfile),
                        "--fixed-map-from", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "init:" not in r.stdout and f"loaded map: {info['N']} features" in r.stdout
    steps = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert len(steps) == 3 and int(steps[0][3]) > 0 and int(steps[0][5]) > 0  # predicted, matches: no template was cut here
    assert r.stdout.count("fixed map: on") == 3
    # one Python engine, the same file, the same frames, the same settings
    frames = golden_frames()
    e = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), 256)
    e.set_template_warp(True)
    e.load_map(blob)
    e.set_fixed_map(True)
    want = []
    for t in (5, 6, 7):
        assert e.step_image(frames[t]).status == 0
        want.append(e.get_state(want_P=False)[0])
    got = read_output_frames(str(out2 / "output.yml"))
    assert len(got) == 3
    for t, (g, x) in enumerate(zip(got, want)):
        pose = np.array([float(v) for v in g["StateEstimation"]["data"]])  # %.16e: the doubles themselves
        assert same_bits(pose, x), (t, pose, x)
