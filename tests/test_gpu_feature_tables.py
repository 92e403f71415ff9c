"""Every per-feature table through every operation that moves, adds, zeroes or replaces a feature's rows (csrc/feature_tables.h,
csrc/map_host.cpp), with the map blob as the window: a save shows FEAT_POS, FEAT_TYPE, DESC, the two counters, TEMPLATES,
WARP_SOURCES, WARP_POSES and PATCH_NORMALS in map order, so one engine is taken through remove, add, convert, replace and load,
and the sections are compared row by row.  Bytes throughout, no tolerance.  The rows the engine does not define (TEMPLATES and
WARP_SOURCES of features just added) are not asserted; that a map replacement leaves those two tables as they were is pinned."""
import numpy as np
import pytest

import map_blob_ref as mb
from openekfmonoslam_amd.ekftypes import DESC_BYTES, FEATURE_DEPTH, FEATURE_INVERSE_DEPTH, s3_camera, s3_params
from tests.test_gpu_map_blob import F32, F64, NF, SWEEP_LAUNCHES, eng_mod, golden_engine, golden_frames  # noqa: F401

pytestmark = pytest.mark.gpu

# bytes of one feature's row in each per-feature section
ROW_BYTES = {mb.FEAT_POS: 48, mb.FEAT_TYPE: 4, mb.DESC: DESC_BYTES, mb.TIMES_PREDICTED: 4, mb.TIMES_MATCHED: 4, mb.TEMPLATES: 363,
             mb.WARP_SOURCES: 3 * 41 * 41, mb.WARP_POSES: 72, mb.PATCH_NORMALS: 48}
ZEROED = (mb.TIMES_PREDICTED, mb.TIMES_MATCHED, mb.WARP_POSES, mb.PATCH_NORMALS)  # what an added feature and a replaced map start from
INVALID_ARG = 1


def S(e):
    """{section: uint8 [N, row bytes]} of the per-feature sections of the engine's own blob (absent ones left out)"""
    p = mb.parse(e.save_map())
    return {sid: np.frombuffer(p["sections"][sid], np.uint8).reshape(e.N, w) for sid, w in ROW_BYTES.items() if sid in p["sections"]}


def same_rows(a, b, what, only=None, but=()):
    assert set(a) == set(b) == set(ROW_BYTES), what
    for sid in (only or ROW_BYTES):
        if sid not in but:
            assert a[sid].shape == b[sid].shape and a[sid].tobytes() == b[sid].tobytes(), (what, mb.NAMES[sid])


def types_of(s):
    return s[mb.FEAT_TYPE].copy().view("<i4").reshape(-1)


@pytest.mark.parametrize("precision", [F64, F32])
def test_every_table_follows_every_operation(eng_mod, precision):
    frames = golden_frames()
    rng = np.random.default_rng(7)
    e, uv = golden_engine(eng_mod, frames, 3, cap=NF + 4, precision=precision, desc=rng.integers(1, 256, (NF, DESC_BYTES), dtype=np.uint8))
    e.set_patch_normal(3, [0.25, -0.125], (2.0, 0.5, 3.0))
    blob_a = e.save_map()
    A = S(e)
    for sid in ROW_BYTES:  # nothing below compares zeros with zeros
        assert A[sid].any(), mb.NAMES[sid]
    assert A[mb.WARP_POSES].any(axis=1).all() and A[mb.PATCH_NORMALS][3].any()

    # 1. remove: the survivors' rows of every table follow them
    drop = np.array([1, 5, 6, NF - 1], dtype=np.int32)  # the second, an adjacent pair in the middle, the last
    keep = np.setdiff1d(np.arange(NF), drop)
    e.remove_features(drop)
    B = S(e)
    assert e.N == len(keep)
    same_rows({sid: A[sid][keep] for sid in A}, B, "after remove_features")

    # 2. add: the old rows stay, the new ones start from zero and carry the given descriptors
    new_desc = rng.integers(1, 256, (2, DESC_BYTES), dtype=np.uint8)
    e.add_features(np.array([[100.5, 80.25], [201.0, 150.75]]), new_desc)
    C = S(e)
    K = len(keep)
    assert e.N == K + 2
    same_rows(B, {sid: C[sid][:K] for sid in C}, "old rows after add_features")
    for sid in ZEROED:
        assert not C[sid][K:].any(), ("new rows", mb.NAMES[sid])
    assert C[mb.DESC][K:].tobytes() == new_desc.tobytes()
    assert (types_of(C)[K:] == FEATURE_INVERSE_DEPTH).all()

    # 3. convert: a map whose inverse depths are known to 0.002 (as test_gpu_template_warp.test_tables_follow_map_management) is
    # convertible.  The set_state that makes it so zeroes counters, poses and normals (step 4 pins that), so some are planted again.
    x, fp, P = e.get_state()
    t, covpos = e.feature_layout()
    k = 0.002 / s3_params().inverseDepthRhoSD
    rows = covpos[t == FEATURE_INVERSE_DEPTH] + 5
    P[rows, :] *= k
    P[:, rows] *= k
    e.set_state(x, fp, t, e.get_map_features()[0], P)
    e.capture_templates(np.array([0, 4, K]), np.vstack([uv[keep][[0, 4]], [[100.5, 80.25]]]))  # (the last step's image is still loaded)
    e.set_patch_normal(2, [0.5, 0.25])
    e.set_patch_normal(K + 1, [-0.25, 0.125], (3.0, 0.25, 2.0))
    D = S(e)
    assert D[mb.DESC].any() and D[mb.WARP_POSES][[0, 4, K]].any(axis=1).all() and D[mb.PATCH_NORMALS][[2, K + 1]].any(axis=1).all()
    one = e.convert_inverse_depth_to_depth()  # through the compaction: rows of P dropped, no feature dropped
    assert one >= 0
    E = S(e)
    same_rows(D, E, "after a conversion", but=(mb.FEAT_TYPE, mb.FEAT_POS))
    assert np.flatnonzero(types_of(D) != types_of(E)).tolist() == [one] and types_of(E)[one] == FEATURE_DEPTH
    more = e.convert_all_inverse_depth_to_depth()  # the batch pass: no compaction
    assert len(more) >= 1
    F = S(e)
    same_rows(E, F, "after the batch conversion", but=(mb.FEAT_TYPE, mb.FEAT_POS))
    assert np.flatnonzero(types_of(E) != types_of(F)).tolist() == more.tolist() and (types_of(F)[more] == FEATURE_DEPTH).all()

    # 4. replace: counters, poses, normals and (none given) descriptors are zero; templates and source patches stay as they were
    x, fp, P = e.get_state()
    t, _ = e.feature_layout()
    e.set_state(x, fp, t, None, P)
    G = S(e)
    for sid in ZEROED + (mb.DESC,):
        assert not G[sid].any(), ("after set_state", mb.NAMES[sid])
    same_rows(F, G, "after set_state", only=(mb.TEMPLATES, mb.WARP_SOURCES, mb.FEAT_TYPE, mb.FEAT_POS))

    # 5. load: the first blob into a plain engine, which gets the tables it lacks and keeps its modes off
    dst = eng_mod.EkfEngine(s3_camera(320, 240), s3_params(), NF + 4, precision=precision)
    dst.set_sweep_mode(SWEEP_LAUNCHES)
    dst.load_map(blob_a)
    same_rows(A, S(dst), "after load_map")
    with pytest.raises(eng_mod.EkfError) as ei:  # the template warp is still off: its patch normals cannot be switched on
        dst.set_patch_normals(True)
    assert ei.value.code == INVALID_ARG and "template warp is off" in str(ei.value)
    assert dst.template_warp_counts() == (0, 0) and dst.patch_normal_counts() == (0, 0)
