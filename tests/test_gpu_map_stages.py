"""Stage tests of map management (csrc/kernels_map.hip: k_addfeat_prepare / _rows / _corner, k_compact_P, k_linearity,
k_convert_prepare / _rows / _apply; host halves ekf_add_features, compact_map, ekf_convert_inverse_depth_to_depth in csrc/map_host.cpp)
through the C ABI, PER ENTRY against tests/map_ref.py (numpy, np.longdouble), at the sizes where the launches change shape.

Every bound is derived, not measured (map_ref.py: u_store |ref| + K u64 sum|terms|, K counted from the kernel's operations; moved
or untouched entries: bit for bit); the tests print the worst |device - reference| / tolerance per output so that the margin is on
record (DESIGN.md lists what the MI355X gave).  tests/test_map_ref_cpu.py holds the reference to the oracle within the same bounds
and checks the input conditions assumed here.  Everything is read through get_state, feature_layout (the host mirrors), map_points
(type, covpos and the counters come from the device arrays) and get_map_features."""
import numpy as np
import pytest

import map_ref as mr
import predict_ref as pr
from openekfmonoslam_amd.ekftypes import (DESC_BYTES, FEATURE_DEPTH, FEATURE_INVERSE_DEPTH, KEYPOINT_DTYPE, STATUS_NAMES, s3_camera,
                                          s3_params)
from openekfmonoslam_amd.synth import SyntheticSequence

pytestmark = pytest.mark.gpu

F64, F32, F32_EXACT, F64_EXACT = 0, 1, 2, 3
NO_KPS = (np.zeros(0, dtype=KEYPOINT_DTYPE), np.zeros((0, DESC_BYTES), dtype=np.uint8))


def u_store(precision):
    return pr.U32 if precision in (F32, F32_EXACT) else 0.0


def with_precisions(cases, starred):
    """every case in fp64 and fp32 storage, the starred ones also in the two exact configurations"""
    return [(*c, p) for c in cases for p in (F64, F32)] + [(*c, p) for c in starred for p in (F32_EXACT, F64_EXACT)]


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def report(what, n, dev, ref, tol, precision=F64):
    r, at = pr.worst_ratio(dev, ref, tol)
    print(f"\nmap stages: {what:12s} precision {precision} n {n:4d}: worst |dev - ref| / tol = {r:.3f} at {at}", end="")
    return r, at


def descriptors(N, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, DESC_BYTES), dtype=np.uint8)


def snapshot(e):
    """everything a map operation may touch, host mirrors and device arrays"""
    x, fp, P = e.get_state()
    desc, tp, tm = e.get_map_features()
    t, c = e.feature_layout()
    mp = e.map_points()
    return {"n": e.n, "N": e.N, "x": x, "fp": fp, "P": P, "desc": desc, "tp": tp, "tm": tm, "type": t.copy(), "covpos": c.copy(),
            "dev_type": mp["type"].copy(), "dev_covpos": mp["covpos"].copy(), "dev_tp": mp["times_predicted"].copy(),
            "dev_tm": mp["times_matched"].copy()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_unchanged(before, after, what):
    for k in before:
        if isinstance(before[k], np.ndarray):
            assert same_bits(before[k], after[k]), (what, k)
        else:
            assert before[k] == after[k], (what, k)


def check_layout(snap, types, covpos, what=""):
    for k in ("type", "dev_type"):
        np.testing.assert_array_equal(snap[k], types, err_msg=f"{what} {k}")
    for k in ("covpos", "dev_covpos"):
        np.testing.assert_array_equal(snap[k], covpos, err_msg=f"{what} {k}")
    np.testing.assert_array_equal(snap["dev_tp"], snap["tp"])
    np.testing.assert_array_equal(snap["dev_tm"], snap["tm"])


def error_code(call):
    from openekfmonoslam_amd.engine import EkfError

    with pytest.raises(EkfError) as ei:
        call()
    return STATUS_NAMES[ei.value.code]


# ------------------------------------------------------------------------------------------------ add
def check_add(e, cam, par, uv, desc, precision):
    """one ekf_add_features(uv, desc) on e as it stands, per entry against map_ref.add_ref built from the state e returns"""
    b = snapshot(e)
    n_old, N_old, count = b["n"], b["N"], len(uv)
    e.add_features(uv, desc)
    a = snapshot(e)
    assert (a["n"], a["N"]) == (n_old + 6 * count, N_old + count)
    ref = mr.add_ref(b["x"], b["P"], cam, par, uv, u_store(precision))
    g = ref["g"]
    assert (g[:, 0] ** 2 + g[:, 2] ** 2 >= 0.25).all()  # the input condition of the bounds on theta, phi and the Jacobians
    P = a["P"]
    bad = []
    for name, got, (want, tol) in (("feature_pos", a["fp"][N_old:], ref["feature_pos"]),
                                   ("rows", P[n_old:, :n_old].reshape(count, 6, n_old), ref["rows"]),
                                   ("columns", P[:n_old, n_old:].T.reshape(count, 6, n_old), ref["rows"]),
                                   ("corner", P[n_old:, n_old:], ref["corner"])):
        r, at = report(name, n_old, got, want, tol, precision)
        if not (r <= 1.0):  # (a NaN is a failure)
            bad.append((name, r, at))
    assert not bad, bad
    assert same_bits(P[:n_old, :n_old], b["P"]) and same_bits(a["x"], b["x"]) and same_bits(a["fp"][:N_old], b["fp"])
    np.testing.assert_array_equal(P, P.T)
    check_layout(a, np.concatenate([b["type"], np.full(count, FEATURE_INVERSE_DEPTH, dtype=np.int32)]),
                 np.concatenate([b["covpos"], n_old + 6 * np.arange(count, dtype=np.int32)]), "add")
    np.testing.assert_array_equal(a["desc"][:N_old], b["desc"])
    np.testing.assert_array_equal(a["desc"][N_old:], np.zeros((count, DESC_BYTES), np.uint8) if desc is None else desc)
    for k in ("tp", "tm"):
        np.testing.assert_array_equal(a[k][:N_old], b[k])
        assert (a[k][N_old:] == 0).all(), k
    return a


def engine_before_add(eng_mod, n_old, room, precision):
    """a map of n_old columns (13: after reset) with room for `room` more features, one prediction behind it: q, R and P[0:7, :]
    are general"""
    if n_old == 13:
        cam, par = s3_camera(), s3_params()
        e = eng_mod.EkfEngine(cam, par, room, max_keypoints=64, precision=precision)
        e.reset()
    else:
        s = pr.scene_for_n(n_old)
        cam, par = s.cam, s.par
        e = eng_mod.EkfEngine(cam, par, s.n_features + room, max_keypoints=64, precision=precision)
        e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(s.n_features, n_old), s.P0)
    e.predict()
    assert e.n == n_old
    return e, cam, par


ADD_CASES = with_precisions([(n, c) for n in mr.ADD_N_OLD for c in mr.ADD_COUNTS], mr.ADD_STARRED) + [(*mr.ADD_FULL_WORKGROUPS, F64)]


@pytest.mark.parametrize("n_old,count,precision", ADD_CASES)
def test_add_features_per_entry(eng_mod, n_old, count, precision):
    """n_old = 253 / 256 / 259: the last thread of workgroup 0 of k_addfeat_rows idle, busy, and three threads in workgroup 1;
    511 / 514 the same around the second seam.  count = 65: a second block of k_addfeat_prepare and a 65 x 65 corner grid.  The
    n_old = 13 cases fill the map to its capacity: the last row and column of the allocation are written.  n_old = 1024: four
    workgroups full to the last thread (map_ref.ADD_FULL_WORKGROUPS)."""
    e, cam, par = engine_before_add(eng_mod, n_old, count, precision)
    check_add(e, cam, par, mr.add_pixels(count), descriptors(count, 7), precision)


@pytest.mark.parametrize("precision", [F64, F32])
def test_add_up_to_capacity_then_refused_without_a_trace(eng_mod, precision):
    """64 features, then one on top that fills the map exactly (n = 13 + 6 cap); the next one returns EKF_ERR_CAPACITY and changes
    no bit of x, features, P, layouts, descriptors or counters"""
    e, cam, par = engine_before_add(eng_mod, 13, 65, precision)
    uv = mr.add_pixels(66)
    e.add_features(uv[:64], descriptors(64, 1))
    check_add(e, cam, par, uv[64:65], descriptors(1, 2), precision)
    assert (e.N, e.n) == (65, 13 + 6 * 65)
    before = snapshot(e)
    assert error_code(lambda: e.add_features(uv[65:66], descriptors(1, 3))) == "EKF_ERR_CAPACITY"
    assert_unchanged(before, snapshot(e), "refused add")


def test_new_features_get_their_own_descriptors_and_zero_counters(eng_mod, seq50):
    """two frames (non-zero counters), three features removed (their slots behind N keep the old descriptors and counters), two
    added without descriptors -- all zero, not the removed features' -- and two with"""
    seq = seq50
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=len(seq.frames[0][0]) + 64)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for t in range(2):
        e.step(*seq.frames[t])
    b = snapshot(e)
    assert (b["tp"][47:] > 0).all() and (b["tm"][47:] > 0).all() and (b["desc"][47:].max(axis=1) > 0).all()  # what slots 47.. keep
    e.remove_features([3, 20, 49])
    keep = np.delete(np.arange(50), [3, 20, 49])
    a = snapshot(e)
    np.testing.assert_array_equal(a["tp"], b["tp"][keep])
    np.testing.assert_array_equal(a["tm"], b["tm"][keep])
    check_layout(a, b["type"][keep], 13 + 6 * np.arange(47), "remove")
    check_add(e, seq.cam, seq.par, mr.add_pixels(2), None, F64)  # (checks zero descriptors, zero counters, kept counters)
    check_add(e, seq.cam, seq.par, mr.add_pixels(2, salt=5), descriptors(2, 9), F64)
    np.testing.assert_array_equal(e.get_map_features()[1][:47], b["tp"][keep])


STATE_CHANGES = ["set_state", "predict", "step", "update_only_state", "fuse_camera_position"]


@pytest.mark.parametrize("precision", [F64, F32])
@pytest.mark.parametrize("change", STATE_CHANGES)
def test_add_uses_the_rotation_of_the_current_state(eng_mod, seq50, change, precision):
    """the device takes R from the cache beside the state; the reference forms it from the q that get_state returns.  After every
    way the state changes, theta, phi and the new rows must follow q (a cache one change behind differs by the turn of that change)"""
    if change in ("step", "update_only_state"):
        seq = seq50
        cam, par = seq.cam, seq.par
        e = eng_mod.EkfEngine(cam, par, seq.n_features + 8, max_keypoints=len(seq.frames[0][0]) + 64, precision=precision)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        q0 = e.get_state(want_P=False)[0][3:7]
        if change == "step":
            assert e.step(*seq.frames[0]).n_inliers > 0
        else:
            e.predict()
            q0 = e.get_state(want_P=False)[0][3:7]
            e.predict_measurements()
            m = e.match(*seq.frames[0])
            assert len(m) > 0
            e.update_only_state(m)
    else:
        s = pr.scene_for_n(259)
        cam, par = s.cam, s.par
        e = eng_mod.EkfEngine(cam, par, s.n_features + 8, max_keypoints=64, precision=precision)
        e.set_state(s.x_poison, s.feature_pos, s.feature_type, s.desc, s.P0)
        q0 = e.get_state(want_P=False)[0][3:7]
        if change == "set_state":
            e.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, s.P0)
        elif change == "predict":
            e.predict()
        else:
            x = e.get_state(want_P=False)[0]
            out = e.fuse_camera_position(x[:3] + np.array([0.5, -0.3, 0.2]), 1e-6 * np.eye(3))
            assert out["applied"]
    q1 = e.get_state(want_P=False)[0][3:7]
    assert np.abs(q1 - q0).max() > 1e-9, "the change did not turn the camera: a stale R would not show"
    check_add(e, cam, par, mr.add_pixels(5), descriptors(5, 4), precision)


# ------------------------------------------------------------------------------------------------ remove
def check_remove(e, drop, what):
    b = snapshot(e)
    e.remove_features(drop)
    a = snapshot(e)
    new2old, nt, nc = mr.compact_index(b["type"], b["covpos"], drop)
    keep = np.delete(np.arange(b["N"]), drop)
    assert (a["n"], a["N"]) == (len(new2old), len(keep)), what
    assert same_bits(a["P"], b["P"][np.ix_(new2old, new2old)]), what  # a pure gather
    assert same_bits(a["x"], b["x"]) and same_bits(a["fp"], b["fp"][keep]) and same_bits(a["desc"], b["desc"][keep]), what
    check_layout(a, nt, nc, what)
    np.testing.assert_array_equal(a["tp"], b["tp"][keep])
    np.testing.assert_array_equal(a["tm"], b["tm"][keep])
    return a


def engine_for_removal(eng_mod, n0, precision):
    """the mixed map of n0 columns with random descriptors, one step on a frame without keypoints behind it: P is a predicted
    covariance and times_predicted is 1 for the features the camera sees, 0 for the others"""
    s = pr.scene_for_n(n0)
    e = eng_mod.EkfEngine(s.cam, s.par, s.n_features, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(s.n_features, n0), s.P0)
    e.step(*NO_KPS)
    tp = e.get_map_features()[1]
    assert 0 < tp.sum() < s.n_features
    return e


@pytest.mark.parametrize("n_new,kind,precision", with_precisions(mr.REMOVE_CASES, mr.REMOVE_STARRED))
def test_remove_features_is_a_gather_bit_for_bit(eng_mod, n_new, kind, precision):
    """n_new = 253 / 256 / 259 / 511 / 514: k_compact_P's last workgroup short of three threads, full, three threads into the next;
    13: every feature removed"""
    types, drop = mr.remove_case(n_new, kind)
    e = engine_for_removal(eng_mod, mr.layout(types)[1], precision)
    a = check_remove(e, drop, (n_new, kind))
    assert a["n"] == n_new


@pytest.mark.parametrize("precision", [F64, F32])
def test_two_removals_in_a_row(eng_mod, precision):
    """the second gather writes the buffer the first one read from, which still holds the larger matrix"""
    e = engine_for_removal(eng_mod, 514, precision)
    N = e.N
    a = check_remove(e, np.arange(0, N, 2), "first removal")
    check_remove(e, np.array([0, 1, a["N"] // 2, a["N"] - 1]), "second removal")
    e.predict()  # and the filter goes on from the compacted matrix
    x, _, P = e.get_state()
    assert np.isfinite(P).all() and np.array_equal(P, P.T)


def test_invalid_removal_lists_change_nothing(eng_mod):
    e = engine_for_removal(eng_mod, 301, F64)
    before = snapshot(e)
    for idx in ([5, 3], [3, 3], [-1], [e.N], [0, e.N], [2, 7, 7]):
        assert error_code(lambda: e.remove_features(idx)) == "EKF_ERR_INVALID_ARG", idx
        assert_unchanged(before, snapshot(e), idx)


# ------------------------------------------------------------------------------------------------ convert
@pytest.mark.parametrize("n,pos,precision", with_precisions(mr.CONVERT_CASES, mr.CONVERT_STARRED))
def test_convert_to_depth_per_entry(eng_mod, n, pos, precision):
    """the first inverse-depth feature at covariance position pos behind (pos - 13) / 3 XYZ features: 250 -- its block ends at
    column 255, the last of workgroup 0 of k_convert_rows / _apply; 253 -- it straddles the seam; 256 -- it begins workgroup 1;
    (259, 253) and (514, 508): it is the last feature, its block ends at column n - 1"""
    s = mr.convert_scene(n, pos)
    fi = (pos - 13) // 3
    e = eng_mod.EkfEngine(s.cam, mr.convert_params(), s.n_features, max_keypoints=64, precision=precision)
    e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(s.n_features, n + pos), s.P0)
    e.predict()
    b = snapshot(e)
    ref = mr.convert_ref(b["x"], b["fp"], b["type"], b["covpos"], b["P"], fi, u_store(precision))
    assert e.convert_inverse_depth_to_depth() == fi
    a = snapshot(e)
    assert (a["n"], a["N"]) == (n - 3, b["N"])
    mr.check_converted(lambda *args: report(*args, precision=precision), n, b["P"], a["P"], a["fp"], ref, fi, b["fp"])
    np.testing.assert_array_equal(a["P"], a["P"].T)
    nt = b["type"].copy()
    nt[fi] = FEATURE_DEPTH
    check_layout(a, nt, mr.layout(nt)[0], "convert")
    assert same_bits(a["x"], b["x"]) and same_bits(a["desc"], b["desc"]) and same_bits(a["tp"], b["tp"]) and same_bits(a["tm"], b["tm"])


@pytest.mark.parametrize("N,fstar", mr.SELECT_CASES)
def test_conversion_selects_the_one_feature_below_the_threshold(eng_mod, N, fstar):
    """k_linearity with 255 / 257 / 300 features: f* the first and the last thread of workgroup 0, the first of workgroup 1, the
    last feature; its index is a factor 4 below the threshold and every other one a factor 4 or more above (scene and rule:
    map_ref.select_scene, checked in longdouble by tests/test_map_ref_cpu.py).  No feature below it: -1, and no bit changes."""
    s, P, thr = mr.select_scene(N, fstar)
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = thr
    for precision in (F64, F32):
        e = eng_mod.EkfEngine(s.cam, par, N, max_keypoints=64, precision=precision)
        e.set_state(s.x13, s.feature_pos, s.feature_type, descriptors(N, N), P)
        b = snapshot(e)
        got = e.convert_inverse_depth_to_depth()
        a = snapshot(e)
        if fstar is None:
            assert got == -1, precision
            assert_unchanged(b, a, ("no conversion", precision))
        else:
            assert got == fstar, precision
            nt = b["type"].copy()
            nt[fstar] = FEATURE_DEPTH
            check_layout(a, nt, mr.layout(nt)[0], f"selection, precision {precision}")
            assert a["n"] == b["n"] - 3


# ------------------------------------------------------------------------------------------------ history independence
@pytest.mark.parametrize("precision", [F32_EXACT, F64])
def test_steps_after_map_operations_do_not_depend_on_the_history(eng_mod, precision):
    """Engine A: a step, 45 features removed, 10 added, one converted, three more steps.  Engine B: a fresh engine given A's state
    right behind the conversion, and the same three steps.  A's buffers hold what the larger map left beyond n (rows and columns
    of P, slots of the per-feature arrays); B's hold zeros there.  Launch-per-panel sweep: two runs of B (the control) agree bit
    for bit, and then A must equal B bit for bit; where the control does not, the bound is the 1e-12 of max|.| that
    test_concurrent_exact_engines_give_the_sequential_result uses for sums ordered by arrival."""
    seq = SyntheticSequence(100, 4)
    seq.par.inverseDepthLinearityIndexThreshold = 1e9
    mk = len(max((f[0] for f in seq.frames), key=len)) + 64

    def fresh():
        e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 16, max_keypoints=mk, precision=precision)
        e.set_sweep_mode(4)
        return e

    def finish(e):
        infos = [e.step(*seq.frames[t]) for t in (1, 2, 3)]
        assert all(i.status == 0 for i in infos) and infos[0].n_inliers > 0
        x, fp, P = e.get_state()
        return x, fp, P, np.array([(i.n_predicted, i.n_matches, i.n_inliers, i.n_rescued) for i in infos])

    A = fresh()
    A.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    A.step(*seq.frames[0])
    A.remove_features(np.arange(0, 90, 2))
    A.add_features(mr.add_pixels(10), descriptors(10, 8))
    assert A.convert_inverse_depth_to_depth() == 0
    mid = snapshot(A)
    assert (mid["N"], mid["n"]) == (65, 13 + 6 * 65 - 3)
    got = finish(A)
    runs = []
    for _ in range(2):
        B = fresh()
        B.set_state(mid["x"], mid["fp"], mid["type"], mid["desc"], mid["P"])
        assert_unchanged({k: mid[k] for k in ("x", "fp", "P", "type", "covpos")}, snapshot(B), "state handed to B")
        runs.append(finish(B))
    exact = all(same_bits(u, v) for u, v in zip(runs[0], runs[1]))
    print(f"history independence, precision {precision}: control runs bit-identical: {exact}")
    for name, u, v in zip(("x", "feature_pos", "P", "counts"), got, runs[0]):
        if exact:
            assert same_bits(u, v), (name, float(np.max(np.abs(u - v))))
        else:
            assert np.max(np.abs(u - v)) <= 1e-12 * max(np.max(np.abs(v)), 1e-300), (name, float(np.max(np.abs(u - v))))
