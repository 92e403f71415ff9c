"""The EKF update on the device -- the exact int8 downdate k_p_update_i8p, the rows of B from digit planes, k_dx_planes, the
Cholesky sweep in its three forms, the inverse + GEMM route -- against the longdouble restatement of the operation
(tests/update_ref.py), EVERY entry of P and EVERY component of the state under a bound in the entry's own scale (derivation:
update_ref's docstring and DESIGN.md, "Stage tests of the update").  No exclusion list, no outlier share.

Each case: set_state (-> a position fix without information, so that the engine knows P as symmetric and the downdate is
k_p_update_i8p in fp32 storage too: fresh_engine) -> predict -> predict_measurements -> update(the first M predictions, a fraction of a pixel off); the
reference starts from what the engine holds after the two predictions (get_state, feature_layout, its own Hs and Hf) and is
cached per (map, M, stored bits), so one long-double update (compiled: tests/update_ref_fast.py) serves every configuration and route that starts from the same bits.

Maps.  Column edges: the mixed depth / inverse-depth maps of predict_ref.types_for_n at n = 85 ... 514 with a covariance built
by synth.seed_map on those scenes (update_ref.spiky_scene: variance 1 beside 2e-16; predict_ref.make_P0 is flat to three orders
and would hide the entries this file is about), M = 17.  Row edges and routes: SyntheticSequence(170, 1), n = 1033.  A converged
map: the same sequence after CONVERGED_FRAMES steps.

EKF_PRECISION_F32 (the fast configuration) is out of scope: it is documented not to meet component-wise parity
(parity_metric.FAST_COMPONENT_CEILING).  Updates around 2048 rows: tests/test_gpu_update_entries_large.py.  Sharded engines:
DESIGN.md names them among the remaining gaps."""
import hashlib

import numpy as np
import pytest

import update_ref as ur
import update_ref_fast as uf
from parity_metric import F32_TOL, F64_TOL, over_tolerance, parity_report
from openekfmonoslam_amd.synth import SyntheticSequence

pytestmark = pytest.mark.gpu
PRECISIONS = (0, 2, 3)  # fp64, F32_EXACT, F64_EXACT
SWEEP = 1               # EKF_UPDATE_PATH_SWEEP
GEMM = 2                # EKF_UPDATE_PATH_GEMM
MODES = {"auto": 2, "single": 1, "pairs": 0}  # EKF_SWEEP_AUTO (persistent at this size), _SINGLE, _PAIRS
CONVERGED_FRAMES = 8
_CORES = {}
WORST = {}              # (precision, route) -> worst ratios seen, printed by the last test


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    assert engine.load_library().ekf_device_count() >= 1
    return engine


def storage_of(precision):
    return np.float32 if precision == 2 else np.float64


def fresh_engine(eng_mod, kind, n, precision, path=None, mode=None, primed=True):
    """primed: the covariance is known to the engine as bitwise symmetric, as it is from the first applied update on -- the state in
    which an update runs k_p_update_i8p on an fp32-stored P.  (The first update behind an upload averages P with its transpose:
    k_p_update_i8<true> in fp32 storage, k_symmetrize_P in front of the downdate in fp64 storage.)  The engine learns it from an
    applied update, so a position fix at the camera's own position with sigma = 1 km is fused first: dx = 0, B'B is 1e-38 of a
    variance of 2e-16, the stored zeros of P stay zeros, and the reference starts behind it anyway."""
    cam, par, x, fp, t, desc, P0 = ur.case_map(kind, n)
    e = eng_mod.EkfEngine(cam, par, len(fp) + 8, max_keypoints=64, precision=precision)
    assert e.precision == precision
    if path is not None:
        e.set_update_path(path)
    if mode is not None:
        e.set_sweep_mode(mode)
    e.set_state(x, fp, t, desc, P0)
    assert e.n == n
    if primed:
        assert e.fuse_camera_position(x[:3], 1e6 * np.eye(3))["applied"]
    return e, cam


def predicted_inputs(e, cam, M):
    """predict + predict_measurements; -> (matches, everything the reference starts from)"""
    e.predict()
    preds, Hs, Hf = e.predict_measurements()
    assert len(preds) >= M, "every match must be a predicted feature"
    m = ur.matches_for(preds, M)
    x, fp, P = e.get_state()
    t, c = e.feature_layout()
    rows, res = ur.xr.visual_rows(preds[:M], Hs[:M], Hf[:M], m, t, c)
    return m, (x, fp, t, c, P, rows, res, cam.pixelErrorX * np.eye(len(res)))


def reference(label, inputs, precision, update_cov=True, exact=None, min_spread=1e6, c_arith=ur.C_ARITH):
    x, fp, t, c, P, rows, res, R = inputs
    h = hashlib.sha1()
    for a in (x, fp, t, c, P, *rows, res):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (label, h.hexdigest())
    if key not in _CORES:
        _CORES[key] = uf.update_core(x, fp, P, rows, res, R)  # (the compiled restatement: the same bits at these sizes, asserted on the CPU)
    exact = precision in (2, 3) if exact is None else exact
    ref = ur.with_bounds(_CORES[key], t, c, storage_of(precision), exact, update_cov, c_arith)
    cond = float(np.linalg.cond(ref["S"].astype(np.float64)))
    sd = np.sqrt(np.diag(P))
    # the case's input conditions (tests/test_update_ref_cpu.py asserts the same from the oracle's state)
    assert cond < 1e5 and sd.max() >= min_spread * sd[sd > 0].min(), (cond, sd.min(), sd.max())
    assert ref["deadband_margin"] > 1.0, f"a component of dx lies within its tolerance of the dead-band: {ref['deadband_margin']}"
    return ref


def check(e, ref, inputs, label, precision, route="default", update_cov=True):
    """every entry and every component against its bound; the figures are printed before anything is asserted"""
    x, fp, P = e.get_state()
    prior = inputs[4]
    w = {"x": ur.worst(x, ref["x13"], ref["tol_x13"]), "features": ur.worst(fp, ref["feature_pos"], ref["tol_feature_pos"])}
    if update_cov:
        w["P"] = ur.worst(P, ref["P_cmp"], ref["tol_P"])
        over = int((np.abs(P.astype(ur.LD) - ref["P_cmp"]) > ref["tol_P"]).sum())
        off = np.r_[0:3, 7:len(P)]  # (where the diagonal of P is that of P_downdated: the normalisation rescales q's four variances)
        grow = float(((np.diag(P) - np.diag(prior))[off] / np.diag(ref["tol_P"])[off].astype(np.float64)).max())
    # (what the norm-wise gate says about the same result at the tolerance the parity tests hold this configuration to: printed,
    # never asserted)
    old_gate = sorted(over_tolerance(parity_report(x, fp, P, ref["x13"].astype(np.float64), ref["feature_pos"].astype(np.float64),
                                                   ref["P"].astype(np.float64)), F64_TOL if precision == 0 else F32_TOL))
    print(f"{label} precision {precision} route {route}: worst |err| / tol",
          {k: f"{v[0]:.3f} at {v[1]}" for k, v in w.items()}, f"entries of P over: {over}" if update_cov else "",
          f"parity_metric objects to: {old_gate}")
    slot = WORST.setdefault((precision, route), {})
    for k, v in w.items():
        slot[k] = max(slot.get(k, 0.0), v[0])
    assert all(v[0] <= 1.0 for v in w.values()), w
    if update_cov:
        assert abs(np.sqrt(x[3:7] @ x[3:7]) - 1.0) <= 4 * ur.U64
        assert grow <= 1.0, f"a variance grew by {grow} of its tolerance"
        if precision in (2, 3):
            np.testing.assert_array_equal(P, P.T)
    else:
        np.testing.assert_array_equal(P, prior)


def run_fresh(eng_mod, kind, n, M, precision, path=None, mode=None, route="default", dense=False, primed=True):
    e, cam = fresh_engine(eng_mod, kind, n, precision, path, mode, primed)
    if dense:
        e.dense_products(True)
    m, inputs = predicted_inputs(e, cam, M)
    # exact configurations: the rows of B come from digit planes, inside the sweep or (EKF_UPDATE_PATH_GEMM) from the int8 GEMM
    exact = ("gemm" if path == GEMM else "sweep") if precision in (2, 3) else False
    ref = reference((kind, n, M), inputs, precision, exact=exact)
    e.update(m)
    check(e, ref, inputs, f"{kind} n = {n} M = {M}", precision, route)
    return e


# ------------------------------------------------------------------------------------------------ column and row edges
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ur.MIXED_N)
def test_column_edges(eng_mod, n, precision):
    run_fresh(eng_mod, "mixed", n, ur.MIXED_M, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", ur.ROW_M)
def test_row_edges(eng_mod, M, precision):
    e = run_fresh(eng_mod, "seq170", 1033, M, precision)
    if precision in (2, 3):
        # the fresh map is spiky: the downdate takes the step that skips the zero pieces of plane 0.  Three quarters and more of the
        # pieces are zero up to M = 65 (measured: 1 of 33 at M = 1 ... 73 of 297 at M = 65 hold a top digit); at M = 160 of 170
        # features 330 of 660 do, and half of the pieces are zero -- still twice the quarter from which a unit takes that step
        nz, total = e.plane0_pieces()
        print(f"    plane 0: {nz} of {total} pieces hold anything")
        assert total > 0 and (4 * (total - nz) >= 3 * total if M <= 65 else 2 * (total - nz) >= total)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,n,M", [("mixed", 259, 17), ("seq170", 1033, 33)])
def test_first_update_behind_an_upload(eng_mod, kind, n, M, precision):
    """the averaging forms of the downdate: no update has told the engine that P is bitwise symmetric"""
    run_fresh(eng_mod, kind, n, M, precision, route="first update", primed=False)


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("path", [SWEEP, GEMM], ids=["sweep", "gemm"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", [33, 160])
def test_routes(eng_mod, M, precision, path, mode):
    run_fresh(eng_mod, "seq170", 1033, M, precision, path, MODES[mode], route=f"{'sweep' if path == SWEEP else 'gemm'}/{mode}")


# ------------------------------------------------------------------------------------------------ both forms of the step
@pytest.mark.parametrize("precision", [2, 3])
@pytest.mark.parametrize("M", [65, 160])
def test_dense_products_meet_the_same_bound(eng_mod, M, precision):
    """the spiky cases of test_row_edges once more with every digit product multiplied (ekf_debug_dense_products)"""
    run_fresh(eng_mod, "seq170", 1033, M, precision, route="dense products", dense=True)


@pytest.mark.parametrize("precision", [2, 3])
def test_converged_map_takes_the_plain_step(eng_mod, precision):
    if "conv" not in ur._SEQ:
        ur._SEQ["conv"] = SyntheticSequence(170, CONVERGED_FRAMES)
    seq = ur._SEQ["conv"]
    e = eng_mod.EkfEngine(seq.cam, seq.par, seq.n_features + 8, max_keypoints=4 * seq.n_features + 64, precision=precision)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    for kps, desc in seq.frames:
        assert e.step(kps, desc).status == 0
    assert e.n == 1033
    m, inputs = predicted_inputs(e, seq.cam, 160)
    ref = reference(("converged", precision), inputs, precision)
    e.update(m)
    nz, total = e.plane0_pieces()
    print(f"    plane 0 after {CONVERGED_FRAMES} frames: {nz} of {total} pieces hold anything")
    check(e, ref, inputs, f"converged map ({CONVERGED_FRAMES} frames) M = 160", precision, "converged")
    assert total > 0 and 4 * (total - nz) < total  # fewer than a quarter of the pieces are zero: the plain step runs


# ------------------------------------------------------------------------------------------------ state-only update
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", [17, 160])
def test_state_only_update(eng_mod, M, precision):
    """update_cov = false: P keeps its bits; B is formed in fp64 in every configuration (update_route.h: nothing of the downdate's
    machinery is chosen), so the state is held to the bound without the digit term"""
    e, cam = fresh_engine(eng_mod, "seq170", 1033, precision)
    m, inputs = predicted_inputs(e, cam, M)
    ref = reference(("seq170", 1033, M), inputs, precision, update_cov=False, exact=False)
    e.update_only_state(m)
    check(e, ref, inputs, f"state only, n = 1033 M = {M}", precision, "state only", update_cov=False)


def test_print_worst_ratios():
    """(the table of DESIGN.md: worst |err| / tol per precision and route over the cases above)"""
    for (precision, route), w in sorted(WORST.items()):
        print(f"precision {precision} route {route}:", {k: f"{v:.3f}" for k, v in sorted(w.items())})
