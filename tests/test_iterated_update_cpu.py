"""CPU-only checks of the iterated-update reference (tests/iterated_update_ref.py) at the cases of
tests/test_gpu_iterated_update.py, from the ORACLE's state after its prediction (the GPU file starts from the engine's):

  * K = 1 is update_ref.update_ref, exactly;
  * on ("mixed", 85, 17), matches 3 px off, the iteration contracts (each of the first three steps below half the one before) and
    K = 3 differs from K = 1 by more than 100 x F32_TOL under parity_metric -- an un-iterated update cannot pass the GPU gate;
  * sensitivity, reference against reference: x^1 perturbed by F32_TOL relative moves x^3 by no more than F32_TOL (the engine's x^1
    is within its configuration's gate of the reference's, so its x^3 can be held to the same gate);
  * every match stays predicted in every pass, and no dx of the last pass lies at the dead-band in the fp64 configuration; with the
    exact configurations' digit terms some do on the mixed cases at 3 px -- a finding, see test_cases_are_usable_for_the_gpu_gate."""
import numpy as np
import pytest

import iterated_update_ref as ir
import update_ref as ur
import update_ref_fast as uf
from parity_metric import F32_TOL, block_errs, over_tolerance, parity_report

# (kind, n, M, amplitude in pixels): the GPU file's cases
CASES = [("mixed", 85, 17, 3.0), ("mixed", 259, 17, 3.0), ("mixed", 85, 16, 3.0), ("seq170", 1033, 33, 0.3)]
_PRIORS = {}


def prior(ol, kind, n, M, amp):
    """the oracle after predict + predict_measurements -> (oracle, x, fp, t, desc, c, P, matches, pixel error)"""
    key = (kind, n, M, amp)
    if key not in _PRIORS:
        cam, par, x, fp, t, desc, P0 = ur.case_map(kind, n)
        o = ol.Oracle(cam, par, len(fp) + 8)
        o.set_state(x, fp, t, desc, P0)
        o.predict()
        preds, _, _ = o.predict_measurements()
        assert o.n == n and len(preds) >= M
        _PRIORS[key] = (o, o.x13(), o.feature_pos(), t, desc, o.feature_covpos(), o.P(), ir.scaled_matches(preds, M, amp), cam.pixelErrorX)
    return _PRIORS[key]


def run(ol, case, K, **kw):
    o, x, fp, t, desc, c, P, m, px = prior(ol, *case)
    scratch = ol.Oracle(o.cam, o.par, len(fp) + 8)
    return ir.iterated_update_ref(scratch, x, fp, t, desc, c, P, m, px, K, core_fn=uf.update_core, **kw)


def test_one_pass_is_the_plain_update(oracle_lib):
    case = ("mixed", 85, 17, 3.0)
    o, x, fp, t, desc, c, P, m, px = prior(oracle_lib, *case)
    r = run(oracle_lib, case, 1)
    po, Hs, Hf = o.predict_measurements()
    rows, res = ur.xr.visual_rows(*oracle_lib.align_to_matches(po, Hs, Hf, m), m, t, c)
    ref = ur.with_bounds(uf.update_core(x, fp, P, rows, res, px * np.eye(len(res))), t, c)
    assert r["passes_run"] == 1 and r["stop_reason"] == ir.STOP_COUNT
    for k in ("x13", "feature_pos", "P"):
        np.testing.assert_array_equal(r["final"][k], ref[k])


def test_contraction_and_distance_from_one_pass(oracle_lib):
    case = ("mixed", 85, 17, 3.0)
    r4 = run(oracle_lib, case, 4)
    s = r4["steps"]
    print("normalised steps over four passes:", ", ".join(f"{v:.3g}" for v in s))
    # (the fourth is the covariance pass's, taken to the normalised state: it carries the normalisation of q as well)
    assert len(s) == 4 and s[1] < 0.5 * s[0] and s[2] < 0.5 * s[1]
    r1, r3 = run(oracle_lib, case, 1), run(oracle_lib, case, 3)
    f1, f3 = r1["final"], r3["final"]
    be = parity_report(*(f1[k].astype(np.float64) for k in ("x13", "feature_pos", "P")),
                       *(f3[k].astype(np.float64) for k in ("x13", "feature_pos", "P")))
    worst = max(v for k, v in be.items() if k != "features_blockwise")
    print(f"K = 1 against K = 3: worst figure of parity_metric {worst:.3g} ({worst / F32_TOL:.0f} x F32_TOL)")
    assert worst > 100 * F32_TOL and over_tolerance(be, F32_TOL)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-n{c[1]}-M{c[2]}-{c[3]}px")
def test_cases_are_usable_for_the_gpu_gate(oracle_lib, case):
    r3 = run(oracle_lib, case, 3)
    assert r3["passes_run"] == 3 and r3["all_predicted"], "every match must stay predicted in every pass"
    assert r3["final"]["deadband_margin"] > 1.0, r3["final"]["deadband_margin"]
    # The exact configurations' state bound adds the digit terms q_i sum |z| and Delta' |z|, which grow with the innovations.  FINDING: at
    # 3 px the margin does NOT hold with them on the three mixed cases (measured 0.452, 0.389, 0.693; ("seq170", 1033, 33) at 0.3 px:
    # 19.6; 4, 112 and 4 components in the band).  They are parameters of features -- never the camera -- whose correction is below 1e-12; the
    # GPU file holds them, and only them, to |dx_j| + tol_j (iterated_update_ref.deadband_band says why) and every other component to
    # its bound as it stands.
    o, x, fp, t, desc, c, P, m, px = prior(oracle_lib, *case)
    exact = run(oracle_lib, case, 3, storage=np.float32, exact=True)
    core = uf.update_core(x, fp, P, exact["rows"], exact["nu"], px * np.eye(len(exact["nu"])))
    band, _, tol_fp = ir.deadband_band(core, exact["final"], t, c, True)
    margin = exact["final"]["deadband_margin"]
    print(f"{case}: dead-band margin of the last pass {r3['final']['deadband_margin']:.3g}; with the exact configurations' digit terms "
          f"{margin:.3g}, {int(band.sum())} of {len(band)} components in the band, |dx| there at most "
          f"{float(np.abs(exact['final']['dx'])[band].max(initial=0)):.3g}")
    assert (margin > 1.0) == (not band.any())
    if case[0] == "seq170":
        assert margin > 1.0, margin
    else:
        assert band.any() and float(np.abs(exact["final"]["dx"])[band].max()) < 4 * ur.EKF_DELTA
        assert float((tol_fp - exact["final"]["tol_feature_pos"]).max()) < 4 * ur.EKF_DELTA

    def perturb(x, fp):  # every component by F32_TOL of itself, signs alternating
        sx = np.where(np.arange(13) % 2 == 0, 1.0, -1.0)
        sf = np.where(np.arange(fp.size).reshape(fp.shape) % 2 == 0, 1.0, -1.0)
        return x * (1 + F32_TOL * sx), fp * (1 + F32_TOL * sf)

    rp = run(oracle_lib, case, 3, perturb_x1=perturb)
    (xa, fa), (xb, fb) = r3["iterates"][3], rp["iterates"][3]
    be = block_errs(xb, fb, xa, fa)
    worst = max(be.values())
    # measured (printed below), as a fraction of the perturbation: ("mixed", 85, 17) 0.0081, ("mixed", 259, 17) 0.059,
    # ("mixed", 85, 16) 0.010, ("seq170", 1033, 33) 0.00044 -- the iteration damps an error of x^1, it does not amplify it
    print(f"{case}: x^1 perturbed by {F32_TOL:g} relative moves x^3 by {worst:.3g} ({worst / F32_TOL:.3g} of it); steps "
          + ", ".join(f"{v:.3g}" for v in r3["steps"]))
    assert worst <= F32_TOL, be


def test_a_feature_that_leaves_the_image_ends_the_iteration(oracle_lib):
    """the construction of the GPU file's border case: the right-most feature of ("mixed", 85) lies within a pixel of the image's
    edge, every match pulls 3 px to the right; at x^1 it is outside, and the result is the one-pass update"""
    cam, par, x, fp, t, desc, P0 = ur.case_map("mixed", 85)
    o = oracle_lib.Oracle(cam, par, len(fp) + 8)
    o.set_state(x, fp, t, desc, P0)
    o.predict()
    cam2 = ir.border_camera(cam, o.predict_measurements()[0])
    o2 = oracle_lib.Oracle(cam2, par, len(fp) + 8)
    o2.set_state(x, fp, t, desc, P0)
    o2.predict()
    preds = o2.predict_measurements()[0]
    m = ir.border_matches(preds, 17)
    assert cam2.pixelsX - preds["imagePos"][:, 0].max() < 1.0
    scratch = oracle_lib.Oracle(cam2, par, len(fp) + 8)
    args = (o2.x13(), o2.feature_pos(), t, desc, o2.feature_covpos(), o2.P(), m, cam2.pixelErrorX)
    r1 = ir.iterated_update_ref(scratch, *args, 1, core_fn=uf.update_core)
    r3 = ir.iterated_update_ref(scratch, *args, 3, core_fn=uf.update_core)
    assert (r3["stop_reason"], r3["passes_run"], r3["all_predicted"]) == (ir.STOP_FEATURE_LEFT, 1, False)
    assert r3["steps"] == r1["steps"] and r1["final"]["deadband_margin"] > 1.0
    for k in ("x13", "feature_pos", "P"):
        np.testing.assert_array_equal(r3["final"][k], r1["final"][k])
