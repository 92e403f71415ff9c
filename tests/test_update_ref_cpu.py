"""CPU-only checks of the longdouble restatement of the EKF update and its per-entry bounds (tests/update_ref.py; DESIGN.md, "Stage
tests of the update"), at every fresh-map case of tests/test_gpu_update_entries.py, from the ORACLE's state after its prediction
and measurement prediction (the GPU file starts from the engine's):

  * the oracle's ALGORITHMIC update and the fp64 loop restatement (external_update_ref) lie inside the bounds of the reference,
    every entry of P and every component of the state;
  * C_ARITH is measured here (loop restatement against longdouble, never the engine) and printed;
  * the input conditions of the cases: cond S, a spread of sqrt(diag P) of six orders and more, no dx at the dead-band, all M
    matches predicted;
  * the gate the suite had (parity_metric) passes a covariance with 88 % of its entries zeroed or sign-flipped (and, in the max
    norm, one with 97 % zeroed); the new bound rejects each."""
import numpy as np
import pytest

import update_ref as ur
from parity_metric import F32_TOL, over_tolerance, parity_report

_RUNS = {}


def run_case(ol, case, storage=np.float64, exact=False):
    """the oracle after predict + predict_measurements, the first M predictions as matches -> everything the checks need (cached)"""
    key = case + (storage.__name__, exact)
    if key in _RUNS:
        return _RUNS[key]
    kind, n, M = case
    cam, par, x, fp, t, desc, P0 = ur.case_map(kind, n)
    o = ol.Oracle(cam, par, len(fp) + 8)
    o.set_state(x, fp, t, desc, P0)
    o.predict()
    po, Hs, Hf = o.predict_measurements()
    assert o.n == n and len(po) >= M, "every match must be a predicted feature"
    m = ur.matches_for(po, M)
    mp, mHs, mHf = ol.align_to_matches(po, Hs, Hf, m)
    P = o.P()
    if storage is np.float32:  # what an fp32-stored covariance holds: the nearest fp32 values, symmetric
        P = np.triu(P).astype(np.float32).astype(np.float64)
        P = np.triu(P) + np.triu(P, 1).T
        o.set_state(o.x13(), o.feature_pos(), t, desc, P)
    xs, fs, c = o.x13(), o.feature_pos(), o.feature_covpos()
    rows, res = ur.xr.visual_rows(mp, mHs, mHf, m, t, c)
    R = cam.pixelErrorX * np.eye(len(res))
    ref = ur.update_ref(xs, fs, t, c, P, rows, res, R, storage, exact)
    loop = ur.xr.external_update_ref(xs, fs, t, c, P, *rows, res, R, 0.0, storage)
    assert o.update(m, mp, mHs, mHf, ol.ALGORITHMIC) == 0
    _RUNS[key] = dict(inputs=(xs, fs, P, rows, res, R), prior=P, ref=ref, loop=loop, oracle=(o.x13(), o.feature_pos(), o.P()), t=t, c=c)
    return _RUNS[key]


def ratios(got, ref):
    x, fp, P = got
    return {"P": ur.worst(P, ref["P_cmp"], ref["tol_P"]), "x": ur.worst(x, ref["x13"], ref["tol_x13"]),
            "features": ur.worst(fp, ref["feature_pos"], ref["tol_feature_pos"])}


@pytest.mark.parametrize("case", ur.CASES, ids=lambda c: f"{c[0]}-n{c[1]}-M{c[2]}")
def test_oracle_and_loop_restatement_inside_the_bounds(oracle_lib, case):
    r = run_case(oracle_lib, case)
    ref, loop = r["ref"], r["loop"]
    for name, got in (("oracle", r["oracle"]), ("loop", (loop["x13"], loop["feature_pos"], loop["P"]))):
        w = ratios(got, ref)
        print(f"{case}: {name} worst |err| / tol:", {k: f"{v[0]:.3f} at {v[1]}" for k, v in w.items()})
        assert all(v[0] <= 1.0 for v in w.values()), (name, w)
    w = ur.worst(loop["P_downdated"], ref["P_downdated_cmp"], ref["tol_P_downdated"])
    assert w[0] <= 1.0, w
    np.testing.assert_array_equal(ref["P"], ref["P"].T)
    assert np.all(np.diag(ref["P_downdated"]) <= np.diag(r["prior"]))


@pytest.mark.parametrize("case", [("mixed", 85, 17), ("mixed", 259, 17), ("mixed", 514, 17), ("seq170", 1033, 33)],
                         ids=lambda c: f"{c[0]}-n{c[1]}-M{c[2]}")
def test_fp32_storage_and_digit_bound(oracle_lib, case):
    """fp32-stored P: the loop restatement rounds where the reference rounds and stays inside the bound without its digit term;
    the digit term is what the representation says: at least the rounding of B, at most a small multiple of 2^-36 of the scale"""
    r = run_case(oracle_lib, case, np.float32, True)
    ref, loop = r["ref"], r["loop"]
    w = {"P": ur.worst(loop["P"], ref["P_cmp"], ref["tol_P"] - np.where(ref["strip"], ur.normalize_bound(ref["dig"], ref["J"]), ref["dig"])),
         "x": ur.worst(loop["x13"], ref["x13"], ref["tol_x13"]), "features": ur.worst(loop["feature_pos"], ref["feature_pos"], ref["tol_feature_pos"])}
    print(f"{case}: fp32 storage, loop worst |err| / tol without dig:", {k: f"{v[0]:.3f}" for k, v in w.items()})
    assert all(v[0] <= 1.0 for v in w.values()), w
    np.testing.assert_array_equal(ref["P"], ref["P"].astype(np.float32).astype(ur.LD))
    live = ref["scale"] > 0
    e = ur.column_exponents(np.diag(r["prior"]))
    m = len(ref["z"])
    rel = (ur.digit_bound(ref["B"], e)[0][live] / ref["scale"][live]).astype(np.float64)  # parts (a) and (b): the downdate's own digits
    print(f"{case}: (a) + (b) / sqrt(P_ii P_jj): max {rel.max():.2e}, median {np.median(rel):.2e}; m = {m}")
    assert rel.max() <= m * 2.0 ** -34  # (a) <= 2 sqrt(m) 1.001 2^-38 ... (b) <= m 2^-36 (1 + 3/256 + ...): both far below
    for route in ("sweep", "gemm"):  # (c), (d): the rows of B from digit planes
        full = ur.with_bounds(ur.update_core(*r["inputs"]), r["t"], r["c"], np.float32, route)
        rel = (full["dig"][live] / ref["scale"][live]).astype(np.float64)
        print(f"{case}: dig / sqrt(P_ii P_jj) with the rows of B from the planes ({route}): max {rel.max():.2e}, dead-band margin "
              f"{full['deadband_margin']:.1f}")
        assert rel.max() < 2.0 ** -24 and full["deadband_margin"] > 1.0  # still below what fp32 storage costs; the case stays valid
    sd = np.sqrt(np.diag(r["prior"]))
    assert np.all(np.ldexp(1.0, e[sd > 0]) > sd[sd > 0]) and np.all(np.ldexp(1.0, e[sd > 0] - 1) <= sd[sd > 0] * 1.001)
    assert np.all(np.abs(ref["B"]) <= sd[None, :] * (1 + 1e-12))  # |B_kj| <= sqrt(P_jj): what the a-priori scales rest on


def test_c_arith_and_input_conditions(oracle_lib):
    worst_c, rows = 0.0, []
    for case in ur.CASES:
        r = run_case(oracle_lib, case)
        ref, loop = r["ref"], r["loop"]
        live = ref["scale"] > 0
        c = float((np.abs(loop["P_downdated"] - ref["P_downdated_cmp"])[live] / (ur.U64 * ref["scale"][live])).max())
        sd = np.sqrt(np.diag(r["prior"]))
        cond = float(np.linalg.cond(ref["S"].astype(np.float64)))
        spread = float(sd.max() / sd[sd > 0].min())
        rows.append((case, c, cond, spread, ref["deadband_margin"]))
        worst_c = max(worst_c, c)
        assert spread >= 1e6, case           # the case contains the entries the norm-wise gate could not see
        assert cond < 1e5, case              # S is far from singular: C_ARITH means the same thing in every case
        assert ref["deadband_margin"] > 1.0, case
    for case, c, cond, spread, margin in rows:
        print(f"{case}: C_arith {c:.1f}  cond S {cond:.0f}  spread of sqrt diag P {spread:.1e}  dead-band margin {margin:.1f}")
    print(f"C_arith measured {worst_c:.1f} x margin {ur.ARITH_MARGIN:g} = {ur.ARITH_MARGIN * worst_c:.0f}; "
          f"update_ref.C_ARITH = {ur.C_ARITH:g} (from C_ARITH_MEASURED = {ur.C_ARITH_MEASURED:g})")
    assert worst_c <= ur.C_ARITH_MEASURED and worst_c >= 0.5 * ur.C_ARITH_MEASURED  # the recorded figure is the measured one, rounded up
    # the exact configurations' state bound adds q_i sum |z|: the dead-band condition must hold with it too
    for case in [("mixed", 85, 17), ("seq170", 1033, 33)]:
        assert run_case(oracle_lib, case, np.float32, True)["ref"]["deadband_margin"] > 1.0, case


def test_the_old_gate_is_blind_and_the_new_bound_is_not(oracle_lib):
    """n = 1033, M = 160.  Every entry of the reference's P below 1e-5 max|P| zeroed (97.4 % of the matrix): the max-norm gate passes
    it; the Frobenius gate measures 2.1e-4 and does object to this one (the entries between 1e-6 and 1e-5 of the maximum are many).
    Every entry below 1e-7 max|P| (87.8 %) zeroed, or given the wrong sign: over_tolerance passes the whole report at the 1e-5 of
    the fp32-stored configurations.  The per-entry bound rejects all three, hundreds of thousands of entries each."""
    r = run_case(oracle_lib, ("seq170", 1033, 160))
    ref = r["ref"]
    P = ref["P"].astype(np.float64)
    x, fp = ref["x13"].astype(np.float64), ref["feature_pos"].astype(np.float64)
    top = np.abs(P).max()

    def judge(name, bad, mask):
        be = parity_report(x, fp, bad, *r["oracle"])
        w = ur.worst(bad, ref["P_cmp"], ref["tol_P"])
        n_over = int((np.abs(bad - ref["P_cmp"]) > ref["tol_P"]).sum())
        print(f"{name} ({100 * mask.mean():.1f} % of P): parity_metric P_max {be['P_max']:.1e} P_fro {be['P_fro']:.1e} -> "
              f"{sorted(over_tolerance(be, F32_TOL))}; new bound: worst |err| / tol {w[0]:.1e}, {n_over} entries over")
        changed = int((bad != P).sum())  # (two thirds of P are stored zeros: an inverse depth is correlated with nothing yet)
        print(f"    {changed} entries changed")
        # (the changed entries the bound lets pass are correlations below C_ARITH 2^-53 = 5e-13: zero to working precision)
        assert w[0] > 1e3 and n_over > 2e5 and n_over > 0.5 * changed
        return be

    small = np.abs(P) < 1e-5 * top
    assert small.mean() > 0.97
    be = judge("zeroed below 1e-5 max|P|", np.where(small, 0.0, P), small)
    assert be["P_max"] <= F32_TOL and set(over_tolerance(be, F32_TOL)) == {"P_fro"}
    tiny = np.abs(P) < 1e-7 * top
    assert tiny.mean() > 0.85
    assert not over_tolerance(judge("zeroed below 1e-7 max|P|", np.where(tiny, 0.0, P), tiny), F32_TOL)
    assert not over_tolerance(judge("sign flipped below 1e-7 max|P|", np.where(tiny, -P, P), tiny), F32_TOL)
