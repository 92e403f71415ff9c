"""The iterated EKF update (ekf_update_iterated) restated from the oracle's measurement prediction and the update
reference of tests/update_ref.py.  TEST INFRASTRUCTURE (numpy plus the oracle).

With x^, P the state and covariance before the update, z the matched pixels, R = pixelErrorX I and x^0 = x^, pass i = 0 .. K - 1:

    h_i, H_i = Oracle.set_state(x^i, ..., P) -> predict_measurements(the matched features) -> align_to_matches -> visual_rows
    nu_i     = z - (h_i + H_i (x^ - x^i)), dead-banded     (the sparse rows against the stacked parameter vector: columns in
                                                            ascending order, the 13 camera columns first -- the engine's order)
    x^(i+1)  = update_core / with_bounds from x^ with nu_i; update_cov = False for every pass but the last

The oracle's set_state forms R(q) from the un-normalised quaternion, as the engine's state-only update leaves it.  A pass that
does not predict every matched feature ends the iteration: the update is finished (covariance pass) from the last linearisation
point at which all were predicted -- the result of `passes_run` passes.  tol > 0: a pass whose normalised step is below tol makes
the next pass the covariance pass.

step[i] = max_j |x_j^(i+1) - x_j^i| / sqrt(P_jj) over the state columns with P_jj > 0; the last one is taken to the final,
normalised state."""
import numpy as np

import oracle_lib as ol
import update_ref as ur
from external_update_ref import EKF_DELTA, FEATURE_INVERSE_DEPTH, visual_rows

STOP_COUNT, STOP_TOL, STOP_FEATURE_LEFT = 0, 1, 2


def stacked(x13, fp, feature_type, covpos, n):
    """the parameter vector in the order of P's columns"""
    p = np.zeros(n)
    p[:13] = x13
    for f in range(len(fp)):
        d = 6 if int(feature_type[f]) == FEATURE_INVERSE_DEPTH else 3
        p[int(covpos[f]):int(covpos[f]) + d] = fp[f, :d]
    return p


def normalised_step(pa, pb, P):
    d = np.diag(P)
    live = d > 0
    return float((np.abs(pa - pb)[live] / np.sqrt(d[live])).max())


def linearise(o, x, fp, t, desc, P, matches):
    """the oracle's predictions and Jacobians of the matched features at (x, fp), aligned to the matches; None if one is not predicted"""
    o.set_state(x, fp, t, desc, P)
    preds, Hs, Hf = o.predict_measurements(np.asarray(matches["featureIndex"], dtype=np.int32))
    if len(preds) < len(matches):
        return None
    return ol.align_to_matches(preds, Hs, Hf, matches)


def corrected_residual(lin, matches, t, c, p_hat, p_lin):
    """(rows, nu): nu = z - (h + H (p^ - p_lin)), each sum in ascending column order, then the dead-band"""
    mp, mHs, mHf = lin
    rows, _ = visual_rows(mp, mHs, mHf, matches, t, c)
    row_start, col, val = rows
    d = p_hat - p_lin
    nu = np.zeros(len(row_start) - 1)
    for i in range(len(nu)):
        acc = 0.0
        for k in range(row_start[i], row_start[i + 1]):
            acc += val[k] * d[col[k]]
        a = float(matches["imagePos"][i // 2][i % 2]) - (float(mp["imagePos"][i // 2][i % 2]) + acc)
        nu[i] = a if abs(a) > EKF_DELTA else 0.0
    return rows, nu


def iterated_update_ref(o, x13, feature_pos, feature_type, desc, covpos, P, matches, pixel_error, iterations, tol=0.0,
                        storage=np.float64, exact=False, core_fn=ur.update_core, perturb_x1=None):
    """-> dict: iterates (list of (x13, feature_pos) in fp64: x^0 .. x^passes_run, the last one normalised), final (the dict of
    update_ref.with_bounds of the covariance pass, started from x^), steps, passes_run, stop_reason, all_predicted, lin (the
    aligned predictions of the covariance pass), rows / nu of that pass.  perturb_x1: a function (x13, fp) -> (x13, fp) applied to
    x^1 before it is used (the sensitivity check of the CPU tests).  o: an Oracle with room for the map; its state is overwritten."""
    xh = np.array(x13, dtype=np.float64)
    fh = np.array(feature_pos, dtype=np.float64).reshape(-1, 6)
    P = np.array(P, dtype=np.float64)
    n = len(P)
    t, c = np.asarray(feature_type), np.asarray(covpos)
    R = pixel_error * np.eye(2 * len(matches))
    p_hat = stacked(xh, fh, t, c, n)
    iterates, steps = [(xh, fh)], []
    xi, fi = xh, fh
    lin_prev, p_prev = None, None
    stop, last, all_predicted = STOP_COUNT, iterations == 1, True
    for i in range(iterations):
        lin = linearise(o, xi, fi, t, desc, P, matches)
        p_lin = stacked(xi, fi, t, c, n)
        if lin is None:
            assert i >= 1, "a match is not predicted at the prior"
            all_predicted = False
            stop, last = STOP_FEATURE_LEFT, True
            lin, p_lin = lin_prev, p_prev
            iterates.pop()
            steps.pop()
        rows, nu = corrected_residual(lin, matches, t, c, p_hat, p_lin)
        core = core_fn(xh, fh, P, rows, nu, R)
        out = ur.with_bounds(core, t, c, storage, exact, update_cov=last)
        xn, fn = out["x13"].astype(np.float64), out["feature_pos"].astype(np.float64)
        if i == 0 and perturb_x1 is not None and not last:
            xn, fn = perturb_x1(xn, fn)
        step = normalised_step(stacked(xn, fn, t, c, n), p_lin, P)
        steps.append(step)
        iterates.append((xn, fn))
        if last:
            return {"iterates": iterates, "final": out, "steps": steps, "passes_run": len(steps), "stop_reason": stop,
                    "all_predicted": all_predicted, "lin": lin, "rows": rows, "nu": nu, "p_lin": p_lin}
        lin_prev, p_prev = lin, p_lin
        xi, fi = xn, fn
        if tol > 0.0 and step < tol:
            stop, last = STOP_TOL, True
        if i + 1 == iterations - 1:
            last = True
    raise AssertionError("unreachable")


def scaled_matches(preds, M, amplitude):
    """update_ref.matches_for's pattern scaled to `amplitude` pixels (0.3: the pattern itself)"""
    m = ur.matches_for(preds, M)
    off = m["imagePos"] - preds["imagePos"][:M]
    m["imagePos"] = preds["imagePos"][:M] + off * (amplitude / 0.3)
    return m


def border_camera(cam, preds):
    """a copy of `cam` whose image ends less than a pixel to the right of the right-most prediction"""
    cam2 = type(cam).from_buffer_copy(cam)
    cam2.pixelsX = int(np.floor(preds["imagePos"][:, 0].max())) + 1
    return cam2


def border_matches(preds, M, pull=3.0):
    """the M right-most predictions, in prediction order, every match `pull` pixels to the right of its prediction: the first pass
    moves the right-most feature out of border_camera's image"""
    sel = np.sort(np.argsort(-preds["imagePos"][:, 0])[:M])
    m = ur.matches_for(preds[sel], M)
    m["imagePos"] = preds["imagePos"][sel] + np.array([pull, 0.0])
    return m


def deadband_band(core, ref, feature_type, covpos, exact, c_arith=ur.C_ARITH):
    """The components of dx that lie within their own tolerance of the dead-band EKF_DELTA, from the reference alone (the state
    tolerance of update_ref.with_bounds, term by term) -> (in_band [n] bool, relaxed copies of tol_x13 and tol_feature_pos).

    update_ref calls a case valid only while no component lies there (deadband_margin > 1): a correct engine may then decide the
    dead-band of such a component the other way.  Either decision is a correct result -- x^_j, or x^_j + dx_j -- and the engine's
    value lies within the component's tolerance of one of the two, so within |dx_j| + tol_j of the reference's: that is the relaxed
    bound, for those components alone (|dx_j| is 1e-12 there).  A camera component in the band is not handled (the quaternion's
    normalisation would spread it): asserted."""
    dx, z, B = ref["dx"], ref["z"], ref["B"]
    n = len(dx)
    if exact:
        q, dx_b = core["q"], core["route"]["sweep" if exact is True else exact][1]
    else:
        q, dx_b = np.zeros(n, ur.LD), np.zeros(n, ur.LD)
    tol_dx = q * np.abs(z).sum() + dx_b + c_arith * ur.U64 * core["sd"] * np.sqrt(z @ z)
    tol_dx[~np.any(B != 0, axis=0)] = 0
    dist = np.abs(np.abs(dx) - EKF_DELTA)
    margin = float((dist / np.where(tol_dx > 0, tol_dx, ur.LD(1e-300))).min())
    assert np.isclose(margin, ref["deadband_margin"], rtol=1e-9), (margin, ref["deadband_margin"])
    band = (tol_dx > 0) & (dist <= tol_dx)
    assert not band[:13].any(), "a camera component lies at the dead-band"
    tol_x, tol_fp = ref["tol_x13"].copy(), ref["tol_feature_pos"].copy()
    for f in range(len(tol_fp)):
        k = 6 if int(feature_type[f]) == FEATURE_INVERSE_DEPTH else 3
        c = int(covpos[f])
        tol_fp[f, :k] += np.where(band[c:c + k], np.abs(dx[c:c + k]), 0)
    return band, tol_x, tol_fp
