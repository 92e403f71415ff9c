"""The EKF update (ekf_update: Update.cpp:87-218, :303) in np.longdouble, with a tolerance PER ENTRY of the
covariance and PER COMPONENT of the state in their natural scale ("Stage tests of the update").  TEST INFRASTRUCTURE
(numpy only).

The structure is that of tests/external_update_ref.py, whose visual_rows, quat_norm_jacobian, normalize_covariance,
normalize_bound, EKF_DELTA and rounding points are reused: A = H P from the rows of P as stored, S = A H' + R, its lower Cholesky
factor, z = inv(L) nu, B = inv(L) A, dx = B'z with the dead-band, P <- (P + P')/2 - B'B rounded to the storage type, the
normalisation of rows / columns 3..6 rounded again.  Inputs are what the filter itself holds after the prediction and the
measurement prediction -- x, the features and P exactly as stored, its own Hs and Hf (stage-tested elsewhere), R = pixelErrorX I.

Which value is compared.  The device rounds its own sum once; measured against the reference's value BEFORE that rounding the
error of a correctly rounded result is u_store |ref| (half a unit), against the reference's rounded value it could be a whole
unit whenever the two sums straddle a rounding boundary.  So besides P and P_downdated (rounded where the engine rounds) the
reference returns P_cmp: the downdated matrix unrounded outside rows / columns 3..6, and inside them the normalisation of the
ROUNDED downdated matrix, unrounded.

Tolerance of an entry of P_downdated (prior P-, posterior reference `ref`):

    tol_ij = u_store |ref_ij| + dig_ij + C_ARITH 2^-53 sqrt(P-_ii P-_jj)

  u_store = 2^-24 (fp32-stored P) or 0 (fp64-stored: that rounding is part of the last term).  sqrt(P-_ii P-_jj) is the
  entry's natural scale: sum_k B_ki^2 = P-_ii - P+_ii <= P-_ii, so |(B'B)_ij| <= sqrt(P-_ii P-_jj) by Cauchy-Schwarz (the fact the
  a-priori column scales of chol_bplanes.h rest on).
  dig_ij, exact configurations only (digit_planes.h, kernels_pexact.hip).  Column j of B is held as the integers
  X_kj = rint(B_kj 2^(38 - e_j)), 2^e_j the a-priori scale of k_gather: e_j = ilogb(sqrt(P-_jj) 1.001) + 1 (0 where P-_jj <= 0).
  (a) rounding: B_kj = 2^(e_j - 38) X_kj + r_kj, |r_kj| <= q_j = 2^(e_j - 39), so
        |sum_k B_ki B_kj - 2^(e_i + e_j - 76) sum_k X_ki X_kj| <= sum_k (|B_ki| q_j + |B_kj| q_i + q_i q_j).
  (b) dropped levels: X = sum_s d_s 256^(4 - s) with balanced digits d_s in [-128, 127] (the bytes of (X + K) xor K,
      K = 0x8080808080), X_ki X_kj = sum_{s,t} 256^(8 - s - t) d_s(ki) d_t(kj), and the downdate keeps the levels s + t <= 4 exactly
      (int32 sums).  What it drops is bounded term by term: sum over the ten pairs with s + t >= 5 of
      256^(8 - s - t) (|D_s|' |D_t|)_ij, times 2^(e_i + e_j - 76) -- ten products of the digit magnitudes of the reference's own B.
  (c) the rows of B are themselves formed from digit planes (exact=True / "sweep": chol_bplanes.h b_rows_planes, ps_b_rows_planes,
      b_pair_rows_planes).  Row block k is B_k = inv(L_kk) (G_k - sum_{j<k} L_kj B_j) with the sum taken from the planes of L (row
      scales 2^e_r, e_r = ilogb(sqrt(S_rr) 1.001) + 1 as k_assemble_S stores them, qL_r = 2^(e_r - 39)) and of the finished blocks
      of B, levels s + t <= 4 only.  The sum is off by at most
        E_rc = sum_{i < 32 floor(r / 32)} (|L_ri| q_c + qL_r |B_ic| + qL_r q_c) + 2^(e_r + e_c - 76) (dropped levels of |DL| |DB|)_rc,
      and the rows that are formed satisfy L dB = -E, so |dB| <= Delta = |inv(L)| E (zero for the first panel; a pair launch takes
      fewer blocks from the planes: covered).  With (a) and (b) alone the unmodified engine exceeded the bound at n = 85, M = 17.
  (d) exact="gemm" (EKF_UPDATE_PATH_GEMM, k_b_gemm_i8p): B = inv(L) G is one int8 GEMM from the planes of W = inv(L)' and of G under
      their columns' TRUE scales (k_col_exp: the largest exponent field): Delta_rc = sum_k (|W_kr| qG_c + qW_r |G_kc| + qW_r qG_c)
      + the dropped levels of that product.
  (e) exact="measured" (EKF_UPDATE_PATH_SWEEP above 2048 rows: update_route.h leaves planes_b, gemm_planes and apriori false).  The
      rows of B are fp64 (their error is C_ARITH's), dx = B'z is formed from them (k_dx_partial: no digit term in the state), and the
      downdate cuts them into planes under MEASURED scales: k_dx_partial leaves the largest exponent field of column j in Bexp (the
      rule of k_col_exp: |B_kj| < 2^e_j, e_j = Bexp_j - 1022) and k_slice_B forms X_kj = rint(B_kj 2^(38 - e_j)).  (a) + (b) with these
      e_j; neither (c) nor (d).  An all-zero column has no scale and no digits.
  An error Delta of the rows of B costs the downdate |B|' Delta + Delta' |B| + Delta' Delta and the state Delta' |z|.
  Nothing of the kernels' int32 accumulation, unit lists or plane layouts is restated: dig is a bound, not an emulation.
  C_ARITH cannot be counted by rule (it depends on cond S through the factorisation): it is the worst
  |fp64 loop restatement (external_update_ref) - longdouble| / (2^-53 sqrt(P-_ii P-_jj)) over every case of
  tests/test_update_ref_cpu.py -- reference against reference, never the engine -- times ARITH_MARGIN = 8 for the summation orders
  the device is free to choose (MFMA accumulation, 16 k-splits, arrival order in the persistent sweep).  One number for the file.

The bound is carried through the normalisation with normalize_bound (every term of D P D' with its absolute value); rows /
columns 3..6 take the second storage rounding u_store |ref|, K_NORM 2^-53 of the abs-evaluated products for the arithmetic of
J and of the products (J: three squares and two additions, a square root, two products, a division, a product per entry -- 10
roundings, once on each side; two dot products of length 4: 8; K_NORM = 32 covers 28), and 4 max tol(q) / |q| of the same for
the engine's own q in J (dJ/dq is of order J / |q| in each of the four components).

Tolerance of a component of the state:

    |x_i - ref_i| <= q_i sum_k |z_k| + (Delta' |z|)_i + C_ARITH 2^-53 sqrt(P-_ii) |z|_2 + ulp(ref_i)

  (|dx_i| = |sum_k B_ki z_k| <= sqrt(P-_ii) |z|_2; the first two terms, exact configurations only, are dx = B'z formed from the digits of
  B, k_dx_planes).  A column of B that is identically zero in the reference is one whose every term is a product with a stored
  zero of P (the inverse depth of an unmeasured feature of a fresh map is correlated with nothing); sums of zeros are zero in every
  order and every digit of zero is zero, so there the tolerance is ulp(ref_i) alone.  The dead-band acts on the reference's own dx; `deadband_margin` is the smallest ||dx_i| - EKF_DELTA| / tol_i
  -- a case is valid only if it is above 1.  The quaternion is normalised afterwards: with t the tolerances of its four components
  before, n its norm, a component of q / n is off by at most t_i / n + |q_i / n| (sum_j t_j) / n, + 2 ulp."""
import numpy as np

import external_update_ref as xr
from external_update_ref import EKF_DELTA, FEATURE_INVERSE_DEPTH, normalize_bound, normalize_covariance, quat_norm_jacobian

LD = np.longdouble
U64 = 2.0 ** -53
PX_S = 5                     # digits per element of B (engine.h)
PX_BITS = 8 * PX_S - 2       # 38
ARITH_MARGIN = 8.0
C_ARITH_MEASURED = 578.0     # worst figure of tests/test_update_ref_cpu.py (printed there; the test asserts it is not exceeded)
C_ARITH = ARITH_MARGIN * C_ARITH_MEASURED
C_ARITH_LARGE_MEASURED = 358.0  # worst figure of tests/test_update_ref_fast_cpu.py at the large cases (n = 3157, m = 2048 and 2050)
C_ARITH_LARGE = ARITH_MARGIN * C_ARITH_LARGE_MEASURED
K_NORM = 32.0
DEPTH_RHO_SD = 0.01


def u_store_of(storage):
    return 2.0 ** -24 if storage is np.float32 else 0.0


def column_exponents(diagP):
    """e_j of the a-priori column scales (kernels_update.hip gather_body): ilogb(sqrt(P_jj) 1.001) + 1, 0 where P_jj <= 0"""
    d = np.asarray(diagP, dtype=np.float64)
    e = np.zeros(len(d), dtype=np.int64)
    pos = d > 0.0
    e[pos] = np.frexp(np.sqrt(d[pos]) * 1.001)[1]  # s = f 2^E, f in [0.5, 1): ilogb(s) + 1 = E; sqrt and the product round as on the device
    return e


def balanced_digits(X):
    """int64 X, |X| <= 2^38 -> [PX_S, ...] digits in [-128, 127], most significant first: the bytes of (X + K) xor K"""
    K = np.int64(0x8080808080)
    W = (np.asarray(X, dtype=np.int64) + K) ^ K
    return np.stack([((W >> np.int64(8 * (PX_S - 1 - s))) & np.int64(255)).astype(np.uint8).view(np.int8).astype(np.int64)
                     for s in range(PX_S)])


def digit_bound(B, e):
    """dig_ij of the module docstring from the reference's B [m, n] (longdouble) and the column exponents e -> (dig [n, n], q [n])"""
    m, n = B.shape
    q = np.ldexp(LD(1), (e - (PX_BITS + 1)).astype(np.int64)).astype(LD)
    a = np.abs(B).sum(axis=0)
    dig = np.outer(a, q) + np.outer(q, a) + m * np.outer(q, q)
    X = np.rint(B * np.ldexp(LD(1), (PX_BITS - e).astype(np.int64))[None, :])
    assert np.abs(X).max(initial=0) <= 2.0 ** PX_BITS, "a column of B exceeds its a-priori scale"
    D = np.abs(balanced_digits(X.astype(np.int64))).astype(np.float64)  # products and sums below 2^53: exact in fp64
    assert np.array_equal((balanced_digits(X.astype(np.int64)) * (256 ** np.arange(PX_S - 1, -1, -1))[:, None, None]).sum(axis=0),
                          X.astype(np.int64))
    drop = _dropped_levels(D.transpose(0, 2, 1), D).astype(LD)
    scale = np.ldexp(LD(1), (e[:, None] + e[None, :] - 2 * PX_BITS).astype(np.int64))
    return dig + drop * scale, q


def _dropped_levels(DA, DB):
    """sum over the pairs s + t >= PX_S of 256^(2 (PX_S - 1) - s - t) DA_s @ DB_t (digit magnitudes [PX_S, rows, k] and [PX_S, k, cols]),
    regrouped as sum_s DA_s @ (sum_{t >= PX_S - s} 256^(2 (PX_S - 1) - s - t) DB_t): PX_S - 1 products instead of ten.  Integers in fp64:
    exact while every partial sum stays below 2^53, which is asserted (m <= 2080 rows of 128 256^3 (1 + 1/256 + ...) 128: 2^50)"""
    out = np.zeros((DA.shape[1], DB.shape[2]))
    total = 0.0
    for s in range(1, PX_S):
        T = np.zeros(DB.shape[1:])
        for t in range(PX_S - s, PX_S):
            T += 256.0 ** (2 * (PX_S - 1) - s - t) * DB[t]
        total += DA.shape[2] * DA[s].max(initial=0) * T.max(initial=0)
        out += DA[s] @ T
    assert total < 2.0 ** 53, "the dropped levels' sums leave the integers fp64 holds exactly"
    return out


def _digit_magnitudes(V, e_axis, axis):
    """|digits| [PX_S, rows, cols] of V (longdouble) cut under the scales 2^e along `axis` (0: one scale per row, 1: per column)"""
    sh = np.ldexp(LD(1), (PX_BITS - e_axis).astype(np.int64))
    X = np.rint(V * (sh[:, None] if axis == 0 else sh[None, :]))
    assert np.abs(X).max(initial=0) <= 2.0 ** PX_BITS
    return np.abs(balanced_digits(X.astype(np.int64))).astype(np.float64)


def _true_exponents(V, axis):
    """k_col_exp: the largest exponent field of a column, |v| < 2^e; an all-zero column: no scale, no digits"""
    top = np.abs(V).max(axis=axis).astype(np.float64)
    return np.where(top > 0, np.frexp(np.where(top > 0, top, 1.0))[1], -1022).astype(np.int64)


def lower_inverse(L):
    m = len(L)
    W = np.zeros((m, m), LD)
    for i in range(m):
        W[i, i] = 1 / L[i, i]
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
    return W


def sweep_plane_bound(S, L, B, e_col, W):
    """Delta [m, n] >= |B^ - B| for the rows of B that the sweep forms from digit planes (chol_bplanes.h), see the module docstring (c)"""
    m, n = B.shape
    el = np.frexp(np.sqrt(np.diag(S).astype(np.float64)) * 1.001)[1].astype(np.int64)  # k_assemble_S: ilogb(sqrt(S_rr) 1.001) + 1
    qL = np.ldexp(1.0, el - (PX_BITS + 1))
    qc = np.ldexp(1.0, e_col - (PX_BITS + 1))
    first = (np.arange(m) // 32) * 32  # first row of the row's own panel: the blocks before it come from the planes
    mask = (np.arange(m)[None, :] < first[:, None]).astype(np.float64)
    La, Ba = np.abs(L).astype(np.float64) * mask, np.abs(B).astype(np.float64)
    E = La.sum(axis=1)[:, None] * qc[None, :] + qL[:, None] * (mask @ Ba) + (qL * first)[:, None] * qc[None, :]
    DL = _digit_magnitudes(L, el, 0) * mask[None]
    E += _dropped_levels(DL, _digit_magnitudes(B, e_col, 1)) * np.ldexp(1.0, el[:, None] + e_col[None, :] - 2 * PX_BITS)
    return (np.abs(W).astype(np.float64) @ E) * (1 + 2.0 ** -30)  # (the bound itself is formed in fp64)


def gemm_plane_bound(W, A):
    """Delta [m, n] >= |B^ - B| for B = inv(L) G formed by the int8 GEMM from the digit planes of inv(L)' and G (k_b_gemm_i8p), (d)"""
    ew, eg = _true_exponents(W, 1), _true_exponents(A, 0)
    qw, qg = np.ldexp(1.0, ew - (PX_BITS + 1)), np.ldexp(1.0, eg - (PX_BITS + 1))
    Wa, Aa = np.abs(W).astype(np.float64), np.abs(A).astype(np.float64)
    E = Wa.sum(axis=1)[:, None] * qg[None, :] + qw[:, None] * Aa.sum(axis=0)[None, :] + len(A) * qw[:, None] * qg[None, :]
    E += _dropped_levels(_digit_magnitudes(W, ew, 0), _digit_magnitudes(A, eg, 1)) * np.ldexp(1.0, ew[:, None] + eg[None, :] - 2 * PX_BITS)
    return E * (1 + 2.0 ** -30)


def _through_b(Delta, B, z):
    """what an error Delta of the rows of B does to B'B (entrywise bound) and to B'z"""
    Ba = np.abs(B).astype(np.float64)
    M = Ba.T @ Delta
    return (M + M.T + Delta.T @ Delta).astype(LD), (Delta.T @ np.abs(z).astype(np.float64)).astype(LD)


def dense_rows(rows, n):
    row_start, col, val = rows
    H = np.zeros((len(row_start) - 1, n), LD)
    for i in range(len(row_start) - 1):
        H[i, col[row_start[i]:row_start[i + 1]]] = np.asarray(val[row_start[i]:row_start[i + 1]], dtype=np.float64).astype(LD)
    return H


def cholesky_lower(S):
    m = len(S)
    L = np.zeros((m, m), LD)
    for j in range(m):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def rounded(A, storage):
    return np.asarray(A).astype(storage).astype(LD)


class _Routes:
    """route -> (bound of B'B, bound of B'z) for the rows of B formed from digit planes; a route's bound is evaluated when it is
    first asked for (at 2050 rows each costs seconds, and a case asks for one)"""

    def __init__(self, S, L, B, e_col, W, A, z):
        self._in, self._done = (S, L, B, e_col, W, A, z), {}

    def __getitem__(self, route):
        if route not in self._done:
            S, L, B, e_col, W, A, z = self._in
            assert route in ("sweep", "gemm"), route
            Delta = sweep_plane_bound(S, L, B, e_col, W) if route == "sweep" else gemm_plane_bound(W, A)
            self._done[route] = _through_b(Delta, B, z)
        return self._done[route]


def core_of(x13, feature_pos, P, A, S, L, W, B, z, dx, P6):
    """the dict of update_core from the arithmetic's results (longdouble), with the digit bound of the downdate and the routes' bounds
    (numpy, shared by the interpreted and the compiled reference: tests/update_ref_fast.py)"""
    P64 = np.asarray(P, dtype=np.float64)
    sd = np.sqrt(np.maximum(np.diag(P64).astype(LD), 0))
    e_col = column_exponents(np.diag(P64))
    dig, q = digit_bound(B, e_col)
    return {"route": _Routes(S, L, B, e_col, W, A, z), "x": np.asarray(x13, dtype=np.float64).astype(LD),
            "fp": np.asarray(feature_pos, dtype=np.float64).reshape(-1, 6).astype(LD), "Pm": P64.astype(LD), "B": B, "z": z, "S": S, "L": L,
            "dx": dx, "sd": sd, "dig": dig, "q": q, "P6": P6, "W": W, "A": A}


def update_core(x13, feature_pos, P, rows, residual, R):
    """the arithmetic of the update in longdouble, before any rounding or dead-band (what the storage type and the configuration do
    not change: tests share it) -> dict"""
    Pm = np.asarray(P, dtype=np.float64).astype(LD)
    n = len(Pm)
    H = dense_rows(rows, n)
    m = len(H)
    res = np.atleast_1d(np.asarray(residual, dtype=np.float64)).astype(LD)
    A = H @ Pm
    S = A @ H.T + np.asarray(R, dtype=np.float64).reshape(m, m).astype(LD)
    S = xr.mirror_upper(S)
    L = cholesky_lower(S)
    z = np.zeros(m, LD)
    B = np.zeros((m, n), LD)
    for i in range(m):
        z[i] = (res[i] - L[i, :i] @ z[:i]) / L[i, i]
        B[i] = (A[i] - L[i, :i] @ B[:i]) / L[i, i]
    W = lower_inverse(L)
    return core_of(x13, feature_pos, P, A, S, L, W, B, z, B.T @ z, xr.mirror_upper(LD(0.5) * Pm + LD(0.5) * Pm.T - B.T @ B))


def update_ref(x13, feature_pos, feature_type, covpos, P, rows, residual, R, storage=np.float64, exact=False, update_cov=True):
    return with_bounds(update_core(x13, feature_pos, P, rows, residual, R), feature_type, covpos, storage, exact, update_cov)


def with_bounds(core, feature_type, covpos, storage=np.float64, exact=False, update_cov=True, c_arith=C_ARITH):
    """-> dict: x13, feature_pos, P, P_downdated (rounded to `storage` where the engine rounds), P_cmp / tol_P (what the engine's P
    is compared with and by how much, see the module docstring), P_downdated_cmp / tol_P_downdated, tol_x13 / tol_feature_pos,
    deadband_margin, B, z, S, L, dx (longdouble), scale (sqrt(P-_ii P-_jj)), dig (zeros unless exact), q.  Nothing is modified.
    exact: False (fp64 configuration), True or "sweep" (rows of B from digit planes inside the sweep), "gemm" (from the int8 GEMM),
    "measured" (EKF_UPDATE_PATH_SWEEP above 2048 rows: terms (a) + (b) under the columns' true scales, see (e) of the module docstring).
    update_cov False: the state-only update -- q is not normalised, P returned as given."""
    x, fp, Pm, B, z, S, L, dx, sd, P6 = (core[k] for k in ("x", "fp", "Pm", "B", "z", "S", "L", "dx", "sd", "P6"))
    n = len(Pm)
    u = u_store_of(storage)
    scale = np.outer(sd, sd)
    dig, q, dx_b = (core["dig"], core["q"], np.zeros(n, LD)) if exact else (np.zeros((n, n), LD), np.zeros(n, LD), np.zeros(n, LD))
    if exact == "measured":  # fp64 rows of B cut by the downdate under measured column scales; dx from the fp64 rows
        if "dig_measured" not in core:
            core["dig_measured"] = digit_bound(B, _true_exponents(B, 0))[0]
        dig, q = core["dig_measured"], np.zeros(n, LD)
    elif exact:  # True: the default route at these sizes, the rows of B inside the sweep
        dig_b, dx_b = core["route"]["sweep" if exact is True else exact]
        dig = dig + dig_b
    # ---- state
    tol_dx = q * np.abs(z).sum() + dx_b + c_arith * U64 * sd * np.sqrt(z @ z)
    tol_dx[~np.any(B != 0, axis=0)] = 0  # a structurally zero column of B (see the module docstring): dx_i = 0 in any order of summation
    margin = float((np.abs(np.abs(dx) - EKF_DELTA) / np.where(tol_dx > 0, tol_dx, LD(1e-300))).min())
    dxb = np.where(np.abs(dx) > EKF_DELTA, dx, LD(0))
    xn = x + dxb[:13]
    fpn = fp.copy()
    tol_fp = np.zeros(fp.shape, LD)
    for f in range(len(fp)):
        k = 6 if int(feature_type[f]) == FEATURE_INVERSE_DEPTH else 3
        c = int(covpos[f])
        fpn[f, :k] += dxb[c:c + k]
        tol_fp[f, :k] = tol_dx[c:c + k] + np.spacing(np.abs(fpn[f, :k]).astype(np.float64))
    tol_x = tol_dx[:13] + np.spacing(np.abs(xn).astype(np.float64))
    nrm, J = quat_norm_jacobian(xn[3:7])
    if update_cov:  # (the state-only update of the hypothesis test leaves q as it is: RANSAC's R is that of the un-normalised q)
        tq = tol_dx[3:7]
        xn[3:7] = xn[3:7] / nrm
        tol_x[3:7] = tq / nrm + np.abs(xn[3:7]) * tq.sum() / nrm + 2 * np.spacing(np.abs(xn[3:7]).astype(np.float64))
    out = {"x13": xn, "feature_pos": fpn, "tol_x13": tol_x, "tol_feature_pos": tol_fp, "deadband_margin": margin, "B": B, "z": z,
           "S": S, "L": L, "dx": dx, "scale": scale, "dig": dig, "q": q, "J": J}
    if not update_cov:
        out["P"] = out["P_cmp"] = Pm
        return out
    # ---- covariance
    tol6 = u * np.abs(P6) + (1 + u) * (dig + c_arith * U64 * scale)
    P6r = rounded(P6, storage)
    Pn = normalize_covariance(P6r, J)
    strip = np.zeros((n, n), dtype=bool)
    strip[3:7, :] = strip[:, 3:7] = True
    nb = normalize_bound(P6r, J)
    # rows / columns 3..6: the engine normalises its OWN rounded entries, each within tol6 of the reference's unrounded ones and so
    # within tol6 + u |ref| of the reference's rounded ones
    tol = np.where(strip, normalize_bound(tol6 + u * np.abs(P6), J) + u * np.abs(Pn)
                   + (K_NORM * U64 + 4 * float(tol_x[3:7].max())) * nb, tol6)
    out.update({"P_downdated": P6r, "P_downdated_cmp": P6, "tol_P_downdated": tol6, "P": rounded(Pn, storage),
                "P_cmp": np.where(strip, Pn, P6), "tol_P": tol, "strip": strip})
    return out


def worst(dev, ref, tol):
    """(max |dev - ref| / tol, its index); an entry with tol = 0 must be exact"""
    err = np.abs(np.asarray(dev).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0))
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), tuple(int(a) for a in at)


# ------------------------------------------------------------------------------------------------ the cases' maps
def spiky_scene(n):
    """The mixed depth / inverse-depth scene of state dimension n (predict_ref.types_for_n, every feature in view) with a
    covariance of the synthetic sequences' structure: every feature is seeded as an inverse-depth feature by synth.seed_map from
    its pixel in the camera of x13 (variance 1 on the inverse depth beside 2e-16 on the camera's pose and the pixel noise through
    the Jacobians on the angles), and the rows / columns of a depth feature are those of its world point, T P T' with T = dX/dy
    (map_points_ref.world_point) -- symmetric positive semi-definite by construction.  A feature is converted to a point once its
    depth is known: the inverse depth of a feature that becomes a depth feature gets DEPTH_RHO_SD = 0.01 instead of 1 first (it is
    correlated with nothing, so this is one diagonal entry).  With sigma = 1 m along the ray, the state correction of an unmeasured
    point (1e-14, through the camera's 2e-16 alone: dead-banded) would lie within the exact configurations' digit term of the
    dead-band and the case would be invalid (module docstring)."""
    from predict_ref import types_for_n

    return spiky_scene_of_types(("spiky", n), types_for_n(n))


LARGE_FEATURES = 1032
LARGE_N = 3157          # 13 + 16 x 6 + 1016 x 3; n_pad = 3200: 25 tiles of 128, the last with 85 live columns
LARGE_M = (1024, 1025)  # m = 2048: the last size with B in the sweep; m = 2050: m_pad = 2080, 65 steps, the second mask chunk
# The features that M = 1024 leaves unmeasured.  As points of the spiky scene (correlated with the camera through its 2e-16 alone)
# their correction is 1e-14 .. 1e-13, dead-banded, while sum |z| over 2048 rows is 316 and the exact configurations' state terms are
# 1e-12 .. 9e-12 (q_i sum |z|) and 1e-10 (rows of B from the planes in the sweep): deadband_margin 0.004 / 0.1, the case invalid.  They
# are held as uncorrelated landmarks instead, whose correction is a sum of zeros until they are measured (M = 1025 measures the first).
LARGE_UNCORRELATED = tuple(range(1024, 1032))
LARGE_CASES = [("large", LARGE_N, M) for M in LARGE_M]


def large_types():
    """1032 features, all in view: feature f is an inverse-depth feature where f % 64 == 31 (16 of them), every other one XYZ --
    close to the smallest map that allows M = 1025 (all XYZ: n = 3088) with both kinds and a ragged last tile"""
    from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH

    return np.where(np.arange(LARGE_FEATURES) % 64 == 31, FEATURE_INVERSE_DEPTH, FEATURE_DEPTH).astype(np.int32)


def spiky_scene_of_types(key, types, uncorrelated=()):
    """spiky_scene for an explicit list of feature types (cached under `key`); an inverse-depth feature keeps seed_map's sigma = 1 on
    its inverse depth, an XYZ feature gets DEPTH_RHO_SD before the conversion.  uncorrelated: features whose covariances with the
    camera and with every other feature are stored zeros (a landmark taken over from a prior map): while such a feature is not
    measured its columns of B are sums of products with stored zeros, so its state correction is zero in any order of summation."""
    import map_points_ref as mp
    import predict_ref as pr
    from openekfmonoslam_amd import synth

    if key in pr._SCENES:
        return pr._SCENES[key]
    types = np.asarray(types, dtype=np.int32)
    n = 13 + int(sum(6 if t == FEATURE_INVERSE_DEPTH else 3 for t in types))
    s = pr.make_scene(types, vis=np.ones(len(types), dtype=bool), with_P0=False)
    R = synth.quat_to_rot(s.x13[3:7])
    world = np.array([mp.world_point(y, t)[0] for y, t in zip(s.feature_pos, types)])
    uv, h = synth.project(s.cam, s.x13[0:3], R, world)
    assert np.all(h[:, 2] > 0.5)
    _, P13 = synth.initial_state_and_covariance(s.par)
    pos6, P6 = synth.seed_map(s.cam, s.par, s.x13, P13, uv)
    for f, t in enumerate(types):
        if t != FEATURE_INVERSE_DEPTH:
            k = 18 + 6 * f
            assert not np.any(np.delete(P6[k], k))
            P6[k, k] *= DEPTH_RHO_SD ** 2
    T = np.zeros((n, 13 + 6 * len(types)))
    T[:13, :13] = np.eye(13)
    for f, t in enumerate(types):
        c = int(s.covpos[f])
        if t == FEATURE_INVERSE_DEPTH:
            T[c:c + 6, 13 + 6 * f:19 + 6 * f] = np.eye(6)
        else:
            T[c:c + 3, 13 + 6 * f:19 + 6 * f] = mp.world_point(pos6[f], FEATURE_INVERSE_DEPTH)[1]
    P0 = T @ P6 @ T.T
    s.P0 = 0.5 * (P0 + P0.T)
    for f in uncorrelated:  # (a principal block cut loose from the rest: still symmetric positive semi-definite)
        c, k = int(s.covpos[f]), 6 if types[f] == FEATURE_INVERSE_DEPTH else 3
        own = s.P0[c:c + k, c:c + k].copy()
        s.P0[c:c + k, :] = 0.0
        s.P0[:, c:c + k] = 0.0
        s.P0[c:c + k, c:c + k] = own
    pr._SCENES[key] = s
    return s


def matches_for(preds, M):
    """the first M predictions, a fraction of a pixel off"""
    from openekfmonoslam_amd.ekftypes import MATCH_DTYPE

    assert len(preds) >= M
    m = np.zeros(M, dtype=MATCH_DTYPE)
    m["featureIndex"] = preds["featureIndex"][:M]
    m["keypointIndex"] = -1
    k = np.arange(M)
    m["imagePos"] = preds["imagePos"][:M] + np.stack([0.3 * np.cos(0.7 * k + 0.2), -0.2 * np.sin(1.3 * k + 0.4) - 0.1], -1)
    return m


MIXED_N = (85, 127, 130, 253, 256, 259, 511, 514)  # column edges of the downdate's 128-wide tiles and k_dx_planes' 256-column blocks
MIXED_M = 17
ROW_M = (1, 8, 9, 16, 17, 33, 49, 65, 160)         # row edges on SyntheticSequence(170, 1), n = 1033
CASES = [("mixed", n, MIXED_M) for n in MIXED_N] + [("seq170", 1033, M) for M in ROW_M]
_SEQ = {}


def case_map(kind, n):
    """-> (cam, par, x13, feature_pos, feature_type, desc, P0) of a case's map before the prediction"""
    if kind in ("mixed", "large"):
        s = spiky_scene(n) if kind == "mixed" else spiky_scene_of_types(("spiky", "large"), large_types(), LARGE_UNCORRELATED)
        assert s.n == n
        return s.cam, s.par, s.x13, s.feature_pos, s.feature_type, s.desc, s.P0
    from openekfmonoslam_amd.synth import SyntheticSequence

    if "seq170" not in _SEQ:
        _SEQ["seq170"] = SyntheticSequence(170, 1)
    s = _SEQ["seq170"]
    assert s.state_dim == n
    return s.cam, s.par, s.x13, s.feature_pos, s.feature_type, s.feature_desc, s.P0
