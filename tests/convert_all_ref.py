"""TEST INFRASTRUCTURE ONLY: the batch conversion of inverse-depth features to XYZ (ekf_convert_all_inverse_depth_to_depth;
k_convert_all_prepare and k_convert_all_P in csrc/kernels_map.hip) restated in numpy in np.longdouble on top of tests/map_ref.py,
with the per-entry tolerance of every value the device computes, and the scene of the selection test.

With R the block-diagonal matrix of 1 for a kept row and the 3 x 6 Jacobian J_f of every converted feature, the new covariance is
P' = R P R'.  s(u) is the old index of the first source row of new row u, w_u its weights (a row of J_f over six old rows, or the
single weight 1).  As the device defines it:

    u, v both kept     P'[u][v] = P[s(u)][s(v)], moved, in both triangles                         tolerance 0
    otherwise, u <= v  T[u][c] = sum_a w_u[a] P[s(u) + a][c],  P'[u][v] = sum_b T[u][s(v) + b] w_v[b], rounded to storage once
    otherwise, u > v   the copy of P'[v][u]                                                       the tolerance of its twin

The tolerance is map_ref.convert_ref's (u_store |ref| + u64 K sum|terms|) with the same operation counts, because the kernel forms
T and the products the way k_convert_rows and k_convert_apply do: six-term sums from 0.0, T kept in fp64, one rounding to storage.

    converted row u    Tabs = |J_u| |P rows|,  ET = (Jerr_u + 6 |J_u|) |P rows|
    kept row u         Tabs = |P row|,         ET = 0        (a copy)
    kept column v      tol = u_store |ref| + u64 (ET + Tabs)[:, s(v)]          (the rounding to storage)
    converted column   tol = u_store |ref| + u64 (ET[:, cols] |J_v|' + Tabs[:, cols] (Jerr_v + 6 |J_v|)' + Tabs[:, cols] |J_v|')

Both column rules are one expression once a kept row or column is written as the weight vector (1, 0, 0, 0, 0, 0) with error 0."""
import numpy as np

import map_ref as mr
from map_ref import FEATURE_DEPTH, FEATURE_INVERSE_DEPTH, LD, U64, _ld, dim, make_scene


def row_tables(types, covpos, selected):
    """-> s [n'] (first source row of every new row), W [n', 6] (its weights), slot [n'] (3 k + a for row a of the k-th converted
    feature, -1 for a kept row), kept [n'] -- from the layout BEFORE the conversion"""
    types, covpos = np.asarray(types), np.asarray(covpos, dtype=np.int64)
    sel = {int(f): k for k, f in enumerate(selected)}
    s, slot = list(range(13)), [-1] * 13
    for f in range(len(types)):
        if f in sel:
            assert types[f] == FEATURE_INVERSE_DEPTH
            s += [int(covpos[f])] * 3
            slot += [3 * sel[f] + a for a in range(3)]
        else:
            d = dim(types[f])
            s += [int(covpos[f]) + a for a in range(d)]
            slot += [-1] * d
    s, slot = np.array(s, dtype=np.int64), np.array(slot, dtype=np.int64)
    return s, slot, slot < 0


def convert_all_ref(x13, feature_pos, types, covpos, P, selected, u_store=0.0):
    """x13, feature_pos and P [n, n] as stored before the conversion of the inverse-depth features `selected` (ascending) -> dict:
    "types", "covpos", "n": the new layout; "xyz" (ref, tol) [len(selected), 3]; "P" (ref, tol) [n', n']; "kept" [n'] and "s" [n']:
    which new rows are copies and the first source row of every new row"""
    selected = [int(f) for f in selected]
    assert selected == sorted(set(selected))
    P = _ld(P)
    n = P.shape[0]
    fp = np.asarray(feature_pos, dtype=np.float64).reshape(-1, 6)
    s, slot, kept = row_tables(types, covpos, selected)
    n_new = len(s)
    # weights and their errors (units of u64) per new row; a kept row is (1, 0, 0, 0, 0, 0), exactly
    W, WE = np.zeros((n_new, 6), LD), np.zeros((n_new, 6), LD)
    W[kept, 0] = 1
    xyz, xyz_tol = np.zeros((len(selected), 3), LD), np.zeros((len(selected), 3), LD)
    for k, f in enumerate(selected):
        X, J, Jerr = mr.convert_prepare(fp[f])
        for a in range(3):
            u = int(np.nonzero(slot == 3 * k + a)[0][0])
            W[u], WE[u] = J[a], Jerr[a] + 6 * np.abs(J[a])
            xyz[k, a], xyz_tol[k, a] = X[a].v, U64 * X[a].err
    Wabs, Pabs = np.abs(W), np.abs(P)
    idx = [np.minimum(s + a, n - 1) for a in range(6)]  # (beyond a kept row's single source the weight is 0)
    T = sum(W[:, a, None] * P[idx[a], :] for a in range(6))
    Tabs = sum(Wabs[:, a, None] * Pabs[idx[a], :] for a in range(6))
    ET = sum(WE[:, a, None] * Pabs[idx[a], :] for a in range(6))
    ref = sum(T[:, idx[b]] * W[None, :, b] for b in range(6))
    err = sum(ET[:, idx[b]] * Wabs[None, :, b] + Tabs[:, idx[b]] * WE[None, :, b] + Tabs[:, idx[b]] * Wabs[None, :, b] for b in range(6))
    tol = u_store * np.abs(ref) + U64 * err
    upper = np.arange(n_new)[None, :] >= np.arange(n_new)[:, None]
    ref, tol = np.where(upper, ref, ref.T), np.where(upper, tol, tol.T)  # computed for u <= v, copied to the mirror
    moved = kept[:, None] & kept[None, :]
    ref = np.where(moved, P[np.ix_(s, s)], ref)
    tol = np.where(moved, 0, tol)
    nt = np.asarray(types).copy()
    nt[selected] = FEATURE_DEPTH
    nc, nn = mr.layout(nt)
    assert nn == n_new == n - 3 * len(selected)
    return {"types": nt, "covpos": nc, "n": n_new, "xyz": (xyz, xyz_tol), "P": (ref, tol), "kept": kept, "s": s}


def sequential_ref(x13, feature_pos, types, covpos, P, selected):
    """map_ref.convert_ref applied feature by feature in ascending order, in longdouble without a rounding in between -> P'"""
    fp = np.asarray(feature_pos, dtype=np.float64).reshape(-1, 6)
    ty, cp = np.asarray(types).copy(), np.asarray(covpos).copy()
    Ps = np.asarray(P, dtype=LD)
    for f in selected:
        r = mr.convert_ref(x13, fp, ty, cp, Ps, f)
        o2n, p0 = r["old_of_new"], r["pos"]
        Pn = Ps[np.ix_(o2n, o2n)].copy()
        T3 = r["rows"][0]
        Pn[p0:p0 + 3, :] = T3[:, o2n]
        Pn[:, p0:p0 + 3] = T3[:, o2n].T
        Pn[p0:p0 + 3, p0:p0 + 3] = r["block"][0]
        Ps = Pn
        ty[f] = FEATURE_DEPTH
        cp = mr.layout(ty)[0]
    return Ps


# ------------------------------------------------------------------------------------------------ selection of many
SELECT_MANY_N = 300
SELECT_MANY_INVERSE = (0, 100, 254, 255, 256, 299)
SELECT_MANY_CHOSEN = (0, 254, 256, 299)  # both sides of k_linearity's workgroup seam, the first and the last feature
_SCENE = {}


def select_many_scene():
    """300 features, XYZ but for SELECT_MANY_INVERSE -> (scene, P, threshold): the rho row and column of the CHOSEN features scaled
    as map_ref.select_scene does, so that their linearity index is 1/16 of the smallest one of the others (100 and 255); threshold =
    1/4 of that smallest one.  n = 931."""
    if "many" not in _SCENE:
        types = np.full(SELECT_MANY_N, FEATURE_DEPTH, dtype=np.int32)
        types[list(SELECT_MANY_INVERSE)] = FEATURE_INVERSE_DEPTH
        s = make_scene(types)
        P = s.P0.copy()
        L0 = mr.linearity_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, P)[0]
        lmin = float(min(L0[f] for f in SELECT_MANY_INVERSE if f not in SELECT_MANY_CHOSEN))
        for f in SELECT_MANY_CHOSEN:
            scale = (lmin / 16.0) / float(L0[f])  # L is proportional to sqrt(P[rho][rho])
            r = int(s.covpos[f]) + 5
            P[r, :] *= scale
            P[:, r] *= scale
        _SCENE["many"] = (s, P, lmin / 4.0)
    return _SCENE["many"]
