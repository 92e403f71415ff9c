"""TEST INFRASTRUCTURE ONLY: map management (csrc/kernels_map.hip and its host halves in csrc/map_host.cpp) restated in numpy in
np.longdouble -- adding a batch of features, removing features, converting an inverse-depth feature to XYZ, the linearity index --
with the per-entry tolerances of every value the device computes, and the scenes the stage tests run on
(tests/test_gpu_map_stages.py on the device, tests/test_map_ref_cpu.py against the oracle and for the input conditions).

The reference works from what the engine itself stores: x, feature_pos and P as get_state() returns them immediately before the
operation (in fp32 storage that P is the fp32 values, exactly), so the storage rounding of an input is not counted as an error of
the operation.  The formulas are those of EKF/AddMapFeature.cpp:42-90, :109-216, :221-344 and EKF/MapManagement.cpp:168-259,
:312-490 (oracle/ekf_oracle.c:380-617); the oracle itself is not called.  R is formed from q here, in longdouble: the device uses
the R it caches beside the state, and a cache that was not refreshed with q is an error of the device.

Tolerances have the project's form  u_store |ref| + K u64 sum|terms|  (predict_ref.py), u_store = 2^-24 where P is stored in fp32
and 0 otherwise, sum|terms| the same expression evaluated with absolute values.  No K is fitted to device output: each is counted
from the operations of the code under test, and the counting is done by the class V below, which carries every intermediate of
k_addfeat_prepare, k_convert_prepare and linearity_index as (value, abs-evaluated value, K) under these rules (u = 2^-53; an
intermediate x is known to K_x u abs(x)):

    x + y, x - y     K = max(K_x, K_y) + 1      abs = abs(x) + abs(y)          one rounding on top of the worse operand
    x * y            K = K_x + K_y + 1          abs = abs(x) abs(y)
    x / y            K = K_x + K_y + 1          abs = abs(x) abs(y) / y^2      (abs(y) / |y| >= 1 carries y's own cancellation)
    2 x, -x          K = K_x                                                   exact
    sqrt(x)          K = ceil(K_x / 2) + 2      abs = sqrt(x) abs(x) / x       half the relative error of x, 1 ulp = 2 u for the root
    sin, cos         K = 4                      abs = |value|                  2 ulp = 4 u, of an exact argument
    input            K = 0

A fused multiply-add rounds once where the rule counts twice, so contraction (kernels_map.hip is compiled with it) stays inside.
The accuracy table of the device math library is not on the build machines, so atan2, sin and cos take the 2 ulp that the
prediction tests already assume (predict_ref.py, K_F).  The K that result, line by line (K_ADD, K_CONV and K_LIN below hold the
same numbers and are asserted where the code counts them, so this list cannot drift from the code):

  add (k_addfeat_prepare)
    R (cached; quat_to_rot)       4     four squares and three additions on the diagonal (two products and one off it)
    mx = ud - cx                  1
    dxm = dx mx                   2
    rd2 = dxm^2 + dym^2           6     2 + 2 + 1 per square, + 1
    dist = 1 + k1 rd2 + k2 rd2^2  15    (k2 rd2) rd2 = 7 + 6 + 1 = 14, + 1 for the last addition (1 + k1 rd2: 8)
    uu = cx + mx dist             18    mx dist = 1 + 15 + 1 = 17, + 1
    xyz_c = -(cx - uu) / fx       20
    g = R xyz_c                   27    R[.] xyz_c = 4 + 20 + 1 = 25, two additions
    xxzz = g0^2 + g2^2            56    27 + 27 + 1, + 1          sq = sqrt(xxzz): 30        nsq = xxzz + g1^2: 57
    dth = g / xxzz                84    27 + 56 + 1
    dph = g0 g1 / (nsq sq)        144   55 + (57 + 30 + 1) + 1
    dg = d(R(q) xyz_c)/dq         23    2 q[.] xyz_c = 21, two additions
    Jpo[3][3+i] = dth . dg        110   84 + 23 + 1 = 108, two additions     Jpo[4][3+i] = dph . dg: 170
    sub = [dth; dph] R            91 / 151        s2m = sub / f: 92 / 152
    a = k1 + 2 k2 rd2             8     dh = b + mx a (mx dx2): (1 + 8 + 1) + (1 + 1 + 1) + 1 = 14, 16 with b = dist (15)
    Jhr = s2m dh                  170   152 + 16 + 1, + 1
    theta, phi                    |dth| . err(g) (|dph| . err(g)) with err(g) = 27 u abs(g), + 2 ulp |value|; phi also takes the
                                  rounding of its second argument sqrt(xxzz) (3 u relative on top of g's, at most 3 u / 2 in the angle)
  new rows (k_addfeat_rows)       sum_k (K_J Jabs[a,k] + (7 + 1) |J[a,k]|) |P[k,c]|: a 7-term dot product and the rounding to T
  corner (k_addfeat_corner)       W = Jpo_j P77 (7 terms, kept in fp64), W Jpo_i' (7 terms) to first order in both factors,
                                  + 6 on Jhr N Jhr' beside the errors of its two entries of Jhr (two products, two additions, the
                                  addition to the sum), + 3 on everything for that last addition and the rounding to T
  convert (k_convert_prepare)
    m = dir_vec                   9 (cos sin), 4 (-sin)
    X = p + m / rho               11
    J[.][3], J[.][4]              10    cos cos / rho = 4 + 4 + 1, + 1  (J[1][4] = -cos / rho: 5)
    J[.][5] = -m / rho^2          11    9 + 1 + 1
  rows (k_convert_rows)           sum_k (K_J Jabs[a,k] + (6 + 1) |J[a,k]|) |P[pos+k,c]|  (T3 itself stays fp64: 6, + 1 for T)
  block (k_convert_apply)         T3[:, blk] J' (6 terms) to first order in both factors, + 1 for the rounding to T
  linearity_index
    sigma = sqrt(var) / rho^2     4     2 + 1 + 1
    xyz = p + m / rho             11    tc = xyz - r, tf = xyz - p: 12
    dot = tc . tf                 27    12 + 12 + 1 = 25, two additions       df, dc = sqrt(t . t): 16
    L = 4 sigma (dot / (df dc)) / dc    84    4 sigma: 5 (the exact factor 4 is counted); df dc: 33; dot / .: 61; product: 67; / dc

Entries that an operation only moves or leaves alone have tolerance 0; so have the rows of an added feature that are copies of
rows of P (Jpo[0:3] is three unit rows: products with 1.0 and 0.0 and sums with 0.0 are exact) and its rho row (Jpo[5] = 0).
"""
import numpy as np

from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH, FEATURE_INVERSE_DEPTH, s3_params
from predict_ref import LD, U32, U64, _hash01, _quat_to_rot, dim, make_P0, make_scene, types_for_n, worst_ratio  # noqa: F401

ULP_TRIG = 2  # atan2, sin, cos on the device: the 2 ulp the prediction tests assume (no accuracy table on the build machines)
K_TRIG = 2 * ULP_TRIG  # 1 ulp <= 2 u
K_R = 4
K_ADD = {"mx": 1, "dxm": 2, "rd2": 6, "dist": 15, "uu": 18, "xyz_c": 20, "g": 27, "xxzz": 56, "sq": 30, "nsq": 57, "dth": 84, "dph": 144,
         "dg": 23, "Jpo": (110, 170), "sub": (91, 151), "a": 8, "dh": 16, "Jhr": 170}
K_CONV = {"m": 9, "X": 11, "J3": 10, "J14": 5, "J5": 11}
K_LIN = {"sigma": 4, "m": 9, "xyz": 11, "tc": 12, "dot": 27, "df": 16, "L": 84}

# ---- the sizes of the stage tests ("Stage tests of map management"); every n is 1 mod 3
ADD_N_OLD = [13, 253, 256, 259, 511, 514]  # the last thread of k_addfeat_rows' workgroup 0, a full one, three threads in the next; again at 512
ADD_COUNTS = [1, 5, 64, 65]  # 65: a second k_addfeat_prepare block, a 65 x 65 corner grid
ADD_STARRED = [(256, 1), (256, 65), (259, 1), (259, 65)]  # these also in the exact configurations
# 1024 = 13 + 3 * 337 is the smallest map size that is a multiple of 256: four workgroups of k_addfeat_rows full to the last thread.
# A column base that falls short of 256 per workgroup still reaches every column at the sizes above (the workgroups overlap, the
# grid is rounded up); here it leaves the last columns without their new rows.
ADD_FULL_WORKGROUPS = (1024, 1)
# (n_new, drop set), from a start map of 300 < n <= 650 columns: one feature cannot be dropped from such a map down to 259 or fewer
# columns, so the first and the last feature alone are dropped at 511 and 514 ("every other" drops feature 0 at the small sizes)
REMOVE_CASES = [(13, "all"), (253, "straddle"), (253, "every other"), (256, "straddle"), (256, "every other"), (259, "straddle"),
                (259, "every other"), (511, "first"), (511, "last"), (511, "straddle"), (514, "first"), (514, "last"),
                (514, "straddle")]
REMOVE_STARRED = [(256, "straddle"), (259, "every other")]
# (n, pos): XYZ features in front of the first inverse-depth one; 250: its block ends at column 255, 253: it straddles 256;
# (259, 253) and (514, 508): it is the last feature (pos + 6 == n)
CONVERT_CASES = [(259, 13), (259, 250), (259, 253), (514, 13), (514, 250), (514, 253), (514, 256), (514, 508)]
CONVERT_STARRED = [(259, 253), (514, 253), (514, 256)]
# (N, f*): the one feature below the threshold; None: no feature below it
SELECT_CASES = [(255, 0), (255, 254), (257, 0), (257, 255), (257, 256), (300, 0), (300, 255), (300, 256), (300, 299), (300, None)]


# ------------------------------------------------------------------------------------------------ (value, abs, K)
class V:
    """an intermediate of the code under test: value, the same expression with absolute values, roundings on the longest path"""
    __slots__ = ("v", "a", "k")

    def __init__(self, v, a=None, k=0):
        self.v = np.asarray(v, dtype=LD)
        self.a = np.abs(self.v) if a is None else np.asarray(a, dtype=LD)
        self.k = int(k)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(LD(x))

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.a + o.a, max(self.k, o.k) + 1)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.a + o.a, max(self.k, o.k) + 1)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.a * o.a, self.k + o.k + 1)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.v / o.v, self.a * o.a / (o.v * o.v), self.k + o.k + 1)

    def __neg__(self):
        return V(-self.v, self.a, self.k)

    def twice(self):
        return V(2 * self.v, 2 * self.a, self.k)

    def sqrt(self):
        r = np.sqrt(self.v)
        return V(r, r * self.a / self.v, (self.k + 1) // 2 + 2)

    @property
    def err(self):
        """bound of |device - value| in units of u64"""
        return self.k * self.a


def _trig(fn, x):
    return V(fn(np.asarray(x, dtype=LD)), None, K_TRIG)


def _dot(xs, ys):
    """s = 0.0; s += x * y ...: the first addition (to 0.0) is exact"""
    s = xs[0] * ys[0]
    for x, y in zip(xs[1:], ys[1:]):
        s = s + x * y
    return s


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ add
def add_prepare(x13, cam, uv):
    """k_addfeat_prepare for `count` pixels at once -> "theta", "phi": (value, tolerance) [count]; "Jpo" [count, 6, 7] and "Jhr"
    [count, 6, 3]: (value, err) with err = K * abs in units of u64; "g" [count, 3]: the ray of every pixel in world axes"""
    x = _ld(x13)
    q = x[3:7]
    uv = _ld(uv).reshape(-1, 2)
    ud, vd = V(uv[:, 0]), V(uv[:, 1])
    c = cam
    Rl = _quat_to_rot(q)
    r, qx, qy, qz = q
    Rabs = np.array([[r * r + qx * qx + qy * qy + qz * qz, 2 * (abs(qx * qy) + abs(r * qz)), 2 * (abs(qz * qx) + abs(r * qy))],
                     [2 * (abs(qx * qy) + abs(r * qz)), r * r + qx * qx + qy * qy + qz * qz, 2 * (abs(qy * qz) + abs(r * qx))],
                     [2 * (abs(qz * qx) + abs(r * qy)), 2 * (abs(qy * qz) + abs(r * qx)), r * r + qx * qx + qy * qy + qz * qz]], LD)
    R = [[V(Rl[i, j], Rabs[i, j], K_R) for j in range(3)] for i in range(3)]
    mx, my = ud - c.cx, vd - c.cy
    dxm, dym = V.of(c.dx) * mx, V.of(c.dy) * my
    rd2 = dxm * dxm + dym * dym
    dist = 1 + V.of(c.k1) * rd2 + V.of(c.k2) * rd2 * rd2
    uu, vu = c.cx + mx * dist, c.cy + my * dist
    xc = [-(c.cx - uu) / c.fx, -(c.cy - vu) / c.fy, V(np.ones(len(uv), LD))]
    g = [R[i][0] * xc[0] + R[i][1] * xc[1] + R[i][2] * xc[2] for i in range(3)]
    xw, yw, zw = g
    xxzz = xw * xw + zw * zw
    sq = xxzz.sqrt()
    nsq = xxzz + yw * yw
    zero = V(np.zeros(len(uv), LD))
    dth = [zw / xxzz, zero, -xw / xxzz]
    dph = [xw * yw / (nsq * sq), -sq / nsq, zw * yw / (nsq * sq)]
    # jac_rot_by_quat(q, xyz_c): rows = components of g, columns = components of q
    q0, q1, q2, q3 = (V(2 * q[i]) for i in range(4))
    X, Y, Z = xc
    dg = [[q0 * X - q3 * Y + q2 * Z, q1 * X + q2 * Y + q3 * Z, -q2 * X + q1 * Y + q0 * Z, -q3 * X - q0 * Y + q1 * Z],
          [q3 * X + q0 * Y - q1 * Z, q2 * X - q1 * Y - q0 * Z, q1 * X + q2 * Y + q3 * Z, q0 * X - q3 * Y + q2 * Z],
          [-q2 * X + q1 * Y + q0 * Z, q3 * X + q0 * Y - q1 * Z, -q0 * X + q3 * Y - q2 * Z, q1 * X + q2 * Y + q3 * Z]]
    count = len(uv)
    Jpo, Jpo_err = np.zeros((count, 6, 7), LD), np.zeros((count, 6, 7), LD)
    for i in range(3):
        Jpo[:, i, i] = 1
    for i in range(4):
        s1 = _dot(dth, [dg[k][i] for k in range(3)])
        s2 = _dot(dph, [dg[k][i] for k in range(3)])
        ks = (s1.k, s2.k)
        Jpo[:, 3, 3 + i], Jpo_err[:, 3, 3 + i] = s1.v, s1.err
        Jpo[:, 4, 3 + i], Jpo_err[:, 4, 3 + i] = s2.v, s2.err
    sub = [_dot(dth, [R[k][i] for k in range(3)]) for i in range(3)] + [_dot(dph, [R[k][i] for k in range(3)]) for i in range(3)]
    s2m = [sub[0] / c.fx, sub[1] / c.fy, sub[3] / c.fx, sub[4] / c.fy]
    a = c.k1 + (V.of(c.k2) * rd2).twice()
    b = 1 + V.of(c.k1) * rd2 + V.of(c.k2) * rd2 * rd2
    dx2, dy2 = (V.of(c.dx) * c.dx).twice(), (V.of(c.dy) * c.dy).twice()
    dh = [b + mx * a * (mx * dx2), mx * a * (my * dy2), my * a * (mx * dx2), my * a * (my * dy2) + b]
    Jhr, Jhr_err = np.zeros((count, 6, 3), LD), np.zeros((count, 6, 3), LD)
    kh = 0
    for (row, col), h in {(3, 0): s2m[0] * dh[0] + s2m[1] * dh[2], (3, 1): s2m[0] * dh[1] + s2m[1] * dh[3],
                          (4, 0): s2m[2] * dh[0] + s2m[3] * dh[2], (4, 1): s2m[2] * dh[1] + s2m[3] * dh[3]}.items():
        kh = max(kh, h.k)
        Jhr[:, row, col], Jhr_err[:, row, col] = h.v, h.err
    Jhr[:, 5, 2] = 1
    got = {"mx": mx.k, "dxm": dxm.k, "rd2": rd2.k, "dist": dist.k, "uu": uu.k, "xyz_c": xc[0].k, "g": g[0].k, "xxzz": xxzz.k,
           "sq": sq.k, "nsq": nsq.k, "dth": dth[0].k, "dph": max(d.k for d in dph), "dg": dg[0][0].k, "Jpo": ks, "sub": (sub[0].k, sub[3].k),
           "a": a.k, "dh": max(d.k for d in dh), "Jhr": kh}
    assert got == K_ADD, got
    gerr = [gi.err for gi in g]
    theta = np.arctan2(xw.v, zw.v)
    phi = np.arctan2(-yw.v, sq.v)
    tol_theta = U64 * (sum(np.abs(dth[k].v) * gerr[k] for k in range(3)) + K_TRIG * np.abs(theta))
    tol_phi = U64 * (sum(np.abs(dph[k].v) * gerr[k] for k in range(3)) + K_TRIG * np.abs(phi) + LD(1.5))
    return {"theta": (theta, tol_theta), "phi": (phi, tol_phi), "Jpo": (Jpo, Jpo_err), "Jhr": (Jhr, Jhr_err),
            "g": np.stack([gi.v for gi in g], -1)}


EXACT_ROWS = (0, 1, 2, 5)  # rows of a new feature's block that are copies of rows of P, or zero


def add_ref(x13, P, cam, par, uv, u_store=0.0):
    """x13 and P [n_old, n_old] as get_state() returns them before ekf_add_features(uv [count, 2]) -> dict of (ref, tol):
    "feature_pos" [count, 6], "rows" [count, 6, n_old] (= Jpo_j P[0:7, 0:n_old]; the new columns are their transpose) and "corner"
    [6 count, 6 count] (block (j, i) = Jpo_j P77 Jpo_i', + Jhr_j N Jhr_j' where i == j and nowhere else)."""
    pre = add_prepare(x13, cam, uv)
    P = _ld(P)
    n_old = P.shape[0]
    count = len(pre["theta"][0])
    x = _ld(x13)
    fp, fp_tol = np.zeros((count, 6), LD), np.zeros((count, 6), LD)
    fp[:, 0:3] = x[0:3]
    fp[:, 3], fp_tol[:, 3] = pre["theta"]
    fp[:, 4], fp_tol[:, 4] = pre["phi"]
    fp[:, 5] = LD(par.initInvDepthRho)
    J, Jerr = pre["Jpo"]
    Jabs = np.abs(J)
    top = P[0:7, :]
    rows = J @ top
    rows_tol = u_store * np.abs(rows) + U64 * ((Jerr + 8 * Jabs) @ np.abs(top))
    rows_tol[:, EXACT_ROWS, :] = 0
    # corner: W_j = Jpo_j C (fp64, 7 terms), block = W_j Jpo_i' (7 terms)
    C = P[0:7, 0:7]
    W = J @ C
    Wabs = Jabs @ np.abs(C)
    EW = (Jerr + 7 * Jabs) @ np.abs(C)
    blk = np.einsum("jak,ibk->jaib", W, J)
    blk_abs = np.einsum("jak,ibk->jaib", Wabs, Jabs)
    blk_err = np.einsum("jak,ibk->jaib", EW, Jabs) + np.einsum("jak,ibk->jaib", Wabs, Jerr + 7 * Jabs)
    H, Herr = pre["Jhr"]
    N = np.array([LD(cam.pixelErrorX) ** 2, LD(cam.pixelErrorY) ** 2, LD(par.inverseDepthRhoSD) ** 2], LD)
    noise = np.einsum("jak,k,jbk->jab", H, N, H)
    noise_abs = np.einsum("jak,k,jbk->jab", np.abs(H), N, np.abs(H))
    noise_err = (np.einsum("jak,k,jbk->jab", Herr, N, np.abs(H)) + np.einsum("jak,k,jbk->jab", np.abs(H), N, Herr) + 6 * noise_abs)
    for j in range(count):
        blk[j, :, j, :] += noise[j]
        blk_abs[j, :, j, :] += noise_abs[j]
        blk_err[j, :, j, :] += noise_err[j]
    blk_err = blk_err + 3 * blk_abs
    m = 6 * count
    corner = blk.reshape(m, m)
    tol = (u_store * np.abs(blk) + U64 * blk_err)
    ex = np.zeros(6, bool)
    ex[list(EXACT_ROWS)] = True
    exact = ex[None, :, None, None] & ex[None, None, None, :]  # both rows copies (or zero): C[a][b], N[2] or 0, exactly
    tol = np.where(exact, u_store * np.abs(blk), tol)  # (C[a][b] is a stored value already; N[2] is rounded to T)
    tol[:, :3, :, :3] = 0
    tol = tol.reshape(m, m)
    # the device computes block (j, i) for i < j, the upper triangle of block (j, j), and mirrors: the mirrored entry carries the
    # bound of the path that computed it
    jj = np.arange(m) // 6
    computed = (jj[None, :] < jj[:, None]) | ((jj[None, :] == jj[:, None]) & (np.arange(m)[None, :] >= np.arange(m)[:, None]))
    tol = np.where(computed, tol, tol.T)
    return {"feature_pos": (fp, fp_tol), "rows": (rows, rows_tol), "corner": (corner, tol), "g": pre["g"]}


def add_pixels(count, salt=0):
    """`count` distinct pixels 20 px or more inside the 640 x 480 frame"""
    i = np.arange(count)
    return np.stack([20.0 + 600.0 * _hash01(i, 31 + salt), 20.0 + 440.0 * _hash01(i, 32 + salt)], -1)


# ------------------------------------------------------------------------------------------------ remove
def compact_index(types, covpos, drop):
    """feature types and covariance positions, drop = ascending feature indices -> (new2old [n_new] row map, new types, new covpos)"""
    types, covpos = np.asarray(types), np.asarray(covpos)
    dropf = np.zeros(len(types), bool)
    dropf[np.asarray(drop, dtype=np.int64)] = True
    new2old, nt, nc, pos = list(range(13)), [], [], 13
    for f in range(len(types)):
        if dropf[f]:
            continue
        d = dim(types[f])
        new2old += list(range(int(covpos[f]), int(covpos[f]) + d))
        nt.append(int(types[f]))
        nc.append(pos)
        pos += d
    return np.array(new2old, dtype=np.int64), np.array(nt, dtype=np.int32), np.array(nc, dtype=np.int32)


def layout(types):
    types = np.asarray(types)
    d = np.array([dim(t) for t in types], dtype=np.int64)
    covpos = 13 + np.concatenate([[0], np.cumsum(d)[:-1]]) if len(d) else np.zeros(0, np.int64)
    return covpos.astype(np.int32), 13 + int(d.sum())


def drop_set(types, kind):
    """the drop sets of the removal tests on a map of these types (ascending feature indices)"""
    N = len(types)
    if kind == "all":
        return np.arange(N)
    if kind == "first":
        return np.array([0])
    if kind == "last":
        return np.array([N - 1])
    if kind == "every other":
        return np.arange(0, N, 2)
    assert kind == "straddle"
    return None  # sized by remove_case


_REMOVE = {}


def remove_case(n_new, kind):
    """(types of the start map, drop set): the smallest start size in 300 < n0 <= 650 from which `kind` leaves n_new columns.
    "straddle": a run of consecutive features that begins at the last feature starting at or before column 250 and so contains
    columns 255 and 256; "every other": features 0, 2, 4, ... up to the index at which the size is met"""
    key = (n_new, kind)
    if key in _REMOVE:
        return _REMOVE[key]
    for n0 in range(301, 651, 3):
        if n0 <= n_new and kind != "all":
            continue
        types = types_for_n(n0)
        covpos, n = layout(types)
        d = np.array([dim(t) for t in types])
        if kind == "straddle":
            f0 = int(np.nonzero(covpos <= 250)[0][-1])
            cands = [np.arange(f0, f1 + 1) for f1 in range(f0 + 1, len(types))]
        elif kind == "every other":
            cands = [np.arange(0, L, 2) for L in range(3, len(types) + 1)]
        else:
            cands = [drop_set(types, kind)]
        for drop in cands:
            if n0 - int(d[drop].sum()) == n_new and (kind != "straddle" or covpos[drop[-1]] + d[drop[-1]] > 257):
                _REMOVE[key] = (types, drop)
                return _REMOVE[key]
    raise AssertionError(("no start map for", n_new, kind))


# ------------------------------------------------------------------------------------------------ convert
def linearity_ref(x13, feature_pos, types, covpos, P):
    """computeLinearityIndex (EKF/MapManagement.cpp:312-341) of every feature -> (L [N], tol [N]); XYZ features: +inf, tol 0"""
    x = _ld(x13)
    fp = _ld(feature_pos).reshape(-1, 6)
    types, covpos = np.asarray(types), np.asarray(covpos, dtype=np.int64)
    L, tol = np.full(len(types), np.inf, LD), np.zeros(len(types), LD)
    inv = np.nonzero(types == FEATURE_INVERSE_DEPTH)[0]
    if len(inv) == 0:
        return L, tol
    p = [V(fp[inv, k]) for k in range(6)]
    var = V(_ld(np.asarray(P)[covpos[inv] + 5, covpos[inv] + 5]))
    inv_err = var.sqrt()                                     # 2
    sigma = inv_err / (p[5] * p[5])                          # 2 + 1 + 1 = 4
    cp = _trig(np.cos, fp[inv, 4])
    m = [cp * _trig(np.sin, fp[inv, 3]), -_trig(np.sin, fp[inv, 4]), cp * _trig(np.cos, fp[inv, 3])]  # 9, 4, 9
    xyz = [p[k] + m[k] / p[5] for k in range(3)]             # 11
    tc = [xyz[k] - V(x[k]) for k in range(3)]                # 12
    tf = [xyz[k] - p[k] for k in range(3)]                   # 12
    dot = _dot(tc, tf)                                       # 25, + 2 = 27
    df = _dot(tf, tf).sqrt()                                 # 27 -> 16
    dc = _dot(tc, tc).sqrt()                                 # 16
    out = V.of(4.0) * sigma * (dot / (df * dc)) / dc         # 84
    got = {"sigma": sigma.k, "m": m[0].k, "xyz": xyz[0].k, "tc": tc[0].k, "dot": dot.k, "df": df.k, "L": out.k}
    assert got == K_LIN, got
    L[inv], tol[inv] = out.v, U64 * out.k * out.a
    return L, tol


def convert_prepare(p6):
    """k_convert_prepare for one feature -> X (V x 3), J [3, 6] and its err (units of u64)"""
    p = _ld(p6)
    th, ph, rho = p[3], p[4], V(p[5])
    ct, st, cp, sp = _trig(np.cos, th), _trig(np.sin, th), _trig(np.cos, ph), _trig(np.sin, ph)
    mi = [cp * st, -sp, cp * ct]
    X = [V(p[k]) + mi[k] / rho for k in range(3)]
    e = {(0, 3): cp * ct / rho, (2, 3): -(cp * st) / rho,
         (0, 4): -(sp * st) / rho, (1, 4): -cp / rho, (2, 4): -(sp * ct) / rho,
         (0, 5): -mi[0] / (rho * rho), (1, 5): -mi[1] / (rho * rho), (2, 5): -mi[2] / (rho * rho)}
    J, Jerr = np.zeros((3, 6), LD), np.zeros((3, 6), LD)
    for i in range(3):
        J[i, i] = 1
    for (a, k), v in e.items():
        J[a, k], Jerr[a, k] = v.v, v.err
    got = {"m": mi[0].k, "X": X[0].k, "J3": e[0, 3].k, "J14": e[1, 4].k, "J5": e[0, 5].k}
    assert got == K_CONV, got
    return X, J, Jerr


def convert_ref(x13, feature_pos, types, covpos, P, fi, u_store=0.0):
    """feature_pos and P [n, n] as stored before the conversion of inverse-depth feature fi (covariance position pos) -> dict:
    "xyz" (ref, tol) [3]; "rows" (ref, tol) [3, n]: J P[pos:pos+6, :] over the OLD columns (the feature's own six columns hold
    nothing that survives: the 3 x 3 block replaces them); "block" (ref, tol) [3, 3] = J P_blk J'; "old_of_new" [n - 3]: the old
    index of every new row / column (the three new rows are pos .. pos + 2); "linearity" (L, tol) of every feature before it"""
    P = _ld(P)
    n = P.shape[0]
    pos = int(np.asarray(covpos)[fi])
    X, J, Jerr = convert_prepare(np.asarray(feature_pos, dtype=np.float64).reshape(-1, 6)[fi])
    Jabs = np.abs(J)
    six = P[pos:pos + 6, :]
    T3 = J @ six
    T3abs = Jabs @ np.abs(six)
    ET3 = (Jerr + 6 * Jabs) @ np.abs(six)  # T3 as the device holds it (fp64)
    rows_tol = u_store * np.abs(T3) + U64 * (ET3 + T3abs)  # + the rounding to T
    blk = T3[:, pos:pos + 6] @ J.T
    blk_err = ET3[:, pos:pos + 6] @ Jabs.T + T3abs[:, pos:pos + 6] @ (Jerr + 6 * Jabs).T + T3abs[:, pos:pos + 6] @ Jabs.T
    blk_tol = u_store * np.abs(blk) + U64 * blk_err
    blk_tol = np.where(np.arange(3)[None, :] >= np.arange(3)[:, None], blk_tol, blk_tol.T)  # b >= a computed, the rest mirrored
    old_of_new = np.concatenate([np.arange(pos + 3), np.arange(pos + 6, n)])
    xyz = np.array([Xk.v for Xk in X], LD)
    xyz_tol = np.array([U64 * Xk.err for Xk in X], LD)
    return {"xyz": (xyz, xyz_tol), "rows": (T3, rows_tol), "block": (blk, blk_tol), "old_of_new": old_of_new, "pos": pos,
            "linearity": linearity_ref(x13, feature_pos, types, covpos, P)}


def check_converted(report, n, P0, P, fp_after, ref, fi, fp_before):
    """the state after a conversion (P [n - 3, n - 3], feature_pos) against convert_ref, per entry; report(what, n, got, ref, tol) ->
    (worst ratio, where).  Shared by the oracle and the device tests."""
    pos, o2n = ref["pos"], ref["old_of_new"]
    assert P.shape == (n - 3, n - 3)
    bad = []
    other = np.ones(n - 3, bool)
    other[pos:pos + 3] = False
    rows_ref, rows_tol = ref["rows"]
    for name, got, want, tol in (("xyz", fp_after[fi, 0:3], *ref["xyz"]),
                                 ("conv rows", P[pos:pos + 3][:, other], rows_ref[:, o2n[other]], rows_tol[:, o2n[other]]),
                                 ("conv columns", P[:, pos:pos + 3][other].T, rows_ref[:, o2n[other]], rows_tol[:, o2n[other]]),
                                 ("block", P[pos:pos + 3, pos:pos + 3], *ref["block"])):
        r, at = report(name, n, got, want, tol)
        if not (r <= 1.0):
            bad.append((name, r, at))
    assert not bad, bad
    assert (fp_after[fi, 3:6] == 0).all()
    keep = np.arange(len(fp_before)) != fi
    np.testing.assert_array_equal(fp_after[keep], np.asarray(fp_before)[keep])
    np.testing.assert_array_equal(P[np.ix_(other, other)], np.asarray(P0)[np.ix_(o2n[other], o2n[other])])  # moved, bit for bit


def convert_types(n, pos):
    """(pos - 13) / 3 XYZ features, then the first inverse-depth feature at covariance position pos, then inverse-depth and XYZ
    features in turn up to n columns"""
    assert (pos - 13) % 3 == 0 and (n - pos - 6) % 3 == 0 and n >= pos + 6
    t = [FEATURE_DEPTH] * ((pos - 13) // 3) + [FEATURE_INVERSE_DEPTH]
    left, k = n - pos - 6, 0
    while left > 0:
        if k % 2 == 0 and left >= 6:
            t.append(FEATURE_INVERSE_DEPTH)
            left -= 6
        else:
            t.append(FEATURE_DEPTH)
            left -= 3
        k += 1
    return np.array(t, dtype=np.int32)


_SCENES = {}


def convert_scene(n, pos):
    key = ("convert", n, pos)
    if key not in _SCENES:
        _SCENES[key] = make_scene(convert_types(n, pos))
    return _SCENES[key]


def convert_params():
    """every call converts the first inverse-depth feature of the map"""
    par = s3_params()
    par.inverseDepthLinearityIndexThreshold = 1e9
    return par


# ------------------------------------------------------------------------------------------------ selection (k_linearity)
SELECT_INVERSE = (0, 100, 254, 255, 256, 299)  # the inverse-depth features of a selection scene (those below N, and N - 1)


def select_scene(N, fstar):
    """N features, XYZ but for SELECT_INVERSE and N - 1 -> (scene, P, threshold): P = the scene's P0 with the rho row and column
    of f* scaled so that its linearity index is 1/16 of the smallest of the others, threshold = 1/4 of that smallest one (a factor
    4 above f*, a factor 4 or more below every other feature; tests/test_map_ref_cpu.py asserts a factor 2).  fstar None: P0 as it
    is, no feature below the threshold."""
    key = ("select", N, fstar)
    if key in _SCENES:
        return _SCENES[key]
    types = np.full(N, FEATURE_DEPTH, dtype=np.int32)
    for f in SELECT_INVERSE + (N - 1,):
        if f < N:
            types[f] = FEATURE_INVERSE_DEPTH
    s = make_scene(types)
    P = s.P0.copy()
    L0 = linearity_ref(s.x13, s.feature_pos, s.feature_type, s.covpos, P)[0]
    inv = np.nonzero(types == FEATURE_INVERSE_DEPTH)[0]
    if fstar is None:
        thr = float(L0[inv].min()) / 4.0
    else:
        assert types[fstar] == FEATURE_INVERSE_DEPTH
        lmin = float(min(L0[f] for f in inv if f != fstar))
        thr = lmin / 4.0
        scale = (lmin / 16.0) / float(L0[fstar])  # L is proportional to sqrt(P[rho][rho])
        r = int(s.covpos[fstar]) + 5
        P[r, :] *= scale
        P[:, r] *= scale
    _SCENES[key] = (s, P, thr)
    return _SCENES[key]
