// kernels_map.hip -- map management on the device, i.e. the part of EKF::step that changes the
// state dimension between frames (EKF/EKF.cpp:574-612):
//   addFeaturesToStateAndCovariance   EKF/AddMapFeature.cpp:221-359   -> k_addfeat_prepare / _rows / _corner
//   removeFeaturesFromStateAndCovariance EKF/MapManagement.cpp:212-259 -> k_compact_P (+ host-side SoA compaction)
//   computeLinearityIndex / convertToDepth EKF/MapManagement.cpp:312-490 -> k_linearity, k_convert_*
// and the read-only export of the map as 3-D points with covariances (k_map_points; no counterpart in the reference).
// The reference re-allocates and copies all of P for every added feature (O(n^2) each); here P lives in a
// capacity-strided buffer, an append is two 6 x n strip products per feature (all new features in one launch),
// a removal is one gather pass into a second buffer.  All strip kernels are HBM/latency-bound.
#include "engine.h"

namespace ekf {

// ---------------------------------------------------------------------------------------------- add features
// One thread per new feature: initial 6-vector, d f/d (r, q) (6x7) and d f/d (h, rho) (6x3).
// EKF/AddMapFeature.cpp:42-58 (undistort), :65-90, :109-216, :293-344.
__global__ void __launch_bounds__(64)
k_addfeat_prepare(const double *st, CamD c, double rho0, const double *uv, int count, int N_old, int n_old,
                  double *feat_pos, int *feat_type, int *feat_covpos, double *Jpo, double *Jhr)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const double *x = st + ST_X, *R = st + ST_R, *q = x + 3;
    const double ud = uv[2 * j], vd = uv[2 * j + 1];
    // undistortPoint
    const double mx = ud - c.cx, my = vd - c.cy;
    const double dxm = c.dx * mx, dym = c.dy * my;
    const double rd2 = dxm * dxm + dym * dym;
    const double dist = 1 + c.k1 * rd2 + c.k2 * rd2 * rd2;
    const double uu = c.cx + mx * dist, vu = c.cy + my * dist;
    const double xyz_c[3] = {-(c.cx - uu) / c.fx, -(c.cy - vu) / c.fy, 1.0};
    double g[3];
    mat3_vec(R, xyz_c, g);
    double *fp = feat_pos + 6 * (size_t)(N_old + j);
    fp[0] = x[0]; fp[1] = x[1]; fp[2] = x[2];
    fp[3] = atan2(g[0], g[2]);
    fp[4] = atan2(-g[1], sqrt(g[0] * g[0] + g[2] * g[2]));
    fp[5] = rho0;
    feat_type[N_old + j] = EKF_FEATURE_INVERSE_DEPTH;
    feat_covpos[N_old + j] = n_old + 6 * j;
    // Jacobians
    const double xw = g[0], yw = g[1], zw = g[2];
    const double xxzz = xw * xw + zw * zw, sq = sqrt(xxzz), nsq = xxzz + yw * yw;
    const double dth[3] = {zw / xxzz, 0.0, -xw / xxzz};
    const double dph[3] = {xw * yw / (nsq * sq), -sq / nsq, zw * yw / (nsq * sq)};
    double dg[12];
    jac_rot_by_quat(q, xyz_c, dg);
    double *J = Jpo + 42 * (size_t)j;
    for (int i = 0; i < 42; ++i) J[i] = 0.0;
    J[0] = J[8] = J[16] = 1.0;
    for (int i = 0; i < 4; ++i) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            s1 += dth[k] * dg[k * 4 + i];
            s2 += dph[k] * dg[k * 4 + i];
        }
        J[3 * 7 + 3 + i] = s1;
        J[4 * 7 + 3 + i] = s2;
    }
    double sub[6]; // [dtheta; dphi] * R
    for (int i = 0; i < 3; ++i) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            s1 += dth[k] * R[k * 3 + i];
            s2 += dph[k] * R[k * 3 + i];
        }
        sub[i] = s1;
        sub[3 + i] = s2;
    }
    const double s2m[4] = {sub[0] / c.fx, sub[1] / c.fy, sub[3] / c.fx, sub[4] / c.fy}; // * dgc_dhu
    // computeUndistortPointJacobian :65-90
    const double a = c.k1 + 2.0 * c.k2 * rd2, b = 1.0 + c.k1 * rd2 + c.k2 * rd2 * rd2;
    const double dx2 = 2.0 * c.dx * c.dx, dy2 = 2.0 * c.dy * c.dy;
    const double dh[4] = {b + mx * a * (mx * dx2), mx * a * (my * dy2), my * a * (mx * dx2), my * a * (my * dy2) + b};
    double *H = Jhr + 18 * (size_t)j;
    for (int i = 0; i < 18; ++i) H[i] = 0.0;
    H[9] = s2m[0] * dh[0] + s2m[1] * dh[2];
    H[10] = s2m[0] * dh[1] + s2m[1] * dh[3];
    H[12] = s2m[2] * dh[0] + s2m[3] * dh[2];
    H[13] = s2m[2] * dh[1] + s2m[3] * dh[3];
    H[17] = 1.0;
}

// New rows  P[n_old + 6j + a, c] = sum_k Jpo_j[a][k] P[k][c]  for the old columns c < n_old (:272), mirrored into the
// new columns (:273; P[0:n_old, 0:7] Jpo' is the transpose of the same products because P is symmetric).
template <typename T>
__global__ void __launch_bounds__(256) k_addfeat_rows(T *P, int ld, int n_old, const double *Jpo)
{
    __shared__ double sJ[42];
    const int j = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 42) sJ[threadIdx.x] = Jpo[42 * (size_t)j + threadIdx.x];
    __syncthreads();
    if (c >= n_old) return;
    double p[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = (double)P[(size_t)k * ld + c];
    const int r0 = n_old + 6 * j;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) s += sJ[a * 7 + k] * p[k];
        P[(size_t)(r0 + a) * ld + c] = (T)s;
        P[(size_t)c * ld + r0 + a] = (T)s;
    }
}

// New x new blocks (j, i), i <= j:  Jpo_j P77 Jpo_i'  (+ Jhr N Jhr' on the diagonal, :279-281), upper + mirror.
template <typename T>
__global__ void __launch_bounds__(64)
k_addfeat_corner(T *P, int ld, int n_old, int count, const double *Jpo, const double *Jhr, double nx, double ny, double nr)
{
    const int j = blockIdx.x, i = blockIdx.y;
    if (i > j) return;
    __shared__ double C[49], W[42]; // P77, Jpo_j * P77 (6x7)
    const int t = threadIdx.x;
    if (t < 49) C[t] = (double)P[(size_t)(t / 7) * ld + t % 7];
    __syncthreads();
    const double *Jj = Jpo + 42 * (size_t)j, *Ji = Jpo + 42 * (size_t)i;
    if (t < 42) {
        const int a = t / 7, k = t % 7;
        double s = 0.0;
        for (int l = 0; l < 7; ++l) s += Jj[a * 7 + l] * C[l * 7 + k];
        W[t] = s;
    }
    __syncthreads();
    if (t < 36) {
        const int a = t / 6, b = t % 6;
        if (i == j && b < a) return;
        double s = 0.0;
        for (int k = 0; k < 7; ++k) s += W[a * 7 + k] * Ji[b * 7 + k];
        if (i == j) {
            const double *H = Jhr + 18 * (size_t)j;
            s += H[a * 3 + 0] * nx * H[b * 3 + 0] + H[a * 3 + 1] * ny * H[b * 3 + 1] + H[a * 3 + 2] * nr * H[b * 3 + 2];
        }
        const int r = n_old + 6 * j + a, cc = n_old + 6 * i + b;
        P[(size_t)r * ld + cc] = (T)s;
        P[(size_t)cc * ld + r] = (T)s;
    }
}

// ------------------------------------------------------------------------------------------ compaction of P
// P2[i][j] = P[new2old[i]][new2old[j]]  (removeRowsAndColumnsFromMat, EKF/MapManagement.cpp:168-208)
template <typename T>
__global__ void __launch_bounds__(256) k_compact_P(const T *P, T *P2, int ld, int n_new, const int *new2old)
{
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_new) return;
    P2[(size_t)i * ld + j] = P[(size_t)new2old[i] * ld + new2old[j]];
}

// -------------------------------------------------------------------------------- inverse depth -> depth
// computeLinearityIndex, EKF/MapManagement.cpp:312-341 for one inverse-depth feature: p = its six parameters, r = camera
// position, var_rho = the feature's P[rho][rho].  The one copy of the formula (k_linearity, k_map_points).
__device__ __forceinline__ double linearity_index(const double *p, const double *x, double var_rho)
{
    const double inv_err = sqrt(var_rho);
    const double sigma = inv_err / (p[5] * p[5]);
    double m[3];
    dir_vec(p[3], p[4], m);
    const double xyz[3] = {p[0] + m[0] / p[5], p[1] + m[1] / p[5], p[2] + m[2] / p[5]};
    const double tc[3] = {xyz[0] - x[0], xyz[1] - x[1], xyz[2] - x[2]};
    const double tf[3] = {xyz[0] - p[0], xyz[1] - p[1], xyz[2] - p[2]};
    double dot = 0.0;
    for (int k = 0; k < 3; ++k) dot += tc[k] * tf[k];
    const double df = sqrt(tf[0] * tf[0] + tf[1] * tf[1] + tf[2] * tf[2]);
    const double dc = sqrt(tc[0] * tc[0] + tc[1] * tc[1] + tc[2] * tc[2]);
    return 4.0 * sigma * (dot / (df * dc)) / dc;
}

// one thread per feature; depth features get +inf
template <typename T>
__global__ void __launch_bounds__(256)
k_linearity(const double *st, const double *feat_pos, const int *feat_type, const int *feat_covpos, int N, const T *P, int ld,
            double *out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= N) return;
    if (feat_type[f] != EKF_FEATURE_INVERSE_DEPTH) {
        out[f] = 1e300;
        return;
    }
    const double *p = feat_pos + 6 * (size_t)f;
    const int ii = feat_covpos[f] + 5;
    out[f] = linearity_index(p, st + ST_X, (double)P[(size_t)ii * ld + ii]);
}

// d X / d (x0 y0 z0 theta phi rho) of X = (x0 y0 z0) + m(theta, phi) / rho, 3x6 row-major (EKF/MapManagement.cpp:343-392);
// mi = m(theta, phi).  The one copy of the formula (k_convert_prepare, k_map_points).
__device__ __forceinline__ void inverse_depth_to_xyz_jacobian(double theta, double phi, double rho, const double *mi, double *J)
{
    for (int i = 0; i < 18; ++i) J[i] = 0.0;
    J[0] = J[7] = J[14] = 1.0;
    J[0 * 6 + 3] = cos(phi) * cos(theta) / rho;  J[2 * 6 + 3] = -cos(phi) * sin(theta) / rho;
    J[0 * 6 + 4] = -sin(phi) * sin(theta) / rho; J[1 * 6 + 4] = -cos(phi) / rho; J[2 * 6 + 4] = -sin(phi) * cos(theta) / rho;
    J[0 * 6 + 5] = -mi[0] / (rho * rho); J[1 * 6 + 5] = -mi[1] / (rho * rho); J[2 * 6 + 5] = -mi[2] / (rho * rho);
}

// convertToDepth, EKF/MapManagement.cpp:343-392: XYZ position and the 3x6 Jacobian; one thread.
__global__ void k_convert_prepare(double *feat_pos, int *feat_type, int fi, double *J)
{
    if (threadIdx.x != 0) return;
    double *p = feat_pos + 6 * (size_t)fi;
    const double theta = p[3], phi = p[4], rho = p[5];
    double mi[3];
    dir_vec(theta, phi, mi);
    inverse_depth_to_xyz_jacobian(theta, phi, rho, mi, J);
    p[0] += mi[0] / rho; p[1] += mi[1] / rho; p[2] += mi[2] / rho;
    p[3] = p[4] = p[5] = 0.0;
    feat_type[fi] = EKF_FEATURE_DEPTH;
}

// T3[a][c] = sum_k J[a][k] P[pos+k][c]   (subResult_3xn, :436)
template <typename T>
__global__ void __launch_bounds__(256) k_convert_rows(const T *P, int ld, int n, int pos, const double *J, double *T3)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = (double)P[(size_t)(pos + k) * ld + c];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += J[a * 6 + k] * p[k];
        T3[(size_t)a * ld + c] = s;
    }
}

// rows/columns pos..pos+2 <- T3 (columns outside the feature's own block; :441-451), 3x3 block <- T3[:,blk] J' (:439)
template <typename T>
__global__ void __launch_bounds__(256) k_convert_apply(T *P, int ld, int n, int pos, const double *J, const double *T3)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    if (c >= pos && c < pos + 6) {
        if (c < pos + 3) {
            const int a = c - pos;
            for (int b = a; b < 3; ++b) {
                double s = 0.0;
                for (int k = 0; k < 6; ++k) s += T3[(size_t)a * ld + pos + k] * J[b * 6 + k];
                P[(size_t)(pos + a) * ld + pos + b] = (T)s;
                P[(size_t)(pos + b) * ld + pos + a] = (T)s;
            }
        }
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T v = (T)T3[(size_t)a * ld + c];
        P[(size_t)(pos + a) * ld + c] = v;
        P[(size_t)c * ld + pos + a] = v;
    }
}

// ---------------------------------------------------------------- every linear feature at once
// k_convert_prepare for the count features listed in sel (ascending): J of the k-th one to J + 18 k; one thread per feature.
__global__ void __launch_bounds__(64) k_convert_all_prepare(double *feat_pos, int *feat_type, const int *sel, int count, double *J)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= count) return;
    const int fi = sel[k];
    double *p = feat_pos + 6 * (size_t)fi;
    const double theta = p[3], phi = p[4], rho = p[5];
    double mi[3];
    dir_vec(theta, phi, mi);
    inverse_depth_to_xyz_jacobian(theta, phi, rho, mi, J + 18 * (size_t)k);
    p[0] += mi[0] / rho; p[1] += mi[1] / rho; p[2] += mi[2] / rho;
    p[3] = p[4] = p[5] = 0.0;
    feat_type[fi] = EKF_FEATURE_DEPTH;
}

// P2 = R P R', R block diagonal: 1 for a kept row, the 3 x 6 Jacobian of every converted feature.  rows[2 u], rows[2 u + 1]: the
// first source row s(u) of new row u and its row of Jtab (6 weights over rows s(u) .. s(u) + 5), or -1 for a kept row (weight 1).
// One workgroup per 64 x 64 tile (ty, tx), tx >= ty, of the new matrix, and its mirror image:
//   1. CA_ROWS new rows at a time, T[u][c] = sum_a w_u[a] P[s(u) + a][c] over the old columns c the tile's columns read (at most
//      CA_CW of them: 64 new columns touch at most 22 converted features), consecutive threads along c, into LDS as doubles;
//   2. P'[u][v] = sum_b T[u][s(v) + b] w_v[b] (T[u][s(v)] for a kept column), lane = column, rounded to T once, stored along the
//      row where u <= v and kept in LDS;
//   3. the mirror image (tile (tx, ty); in the diagonal tile the entries below the diagonal) is stored along ITS rows: a kept x
//      kept entry is moved from P[s(v)][s(u)], every other entry is the LDS copy of its twin.
// Kept x kept entries pass through a double and back, which is the identity for a float and for a double.  Only the upper
// triangle of P and the diagonal blocks of the converted features reach a computed entry that is stored.  All arithmetic is fp64.
constexpr int CA_ROWS = 16, CA_BATCH = 4, CA_LDT = CA_CW + 1, CA_LDO = CA_TILE + 1; // (CA_TILE, CA_CW: engine.h)

template <typename T>
__global__ void __launch_bounds__(256)
k_convert_all_P(const T *__restrict__ P, T *__restrict__ P2, int ld, int n_new, const int *__restrict__ rows, const double *__restrict__ Jtab)
{
    const int ty = blockIdx.y, tx = blockIdx.x;
    if (tx < ty) return; // (the whole workgroup: no barrier is skipped)
    __shared__ double sT[CA_ROWS * CA_LDT];
    __shared__ T sO[CA_TILE * CA_LDO];
    __shared__ int sS[2][CA_TILE], sJ[2][CA_TILE]; // s(.) and the Jtab row of the tile's rows [0] and columns [1]
    __shared__ double sW[CA_TILE][6];              // the weights of the tile's converted rows
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int u0 = ty * CA_TILE, v0 = tx * CA_TILE;
    if (t < 2 * CA_TILE) {
        const int g = (w ? v0 : u0) + lane;
        sS[w][lane] = g < n_new ? rows[2 * g] : 0;
        sJ[w][lane] = g < n_new ? rows[2 * g + 1] : -1;
    }
    __syncthreads();
    for (int i = t; i < CA_TILE * 6; i += 256)
        sW[i / 6][i % 6] = sJ[0][i / 6] >= 0 ? Jtab[6 * (size_t)sJ[0][i / 6] + i % 6] : 0.0;
    __syncthreads();
    const int vl = min(CA_TILE, n_new - v0) - 1; // the tile's last live column
    const int c0 = sS[1][0], cw = sS[1][vl] + (sJ[1][vl] >= 0 ? 6 : 1) - c0; // the old columns c0 .. c0 + cw - 1; cw <= CA_CW
    const int v = v0 + lane, cs = sS[1][lane] - c0, jv = sJ[1][lane];
    double wv[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) wv[b] = jv >= 0 ? Jtab[6 * (size_t)jv + b] : 0.0;
    for (int h = 0; h < CA_TILE; h += CA_ROWS) {
        // entry e = r cw + cc of the strip to thread e mod 256: CA_BATCH entries per thread with all their loads issued before the
        // first sum (each entry alone would leave one DRAM latency per six loads exposed)
        const int total = min(CA_ROWS, n_new - u0 - h) * cw; // (<= 0 behind the last row)
        for (int e0 = t; e0 < total; e0 += 256 * CA_BATCH) {
            T pv[CA_BATCH][6];
            int at[CA_BATCH], row[CA_BATCH];
#pragma unroll
            for (int k = 0; k < CA_BATCH; ++k) {
                const int e = e0 + 256 * k;
                row[k] = -1;
                if (e >= total) continue;
                const int r = e / cw, cc = e - r * cw;
                row[k] = h + r;
                at[k] = r * CA_LDT + cc;
                const T *p = P + (size_t)sS[0][h + r] * ld + c0 + cc;
                pv[k][0] = p[0];
                if (sJ[0][h + r] >= 0) {
#pragma unroll
                    for (int a = 1; a < 6; ++a) pv[k][a] = p[(size_t)a * ld];
                }
            }
#pragma unroll
            for (int k = 0; k < CA_BATCH; ++k) {
                if (row[k] < 0) continue;
                double s;
                if (sJ[0][row[k]] < 0) {
                    s = (double)pv[k][0];
                } else {
                    s = 0.0;
#pragma unroll
                    for (int a = 0; a < 6; ++a) s += sW[row[k]][a] * (double)pv[k][a];
                }
                sT[at[k]] = s;
            }
        }
        __syncthreads();
        for (int r = w; r < CA_ROWS; r += 4) {
            const int u = u0 + h + r;
            if (u >= n_new || v >= n_new) break;
            const double *tr = sT + r * CA_LDT + cs;
            double s;
            if (jv < 0) {
                s = tr[0];
            } else {
                s = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) s += tr[b] * wv[b];
            }
            const T o = (T)s;
            sO[(h + r) * CA_LDO + lane] = o;
            if (u <= v) P2[(size_t)u * ld + v] = o;
        }
        __syncthreads();
    }
    const int c2 = u0 + lane; // the mirror image: row v0 + i, lanes along its columns
    for (int i = w; i < CA_TILE; i += 4) {
        const int r2 = v0 + i;
        if (r2 >= n_new) break;
        if (c2 >= n_new || r2 <= c2) continue; // (r2 <= c2 only in the diagonal tile)
        const bool moved = sJ[1][i] < 0 && sJ[0][lane] < 0;
        P2[(size_t)r2 * ld + c2] = moved ? P[(size_t)sS[1][i] * ld + sS[0][lane]] : sO[lane * CA_LDO + i];
    }
}

// ------------------------------------------------------------------------------------ map export (read-only)
// ekf_get_map_points: every feature as a world point X with its 3x3 covariance, the same point in the camera's axes with
// a covariance that includes the pose uncertainty, and the linearity index.  z = (r, q, y) with y the feature's d = 6 or
// 3 parameters, Z = P on rows/columns {0..6} u {pos..pos+d-1}:
//     cov     = Jw P[pos.., pos..] Jw'         Jw = d X / d y (3 x d; identity for a depth feature)
//     cov_cam = Jc Z Jc'                       Jc = [ -R' | d(R(q)' a)/dq at a = X - r | R' Jw ]  (3 x (7 + d))
// One 64-lane wavefront per feature, MP_WAVES per workgroup.  The lanes gather Z into LDS as doubles (entry e of the
// D x D matrix to lane e mod 64: runs of 7 and d consecutive columns of one row of P), lane 0 forms X, Jw and Jc, six
// lanes form the upper triangle of each covariance, and 27 lanes store the 216-byte record as 8-byte words.  All
// arithmetic is fp64 whatever T is.  Nothing but out is written.  Latency-bound: <= 1.4 KB read per feature.
constexpr int MP_WAVES = 4, MP_D = 13, MP_WORDS = sizeof(EkfMapPoint) / 8;
static_assert(sizeof(EkfMapPoint) == 216 && MP_WORDS * 8 == sizeof(EkfMapPoint), "EkfMapPoint is 27 packed 8-byte words");

template <typename T>
__global__ void __launch_bounds__(64 * MP_WAVES)
k_map_points(const double *st, const double *feat_pos, const int *feat_type, const int *feat_covpos, const unsigned *times_predicted,
             const unsigned *times_matched, int N, const T *P, int ld, EkfMapPoint *out)
{
    __shared__ double sZ[MP_WAVES][MP_D * MP_D], sJc[MP_WAVES][3 * MP_D], sJw[MP_WAVES][18];
    __shared__ EkfMapPoint sOut[MP_WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * MP_WAVES + w;
    const bool live = f < N; // no early return: the workgroup meets at the barriers below
    const int type = live ? feat_type[f] : EKF_FEATURE_DEPTH, pos = live ? feat_covpos[f] : 0;
    const bool invd = type == EKF_FEATURE_INVERSE_DEPTH;
    const int d = invd ? 6 : 3, D = 7 + d;
    double *Z = sZ[w], *Jc = sJc[w], *Jw = sJw[w];
    EkfMapPoint &o = sOut[w];
    if (live) {
        for (int e = lane; e < D * D; e += 64) {
            const int i = e / D, j = e - i * D;
            const int gi = i < 7 ? i : pos + i - 7, gj = j < 7 ? j : pos + j - 7;
            Z[i * MP_D + j] = (double)P[(size_t)gi * ld + gj];
        }
        if (lane == 0) {
            const double *x = st + ST_X, *y = feat_pos + 6 * (size_t)f;
            double X[3], jw[18], m[3] = {0.0, 0.0, 0.0};
            if (invd) dir_vec(y[3], y[4], m);
            feature_world_point(y, invd, m, X);
            if (invd) {
                inverse_depth_to_xyz_jacobian(y[3], y[4], y[5], m, jw);
            } else {
                for (int i = 0; i < 18; ++i) jw[i] = 0.0;
                jw[0] = jw[7] = jw[14] = 1.0;
            }
            double R[9], dq[12];
            quat_to_rot(x + 3, R);
            const double a[3] = {X[0] - x[0], X[1] - x[1], X[2] - x[2]};
            const double qc[4] = {x[3], -x[4], -x[5], -x[6]}; // R(q)' = R(conj q); chain rule: vector columns negated
            jac_rot_by_quat(qc, a, dq);
            for (int i = 0; i < 3; ++i) {
                o.xyz[i] = X[i];
                o.cam[i] = R[i] * a[0] + R[3 + i] * a[1] + R[6 + i] * a[2];
                for (int k = 0; k < 3; ++k) Jc[i * MP_D + k] = -R[k * 3 + i];
                Jc[i * MP_D + 3] = dq[i * 4];
                for (int k = 1; k < 4; ++k) Jc[i * MP_D + 3 + k] = -dq[i * 4 + k];
                for (int k = 0; k < 6; ++k) {
                    Jw[i * 6 + k] = jw[i * 6 + k];
                    Jc[i * MP_D + 7 + k] = R[i] * jw[k] + R[3 + i] * jw[6 + k] + R[6 + i] * jw[12 + k];
                }
            }
            o.type = type;
            o.covpos = pos;
            o.times_predicted = times_predicted[f];
            o.times_matched = times_matched[f];
        }
    }
    __syncthreads();
    if (live) {
        // lanes 0..5: upper triangle of cov_cam; lanes 8..13: upper triangle of cov; lane 16: linearity
        const int t = lane & 7;
        const int ra = t < 3 ? 0 : (t < 5 ? 1 : 2), rb = t < 3 ? t : (t < 5 ? t - 2 : 2);
        if (lane < 6) {
            double s = 0.0;
            for (int i = 0; i < D; ++i) {
                double u = 0.0;
                for (int j = 0; j < D; ++j) u += Z[i * MP_D + j] * Jc[rb * MP_D + j];
                s += Jc[ra * MP_D + i] * u;
            }
            o.cov_cam[ra * 3 + rb] = s;
            o.cov_cam[rb * 3 + ra] = s;
        } else if (lane >= 8 && lane < 14) {
            double s;
            if (invd) {
                s = 0.0;
                for (int i = 0; i < 6; ++i) {
                    double u = 0.0;
                    for (int j = 0; j < 6; ++j) u += Z[(7 + i) * MP_D + 7 + j] * Jw[rb * 6 + j];
                    s += Jw[ra * 6 + i] * u;
                }
            } else {
                s = Z[(7 + ra) * MP_D + 7 + rb]; // the stored block itself
            }
            o.cov[ra * 3 + rb] = s;
            o.cov[rb * 3 + ra] = s;
        } else if (lane == 16) {
            o.linearity = invd ? linearity_index(feat_pos + 6 * (size_t)f, st + ST_X, Z[12 * MP_D + 12]) : 1e300;
        }
    }
    __syncthreads();
    if (live && lane < MP_WORDS)
        reinterpret_cast<unsigned long long *>(out + f)[lane] = reinterpret_cast<const unsigned long long *>(&o)[lane];
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_add_features(EkfEngine *e, const double *d_uv, int count, double *d_Jpo, double *d_Jhr)
{
    hipStream_t s = e->stream;
    const int n_old = e->n, N_old = e->N;
    k_addfeat_prepare<<<(count + 63) / 64, 64, 0, s>>>(e->d.state, e->cam, e->cfg.par.initInvDepthRho, d_uv, count, N_old, n_old,
                                                       e->d.feat_pos, e->d.feat_type, e->d.feat_covpos, d_Jpo, d_Jhr);
    const double nx = e->cfg.cam.pixelErrorX * e->cfg.cam.pixelErrorX, ny = e->cfg.cam.pixelErrorY * e->cfg.cam.pixelErrorY;
    const double nr = e->cfg.par.inverseDepthRhoSD * e->cfg.par.inverseDepthRhoSD;
    dim3 g1((n_old + 255) / 256, count), g2(count, count);
    if (e->f32) {
        k_addfeat_rows<float><<<g1, 256, 0, s>>>((float *)e->d.P, e->ldP, n_old, d_Jpo);
        k_addfeat_corner<float><<<g2, 64, 0, s>>>((float *)e->d.P, e->ldP, n_old, count, d_Jpo, d_Jhr, nx, ny, nr);
    } else {
        k_addfeat_rows<double><<<g1, 256, 0, s>>>((double *)e->d.P, e->ldP, n_old, d_Jpo);
        k_addfeat_corner<double><<<g2, 64, 0, s>>>((double *)e->d.P, e->ldP, n_old, count, d_Jpo, d_Jhr, nx, ny, nr);
    }
}

void launch_compact_P(EkfEngine *e, int n_new, const int *d_new2old)
{
    if (n_new <= 0) return;
    dim3 g((n_new + 255) / 256, n_new);
    if (e->f32) k_compact_P<float><<<g, 256, 0, e->stream>>>((const float *)e->d.P, (float *)e->d.P2, e->ldP, n_new, d_new2old);
    else k_compact_P<double><<<g, 256, 0, e->stream>>>((const double *)e->d.P, (double *)e->d.P2, e->ldP, n_new, d_new2old);
    void *t = e->d.P;
    e->d.P = e->d.P2;
    e->d.P2 = t;
}

void launch_linearity(EkfEngine *e, double *d_out)
{
    if (e->N <= 0) return;
    const int nb = (e->N + 255) / 256;
    if (e->f32)
        k_linearity<float><<<nb, 256, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos, e->N,
                                                     (const float *)e->d.P, e->ldP, d_out);
    else
        k_linearity<double><<<nb, 256, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos, e->N,
                                                      (const double *)e->d.P, e->ldP, d_out);
}

void launch_convert(EkfEngine *e, int fi, int pos, double *d_J, double *d_T3)
{
    hipStream_t s = e->stream;
    k_convert_prepare<<<1, 64, 0, s>>>(e->d.feat_pos, e->d.feat_type, fi, d_J);
    const int nb = (e->n + 255) / 256;
    if (e->f32) {
        k_convert_rows<float><<<nb, 256, 0, s>>>((const float *)e->d.P, e->ldP, e->n, pos, d_J, d_T3);
        k_convert_apply<float><<<nb, 256, 0, s>>>((float *)e->d.P, e->ldP, e->n, pos, d_J, d_T3);
    } else {
        k_convert_rows<double><<<nb, 256, 0, s>>>((const double *)e->d.P, e->ldP, e->n, pos, d_J, d_T3);
        k_convert_apply<double><<<nb, 256, 0, s>>>((double *)e->d.P, e->ldP, e->n, pos, d_J, d_T3);
    }
}

void launch_convert_all(EkfEngine *e, int count, int n_new)
{
    hipStream_t s = e->stream;
    k_convert_all_prepare<<<(count + 63) / 64, 64, 0, s>>>(e->d.feat_pos, e->d.feat_type, e->d.ca_sel, count, e->d.ca_J);
    const int nt = (n_new + CA_TILE - 1) / CA_TILE;
    dim3 g(nt, nt);
    if (e->f32) k_convert_all_P<float><<<g, 256, 0, s>>>((const float *)e->d.P, (float *)e->d.P2, e->ldP, n_new, e->d.ca_rows, e->d.ca_J);
    else k_convert_all_P<double><<<g, 256, 0, s>>>((const double *)e->d.P, (double *)e->d.P2, e->ldP, n_new, e->d.ca_rows, e->d.ca_J);
    void *t = e->d.P;
    e->d.P = e->d.P2;
    e->d.P2 = t;
}

void launch_map_points(EkfEngine *e, EkfMapPoint *d_out)
{
    if (e->N <= 0) return;
    const int nb = (e->N + MP_WAVES - 1) / MP_WAVES;
    if (e->f32)
        k_map_points<float><<<nb, 64 * MP_WAVES, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos,
                                                                 e->d.feat_times_predicted, e->d.feat_times_matched, e->N,
                                                                 (const float *)e->d.P, e->ldP, d_out);
    else
        k_map_points<double><<<nb, 64 * MP_WAVES, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos,
                                                                  e->d.feat_times_predicted, e->d.feat_times_matched, e->N,
                                                                  (const double *)e->d.P, e->ldP, d_out);
}

// Measurement aid (ekf_round_covariance_to_f32): every stored entry of an fp64 covariance replaced by its nearest fp32 value.
__global__ void __launch_bounds__(256) k_round_P_f32(double *P, int ld, int n, int rows)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (i < rows && j < n) P[(size_t)i * ld + j] = (double)(float)P[(size_t)i * ld + j];
}

void launch_round_P_f32(EkfEngine *e)
{
    const int rows = e->shard_world > 1 ? local_row(e->rm, e->rm.r1 - 1) + 1 : e->n;
    k_round_P_f32<<<dim3((e->n + 255) / 256, rows), 256, 0, e->stream>>>((double *)e->d.P, e->ldP, e->n, rows);
}

} // namespace ekf
