// kernels_reloc.hip -- relocalisation on the map (ekf_relocalise; no counterpart in the reference, which has no way
// back once tracking is lost).  Nothing here looks at the predicted camera pose:
//   k_reloc_match    one workgroup per feature: its world point, whether it takes part, the Hamming distance to EVERY keypoint
//   k_reloc_compact  one workgroup: the candidates in ascending feature order, their bearings and world points, the counts
//   k_reloc_p3p      one wavefront per hypothesis: counter-based triple, P3P on lane 0, every lane scores
//   k_reloc_select   one workgroup: the best hypothesis, the inlier mask, the result; the state and the camera strip of P if asked
// The contract is tests/relocalise_ref.py, step for step; all arithmetic is fp64 whatever the covariance's storage type is.  Every
// loop of the solver has a fixed trip count, and a non-finite intermediate drops its solution.
#include "engine.h"

namespace ekf {

constexpr int RL_NONE = 0x7fffffff; // distance / index of "no keypoint"
constexpr int RL_CUBIC_POLISH = 3, RL_QUARTIC_POLISH = 4;
constexpr double RL_BEARING_TOL = 1e-6;
constexpr double RL_COS_MAX = 1.0 - 1e-12; // two bearings of a triple closer than 1.4e-6 rad count as one: no solution

// ------------------------------------------------------------------------------------------------ global match
struct RlBest {
    int d1, k1, d2; // smallest distance, its keypoint (the lowest index among equals), the smallest distance over the others
};
__device__ __forceinline__ RlBest rl_merge(const RlBest &a, const RlBest &b)
{
    const bool a_first = a.d1 < b.d1 || (a.d1 == b.d1 && a.k1 < b.k1);
    RlBest o;
    o.d1 = a_first ? a.d1 : b.d1;
    o.k1 = a_first ? a.k1 : b.k1;
    o.d2 = a_first ? min(a.d2, b.d1) : min(b.d2, a.d1);
    return o;
}

// feat_flag[f]: 0 = takes no part, 1 = takes part, 2 = candidate (then feat_kp / feat_dist hold its keypoint and distance)
template <typename T>
__global__ void __launch_bounds__(256)
k_reloc_match(const double *feat_pos, const int *feat_type, const int *feat_covpos, const uint8_t *feat_desc, int N, const T *P, int ld,
              const uint8_t *kdesc, int n_kp, const int *d_nkp, double max_distance, double coef, double max_rel_sd, double *X_out,
              int *feat_flag, int *feat_kp, int *feat_dist)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= N) return;
    if (d_nkp) n_kp = min(*d_nkp, n_kp); // keypoints detected on the device: n_kp = the capacity
    const double *y = feat_pos + 6 * (size_t)f;
    const bool invd = feat_type[f] == EKF_FEATURE_INVERSE_DEPTH;
    bool used = true;
    if (invd) { // (the same for every thread: no barrier is skipped by a part of the workgroup)
        const double rho = y[5];
        const int ii = feat_covpos[f] + 5;
        used = rho > 0.0 && (max_rel_sd == 0.0 || sqrt((double)P[(size_t)ii * ld + ii]) / rho <= max_rel_sd);
    }
    if (tid == 0) {
        double m[3] = {0.0, 0.0, 0.0}, X[3];
        if (invd) dir_vec(y[3], y[4], m);
        feature_world_point(y, invd, m, X);
        X_out[3 * (size_t)f] = X[0];
        X_out[3 * (size_t)f + 1] = X[1];
        X_out[3 * (size_t)f + 2] = X[2];
        if (!used) feat_flag[f] = 0;
    }
    if (!used) return;
    uint32_t q[8];
    const uint32_t *qd = (const uint32_t *)(feat_desc + (size_t)f * EKF_DESC_BYTES);
#pragma unroll
    for (int w = 0; w < 8; ++w) q[w] = qd[w];
    RlBest b{RL_NONE, RL_NONE, RL_NONE};
    for (int k = tid; k < n_kp; k += 256) { // ascending per thread: the strict comparisons keep the lower index among equals
        const uint4 *cd = (const uint4 *)(kdesc + (size_t)k * EKF_DESC_BYTES);
        const uint4 c0 = cd[0], c1 = cd[1];
        const int d = __popc(c0.x ^ q[0]) + __popc(c0.y ^ q[1]) + __popc(c0.z ^ q[2]) + __popc(c0.w ^ q[3]) + __popc(c1.x ^ q[4]) +
                      __popc(c1.y ^ q[5]) + __popc(c1.z ^ q[6]) + __popc(c1.w ^ q[7]);
        if (d < b.d1) {
            b.d2 = b.d1;
            b.d1 = d;
            b.k1 = k;
        } else if (d < b.d2) {
            b.d2 = d;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RlBest other;
        other.d1 = __shfl_xor(b.d1, o, 64);
        other.k1 = __shfl_xor(b.k1, o, 64);
        other.d2 = __shfl_xor(b.d2, o, 64);
        b = rl_merge(b, other);
    }
    __shared__ RlBest sb[4];
    if ((tid & 63) == 0) sb[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        b = rl_merge(rl_merge(sb[0], sb[1]), rl_merge(sb[2], sb[3]));
        const bool cand = b.k1 != RL_NONE && (double)b.d1 <= max_distance &&
                          (coef == 0.0 || b.d2 == RL_NONE || (double)b.d1 < coef * (double)b.d2);
        feat_flag[f] = cand ? 2 : 1;
        feat_kp[f] = cand ? b.k1 : -1;
        feat_dist[f] = cand ? b.d1 : 0;
    }
}

// the bearing of a distorted pixel: undistortPoint (EKF/AddMapFeature.cpp:42-58, as k_addfeat_prepare has it), then the unit vector
__device__ __forceinline__ void rl_bearing(const CamD &c, double ud, double vd, double *f)
{
    const double mx = ud - c.cx, my = vd - c.cy;
    const double dxm = c.dx * mx, dym = c.dy * my;
    const double rd2 = dxm * dxm + dym * dym;
    const double dist = 1 + c.k1 * rd2 + c.k2 * rd2 * rd2;
    const double uu = c.cx + mx * dist, vu = c.cy + my * dist;
    const double b0 = (uu - c.cx) / c.fx, b1 = (vu - c.cy) / c.fy;
    const double nrm = sqrt(b0 * b0 + b1 * b1 + 1.0);
    f[0] = b0 / nrm;
    f[1] = b1 / nrm;
    f[2] = 1.0 / nrm;
}

__global__ void __launch_bounds__(1024)
k_reloc_compact(CamD c, int N, const int *feat_flag, const int *feat_kp, const int *feat_dist, const double *X, const EkfKeypoint *kps,
                EkfMatch *cand, double *cX, double *cf, RelocCtl *ctl)
{
    __shared__ int wtot[16];
    const int tid = threadIdx.x;
    int n_cand = 0, n_used = 0;
    for (int base = 0; base < N; base += 1024) { // (N is the same for every thread)
        const int f = base + tid;
        const int flag = f < N ? feat_flag[f] : 0;
        int tot;
        const int at = n_cand + block_exclusive_scan_1024(flag == 2 ? 1 : 0, wtot, &tot);
        n_cand += tot;
        __syncthreads();
        (void)block_exclusive_scan_1024(flag >= 1 ? 1 : 0, wtot, &tot);
        n_used += tot;
        __syncthreads();
        if (flag == 2) {
            const int k = feat_kp[f];
            const EkfKeypoint kp = kps[k];
            EkfMatch m;
            m.featureIndex = f;
            m.keypointIndex = k;
            m.imagePos[0] = (double)kp.x;
            m.imagePos[1] = (double)kp.y;
            m.distance = (float)feat_dist[f];
            m._pad = 0.f;
            cand[at] = m;
            double b[3];
            rl_bearing(c, m.imagePos[0], m.imagePos[1], b);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                cX[3 * (size_t)at + i] = X[3 * (size_t)f + i];
                cf[3 * (size_t)at + i] = b[i];
            }
        }
    }
    if (tid == 0) {
        ctl->n_used = n_used;
        ctl->n_cand = n_cand;
    }
}

// ------------------------------------------------------------------------------------------------------ sampling
__device__ __forceinline__ unsigned long long rl_splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// three distinct indices below C (C >= 3): a taken index steps to the next one mod C, tested twice against both earlier ones
__device__ __forceinline__ void rl_triple(unsigned long long seed, int h, int C, int *idx)
{
    idx[0] = idx[1] = idx[2] = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int i = (int)(rl_splitmix64(seed + 3ull * (unsigned long long)h + (unsigned long long)k) % (unsigned long long)C);
#pragma unroll
        for (int rep = 0; rep < 2; ++rep)
            if (i == idx[0] || i == idx[1]) i = i + 1 == C ? 0 : i + 1;
        idx[k] = i;
    }
}

// ----------------------------------------------------------------------------------------------------------- P3P
// largest real root of z^3 + a2 z^2 + a1 z + a0: closed form, then a fixed number of Newton steps
__device__ __forceinline__ double rl_largest_cubic_root(double a2, double a1, double a0)
{
    const double Q = (a2 * a2 - 3.0 * a1) / 9.0;
    const double R = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0;
    const double Q3 = Q * Q * Q;
    double z;
    if (R * R < Q3) {
        const double th = acos(R / sqrt(Q3));
        z = -2.0 * sqrt(Q) * cos((th + 2.0 * 3.14159265358979323846) / 3.0) - a2 / 3.0;
    } else {
        const double A = -copysign(1.0, R) * cbrt(fabs(R) + sqrt(R * R - Q3));
        const double B = A != 0.0 ? Q / A : 0.0;
        z = A + B - a2 / 3.0;
    }
#pragma unroll
    for (int it = 0; it < RL_CUBIC_POLISH; ++it) {
        const double f = ((z + a2) * z + a1) * z + a0;
        const double fp = (3.0 * z + 2.0 * a2) * z + a1;
        if (fp != 0.0) z = z - f / fp;
    }
    return z;
}

__device__ __forceinline__ void rl_order(double &a, double &b)
{
    if (b < a) {
        const double t = a;
        a = b;
        b = t;
    }
}

// real roots of k[0] + k[1] v + .. + k[4] v^4 into v[0..3], ascending, +inf in the slots behind them; returns their number
__device__ __forceinline__ int rl_quartic_real_roots(const double *k, double *v)
{
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    v[0] = v[1] = v[2] = v[3] = INF;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) fin = fin && isfinite(k[i]);
    if (!fin || k[4] == 0.0) return 0;
    const double A = k[3] / k[4], B = k[2] / k[4], C = k[1] / k[4], D = k[0] / k[4];
    const double A2 = A * A;
    const double p = B - 3.0 * A2 / 8.0;
    const double q = C - A * B / 2.0 + A2 * A / 8.0;
    const double r = D - A * C / 4.0 + A2 * B / 16.0 - 3.0 * A2 * A2 / 256.0;
    double z = rl_largest_cubic_root(2.0 * p, p * p - 4.0 * r, -q * q);
    if (!isfinite(z)) return 0;
    double s, qs;
    if (z > 0.0) {
        s = sqrt(z);
        qs = q / s;
    } else { // biquadratic
        z = 0.0;
        s = 0.0;
        const double disc = p * p - 4.0 * r;
        if (!(disc >= 0.0)) return 0;
        qs = sqrt(disc);
    }
    const double t[2] = {(p + z - qs) / 2.0, (p + z + qs) / 2.0}; // (y^2 + s y + t0)(y^2 - s y + t1)
    const double lin[2] = {s, -s};
    int n = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const double disc = lin[m] * lin[m] - 4.0 * t[m];
        if (!(disc >= 0.0)) continue;
        const double sq = sqrt(disc);
        const double w = -(lin[m] + copysign(sq, lin[m])) / 2.0;
        double yy[2] = {w, w != 0.0 ? t[m] / w : 0.0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double x = yy[j] - A / 4.0;
#pragma unroll
            for (int it = 0; it < RL_QUARTIC_POLISH; ++it) {
                const double f = (((x + A) * x + B) * x + C) * x + D;
                const double fp = ((4.0 * x + 3.0 * A) * x + 2.0 * B) * x + C;
                if (fp != 0.0) x = x - f / fp;
            }
            if (isfinite(x)) {
                v[2 * m + j] = x;
                ++n;
            }
        }
    }
    // five compare-exchanges sort four values (the empty slots hold +inf and end up behind the roots)
    rl_order(v[0], v[1]);
    rl_order(v[2], v[3]);
    rl_order(v[0], v[2]);
    rl_order(v[1], v[3]);
    rl_order(v[1], v[2]);
    return n;
}

__device__ __forceinline__ void rl_cross(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void rl_unit(double *a)
{
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    a[0] = a[0] / n;
    a[1] = a[1] / n;
    a[2] = a[2] / n;
}
// rows of E: e1 = unit(P2 - P1), e2 = e3 x e1, e3 = unit(e1 x (P3 - P1))
__device__ __forceinline__ void rl_triad(const double *P1, const double *P2, const double *P3, double *E)
{
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        E[i] = P2[i] - P1[i];
        d[i] = P3[i] - P1[i];
    }
    rl_unit(E);
    rl_cross(E, d, E + 6);
    rl_unit(E + 6);
    rl_cross(E + 6, E, E + 3);
}

// q (w x y z), normalised, w >= 0, of a rotation matrix: the branch of the largest of (trace, R00, R11, R22), the first among equals
__device__ __forceinline__ void rl_rot_to_quat(const double *R, double *q)
{
    const double tr = R[0] + R[4] + R[8];
    int best = 0;
    double val = tr;
    if (R[0] > val) { best = 1; val = R[0]; }
    if (R[4] > val) { best = 2; val = R[4]; }
    if (R[8] > val) { best = 3; val = R[8]; }
    if (best == 0) {
        const double s = sqrt(1.0 + tr) * 2.0;
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (best == 1) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (best == 2) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = q[0] / n < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sg * (q[i] / n);
}

// squared pixel error of world point X at pixel (u, v) seen from (r, Rinv): predict_pixel of the filter for a depth feature
__device__ __forceinline__ bool rl_pixel_error(const CamD &c, const double *r, const double *Rt, const double *Rinv, const double *X,
                                               double u, double v, double *e2)
{
    double uv[2];
    if (!predict_pixel(c, r, Rt, Rinv, X, EKF_FEATURE_DEPTH, uv)) return false;
    const double du = u - uv[0], dv = v - uv[1];
    *e2 = du * du + dv * dv;
    return true;
}

// the rotation tables of a pose: R(q), its transpose and its adjugate inverse (what the filter's prediction hands predict_pixel)
__device__ __forceinline__ void rl_pose_tables(const double *q, double *Rt, double *Rinv)
{
    double R[9];
    quat_to_rot(q, R);
    inv3(R, Rinv);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rt[3 * i + j] = R[3 * j + i];
}

constexpr int RL_SOL = 8; // doubles per solution in LDS: r (3), q (4), one unused

// One wavefront (= one workgroup) per hypothesis.  Lane 0 solves; the solutions go through LDS; every lane scores the candidates
// lane + 64 i, and the squared errors of a chunk's inliers are added in candidate order, one broadcast per inlier.
__global__ void __launch_bounds__(64)
k_reloc_p3p(CamD c, const RelocCtl *ctl, const EkfMatch *cand, const double *cX, const double *cf, unsigned long long seed, int H,
            double inlier_px, EkfRelocHypothesis *hyp)
{
    __shared__ double sol[4 * RL_SOL];
    __shared__ int s_nsol, s_idx[3];
    const int h = blockIdx.x, lane = threadIdx.x;
    if (h >= H) return;
    const int C = ctl->n_cand;
    if (C < 3) { // (the same for the whole workgroup)
        if (lane == 0) {
            EkfRelocHypothesis o;
            o.cand[0] = o.cand[1] = o.cand[2] = -1;
            o.n_solutions = o.inliers = o._pad = 0;
            o.sse = 0.0;
            o.r[0] = o.r[1] = o.r[2] = 0.0;
            o.q[0] = o.q[1] = o.q[2] = o.q[3] = 0.0;
            hyp[h] = o;
        }
        return;
    }
    if (lane == 0) {
        int idx[3];
        rl_triple(seed, h, C, idx);
        double X[9], f[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s_idx[i] = idx[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                X[3 * i + j] = cX[3 * (size_t)idx[i] + j];
                f[3 * i + j] = cf[3 * (size_t)idx[i] + j];
            }
        }
        const double *X1 = X, *X2 = X + 3, *X3 = X + 6, *f1 = f, *f2 = f + 3, *f3 = f + 6;
        double a = 0.0, b = 0.0, cc = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double d23 = X2[i] - X3[i], d13 = X1[i] - X3[i], d12 = X1[i] - X2[i];
            a += d23 * d23;
            b += d13 * d13;
            cc += d12 * d12;
        }
        const double ca = f2[0] * f3[0] + f2[1] * f3[1] + f2[2] * f3[2];
        const double cb = f1[0] * f3[0] + f1[1] * f3[1] + f1[2] * f3[2];
        const double cg = f1[0] * f2[0] + f1[1] * f2[1] + f1[2] * f2[2];
        // q = 1 - 2 cb v + v^2, N = (a - c) q + b (1 - v^2), D = 2 b (cg - ca v), ascending coefficients; the quartic is
        // b (D^2 + N^2 - 2 cg N D) - c q D^2, formed by multiplying the small arrays
        const double qp[3] = {1.0, -2.0 * cb, 1.0};
        const double Np[3] = {(a - cc) + b, -2.0 * cb * (a - cc), (a - cc) - b};
        const double Dp[2] = {2.0 * b * cg, -2.0 * b * ca};
        double D2[3] = {0.0, 0.0, 0.0}, N2[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, ND[4] = {0.0, 0.0, 0.0, 0.0}, qD2[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) D2[i + j] = D2[i + j] + Dp[i] * Dp[j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) N2[i + j] = N2[i + j] + Np[i] * Np[j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) ND[i + j] = ND[i + j] + Np[i] * Dp[j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) qD2[i + j] = qD2[i + j] + qp[i] * D2[j];
        double k[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double d2 = i < 3 ? D2[i] : 0.0, nd = i < 4 ? ND[i] : 0.0;
            k[i] = b * (d2 + N2[i] - 2.0 * cg * nd) - cc * qD2[i];
        }
        double roots[4];
        (void)rl_quartic_real_roots(k, roots);
        if (!(ca < RL_COS_MAX && cb < RL_COS_MAX && cg < RL_COS_MAX)) // two bearings coincide (two features on one keypoint), or a NaN
            roots[0] = roots[1] = roots[2] = roots[3] = __longlong_as_double(0x7ff0000000000000ll);
        double G[9];
        rl_triad(X1, X2, X3, G);
        int nsol = 0;
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) {
            const double v = roots[ri];
            if (!isfinite(v)) continue; // an empty slot
            const double qv = (v + qp[1]) * v + qp[0];
            const double Nv = (Np[2] * v + Np[1]) * v + Np[0];
            const double Dv = Dp[1] * v + Dp[0];
            const double u = Nv / Dv;
            if (!(v > 0.0 && u > 0.0 && qv > 0.0)) continue;
            const double d1 = sqrt(b / qv), d2 = u * d1, d3 = v * d1;
            double Y[9], E[9], R[9], q[4], Rq[9], r[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Y[i] = d1 * f1[i];
                Y[3 + i] = d2 * f2[i];
                Y[6 + i] = d3 * f3[i];
            }
            rl_triad(Y, Y + 3, Y + 6, E);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    R[3 * i + j] = G[i] * E[j] + G[3 + i] * E[3 + j] + G[6 + i] * E[6 + j]; // sum_k g_k e_k': R e_k = g_k
                    fin = fin && isfinite(R[3 * i + j]);
                }
            if (!fin) continue;
            rl_rot_to_quat(R, q);
            quat_to_rot(q, Rq);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                r[i] = X1[i] - (Rq[3 * i] * Y[0] + Rq[3 * i + 1] * Y[1] + Rq[3 * i + 2] * Y[2]);
                fin = fin && isfinite(r[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) fin = fin && isfinite(q[i]);
            if (!fin) continue;
            bool ok = true;
#pragma unroll
            for (int p = 0; p < 3; ++p) { // the solution must reproduce its three bearings
                const double dx[3] = {X[3 * p] - r[0], X[3 * p + 1] - r[1], X[3 * p + 2] - r[2]};
                double ci[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) ci[i] = Rq[i] * dx[0] + Rq[3 + i] * dx[1] + Rq[6 + i] * dx[2];
                rl_unit(ci);
                const double dev = fmax(fmax(fabs(ci[0] - f[3 * p]), fabs(ci[1] - f[3 * p + 1])), fabs(ci[2] - f[3 * p + 2]));
                if (!(dev <= RL_BEARING_TOL)) ok = false; // (a NaN fails)
            }
            if (!ok) continue;
            double *o = sol + RL_SOL * nsol; // (nsol < 4: one solution per root at most)
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
            o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
            ++nsol;
        }
        s_nsol = nsol;
    }
    __syncthreads();
    const int nsol = s_nsol;
    const double thr2 = inlier_px * inlier_px;
    int best_n = 0, best_s = -1;
    double best_sse = 0.0;
    for (int s = 0; s < nsol; ++s) { // (nsol <= 4, the same for every lane)
        double r[3], q[4], Rt[9], Rinv[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = sol[RL_SOL * s + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = sol[RL_SOL * s + 3 + i];
        rl_pose_tables(q, Rt, Rinv);
        int n = 0;
        double sse = 0.0;
        for (int base = 0; base < C; base += 64) {
            const int j = base + lane;
            double e2 = 0.0;
            bool inl = false;
            if (j < C) {
                const double X[3] = {cX[3 * (size_t)j], cX[3 * (size_t)j + 1], cX[3 * (size_t)j + 2]};
                double err;
                if (rl_pixel_error(c, r, Rt, Rinv, X, cand[j].imagePos[0], cand[j].imagePos[1], &err)) {
                    inl = err <= thr2;
                    if (inl) e2 = err;
                }
            }
            // the inliers' squared errors in candidate order, one broadcast each (the others would add an exact zero: skipped, the
            // sum is the same to the bit); the ballot is the same in every lane, and so is the trip count, at most 64
            unsigned long long in_chunk = __ballot(inl);
            n += __popcll(in_chunk);
            while (in_chunk) {
                sse += __shfl(e2, (int)__ffsll((long long)in_chunk) - 1, 64);
                in_chunk &= in_chunk - 1;
            }
        }
        if (s == 0 || n > best_n || (n == best_n && sse < best_sse)) {
            best_n = n;
            best_sse = sse;
            best_s = s;
        }
    }
    if (lane == 0) {
        EkfRelocHypothesis o;
        o.cand[0] = s_idx[0]; o.cand[1] = s_idx[1]; o.cand[2] = s_idx[2];
        o.n_solutions = nsol;
        o.inliers = best_n;
        o._pad = 0;
        o.sse = best_sse;
#pragma unroll
        for (int i = 0; i < 3; ++i) o.r[i] = best_s >= 0 ? sol[RL_SOL * best_s + i] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.q[i] = best_s >= 0 ? sol[RL_SOL * best_s + 3 + i] : 0.0;
        hyp[h] = o;
    }
}

// ----------------------------------------------------------------------------------------------- select + install
struct RlKey {
    int n, h; // inliers and hypothesis; h = RL_NONE: none
    double sse;
};
__device__ __forceinline__ bool rl_key_before(const RlKey &a, const RlKey &b) // a is the better one (a total order: h breaks ties)
{
    if (a.h == RL_NONE || b.h == RL_NONE) return b.h == RL_NONE && a.h != RL_NONE;
    if (a.n != b.n) return a.n > b.n;
    if (a.sse != b.sse) return a.sse < b.sse;
    return a.h < b.h;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_reloc_select(CamD c, RelocCtl *ctl, const EkfMatch *cand, const double *cX, const EkfRelocHypothesis *hyp, int H, int min_inliers,
               double inlier_px, int install, double var_r, double var_q, double var_v, double var_w, double *st, T *P, int ld, int n,
               uint8_t *mask)
{
    __shared__ RlKey sk[256];
    const int tid = threadIdx.x;
    const int C = ctl->n_cand;
    RlKey k{0, RL_NONE, 0.0};
    int valid = 0;
    if (C >= 3)
        for (int h = tid; h < H; h += 256) {
            if (hyp[h].n_solutions <= 0) continue;
            ++valid;
            const RlKey o{hyp[h].inliers, h, hyp[h].sse};
            if (rl_key_before(o, k)) k = o;
        }
    __shared__ int s_valid;
    sk[tid] = k;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    atomicAdd(&s_valid, valid); // integers: the order of the additions does not matter
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o && rl_key_before(sk[tid + o], sk[tid])) sk[tid] = sk[tid + o];
        __syncthreads();
    }
    const RlKey best = sk[0];
    const bool any = best.h != RL_NONE;
    const bool found = any && best.n >= min_inliers;
    double r[3] = {0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (any) {
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = hyp[best.h].r[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = hyp[best.h].q[i];
    }
    // the inlier mask of the best pose over the candidates
    double Rt[9], Rinv[9];
    rl_pose_tables(q, Rt, Rinv);
    const double thr2 = inlier_px * inlier_px;
    for (int j = tid; j < C; j += 256) {
        uint8_t in = 0;
        if (any) {
            const double X[3] = {cX[3 * (size_t)j], cX[3 * (size_t)j + 1], cX[3 * (size_t)j + 2]};
            double err;
            if (rl_pixel_error(c, r, Rt, Rinv, X, cand[j].imagePos[0], cand[j].imagePos[1], &err)) in = err <= thr2 ? 1 : 0;
        }
        mask[j] = in;
    }
    const bool inst = found && install != 0;
    if (tid == 0) {
        EkfRelocResult o;
        o.found = found ? 1 : 0;
        o.installed = inst ? 1 : 0;
        o.n_features_used = ctl->n_used;
        o.n_candidates = C;
        o.n_hypotheses = H;
        o.n_valid_hypotheses = s_valid;
        o.best_hypothesis = any ? best.h : -1;
        o.n_inliers = any ? best.n : 0;
        o.rms_px = any && best.n > 0 ? sqrt(best.sse / (double)best.n) : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) o.r[i] = r[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) o.q[i] = q[i];
        ctl->res = o;
    }
    if (!inst) return; // (the same for every thread; nothing of x, P or the map has been written)
    if (tid == 0) {
        // the state as initState leaves the velocities (EKF/CommonFunctions.cpp:39-52), and the cached rotation
        double *x = st + ST_X;
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = r[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[3 + i] = q[i];
        x[7] = x[8] = x[9] = 0.0;
        x[10] = x[11] = x[12] = EKF_EPSILON;
        quat_to_rot(q, st + ST_R);
    }
    // the camera's 13 rows and columns of P: the stated diagonal, zero everywhere else; both places of a pair get the same value
    for (int j = tid; j < n; j += 256) {
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            const double d = i < 3 ? var_r : (i < 7 ? var_q : (i < 10 ? var_v : var_w));
            const T val = (T)(i == j ? d : 0.0);
            P[(size_t)i * ld + j] = val;
            P[(size_t)j * ld + i] = val;
        }
    }
}

// ------------------------------------------------------------------------------------------------------ launcher
void launch_relocalise(EkfEngine *e, const RelocCall &rc)
{
    hipStream_t s = e->stream;
    DeviceArrays &d = e->d;
    const EkfRelocParams &p = *rc.params;
    const int N = e->N, H = p.hypotheses;
    if (N > 0) {
        if (e->f32)
            k_reloc_match<float><<<N, 256, 0, s>>>(d.feat_pos, d.feat_type, d.feat_covpos, d.feat_desc, N, (const float *)d.P, e->ldP, rc.kdesc,
                                                   rc.n_kp, rc.d_nkp, p.max_distance, p.second_best_coef, p.max_rel_depth_sd, d.reloc_X,
                                                   d.reloc_flag, d.reloc_kp, d.reloc_dist);
        else
            k_reloc_match<double><<<N, 256, 0, s>>>(d.feat_pos, d.feat_type, d.feat_covpos, d.feat_desc, N, (const double *)d.P, e->ldP, rc.kdesc,
                                                    rc.n_kp, rc.d_nkp, p.max_distance, p.second_best_coef, p.max_rel_depth_sd, d.reloc_X,
                                                    d.reloc_flag, d.reloc_kp, d.reloc_dist);
    }
    k_reloc_compact<<<1, 1024, 0, s>>>(e->cam, N, d.reloc_flag, d.reloc_kp, d.reloc_dist, d.reloc_X, rc.kps, d.reloc_cand, d.reloc_cX,
                                       d.reloc_cf, d.reloc_ctl);
    k_reloc_p3p<<<H, 64, 0, s>>>(e->cam, d.reloc_ctl, d.reloc_cand, d.reloc_cX, d.reloc_cf, (unsigned long long)p.seed, H, p.inlier_px,
                                 d.reloc_hyp);
    const double var_r = p.sigma_position * p.sigma_position, var_q = 0.25 * (p.sigma_angle * p.sigma_angle);
    const double var_v = e->cfg.par.initLinearAccelSD * e->cfg.par.initLinearAccelSD;
    const double var_w = e->cfg.par.initAngularAccelSD * e->cfg.par.initAngularAccelSD;
    if (e->f32)
        k_reloc_select<float><<<1, 256, 0, s>>>(e->cam, d.reloc_ctl, d.reloc_cand, d.reloc_cX, d.reloc_hyp, H, p.min_inliers, p.inlier_px,
                                                p.install, var_r, var_q, var_v, var_w, d.state, (float *)d.P, e->ldP, e->n, d.reloc_mask);
    else
        k_reloc_select<double><<<1, 256, 0, s>>>(e->cam, d.reloc_ctl, d.reloc_cand, d.reloc_cX, d.reloc_hyp, H, p.min_inliers, p.inlier_px,
                                                 p.install, var_r, var_q, var_v, var_w, d.state, (double *)d.P, e->ldP, e->n, d.reloc_mask);
}

} // namespace ekf
