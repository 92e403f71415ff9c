// patch_normal.h -- constants and the per-feature record of the patch-normal estimator (k_ncc_normal), and the
// host + device functions of a patch's plane.  The numpy restatement tests/patch_normal_ref.py carries the same values; change
// them in both places.
#pragma once
#include <cmath>
#include <cstdint>

#include "device_math.h"

namespace ekf {

constexpr double PN_FD_STEP = 1.0 / 1024.0;    // central-difference step in p and q (2^-10)
constexpr double PN_S_MIN = 1.0 / 256.0;       // floor of the residual's standard deviation per pixel of the normalised vectors
constexpr double PN_STEP_MAX = 0.25;           // longest step in (p, q) per update
constexpr double PN_PRIOR_INFO = 1.0;          // information of the first update's prior: identity times this
constexpr double PN_MIN_SS = 0.5;              // a vector whose sum of squared deviations is not above this is constant

// one per feature, in d.wnorm: slope of the patch plane in the capture camera's axes, its information matrix (l00, l01, l11),
// and how many estimator steps it has taken (0: no estimate, k_ncc_warp uses the rule of DESIGN.md 4.6)
struct PatchNormalRec {
    double pq[2];
    double info[3];
    int32_t updates;
    int32_t pad;
};
static_assert(sizeof(PatchNormalRec) == 48, "d.wnorm is sized and compacted by this");

// The pieces of the patch geometry that the host reads back as well (ekf_get_patch_normals): the same operations in the same
// order on both sides; the host's sin / cos may differ from the device's in the last place.

// a capture pose record (d.wpose: r0, q0, capture pixel) with a zero quaternion means "no source patch"
__host__ __device__ __forceinline__ bool patch_has_source(const double *pose)
{
    return pose[3] != 0.0 || pose[4] != 0.0 || pose[5] != 0.0 || pose[6] != 0.0;
}

// world point of the feature y (a row of d.feat_pos): the point itself, or origin + m(theta, phi) / rho for inverse depth
__host__ __device__ __forceinline__ void patch_world_point(const double *y, int type, double *X)
{
    X[0] = y[0]; X[1] = y[1]; X[2] = y[2];
    if (type == EKF_FEATURE_INVERSE_DEPTH) {
        double m[3];
        dir_vec(y[3], y[4], m);
        X[0] += m[0] / y[5]; X[1] += m[1] / y[5]; X[2] += m[2] / y[5];
    }
}

// unit normal in world axes of the slope (p, q) in the capture camera's axes: R0 (p, q, -1) / |(p, q, -1)|
__host__ __device__ __forceinline__ void pn_normal(const double *R0, double p, double q, double *n)
{
    const double nrm = sqrt(p * p + q * q + 1.0);
    for (int i = 0; i < 3; ++i) n[i] = (R0[3 * i] * p + R0[3 * i + 1] * q - R0[3 * i + 2]) / nrm;
}

// the rule of DESIGN.md 4.6 (the plane faces the capture camera) as a slope: p = -h0 / h2, q = -h1 / h2 of h = R0' (X - r0)
__host__ __device__ __forceinline__ void pn_rule_slope(const double *R0, const double *X, const double *r0, double *pq)
{
    const double w[3] = {X[0] - r0[0], X[1] - r0[1], X[2] - r0[2]};
    const double h0 = R0[0] * w[0] + R0[3] * w[1] + R0[6] * w[2];
    const double h1 = R0[1] * w[0] + R0[4] * w[1] + R0[7] * w[2];
    const double h2 = R0[2] * w[0] + R0[5] * w[1] + R0[8] * w[2];
    pq[0] = -h0 / h2;
    pq[1] = -h1 / h2;
}

} // namespace ekf
