// patch_normal.h -- constants and the per-feature record of the patch-normal estimator (k_ncc_normal).
// The numpy restatement tests/patch_normal_ref.py carries the same values; change them in both places.
#pragma once
#include <cstdint>

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

} // namespace ekf
