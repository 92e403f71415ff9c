/*
 * ekf_types.h -- plain-old-data types shared by the C ABI (ekf_engine.h), the C++ compat layer and the
 * test oracle.  C99 / C++ compatible, no dependencies.
 *
 * Reference citations are relative to /root/reference/kalmanFilter/modules/ :
 *   EKF/ = 1PointRansacEKF/, Cfg/ = Configuration/ConfigurationDataReader/.
 */
#ifndef EKF_TYPES_H
#define EKF_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Camera intrinsics consumed on the hot path.
 * Mirrors class CameraCalibration, Cfg/CameraCalibrationConfiguration/CameraCalibration.h:37-63
 * (same field names, same meaning; the std::string name is dropped). */
typedef struct EkfCamera {
    int32_t pixelsX;
    int32_t pixelsY;
    double fx, fy;
    double k1, k2;
    double cx, cy;
    double dx, dy;
    double pixelErrorX, pixelErrorY;
    double angularVisionX, angularVisionY; /* degrees */
} EkfCamera;

/* Filter parameters consumed on the hot path.
 * Mirrors class ExtendedKalmanFilterParameters,
 * Cfg/ExtendedKalmanFilterConfiguration/ExtendedKalmanFilterParameters.h:37-76
 * (only the fields read by stages A1..A9 of SURVEY.md section 8(a), plus those the map-management row
 * 8(f)-1 reads: new-feature initialisation, bad-feature removal, inverse-depth -> depth conversion). */
typedef struct EkfParams {
    double initInvDepthRho;
    double initLinearAccelSD;
    double initAngularAccelSD;
    double linearAccelSD;
    double angularAccelSD;
    double inverseDepthRhoSD;
    double matchingCompCoefSecondBestVSFirst;
    double ransacThresholdPredictDistance;
    double ransacAllInliersProbability;
    double ransacChi2Threshold;
    double goodFeatureMatchingPercent;          /* removeBadMapFeatures, EKF/MapManagement.cpp:279-308        */
    double inverseDepthLinearityIndexThreshold; /* convertMapFeaturesInverseDepthToDepth, MapManagement.cpp:494 */
} EkfParams;

/* Map feature parametrisation, enum MapFeatureType EKF/MapFeature.h:39-44 (same numeric values). */
enum {
    EKF_FEATURE_INVALID = 0,
    EKF_FEATURE_DEPTH = 1,        /* 3 parameters: x y z                 */
    EKF_FEATURE_INVERSE_DEPTH = 2 /* 6 parameters: x y z theta phi rho   */
};

/* Binary descriptor width used by the reference's configured extractor (BRIEF-32,
 * Cfg/DescriptorExtractorConfiguration/DescriptorExtractorFactory.cpp:114-123). */
#define EKF_DESC_BYTES 32

/* A predicted measurement: class ImageFeaturePrediction, EKF/ImageFeaturePrediction.h:37-50. */
typedef struct EkfPrediction {
    int32_t featureIndex;
    int32_t _pad;
    double imagePos[2];
    double covarianceMatrix[4]; /* 2x2 row-major innovation covariance S_i (R_i = I) */
} EkfPrediction;

/* A match: class FeatureMatch, EKF/Matching.h:38-48 (descriptor omitted; keypointIndex added so a
 * caller can fetch it from its own descriptor matrix). */
typedef struct EkfMatch {
    int32_t featureIndex;
    int32_t keypointIndex;
    double imagePos[2];
    float distance;
    float _pad;
} EkfMatch;

/* A detected keypoint position: cv::KeyPoint::pt (float x, y) as read at EKF/Matching.cpp:232,250-256. */
typedef struct EkfKeypoint {
    float x, y;
} EkfKeypoint;

/* What the NCC matcher's distinctiveness test (ekf_set_ncc_distinct) found for one prediction.  No counterpart in the
 * reference, whose two-best test (Matching.cpp:188-262) lives in the descriptor matcher. */
typedef struct EkfNccRival {
    int32_t featureIndex;
    int32_t state;       /* 0 = no valid match, 1 = valid and no rival in the gate, 2 = rival and kept, 3 = rival and rejected */
    float rivalPos[2];   /* level-0 pixel of the rival (states 2, 3; else 0)                                              */
    float distance;      /* 1 - zncc of the best place (states 1, 2, 3; else 0): the match's distance                    */
    float rivalDistance; /* ... and of the rival (states 2, 3; else 0)                                                   */
} EkfNccRival;           /* 24 bytes, no padding                                                                         */

/* One landmark of the map as a 3-D point (ekf_get_map_points).  No counterpart in the reference, whose map is only
 * ever read in the filter's own parametrisation.  r, q = camera position and orientation (state elements 0..2, 3..6),
 * R(q) = Core/EKFMath.cpp:133-155, m(theta, phi) = Core/EKFMath.cpp:159-166. */
typedef struct EkfMapPoint {
    double xyz[3];     /* world position X: (x y z) of a depth feature, (x0 y0 z0) + m(theta, phi) / rho otherwise  */
    double cov[9];     /* 3x3 row-major covariance of X (world axes), exactly symmetric                              */
    double cam[3];     /* the same point in the camera's axes: R(q)' (X - r)                                         */
    double cov_cam[9]; /* 3x3 covariance of cam, camera position and orientation uncertainty included                */
    double linearity;  /* computeLinearityIndex (EKF/MapManagement.cpp:312-341); 1e300 for a depth feature           */
    int32_t type;      /* EKF_FEATURE_DEPTH / EKF_FEATURE_INVERSE_DEPTH                                              */
    int32_t covpos;    /* first row of the feature in P                                                              */
    uint32_t times_predicted, times_matched;
} EkfMapPoint;         /* 25 doubles + 4 x 32 bit = 216 bytes, no padding                                            */

/* Filter consistency (ekf_set_consistency): one record per covariance update, and one per match of such an update.  No
 * counterpart in the reference.  With S = H P H' + pixelErrorX I of the update, L its Cholesky factor and nu the dead-banded
 * innovation in the update's order: z = inv(L) nu, nis = sum of z_k^2 (chi-square with `rows` degrees of freedom for a
 * consistent filter). */
typedef struct EkfUpdateConsistency {
    int32_t stage;   /* 0 = ekf_update, 1 = a step's first (low-innovation) update, 2 = its second (high-innovation) update */
    int32_t matches; /* M                                                                                                   */
    int32_t rows;    /* m = 2 M: the degrees of freedom of nis                                                              */
    int32_t _pad;
    double nis;
} EkfUpdateConsistency; /* 24 bytes */

typedef struct EkfInnovation {
    int32_t featureIndex;
    int32_t stage;
    double nu[2];           /* innovation: imagePos - predicted distorted pixel, 0 where |.| <= EKF_DELTA                   */
    double d2_marginal;     /* nu' inv(S_i) nu with S_i the match's own 2x2 block of S; 1e300 when det(S_i) <= 0             */
    double nis_conditional; /* z_2i^2 + z_2i+1^2: the match's share of nis, conditional on the matches before it in the list */
    double _reserved;
} EkfInnovation; /* 48 bytes, no padding */

/* Measurement budget (ekf_set_measurement_budget): one record per feature the step's full prediction saw.  No counterpart in
 * the reference.  S_i = H_i P H_i' + pixelErrorX I is the feature's 2x2 innovation covariance, r = pixelErrorX. */
typedef struct EkfMeasurementRank {
    int32_t featureIndex;
    int32_t rank;     /* 0 = most informative; ties go to the lower feature index                                      */
    int32_t selected; /* 1: handed on to the H P pass, the matcher and the updates; 0: left for a later frame            */
    int32_t _pad;
    double key;       /* det(S_i); -1 when it is NaN or not positive (such a feature ranks last)                        */
    double gain;      /* 0.5 * log(key / (r * r)): the information the measurement carries, in nats; 0 when key = -1    */
} EkfMeasurementRank; /* 32 bytes, no padding */

/* External measurement update (ekf_update_external): any linearised measurement z = h(x) + noise(R), handed in as sparse rows of
 * its Jacobian H.  No counterpart in the reference, whose only measurement is the camera's. */
#define EKF_EXT_MAX_ROWS 16 /* measurement rows per call */
#define EKF_EXT_MAX_NNZ 32  /* non-zero entries per row of H */

typedef struct EkfExternalUpdate {
    double nis;                 /* z'z, z = inv(L) residual, S = H P H' + R = L L': chi-square with `rows` degrees of freedom */
    double z[EKF_EXT_MAX_ROWS]; /* the whitened residual; entries >= rows are 0 */
    int32_t rows;
    int32_t applied;            /* 1: x and P were updated; 0: the gate rejected it, nothing changed */
} EkfExternalUpdate;            /* 144 bytes, no padding */

/* Iterated update (ekf_update_iterated / ekf_set_update_iterations): one record per iterated update of the last call.  No
 * counterpart in the reference, which linearises once. */
#define EKF_MAX_UPDATE_ITERATIONS 8
enum { EKF_ITER_STOP_COUNT = 0, EKF_ITER_STOP_TOL = 1, EKF_ITER_STOP_FEATURE_LEFT = 2, EKF_ITER_STOP_FAILED = 3 };

typedef struct EkfIterationRecord {
    int32_t stage;       /* 0 = ekf_update_iterated, 1 = a step's first (low-innovation) update, 2 = its second                   */
    int32_t passes_run;  /* the result is the iterated update of this many passes (1: the plain update)                          */
    int32_t stop_reason; /* EKF_ITER_STOP_*: the pass count, the tolerance, a matched feature left the image, a sweep failed      */
    int32_t _pad;
    double step[EKF_MAX_UPDATE_ITERATIONS]; /* step[i] = max_j |x_j^(i+1) - x_j^i| / sqrt(P_jj) over the state columns with P_jj > 0,
                                             * P the covariance before the update; 0 from passes_run on                           */
} EkfIterationRecord; /* 80 bytes, no padding */

/* What the header of a map blob says (ekf_save_map / ekf_load_map / ekf_map_blob_info; the format: DESIGN.md 9.3).  No
 * counterpart in the reference, which cannot save its map. */
typedef struct EkfMapBlobInfo {
    uint32_t version;      /* 1                                                                                      */
    int32_t N, n;          /* features, state dimension                                                              */
    int32_t p_elem_bytes;  /* 4 or 8: P is stored as the saving engine stored it                                     */
    int32_t p_layout;      /* 0 = packed upper triangle (P was bitwise symmetric), 1 = full square                   */
    int32_t desc_bytes;    /* bytes per descriptor row                                                               */
    int32_t desc_flags;    /* EkfEngineConfig::flags of the saving engine                                            */
    uint32_t section_mask; /* EKF_MAP_* of the optional sections present                                             */
    uint64_t total_bytes;
    EkfCamera cam;         /* the camera the blob was saved under: reported, never compared                          */
} EkfMapBlobInfo;          /* 40 + 104 = 144 bytes, no padding                                                       */

/* Relocalisation on the map (ekf_relocalise): parameters, result and the record of one hypothesis.  No counterpart
 * in the reference, which has no way back once tracking is lost. */
#define EKF_RELOC_MAX_HYPOTHESES 4096

typedef struct EkfRelocParams {
    int32_t hypotheses;      /* 1..EKF_RELOC_MAX_HYPOTHESES                                                            */
    int32_t min_inliers;     /* >= 4: inliers of the best hypothesis from which the pose counts as found               */
    uint64_t seed;           /* the triple of hypothesis h comes from splitmix64(seed + 3 h + k), k = 0, 1, 2          */
    double max_distance;     /* Hamming, >= 0: the best keypoint of a feature must be this close                       */
    double second_best_coef; /* 0 = off, else (0,1]: ... and closer than coef times the second best                    */
    double inlier_px;        /* > 0: reprojection error of an inlier, pixels                                           */
    double max_rel_depth_sd; /* 0 = no filter, else an inverse-depth feature takes part when sd(rho) / rho is at most this */
    double sigma_position;   /* > 0: standard deviation of the installed position, per axis                            */
    double sigma_angle;      /* > 0, rad: ... and of the installed orientation (a quaternion component gets half of it) */
    int32_t install;         /* != 0: a found pose replaces the camera state and the camera's rows and columns of P    */
    int32_t _pad;
} EkfRelocParams;            /* 72 bytes, no padding */

typedef struct EkfRelocResult {
    int32_t found;              /* 1: the best hypothesis has min_inliers inliers or more                               */
    int32_t installed;          /* 1: found, and the pose was installed                                                 */
    int32_t n_features_used;    /* features that took part                                                              */
    int32_t n_candidates;       /* ... and those that found a keypoint                                                  */
    int32_t n_hypotheses;
    int32_t n_valid_hypotheses; /* hypotheses with one P3P solution or more                                             */
    int32_t best_hypothesis;    /* -1: none was valid                                                                   */
    int32_t n_inliers;
    double rms_px;              /* sqrt(sum of squared inlier errors / n_inliers) of the best hypothesis                */
    double r[3];                /* its pose (zeros when none was valid): camera position ...                            */
    double q[4];                /* ... and orientation (w x y z, w >= 0), R(q) camera -> world                          */
} EkfRelocResult;               /* 96 bytes, no padding */

typedef struct EkfRelocHypothesis {
    int32_t cand[3];     /* the three candidates (indices into the candidate list); -1 with fewer than 3 candidates     */
    int32_t n_solutions; /* P3P solutions that passed every test, 0..4                                                  */
    int32_t inliers;     /* of its best solution                                                                        */
    int32_t _pad;
    double sse;          /* sum of the squared inlier errors of that solution, added in candidate order                 */
    double r[3];
    double q[4];
} EkfRelocHypothesis;    /* 88 bytes, no padding */

/* Numeric constants of the reference, Core/EKFMath.h:37-41 (long double literals there; used as double). */
#define EKF_EPSILON 2.22e-16
#define EKF_DELTA 1.0e-12
#define EKF_PI 3.14159265
#define EKF_CHISQ_95_2 5.9915

/* Status codes returned across the C ABI. */
enum {
    EKF_OK = 0,
    EKF_ERR_INVALID_ARG = 1,
    EKF_ERR_CAPACITY = 2,
    EKF_ERR_NOT_POSITIVE_DEFINITE = 3, /* S = H P H' + R failed to factorise (reference: silent zeros from cv::invert) */
    EKF_ERR_NON_FINITE = 4,
    EKF_ERR_HIP = 5,
    EKF_ERR_NO_DEVICE = 6,
    EKF_ERR_COMM = 7,
    EKF_ERR_TIMEOUT = 8 /* a device-side wait of the persistent Cholesky sweep exceeded its bound (its workgroups were not all resident:
                           another persistent launch of another process on the same GPU?); the update is incomplete */
};

#ifdef __cplusplus
}
#endif
#endif /* EKF_TYPES_H */
