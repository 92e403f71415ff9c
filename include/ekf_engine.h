/*
 * ekf_engine.h -- C ABI of the MI355X-native EKF engine (libekf_engine.so).
 *
 * Drop-in boundary for the per-frame hot path of segeschecho/OpenEKFMonoSLAM.  The reference has no FFI or
 * plugin interface; its seam is the set of free functions in kalmanFilter/modules/1PointRansacEKF/ headers that
 * EKF::step calls.  Each entry point below replaces one of them (file:line given per function, relative to
 * /root/reference/kalmanFilter/modules/, EKF/ = 1PointRansacEKF/).  The C++ headers under
 * openekfmonoslam_amd/compat/ re-create the reference's own signatures on top of this ABI.
 *
 * Conventions
 *  - plain pointers and sizes only, caller-owned buffers, int status codes (ekf_types.h), no exceptions;
 *  - one engine = one host thread + its own HIP stream; several engines may coexist (no globals);
 *  - state, covariance P, the map and all per-frame intermediates stay resident in HBM between calls;
 *    ekf_set_state / ekf_get_state are the explicit host<->device synchronisation points;
 *  - predictions, Jacobian blocks and the H*P row pairs produced by ekf_predict_measurements stay on the
 *    device, keyed by featureIndex; ekf_match / ekf_ransac / ekf_update / ekf_rescue consume them, which is how
 *    the reference's index-aligned (prediction, Jacobian, match) vectors (EKF/Update.h:47) are expressed here.
 *  - there is no CPU fallback: every compute entry point returns EKF_ERR_NO_DEVICE without a usable GPU.
 */
#ifndef EKF_ENGINE_H
#define EKF_ENGINE_H

#include <stddef.h>

#include "ekf_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct EkfEngine EkfEngine;

enum {
    EKF_PRECISION_F64 = 0, /* covariance and work matrices in fp64 (reference arithmetic)                   */
    EKF_PRECISION_F32 = 1, /* covariance, H*P and the rank-m downdate in fp32 (MFMA f32); S, its Cholesky     */
                           /* factor, the state and all Jacobians stay fp64                                   */
    EKF_PRECISION_F32_EXACT = 2, /* fp32 STORAGE of the covariance and of H*P, reference-class arithmetic: B = inv(L) H P in
                                 * fp64 and the rank-m downdate P - B'B accumulated EXACTLY (int8 digit planes of B on the
                                 * int8 MFMA, int32 sums), rounded to fp32 once per entry and update.  The reference computes
                                 * in double throughout (Core/Base.h:67; Update.cpp:105-108, 214-218). */
    EKF_PRECISION_F64_EXACT = 3, /* fp64 STORAGE of the covariance with the same exact int8 update: the sums are subtracted from an
                                 * fp64-stored P, no rounding to fp32 -- for maps on which fp32 storage alone leaves the reference's
                                 * 1e-5 (fresh maps of >= ~1400 features); about 2.5 x the speed of EKF_PRECISION_F64 there. */
    EKF_PRECISION_AUTO = 4      /* the fastest configuration that holds every feature parameter within 1e-5 of the fp64 reference
                                 * at this capacity (measured): EKF_PRECISION_F32_EXACT up to
                                 * EKF_AUTO_F32_MAX_FEATURES features, EKF_PRECISION_F64_EXACT up to EKF_AUTO_EXACT_MAX_FEATURES,
                                 * EKF_PRECISION_F64 above; ekf_get_precision reports the choice */
};
#define EKF_AUTO_F32_MAX_FEATURES 1024
#define EKF_AUTO_EXACT_MAX_FEATURES 2048

typedef struct EkfEngineConfig {
    EkfCamera cam;
    EkfParams par;
    int32_t max_features;  /* map capacity N_max; state capacity is 13 + 6 N_max                            */
    int32_t max_keypoints; /* per-frame keypoint capacity                                                    */
    int32_t precision;     /* EKF_PRECISION_*                                                                */
    int32_t device;        /* HIP device ordinal, or -1 for the current device                               */
    int32_t ransac_batch;  /* hypotheses evaluated per launch (0 = default 32)                               */
    int32_t flags;         /* descriptor format, EKF_DESCRIPTOR_* (0 = 32-byte binary / Hamming)                  */
} EkfEngineConfig;

/* Descriptor format of the map features and keypoints = the two branches of computeDistance
 * (EKF/Matching.cpp:47-92):
 *   EKF_DESCRIPTOR_U8_HAMMING      CV_8U, EKF_DESC_BYTES bytes per descriptor, Hamming distance (:76-92; BRIEF-32, the
 *                                  shipped configuration)
 *   EKF_DESCRIPTOR_F32_L2(cols)    CV_32F, `cols` floats per descriptor (1..1024), L2 distance (:60-73; SURF / SIFT
 *                                  style extractors of Cfg/DescriptorExtractorFactory.cpp)
 * Every `desc32` argument of this ABI is a row-major matrix with ekf_descriptor_bytes(e) bytes per row. */
#define EKF_DESCRIPTOR_U8_HAMMING 0
#define EKF_DESCRIPTOR_F32_L2(cols) (1 | ((cols) << 8))

/* Per-step counters; same layout as the oracle's OrcStepInfo. */
typedef struct EkfStepInfo {
    int32_t n_predicted;
    int32_t n_matches;
    int32_t n_hypotheses;
    int32_t n_inliers;
    int32_t n_outliers;
    int32_t n_rescued;
    int32_t status;
    int32_t n_sweep_retries; /* updates of this step whose persistent Cholesky sweep timed out and that were run again, transparently,
                              * on the launch-per-panel sweep (the slot the oracle's OrcStepInfo leaves as padding; 0 in normal
                              * operation; ekf_get_sweep_retries totals them) */
} EkfStepInfo;

/* Accumulated GPU time per stage, in milliseconds, under the reference's own stage names
 * (EKF/EKF.cpp:291,344,410,437,513,539) plus the dominant kernel on its own. */
typedef struct EkfStageTimes {
    double prediction_ms;
    double matching_ms;
    double ransac_ms;
    double update_li_ms;
    double rescue_ms;
    double update_hi_ms;
    double p_update_kernel_ms; /* sum over launches of the P <- P - B'B kernel (HIP events on the engine stream) */
    int64_t p_update_launches;
    double p_update_flops;     /* algorithmic flops of those launches: n^2 * m each (upper triangle)          */
    double p_update_bytes;     /* algorithmic bytes: 2 * n^2 * w / 2 ... see DESIGN.md                        */
    int64_t steps;
} EkfStageTimes;

/* -- life cycle ------------------------------------------------------------------------------------------ */
/* Replaces EKF::EKF (EKF/EKF.cpp:124-165) minus file I/O: the two config PODs are passed by value. */
int ekf_engine_create(const EkfEngineConfig *cfg, EkfEngine **out);
void ekf_engine_destroy(EkfEngine *e);
const char *ekf_last_error(const EkfEngine *e);
int ekf_abi_version(void);
/* Number of usable HIP devices (0 when none); never fails. */
int ekf_device_count(void);

/* -- host <-> device synchronisation --------------------------------------------------------------------- */
/* Loads State (EKF/State.h:40-81: position, orientation, linearVelocity, angularVelocity as x13 =
 * r(3) q(4: w x y z) v(3) w(3); mapFeatures as 6 doubles per feature + type + 32-byte descriptor) and
 * EKF::stateCovarianceMatrix (n x n row-major doubles, leading dimension n).  Covariance positions are assigned
 * in map order exactly as MapFeature::covarianceMatrixPos (EKF/MapFeature.h:68). */
int ekf_set_state(EkfEngine *e, const double x13[13], int n_features, const double *feature_pos,
                  const int32_t *feature_type, const uint8_t *desc32, const double *P);
/* Any output pointer may be NULL.  P is written as n x n doubles. */
int ekf_get_state(EkfEngine *e, double x13[13], double *feature_pos, double *P);
/* Per-feature bookkeeping updateMapFeatures maintains every step (EKF/MapManagement.cpp:77-113): the current map
 * descriptors (32 bytes each) and MapFeature::timesPredicted / timesMatched.  Any pointer may be NULL. */
int ekf_get_map_features(EkfEngine *e, uint8_t *desc32, uint32_t *times_predicted, uint32_t *times_matched);
int ekf_state_dim(const EkfEngine *e);
int ekf_descriptor_bytes(const EkfEngine *e); /* bytes per descriptor row (32, or 4 * cols for CV_32F) */
int ekf_get_precision(const EkfEngine *e);    /* the EKF_PRECISION_* in use (what EKF_PRECISION_AUTO resolved to) */
int ekf_num_features(const EkfEngine *e);

/* -- the whole map in one buffer ------------------------------------------------------------- */
/* A map blob is the complete filter and map, bit for bit: x13, the feature parameters, types, descriptors, timesPredicted /
 * timesMatched and P always; with the bits of `sections` also the NCC templates, the template warp's source patches with their
 * capture poses, and the patch normals (a table the engine never allocated is simply absent: no error).  It is little-endian,
 * versioned, self-describing and checksummed; its format is a contract, written down in DESIGN.md 9.3.  P is stored in the
 * engine's storage type, as the packed upper triangle (n (n + 1) / 2 elements) when it is bitwise symmetric (known after a
 * covariance update, else found out by a read-only pass on the device: a predicted covariance is) and as the full square
 * otherwise: both triangles are always recoverable bit for bit, and it is packed and checksummed on the device (kernels_mapblob.hip), so one copy moves n (n + 1) / 2 * w bytes.  The blob carries no
 * modes or settings.  No counterpart in the reference. */
enum { EKF_MAP_TEMPLATES = 1, EKF_MAP_WARP_SOURCES = 2, EKF_MAP_PATCH_NORMALS = 4, EKF_MAP_ALL = 7 };
/* The size ekf_save_map would write now. */
int ekf_map_blob_bytes(EkfEngine *e, int sections, size_t *bytes);
/* Writes the blob; *bytes receives its size.  EKF_ERR_CAPACITY when `capacity` is too small (*bytes: the size needed, nothing
 * written).  Read-only: no state, no P and no per-feature table is written (the second covariance buffer of the out-of-place map
 * passes is the staging buffer, allocated on first use).  Synchronises the stream and first reports a pending asynchronous error
 * as ekf_update_external does, and then does nothing else.  A sharded engine: EKF_ERR_INVALID_ARG. */
int ekf_save_map(EkfEngine *e, int sections, void *blob, size_t capacity, size_t *bytes);
/* Replaces the engine's filter and map by the blob's.  The blob is untrusted: everything is validated on the host first (never
 * reading outside [blob, blob + bytes)), then P is uploaded and checked on the device (checksum, every entry finite, diagonal
 * > 0), and only then is anything written: a load that is refused leaves the engine bit for bit as it was (a table the blob needs
 * and the engine lacks is allocated, zero-filled, before; the modes stay as they are).  EKF_ERR_INVALID_ARG: malformed, truncated
 * or corrupt blob, another descriptor format than the engine's, a sharded engine (ekf_last_error names the field);
 * EKF_ERR_CAPACITY: more features than max_features; EKF_ERR_NON_FINITE: the device check found a bad entry of P.  P may have
 * another element size than the engine's: fp32 widens exactly, fp64 is rounded once to nearest.  Afterwards the engine is where
 * ekf_set_state would leave it, except that the counters, templates, source patches, capture poses and normals hold the blob's
 * values (zero for features 0..N-1 where the section is absent), P counts as bitwise symmetric exactly for a triangle blob, and no
 * retry of an earlier update is pending.  Settings and modes are untouched; the blob's camera is reported in *info (may be NULL)
 * and not compared.  Pending asynchronous errors: as ekf_save_map. */
int ekf_load_map(EkfEngine *e, const void *blob, size_t bytes, EkfMapBlobInfo *info);
/* Host only (no engine, no device): validates the blob, all checksums included, and reports its header. */
int ekf_map_blob_info(const void *blob, size_t bytes, EkfMapBlobInfo *info);

/* -- map management: the state dimension changes, P is edited in place on the device ------ */
/* initState + initCovariance                              EKF/CommonFunctions.cpp:39-80 (empties the map) */
int ekf_reset(EkfEngine *e);
/* addFeaturesToStateAndCovariance(measurements, state, P) EKF/AddMapFeature.h (.cpp:354; per feature :293-344,
 * covariance :221-289): uv = distorted pixel of each new feature (2 doubles each), desc32 = its descriptor. */
int ekf_add_features(EkfEngine *e, const double *uv, const uint8_t *desc32, int count);
/* removeFeaturesFromStateAndCovariance(featuresToRemove, state, P)  EKF/MapManagement.cpp:212-259;
 * ascending feature indices (map order, as the reference requires sorted ranges). */
int ekf_remove_features(EkfEngine *e, const int32_t *feat_idx, int count);
/* removeBadMapFeatures(state, P)                          EKF/MapManagement.cpp:279-308 */
int ekf_remove_bad_features(EkfEngine *e, int *n_removed);
/* convertMapFeaturesInverseDepthToDepth(state, P)         EKF/MapManagement.cpp:494-521 (at most one per call;
 * converted_index receives the feature index or -1) */
int ekf_convert_inverse_depth_to_depth(EkfEngine *e, int *converted_index);
/* Converts EVERY inverse-depth feature whose linearity index (computeLinearityIndex, on the current state and P) is below
 * inverseDepthLinearityIndexThreshold, in one pass; the reference converts one per call (MapManagement.cpp:494-521).
 * *count receives the number of features converted; the first min(count, capacity) of their indices are written to
 * converted_idx in ascending order (converted_idx may be NULL; a small capacity never prevents the conversion).  With R the
 * block-diagonal matrix of I for kept rows and the 3x6 Jacobian of each converted feature, P' = R P R' is formed in one
 * out-of-place pass in fp64 from the upper triangle of P (row transform, then column transform; each computed entry is
 * rounded to the storage type once and copied to its mirror; kept x kept entries are moved bit for bit); the state dimension
 * falls by 3 * count and no feature index changes, so descriptors, counters, templates, source patches, capture poses, patch
 * normals and the unseen list stay where they are.  For a bitwise symmetric P the result is that of the single conversions
 * applied in ascending order, up to rounding.  Synchronises the stream and first reports a pending
 * asynchronous error as ekf_update_external does (then nothing is converted).  Nothing below the threshold, or an empty map:
 * EKF_OK, *count = 0 and no byte of the engine changes.  A sharded engine: EKF_ERR_INVALID_ARG. */
int ekf_convert_all_inverse_depth_to_depth(EkfEngine *e, int32_t *converted_idx, int capacity, int *count);
/* the 13x13 camera block of the covariance, row-major: what EKF::step logs as StateCovarianceMatrixEstimation
 * (EKF/EKF.cpp:626) -- without moving the whole matrix */
int ekf_get_camera_covariance(EkfEngine *e, double P13[169]);
/* The map as 3-D points (EkfMapPoint per feature, map order), computed on the device: world position and 3x3
 * covariance, the same point in the camera's axes with the pose uncertainty included, the linearity index and the
 * feature's bookkeeping -- 216 bytes per feature cross the bus instead of P.  Read-only: x, P and the map tables are
 * untouched.  Synchronises the stream and reports a pending asynchronous error as ekf_get_state does (the points are
 * still produced).  points may be NULL (count only).  capacity < number of features -> EKF_ERR_CAPACITY, *count =
 * number needed.  Not available on a sharded engine. */
int ekf_get_map_points(EkfEngine *e, EkfMapPoint *points, int capacity, int *count);
/* features the last full prediction did not see (unseenFeatures of predictCameraMeasurements,
 * EKF/MeasurementPrediction.cpp:705; EKF::step removes them under the conditions of EKF/EKF.cpp:583-592).
 * Ascending feature indices; feat_idx may be NULL to get the count only. */
int ekf_get_unseen_features(EkfEngine *e, int32_t *feat_idx, int *count);
/* MapFeature::featureType / covarianceMatrixPos of every feature (EKF/MapFeature.h:60-68) */
int ekf_get_feature_layout(EkfEngine *e, int32_t *type, int32_t *covpos);
/* predictedDistortedFeatures of the step's predictCameraMeasurements as they were BEFORE the updates -- what
 * drawPrediction receives for the per-frame prediction image (EKF/EKF.cpp:294-305, Gui/Draw.cpp:266-310).  Off by
 * default (one extra small launch per frame when on); preds may be NULL to get the count only. */
int ekf_keep_step_predictions(EkfEngine *e, int on);
int ekf_get_step_predictions(EkfEngine *e, EkfPrediction *preds, int *n_preds);

/* Filter consistency (opt-in; off: no extra launch, allocation or read-back, every result bit for bit).  With the mode on
 * every covariance update -- ekf_update, and the first and the second update inside ekf_step, ekf_step_frame, ekf_step_image
 * and ekf_step_staged_image; not ekf_update_only_state, not RANSAC hypotheses -- is followed by one small launch that records
 * its normalised innovation squared and, per match, the innovation, its marginal Mahalanobis distance and its conditional
 * share of the NIS (EkfUpdateConsistency / EkfInnovation, ekf_types.h).  Records and running totals stay on
 * the device until a getter asks; a step gains no read-back.  An update that was skipped (no matches, S not positive definite)
 * leaves no record.  Allocates 48 bytes x 2 x max_features plus a 96-byte control block on first use.  EKF_ERR_INVALID_ARG on a
 * sharded engine. */
int ekf_set_consistency(EkfEngine *e, int on);
/* the updates recorded since the last step or ekf_update began: 0 to 2 records, in the order they ran.  The getters below
 * synchronise the stream and report a pending asynchronous error as ekf_get_state does.  out may be NULL (count only);
 * capacity < *count -> EKF_ERR_CAPACITY with *count = number needed. */
int ekf_get_consistency(EkfEngine *e, EkfUpdateConsistency *out, int capacity, int *count);
/* the matches of record `which` of ekf_get_consistency, in the update's order */
int ekf_get_innovations(EkfEngine *e, int which, EkfInnovation *out, int capacity, int *count);
/* sums over every update recorded since the engine was created or the totals were last reset, added on the device in the
 * order the updates ran (two runs give the same bits); any pointer may be NULL */
int ekf_get_consistency_totals(EkfEngine *e, double *nis_sum, int64_t *rows_sum, int64_t *updates);
int ekf_reset_consistency_totals(EkfEngine *e);

/* Measurement budget (opt-in; K = 0, the default, is off: no extra launch, allocation or read-back, every result bit for bit).
 * With 0 < K < number of map features, the full prediction of ekf_step, ekf_step_frame, ekf_step_image and
 * ekf_step_staged_image (both image matchers) ranks the features it sees by the information their measurement carries,
 * 0.5 ln(det S_i / det R) -- with R = pixelErrorX I the ranking of det S_i, formed in fp64 from 13 x 13 entries of P per
 * feature -- and hands the K best on, in feature order: only they get H P rows, are searched for, enter RANSAC, the updates,
 * the rescue and the consistency records, and only their timesPredicted / timesMatched move (removeBadMapFeatures' ratio is
 * then over the frames a feature was searched in).  EkfStepInfo.n_predicted = min(predicted, K).  What describes the whole
 * prediction is unchanged: ekf_get_unseen_features (a visible, unselected feature is not unseen), ekf_get_step_predictions
 * and the gates behind ekf_detect_new_features and the keypoint detector cover every predicted feature.  With K >= number
 * of map features the budget cannot bind and the step is today's.  An active budget puts ekf_step on the path that reads the
 * counts back after each stage (as ekf_keep_step_predictions does).  ekf_predict_measurements and the other stage calls
 * ignore the budget.  Allocates 48 bytes x max_features on the first call with K > 0.  K < 0, or K > 0 on a sharded engine:
 * EKF_ERR_INVALID_ARG, nothing changes.  DESIGN.md 4.12. */
int ekf_set_measurement_budget(EkfEngine *e, int K);
/* one record per feature predicted by the last step, in feature order, if the budget was active in it; *count = 0 otherwise.
 * The records stay on the device until asked for.  Synchronises the stream and reports a pending asynchronous error as
 * ekf_get_state does.  out may be NULL (count only); capacity < *count -> EKF_ERR_CAPACITY with *count = number needed. */
int ekf_get_measurement_ranks(EkfEngine *e, EkfMeasurementRank *out, int capacity, int *count);
/* the last step's full prediction: features predicted and features handed on (equal when the budget did not bind); either
 * pointer may be NULL */
int ekf_get_measurement_budget_counts(const EkfEngine *e, int *predicted, int *selected);

/* External measurements: an EKF update with any linearised measurement, between steps.  H is given by rows in
 * CSR form over STATE indices -- the indices of P: 0..12 the camera (r, q, v, w), covpos + k parameter k of a feature
 * (ekf_get_feature_layout) -- with row i holding the entries row_start[i] .. row_start[i + 1] - 1 of col / val, 1 to
 * EKF_EXT_MAX_NNZ of them, columns strictly ascending; m = 1 .. EKF_EXT_MAX_ROWS rows.  residual = z - h(x) as the caller
 * linearised it; R is m x m row-major and only its upper triangle is read.  With S = H P H' + R = L L':
 *     z = inv(L) residual,  nis = z'z,  B = inv(L) H P,  x += B'z (dead-band EKF_DELTA per component, then the quaternion is
 *     normalised),  P <- 0.5 (P + P') - B'B, then normalizeCovariance as after every update (EKF/Update.cpp:64-85, 303-312)
 * in fp64 whatever the precision configuration; P is rounded to its storage type once per step and is bitwise symmetric
 * afterwards.  gate_nis > 0: the update is applied only if nis <= gate_nis (else EKF_OK with out->applied = 0 and nothing
 * changed); 0: no gate.  S not positive definite: EKF_ERR_NOT_POSITIVE_DEFINITE, nothing changed.  The tables of the last
 * prediction are left as they are (as after ekf_update: a caller of the stage functions predicts again); no consistency
 * record is written (the NIS comes back in out, which may be NULL).  Reports a pending asynchronous error first, as
 * ekf_get_state does, and then does nothing else.  Synchronises the stream.  EKF_ERR_INVALID_ARG, with nothing enqueued: m or
 * a row's length out of range, columns not strictly ascending or outside the state, a non-finite value, gate_nis < 0 or NaN,
 * a sharded engine. */
int ekf_update_external(EkfEngine *e, int m, const int32_t *row_start /* m + 1 */, const int32_t *col, const double *val,
                        const double *residual /* m */, const double *R /* m x m */, double gate_nis,
                        EkfExternalUpdate *out /* may be NULL */);
/* a fix r of the camera position with covariance R (3 x 3 row-major, upper triangle read): H = [I3 0 ...], residual = r - x[0:3] */
int ekf_fuse_camera_position(EkfEngine *e, const double r[3], const double R[9], double gate_nis, EkfExternalUpdate *out);
/* a measured distance between two map features (what fixes the monocular scale): h = |X_i - X_j| with X the world point of
 * ekf_get_map_points, one row u' Jw_i on feature i's columns and -u' Jw_j on feature j's (u = (X_i - X_j) / h, Jw = dX/dy),
 * residual = distance - h, R = sigma^2.  EKF_ERR_INVALID_ARG: feat_i == feat_j, an index out of range, h = 0, sigma <= 0,
 * distance <= 0. */
int ekf_fuse_feature_distance(EkfEngine *e, int feat_i, int feat_j, double distance, double sigma, double gate_nis,
                              EkfExternalUpdate *out);

/* Localisation on a fixed map: the Schmidt-Kalman ("consider") update.  The gain rows of the map states are
 * zero; the map still enters S = H P H' + R with its full uncertainty and its correlations, and only the camera state and the
 * camera's rows and columns of P move.  With B = inv(L) H P, B_c its first 13 columns and z = inv(L) nu:
 *     x[0:13]   += B_c' z   (dead-band EKF_DELTA per component, then the quaternion is normalised)
 *     P[0:13,:] <- (0.5 P + 0.5 P')[0:13,:] - B_c' B,   P[:,0:13] = its transpose,   then normalizeCovariance on rows / columns 3..6
 * -- the camera strip of the full update and nothing else: P stays a valid joint covariance, never smaller than the full update's
 * result, and mapping can resume from it.  P[13:,13:], the feature parameters, their types and the layout are not written at all
 * (an uploaded asymmetric map block stays asymmetric and is still symmetrised by the next full update).  The n x n x m downdate
 * is not launched: what is left behind the Cholesky sweep is a 13 x n strip (above 2048 measurement rows, and on maps of 8192 state
 * columns or more, B is not formed either: the inverse of L and two m x 13 tables).  fp64 arithmetic in every supported configuration; P
 * is rounded to its storage type after the downdate and after the normalisation, as by ekf_update_external; the 13 x 13 block is
 * bitwise symmetric afterwards and P[j][i] == P[i][j] bitwise for i < 13.
 *
 * ekf_update_fixed_map is the stage, whatever the mode: arguments, validation, preconditions (one match per featureIndex, the
 * predictions of the last full ekf_predict_measurements) and failure as ekf_update -- S not positive definite returns
 * EKF_ERR_NOT_POSITIVE_DEFINITE with nothing changed, a timed-out persistent sweep is run again on the launch-per-panel sweep;
 * S, L, nu, z and therefore the consistency record (stage 0 here, 1 or 2 inside a step) are those of ekf_update on the same
 * inputs.  The tables of the last prediction are left as after ekf_update.  ekf_set_update_path and ekf_set_sweep_mode reach it.
 *
 * ekf_set_fixed_map with on != 0 turns BOTH covariance updates inside ekf_step, ekf_step_frame, ekf_step_image and
 * ekf_step_staged_image into fixed-map updates.  Prediction, matching, RANSAC (its hypotheses keep the full gain: selection is
 * unchanged), the rescue and the bookkeeping of the map features (descriptors, timesPredicted, timesMatched) run as always; a step
 * gains no read-back and no allocation, ekf_set_async_errors, ekf_set_consistency and ekf_set_measurement_budget work unchanged.
 * The mode can be switched between frames; off is the engine without it, bit for bit.  NOT affected by the mode: ekf_update,
 * ekf_update_only_state, ekf_update_external with its two helpers, and map management (add, remove, convert) -- a caller who
 * fuses a position fix or adds features while the mode is on moves the map and should know it.
 *
 * EKF_ERR_INVALID_ARG with nothing changed, for the stage and for the setter with on != 0: a sharded engine, and
 * EKF_PRECISION_F32 (the fast configuration: its fp32 rows of B with the fp64 repair of the camera rows are a separate design;
 * AUTO never resolves to it).  The first use allocates 256 bytes of scratch per measurement row of the engine's capacity.
 * ekf_get_fixed_map: the mode, and the fixed-map updates applied since the engine was created (counted on the device; asking
 * for it synchronises the stream); either pointer may be NULL. */
int ekf_update_fixed_map(EkfEngine *e, const EkfMatch *matches, int M);
int ekf_set_fixed_map(EkfEngine *e, int on);
int ekf_get_fixed_map(const EkfEngine *e, int *on, int64_t *updates);

/* Relocalisation on the map (no counterpart in the reference).  Every matcher of a step searches inside the gate
 * of the PREDICTED measurement, so a filter whose camera pose is far off -- tracking lost, or a map loaded for a session that starts
 * somewhere else -- never recovers by stepping.  ekf_relocalise finds the pose from the map and one frame's keypoints alone:
 *   1. every depth feature takes part, and every inverse-depth feature with rho > 0 and (max_rel_depth_sd == 0 or
 *      sqrt(P[rho,rho]) / rho <= max_rel_depth_sd), as the world point ekf_get_map_points reports;
 *   2. such a feature becomes a candidate when its smallest Hamming distance d1 over ALL keypoints (ties: the lower keypoint index)
 *      is <= max_distance and (second_best_coef == 0 or d1 < second_best_coef * d2), d2 the smallest over the other keypoints;
 *   3. hypothesis h = 0 .. hypotheses - 1 takes three candidates by splitmix64(seed + 3 h + k) mod C, solves P3P in closed form, scores
 *      every solution against every candidate with the filter's own projection (inlier: predicted, and squared pixel error <=
 *      inlier_px^2) and keeps its best: most inliers, then the smaller sum of squared inlier errors, then the lower solution index;
 *   4. the best hypothesis by the same order (ties: the lowest h) is the result; found = its inliers >= min_inliers.
 * With found and install != 0 the pose becomes the camera state (velocities as after ekf_reset), the camera's rows and columns of P
 * become diag(sigma_position^2 x3, sigma_angle^2 / 4 x4, initLinearAccelSD^2 x3, initAngularAccelSD^2 x3) with zero cross terms, and
 * the prediction tables are stale as after ekf_set_state: predict again.  The features, their block of P and every per-feature
 * table are not written.  Without found, or with install == 0, nothing of the filter changes.  The pose is not refined: the filter's
 * next step does that.
 *
 * ekf_relocalise takes n_kp keypoints with 32-byte descriptors from the host (n_kp = 0 is allowed); ekf_relocalise_image detects and
 * describes them on the current image (ekf_image_upload; unmasked, threshold min_response, at most max_keypoints of them), and
 * their count stays on the device.  Both synchronise the stream; a pending asynchronous error (ekf_set_async_errors) is reported
 * first and nothing else is done, as ekf_update_external does.  Fewer than 3 candidates, or no valid hypothesis, is EKF_OK with
 * found = 0.  EKF_ERR_INVALID_ARG with a message and nothing enqueued: a parameter outside the range stated in EkfRelocParams (NaN
 * included), n_kp < 0 or > max_keypoints, a sharded engine, an engine that is not EKF_DESCRIPTOR_U8_HAMMING.  The first call
 * allocates the scratch: about 120 bytes per feature of the engine's capacity and 88 bytes per hypothesis of the maximum.
 *
 * ekf_get_relocalise_candidates / _hypotheses: the candidate list (ascending feature order; inlier_mask, which may be NULL, marks
 * the inliers of the best hypothesis) and the hypothesis records of the last call; *count is always set, out may be NULL to ask for
 * it, and capacity < *count is EKF_ERR_CAPACITY (the convention of ekf_get_consistency). */
int ekf_relocalise(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, const EkfRelocParams *params,
                   EkfRelocResult *out);
int ekf_relocalise_image(EkfEngine *e, double min_response, const EkfRelocParams *params, EkfRelocResult *out);
int ekf_get_relocalise_candidates(EkfEngine *e, EkfMatch *out, uint8_t *inlier_mask, int capacity, int *count);
int ekf_get_relocalise_hypotheses(EkfEngine *e, EkfRelocHypothesis *out, int capacity, int *count);

/* Iterated EKF update (opt-in: with 1 pass everything is the engine without it, bit for bit).  Gauss-Newton on
 * the update's own MAP cost: the camera measurement is linearised again at the new estimate and the update is solved again from
 * the PRIOR.  With x^, P the state and covariance before the update, z the matched pixels, R = pixelErrorX I and x^0 = x^, pass
 * i = 0 .. K - 1 forms
 *     h_i, H_i = the predictions and Jacobians of the matched features at x^i (P is still the prior)
 *     nu_i     = z - h_i - H_i (x^ - x^i)      (plain differences of the stored parameters, the quaternion included)
 *     S_i      = H_i P H_i' + R,   x^(i+1) = x^ + P H_i' inv(S_i) nu_i
 * The passes before the last are state-only updates (q is not normalised, P is not touched, as ekf_update_only_state); the last is
 * the covariance update P+ = sym(P) - B'B with B = inv(L) H_(K-1) P, followed by the normalisation of q and its Jacobian on P.  The
 * dead-bands of ekf_update apply to nu_i and to the whole step from x^.  iterations = 1 is ekf_update, bit for bit.
 *
 * The iteration ends early, and the pass that then runs is the covariance pass: (tol > 0) once a pass moved no state by tol standard
 * deviations of the prior -- step[i] < tol -- and when a matched feature is not predicted at x^i (it left the image): the update is
 * then finished from the last linearisation point at which every match was predicted.  Undamped Gauss-Newton need not contract
 * (large innovations on a fresh map): the per-pass steps of the record show it.
 *
 * ekf_update_iterated: the stage; arguments, validation, preconditions and failure as ekf_update (S of a pass not positive
 * definite: EKF_ERR_NOT_POSITIVE_DEFINITE, x and P as before the call, the remaining passes not run).  iterations 1 ..
 * EKF_MAX_UPDATE_ITERATIONS, tol >= 0 and finite.  ekf_set_update_iterations: the mode of ekf_step, ekf_step_frame, ekf_step_image
 * and ekf_step_staged_image -- both updates of a step are iterated; such a step reads its counts back after every stage (as with
 * ekf_keep_step_predictions) and launches no early gather.  Default 1, 0.  Filter consistency (ekf_set_consistency) records the
 * covariance pass alone, with nu_(K-1).  After an iterated update the prediction tables of the matched features (what
 * ekf_predict_measurements left) hold the predictions, Jacobians and H P rows at x^(K-1).
 *
 * EKF_ERR_INVALID_ARG with a message and nothing written: a sharded engine; iterations outside 1 .. 8; tol < 0 or not finite;
 * iterations > 1 while the fixed-map mode is on, and ekf_set_fixed_map(on) while iterations > 1 (the fixed-map update has no
 * state-only form).  EKF_PRECISION_F32 is allowed.  The first use allocates 212 bytes per feature of the engine's capacity.
 *
 * ekf_get_iteration_records: one record per iterated update of the last ekf_update_iterated or step (0 .. 2, in the order they
 * ran; a step with iterations = 1 keeps none).  ekf_get_linearisation_point: x^(K-1) of the last iterated update -- the 13 camera
 * values and 6 doubles per feature of the map as it is now, ekf_num_features (feature_pos may be NULL); EKF_ERR_INVALID_ARG before
 * the first, and again once the map was replaced or its layout changed (ekf_set_state, ekf_load_map, ekf_reset, features added,
 * removed or converted): the point described the map that was.  Both synchronise the stream.
 * out may be NULL (count only); capacity < *count -> EKF_ERR_CAPACITY with *count = number needed.
 * A record whose pass failed: stop_reason = failed, passes_run = the passes that ran before it, x and P as before the update.  Inside a
 * step, the covariance pass of the second update is retried (a timed-out persistent sweep) or found failed only at the step's last
 * read-back: step[passes_run - 1] of that record was then taken from the frozen state and is |x^ - x^(K-1)|, and a failure shows in
 * EkfStepInfo.status, not in the record. */
int ekf_update_iterated(EkfEngine *e, const EkfMatch *matches, int M, int iterations, double tol);
int ekf_set_update_iterations(EkfEngine *e, int iterations, double tol);
int ekf_get_update_iterations(const EkfEngine *e, int *iterations, double *tol);
int ekf_get_iteration_records(EkfEngine *e, EkfIterationRecord *out, int capacity, int *count);
int ekf_get_linearisation_point(EkfEngine *e, double x13[13], double *feature_pos);

/* -- stages ---------------------------------------------------------------------------------------------- */
/* stateAndCovariancePrediction(State&, Matd&)            EKF/StateAndCovariancePrediction.h:41 (.cpp:244-253) */
int ekf_predict(EkfEngine *e);

/* Frame intervals.  The reference predicts over dt = 1 (StateAndCovariancePrediction.cpp:246); here the interval
 * is a number: r += v dt, q <- q (x) quat(w dt), Q = diag(SD^2 dt^2).  One unit is the period linearAccelSD and angularAccelSD
 * were tuned for -- the nominal frame period -- so a frame that follows k dropped ones gets dt = k + 1.  One prediction over
 * dt = 2 is not two over dt = 1: the velocity impulse is drawn once per prediction.
 * ekf_set_frame_interval: the interval ekf_predict and every step function (ekf_step, ekf_step_frame, ekf_step_image,
 * ekf_step_staged_image) use from now on.  Default 1.0, with which every result is bit for bit that of an engine that was never
 * told an interval.  ekf_predict_dt: one prediction over dt; the set interval is left alone.
 * ekf_set_staged_intervals: per-index intervals of a pre-staged sequence, kept on the host (the value reaches the kernel as an
 * argument: no copy, no synchronisation per frame).  ekf_step_frame(i) and ekf_step_staged_image(i) use dt[i] for i < n and the
 * set interval otherwise; n = 0 clears the table (dt may then be NULL).
 * EKF_ERR_INVALID_ARG, with a message in ekf_last_error, nothing launched and nothing changed: a dt -- or any entry of a table --
 * that is not finite or not greater than 0; n < 0; n > 0 with dt NULL.
 * A sharded engine accepts all of these; EVERY rank must be given the same value (the prediction is replicated arithmetic on the
 * camera rows: with equal intervals P[a][j] on one rank stays bitwise P[j][a] on the owner of row j, as with dt = 1).  The fixed
 * map, the measurement budget, consistency and the NCC options are independent of the interval. */
int ekf_set_frame_interval(EkfEngine *e, double dt);
int ekf_get_frame_interval(const EkfEngine *e, double *dt);
int ekf_predict_dt(EkfEngine *e, double dt);
int ekf_set_staged_intervals(EkfEngine *e, int n, const double *dt);
/* Look-ahead of the camera: the camera state (x13: r, q, v, w) and the 13 x 13 camera covariance F P_cc F' + G Q G' (row-major)
 * a prediction over tau would leave, WITHOUT making it -- where will the camera be tau from now, and how sure is the filter
 * (latency compensation for rendering or control).  One one-workgroup launch, fp64, from the current state and the camera corner
 * of P, with the operations of ekf_predict_dt(tau) in its order: P13 is the value that prediction rounds to the storage type of P
 * (in the fp64-stored configurations: the corner it leaves, bit for bit).  Read-only: the kernel writes its own 182-double
 * buffer (allocated at creation) and nothing else -- not the state, not P, no per-frame table.  Either output may be NULL.
 * Synchronises the stream.  tau is validated as dt above.  On a sharded engine the camera rows are replicated: any rank answers. */
int ekf_predict_camera_ahead(const EkfEngine *e, double tau, double x13[13], double P13[169]);

/* predictCameraMeasurements(state, P, features, featureIndexes, preds, jacobians, notPredicted)
 *                                                        EKF/MeasurementPrediction.h:59 (.cpp:705-719)
 * feat_idx == NULL / count == 0 predicts every map feature.  Outputs (all optional): predictions in input order,
 * Hs (2x13 doubles each) and Hf (2x6 doubles each) Jacobian blocks. */
int ekf_predict_measurements(EkfEngine *e, const int32_t *feat_idx, int count, EkfPrediction *preds, int *n_preds,
                             double *Hs, double *Hf);

/* predictMeasurementState(state, features, featureIndexes, preds, notPredicted)
 *                                                        EKF/MeasurementPrediction.h:41 (.cpp:203-265)
 * on the engine's current state, all features; no Jacobians, device tables untouched. */
int ekf_predict_measurement_state(EkfEngine *e, EkfPrediction *preds, int *n_preds);

/* matchPredictedFeatures(image, features, predictions, matches)   EKF/Matching.h:66 (.cpp:181-264),
 * the stage downstream of the detector/descriptor (ellipse gate + descriptor distance + 2-best selection,
 * .cpp:217-262) for the keypoints of this frame, against the predictions of the last full
 * ekf_predict_measurements call. */
int ekf_match(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, EkfMatch *matches,
              int *n_matches);

/* ransac(state, P, preds, jacobians, matches, inliers, inlierPreds, inlierJacobians, outliers)
 *                                                        EKF/1PointRansac.h:42 (.cpp:101-234)
 * inlier_mask[i] = 1 for matches kept as low-innovation inliers.  n_hypotheses (optional) = hypotheses the
 * sequential reference loop would have evaluated. */
int ekf_ransac(EkfEngine *e, const EkfMatch *matches, int M, uint8_t *inlier_mask, int *n_hypotheses);
/* ekf_ransac / ekf_update / ekf_update_only_state / ekf_rescue: at most ONE match per featureIndex (what
 * matchPredictedFeatures produces); a list with a repeated featureIndex returns EKF_ERR_INVALID_ARG. */

/* update(state, P, matches, preds, jacobians)            EKF/Update.h:48 (.cpp:282-319) */
int ekf_update(EkfEngine *e, const EkfMatch *matches, int M);

/* updateOnlyState(preds, matches, jacobians, state, P)   EKF/Update.h:42 (.cpp:269-275) */
int ekf_update_only_state(EkfEngine *e, const EkfMatch *matches, int M);

/* rescueOutliers(outlierMatches, preds, jacobians, rescued...)    EKF/EKF.cpp:68-119
 * against the predictions of the last ekf_predict_measurements call that covered those features. */
int ekf_rescue(EkfEngine *e, const EkfMatch *outliers, int M, uint8_t *rescued_mask);

/* EKF::step(image) with a fixed map                      EKF/EKF.h:57 (.cpp:242-572, including updateMapFeatures),
 * fed the frame's keypoints.  Its prediction runs over the interval of ekf_set_frame_interval (default 1). */
int ekf_step(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, EkfStepInfo *info);

/* -- pre-staged sequences (inputs resident in HBM before a timed region) ---------------------------------- */
int ekf_frames_upload(EkfEngine *e, int n_frames, const int32_t *kp_counts, const EkfKeypoint *kps_concat,
                      const uint8_t *desc_concat);
int ekf_step_frame(EkfEngine *e, int frame, EkfStepInfo *info);
/* on: ekf_step / ekf_step_frame return without the final read-back of the error flag (they then return as soon as the
 * second update is ENQUEUED).  A failed factorisation of that update (EKF_ERR_NOT_POSITIVE_DEFINITE) is reported by the
 * next ekf_step*, ekf_synchronize or ekf_get_state, whichever comes first (the flag is sticky on the device until one of
 * them reports and clears it) -- the reference reports nothing at all (cv::invert returns zeros).  Default off. */
int ekf_set_async_errors(EkfEngine *e, int on);
/* How an update forms B = inv(L) (H P), the factor of the covariance downdate (replaces K = P H' inv(S),
 * EKF/Update.cpp:105-108): EKF_UPDATE_PATH_AUTO by the number of measurement rows (the default), EKF_UPDATE_PATH_SWEEP
 * always inside the launches of the Cholesky sweep (forward substitution, no explicit inverse), EKF_UPDATE_PATH_GEMM
 * always by inverting L and one GEMM.  Same result to rounding; a tuning / test knob. */
enum { EKF_UPDATE_PATH_AUTO = 0, EKF_UPDATE_PATH_SWEEP = 1, EKF_UPDATE_PATH_GEMM = 2 };
int ekf_set_update_path(EkfEngine *e, int path);
/* How the blocked Cholesky sweep of S (replaces S.inv(), EKF/Update.cpp:108) is launched: EKF_SWEEP_SINGLE one 32-row panel per
 * launch, EKF_SWEEP_PAIRS two panels per launch with a 64 x 64 look-ahead inverse, EKF_SWEEP_PERSISTENT ONE launch per update
 * (a resident critical workgroup factorises panel after panel, tile and row-block workers follow it through flags; updates of at
 * most 2048 rows on an unsharded engine in the fp64 and the exact configuration whose grid fits the device, otherwise launches as
 * under AUTO; a sweep whose waits time out is run again on the launch-per-panel path, see ekf_get_sweep_retries),
 * EKF_SWEEP_LAUNCHES the round-4 rule (single launches while a launch is bound by its look-ahead factorisation, pairs once the
 * rows of B = inv(L) H P are the longest role), EKF_SWEEP_AUTO (the default): persistent where it applies AND the map has fewer
 * than 8192 state columns (above, its row-block workers take several blocks of columns each and two panels per launch are faster:
 * N = 2000, 14.0 against 20.4 us per panel), else LAUNCHES.  Same result to rounding; a tuning / test knob. */
enum { EKF_SWEEP_PAIRS = 0, EKF_SWEEP_SINGLE = 1, EKF_SWEEP_AUTO = 2, EKF_SWEEP_PERSISTENT = 3, EKF_SWEEP_LAUNCHES = 4 };
int ekf_set_sweep_mode(EkfEngine *e, int mode);

/* -- matcher mode B: image in, no detector ----------------------------------------------------------------
 * matchPredictedFeatures(const cv::Mat &image, ...)  EKF/Matching.h:66 and EKF::step(const cv::Mat &image)
 * EKF/EKF.h:57 take the frame itself.  Mode B keeps that signature: the frame is uploaded (1, 3 = BGR or
 * 4 = RGBA bytes per pixel, as Img/FileSequenceImageGenerator.cpp:82 and android jni/EKFNative.cpp:163 deliver
 * it), reduced to a 3-level gray pyramid on the device, and each predicted feature is matched by zero-mean NCC
 * of its 11x11 template inside the predicted ellipse (gate of Matching.cpp:217-241), coarse to fine.  The coarse
 * level looks at most 16 coarse pixels (about 66 px) away from the prediction: a gate whose major semi-axis is 64 px
 * or more is searched only that far unless ekf_set_ncc_wide_search (below) is on.  The
 * reference has no such matcher (it runs an OpenCV detector + descriptor on the host, Matching.cpp:188-210);
 * the definition is this build's and is restated on the CPU in oracle/ekf_oracle.c for the parity tests.
 * Matches carry keypointIndex = -1 and integer pixel positions (sub-pixel positions with ekf_set_subpixel_matches,
 * below); templates are captured once and kept. */
int ekf_image_upload(EkfEngine *e, const uint8_t *image, int width, int height, int stride, int channels);
int ekf_get_image_level(EkfEngine *e, int level, uint8_t *out, int *width, int *height); /* readback for tests */
/* templates of the listed map features, cut from the CURRENT image around uv (the pixel a feature was
 * initialised at: addFeaturesToStateAndCovariance keeps the descriptor there, EKF/AddMapFeature.cpp:317-337) */
int ekf_capture_templates(EkfEngine *e, const int32_t *feat_idx, const double *uv, int count);
int ekf_match_ncc(EkfEngine *e, EkfMatch *matches, int *n_matches);
/* Predicted appearance (opt-in; off: the path above, bit for bit).  A template is treated as a small plane through the
 * feature's world point that faces the camera which captured it; with the mode on, a capture also keeps a 41x41 source
 * patch per pyramid level and the capture pose, and every NCC search compares a template re-rendered from the current
 * pose estimate.  A level whose samples leave the source patch, or a feature captured with the mode
 * off (or present at ekf_set_state), uses the stored template.  Allocates 3 x 1681 + 363 bytes + 9 doubles per feature
 * of capacity on first use; turning it off keeps the tables.  EKF_ERR_INVALID_ARG on a sharded engine;
 * EKF_IMAGE_MATCHER_KEYPOINTS ignores the mode. */
int ekf_set_template_warp(EkfEngine *e, int on);
/* levels re-rendered / fallen back in the last NCC match: 3 x predictions in total with the mode on, 0 and 0 with it off */
int ekf_get_template_warp_counts(const EkfEngine *e, int *warped_levels, int *fallback_levels);
/* the 3 x 121 bytes the last NCC match compared for the listed features (features it did not predict: the stored
 * template).  The re-rendered table is not carried through a change of the map: after ekf_add_features, a removal, a
 * conversion, ekf_set_state or ekf_reset, and until the next match, the stored templates are returned.  Readback for tests */
int ekf_get_match_templates(EkfEngine *e, const int32_t *feat_idx, int count, uint8_t *tmpl363);
/* Sub-pixel matches (opt-in; off: integer pixels as above, bit for bit).  With the mode on, each axis of a match's
 * imagePos is the vertex of the parabola through the ZNCC^2 keys of the best level-0 pixel and its two neighbours on
 * that axis, compared against the template the search compared (the re-rendered one with the template warp):
 *     a = km - kp,  b = (km - 2 k0) + kp,  offset = (0.5 a) / b clamped to [-0.5, 0.5],  pos = (float)((double)best + offset)
 * in fp64, on the device.  An axis stays at the integer when a neighbour's centre is outside the frame,
 * a neighbour has no score or scores above the best pixel, or b >= 0.  Which features match, their order, the gate test
 * (on the integer pixel) and the distances do not change.  EKF_ERR_INVALID_ARG on a sharded engine;
 * EKF_IMAGE_MATCHER_KEYPOINTS ignores the mode. */
int ekf_set_subpixel_matches(EkfEngine *e, int on);
/* axes of the last NCC match's matches that the fit moved / that stayed at the integer: 2 x matches in total with the
 * mode on, 0 and 0 with it off */
int ekf_get_subpixel_counts(const EkfEngine *e, int *refined_axes, int *integer_axes);
/* Wide search (opt-in; off: the path above, bit for bit).  With the mode on, a prediction whose gate exceeds the coarse
 * window -- (major semi-axis >> 2) + 1 > 16, i.e. a major semi-axis of 64 px or more -- has its coarse level searched
 * over the whole gate within the frame, as the default search would with an unbounded window: same candidates rule, same
 * key, ties to the first pixel in raster order; then the same two finer levels, acceptance test and optional sub-pixel
 * fit.  Predictions whose gate fits the window keep the default path's result, bit for bit.  Takes
 * effect with the next match (ekf_step_image, ekf_step_staged_image, ekf_match_ncc); composes with the two modes above.
 * EKF_ERR_INVALID_ARG on a sharded engine; EKF_IMAGE_MATCHER_KEYPOINTS ignores the mode. */
int ekf_set_ncc_wide_search(EkfEngine *e, int on);
/* of the last NCC match: predictions searched wide, and the coarse candidates evaluated for them (saturating at
 * INT_MAX); 0 and 0 with the mode off */
int ekf_get_ncc_wide_counts(const EkfEngine *e, int *wide_slots, int *wide_candidates);
/* Distinctiveness test (opt-in; coef = 0 is off and the default: the path above, bit for bit).  With 0 < coef <= 1 an NCC
 * match is accepted only if no second place in its gate scores nearly as well.  The rival is the best
 * coarse candidate of the same search (same candidates, capped or wide) outside the 5 x 5 coarse pixels around the coarse
 * best, first in raster order among equals, refined through the same two finer levels against the same templates; it
 * counts only if its refined key is not negative and its pixel lies in the gate.  With d1 = (float)(1 - sqrt(key)) of the
 * best (the match's distance) and d2 that of the rival, a match with a rival is kept when (double)d1 < (double)d2 * coef,
 * strictly: two perfect repetitions (0 against 0) are ambiguous.  A rejected match leaves the list; the matches that stay,
 * their positions, distances and order do not change, and the sub-pixel counts cover them only.  Takes effect with the
 * next match (ekf_step_image, ekf_step_staged_image, ekf_match_ncc); composes with the modes above.  EKF_ERR_INVALID_ARG
 * for a coef outside [0, 1] (NaN included; nothing changes) and for a non-zero coef on a sharded engine;
 * EKF_IMAGE_MATCHER_KEYPOINTS ignores the mode.  Allocates 20 bytes per feature of capacity on first use. */
int ekf_set_ncc_distinct(EkfEngine *e, double coef);
/* of the last NCC match: accepted matches that had a rival, and those of them the test rejected; 0 and 0 with the mode off */
int ekf_get_ncc_distinct_counts(const EkfEngine *e, int *with_rival, int *rejected);
/* one record per prediction slot of the last NCC match, in slot order (the order of its predictions); *count receives
 * their number, 0 with the mode off or before the first such match.  EKF_ERR_INVALID_ARG if capacity is smaller */
int ekf_get_ncc_rivals(EkfEngine *e, EkfNccRival *out, int capacity, int *count);
/* Patch normals (opt-in; off: the path above, bit for bit; needs the template warp).  The warp's patch plane faces the
 * camera that captured the feature; with this mode on each feature's plane has a slope (p, q) in that camera's axes --
 * normal n = R(q0) (p, q, -1) / |(p, q, -1)| in world axes -- estimated on the device by aligning the stored source
 * patches to the current frame: ekf_step_image / ekf_step_staged_image run one estimator step per frame,
 * after the frame's last update, for the features that ended it as inliers or rescued, and the warp renders a feature
 * that has an estimate with it.  A feature without an estimate (updates = 0: fresh capture, re-capture, no step yet)
 * warps exactly as with the template warp alone.  Allocates 48 + 32 bytes per feature of capacity on first use.
 * EKF_ERR_INVALID_ARG on a sharded engine and while the template warp is off; ekf_set_template_warp(e, 0) turns this
 * mode off too; EKF_IMAGE_MATCHER_KEYPOINTS ignores the mode. */
typedef struct EkfPatchNormal {
    double pq[2];     /* slope of the patch plane in the capture camera's axes */
    double info[3];   /* its information matrix: (0,0), (0,1), (1,1) */
    double normal[3]; /* unit normal in world axes */
    int32_t updates;  /* estimator steps taken; 0: no estimate, pq / normal are the facing-the-camera rule, info the prior */
    int32_t pad;
} EkfPatchNormal;
int ekf_set_patch_normals(EkfEngine *e, int on);
/* one estimator step, as a stage of its own, on the current image and state: matches[i].imagePos (rounded to whole
 * pixels) is where feature matches[i].featureIndex is seen; a feature may be listed once */
int ekf_refine_patch_normals(EkfEngine *e, const EkfMatch *matches, int M);
/* a feature without a source patch reports zeros */
int ekf_get_patch_normals(EkfEngine *e, const int32_t *feat_idx, int count, EkfPatchNormal *out);
/* sets a feature's estimate (tests; restoring a saved map); its update count becomes at least 1 */
int ekf_set_patch_normal(EkfEngine *e, int feat, const double pq[2], const double info[3]);
/* features updated / left alone by the last estimator run (a step with the mode on, or ekf_refine_patch_normals) */
int ekf_get_patch_normal_counts(const EkfEngine *e, int *updated, int *skipped);
int ekf_step_image(EkfEngine *e, const uint8_t *image, int width, int height, int stride, int channels,
                   EkfStepInfo *info); /* (matcher: ekf_set_image_matcher) */
/* detectNewImageFeatures(image, featuresPrediction, newImageFeaturesMaxSize, newImageFeatures)
 *                                                              EKF/DetectNewImageFeatures.cpp:337
 * on the CURRENT image, masked by the gate ellipses of the last full prediction made while an image was loaded
 * (buildImageMask :102).  The detector is this build's own (integer Harris-type measure, best unmasked pixel per
 * 16x16 cell, kernels_detect.hip; the reference's OpenCV STAR is third-party code that is not here); the zone
 * heuristic is the reference's searchFeaturesByZone (:171) with rand() replaced by "strongest candidate of the
 * zone".  divide_times = DetectNewFeaturesImageAreasDivideTimes, mask_ellipse_size =
 * DetectNewFeaturesImageMaskEllipseSize, min_response = detector threshold on the integer measure.
 * Writes up to max_new pixel positions (x, y) to uv_out; the caller then adds them (ekf_add_features) and cuts their
 * templates (ekf_capture_templates). */
int ekf_detect_new_features(EkfEngine *e, int max_new, int divide_times, double mask_ellipse_size,
                            double min_response, double *uv_out, int *count);

/* pre-staged image sequence (n_frames images of identical geometry, concatenated) */
int ekf_images_upload(EkfEngine *e, int n_frames, const uint8_t *images, int width, int height, int stride,
                      int channels);
int ekf_select_staged_image(EkfEngine *e, int frame); /* build the pyramid of a staged frame */
int ekf_step_staged_image(EkfEngine *e, int frame, EkfStepInfo *info);

/* -- image in, descriptor matcher: keypoint detector + BRIEF-32 on the device ---------------------------------
 * The reference's shipped matcher, STAR keypoints + BRIEF-32 + Hamming distance (EKF/Matching.cpp:188-210), with this
 * build's own detector and descriptor in front of the matcher of ekf_match (no bit-parity with
 * OpenCV's STAR or its BRIEF pattern is claimed):
 *   keypoint   the integer corner measure of ekf_detect_new_features, R >= min_response, >= 16 px from every edge,
 *              5x5 non-maximum suppression (strictly above the window's earlier pixels in raster order, >= the later ones);
 *   BRIEF-32   256 tests S(c + a_i) < S(c + b_i) on the pairs of csrc/brief_pattern.h (offsets in [-19, 19]), S = sum of
 *              the 9x9 gray box, reads clamped to the frame; test i sets bit 7 - i % 8 of byte i / 8.
 * Keypoints are listed in raster order (y, then x) at integer pixels. */
enum { EKF_IMAGE_MATCHER_NCC = 0, EKF_IMAGE_MATCHER_KEYPOINTS = 1 };
/* how ekf_step_image / ekf_step_staged_image match: NCC templates (default, unchanged) or detector + BRIEF-32 + the Hamming
 * matcher of ekf_match; KEYPOINTS needs an EKF_DESCRIPTOR_U8_HAMMING, unsharded engine (else EKF_ERR_INVALID_ARG) */
int ekf_set_image_matcher(EkfEngine *e, int matcher, double min_response);
/* detector + descriptors on the CURRENT image; masked = 1: inside the gates of the last full prediction, 0: whole frame.
 * Writes min(found, capacity) keypoints in raster order; *n_found = found. kps / desc32 may be NULL (count only). */
int ekf_detect_keypoints(EkfEngine *e, double min_response, int masked, EkfKeypoint *kps, uint8_t *desc32, int capacity,
                         int *n_found);
/* BRIEF-32 of the current image at the given pixels (what a new map feature keeps, AddMapFeature.cpp:317-337); the centre
 * of (u, v) is the pixel (floor(u + 0.5), floor(v + 0.5)) */
int ekf_describe(EkfEngine *e, const double *uv, int count, uint8_t *desc32);
/* keypoints the last KEYPOINTS-mode image step detected and kept (kept < detected: capacity max_keypoints reached) */
int ekf_get_step_keypoints(const EkfEngine *e, int *detected, int *kept);

/* -- instrumentation ------------------------------------------------------------------------------------- */
int ekf_timing_enable(EkfEngine *e, int on); /* HIP-event timing of stages and of the P-update kernel */
int ekf_timing_reset(EkfEngine *e);
int ekf_timing_get(EkfEngine *e, EkfStageTimes *out);
int ekf_synchronize(EkfEngine *e);
/* Per-launch record of the P-update kernel since the last ekf_timing_reset: rows m of B (k-depth) and the
 * HIP-event duration in ms.  Writes at most `capacity` entries; *count receives the number available. */
int ekf_timing_p_update_launches(EkfEngine *e, int capacity, int32_t *m_rows, float *ms, int *count);
/* The blocked Cholesky sweep of S = H P H' + R (replaces S.inv(), EKF/Update.cpp:108) since the last ekf_timing_reset:
 * HIP-event time over the sweep's launches of every update, their number (panels of 32 rows) and of updates, the fp64
 * flops of the factorisation (m^3 / 3 each) and the flops of B = inv(L) (H P) formed in the same launches (m^2 n each;
 * 0 for updates that went through the explicit inverse + GEMM).  Any output pointer may be null. */
int ekf_timing_sweep(EkfEngine *e, double *kernel_ms, int64_t *panels, int64_t *updates, double *flops_fp64, double *flops_b);
/* ... and the number of kernel launches behind those panels (a launch of the two-panels-per-launch scheme covers two), plus,
 * EKF_PRECISION_F32_EXACT only, the HIP-event time between the end of each update's sweep and the start of its downdate kernel
 * (dx, the state update and, above 2048 rows, the triangular inverse and the int8 GEMM B = inv(L) G). */
int ekf_timing_sweep_launches(EkfEngine *e, int64_t *launches, double *slice_ms);
/* Measurement aid, EKF_PRECISION_F64 engines only: replaces every entry of the device-resident covariance by its nearest fp32
 * value, in place (asynchronous, on the engine's stream).  Called between the stage functions at the points where an
 * fp32-storage configuration rounds P (after ekf_set_state, ekf_predict and each ekf_update) it yields the filter "fp32 storage,
 * fp64 arithmetic": the accuracy floor of EKF_PRECISION_F32 / _F32_EXACT on a sequence (scripts/storage_floor_gpu.py).  The
 * reference keeps everything in double (Core/Base.h:67). */
int ekf_round_covariance_to_f32(EkfEngine *e);
/* Updates re-run on the launch-per-panel sweep since the engine was created because their persistent sweep
 * (EKF_SWEEP_PERSISTENT / _AUTO) timed out: the sweep needs all of its workgroups resident at once, which another process's
 * kernels on the device or a device partition can prevent; its waits are bounded (30 ms), the kernels behind a failed sweep leave
 * x and P untouched, and the engine runs the same update again from the same P -- the caller sees EKF_OK and this counter.
 * (The fault-injection hook that exercises this path is declared in ekf_test_hooks.h, not here.) */
int ekf_get_sweep_retries(const EkfEngine *e);

/* -- row-sharded filter (multi-GPU) ----------------------------------------------------------
 * One engine per GPU / rank.  Rank g stores the 13 camera rows of P (replicated, updated identically everywhere)
 * and the rows of the features [f0_g, f1_g) it owns, each with all n columns; everything else (state, map, H.P rows,
 * S, its factor, B) is replicated.  Owned rows are predicted, multiplied (H_f P) and downdated locally; the one
 * exchange per prediction is an all-gather of the H.P row blocks (and of the 2x2 S_i of the owned features), done by
 * the callback the host installs: RCCL broadcasts/all-gather between processes, device-to-device copies when
 * several ranks share a GPU (tests).  Map management is not available on a sharded engine.
 * EKF_PRECISION_F32_EXACT (round 4): B is NOT replicated -- every rank forms the columns of B = inv(L) H P that belong to the state
 * rows it holds and the ranks all-gather B's int8 digit planes (EKF_XCHG_BPLANES; EKF_XCHG_PDIAG carries the diagonal of P behind
 * their column scales); for updates of at most 2048 rows no rows of H P travel either: G[:, own columns] follows from the own rows
 * of P by symmetry and S is assembled by block columns and all-gathered (EKF_XCHG_SCOLS).  DESIGN.md section 8. */
typedef int (*EkfExchangeFn)(void *user, int what, void *device_base, size_t row_bytes, const int32_t *row_begin,
                             int world, int rank);
enum { EKF_XCHG_HP = 0, EKF_XCHG_PRED_S = 1, EKF_XCHG_HPC = 2, EKF_XCHG_PDIAG = 3, EKF_XCHG_BPLANES = 4, EKF_XCHG_SCOLS = 5,
       /* round 6 -- matching and RANSAC divided by feature ownership: the per-prediction match tables (valid flag,
        * keypoint index or matched pixel, distance; rows = prediction slots) and a RANSAC batch's support counts and inlier masks
        * (rows = hypotheses of the batch) */
       EKF_XCHG_MATCH_VALID = 6, EKF_XCHG_MATCH_KP = 7, EKF_XCHG_MATCH_DIST = 8, EKF_XCHG_MATCH_XY = 9,
       EKF_XCHG_HYP_COUNT = 10, EKF_XCHG_HYP_FLAGS = 11 };
/* what: which replicated table is being completed; device_base: its first row on this rank's GPU; rank r owns rows
 * [row_begin[r], row_begin[r+1]) of row_bytes each and has just written them.  The callback returns when this
 * rank's table holds every rank's rows (0 = ok).  It is called with the engine's stream idle. */
int ekf_engine_create_sharded(const EkfEngineConfig *cfg, int rank, int world, EkfEngine **out);
int ekf_set_exchange(EkfEngine *e, EkfExchangeFn fn, void *user);
/* In-engine transport, one process per GPU: an RCCL communicator owned by the engine.  The exchange is then a grouped
 * ncclSend / ncclRecv of the row blocks between every pair of ranks (the direct schedule for point-to-point xGMI: every
 * rank's block travels over its own link to each peer), enqueued on the engine's stream -- no stream drain, no host
 * callback.  Rank 0 obtains the id, the host distributes it (any out-of-band channel), every rank calls
 * ekf_comm_init (collective).  RCCL is loaded at run time (librccl.so.1); EKF_ERR_COMM if it is not there.
 * A callback installed with ekf_set_exchange takes precedence over the communicator (a host whose ranks could not all
 * form one falls back to its own transport on every rank); ekf_set_exchange(e, NULL, NULL) hands it back. */
#define EKF_COMM_ID_BYTES 128
int ekf_comm_unique_id(uint8_t id[EKF_COMM_ID_BYTES]);
int ekf_comm_init(EkfEngine *e, const uint8_t id[EKF_COMM_ID_BYTES]);
/* P rows held by this rank: [*row_begin, *row_end) of the state (rank 0's range starts at 0: the camera rows,
 * which every rank also keeps).  On a sharded engine ekf_set_state takes the full n x n matrix and keeps its rows;
 * ekf_get_state fills only those rows of the caller's n x n buffer (camera rows + owned rows). */
int ekf_shard_info(const EkfEngine *e, int *rank, int *world, int *row_begin, int *row_end);
/* EKF_PRECISION_F32_EXACT on a sharded engine: a rank forms the rows of B = inv(L) H P for its own column blocks only and receives
 * the others' int8 digit planes (5 bytes per element of B).  plane_bytes_received: total since creation; [own_columns_begin,
 * own_columns_end): the columns whose rows of B this rank formed in its LAST update -- they end exactly at the ownership boundaries
 * on the by-symmetry route (updates of <= 2048 rows) and at multiples of 32 on the inverse + GEMM route; before the first update:
 * the ownership boundaries rounded to 32.  Tests compare both with the cost model. */
int ekf_shard_counters(EkfEngine *e, int64_t *plane_bytes_received, int32_t *own_columns_begin, int32_t *own_columns_end);
/* device-to-device copy on the engine's device, synchronous: the exchange primitive when ranks share a GPU */
int ekf_device_copy(EkfEngine *e, void *dst, const void *src, size_t bytes);

/* -- partition of the covariance rows across ranks; pure host arithmetic ------------------------------------- */
/* Row block [row_begin, row_end) of P owned by `rank` of `world` for a map of n_features inverse-depth features:
 * the 13 camera rows go to rank 0, features are split contiguously. */
int ekf_shard_rows(int n_features, int world, int rank, int *row_begin, int *row_end);

#ifdef __cplusplus
}
#endif
#endif /* EKF_ENGINE_H */
