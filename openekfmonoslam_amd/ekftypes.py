"""ctypes / numpy mirrors of include/ekf_types.h (plain-old-data crossing the C ABI).

Field names follow the reference's own classes (CameraCalibration.h:37-63,
ExtendedKalmanFilterParameters.h:37-76, ImageFeaturePrediction.h:37-50, Matching.h:38-48).
"""
import ctypes as C

import numpy as np


class EkfCamera(C.Structure):
    _fields_ = [
        ("pixelsX", C.c_int32),
        ("pixelsY", C.c_int32),
        ("fx", C.c_double),
        ("fy", C.c_double),
        ("k1", C.c_double),
        ("k2", C.c_double),
        ("cx", C.c_double),
        ("cy", C.c_double),
        ("dx", C.c_double),
        ("dy", C.c_double),
        ("pixelErrorX", C.c_double),
        ("pixelErrorY", C.c_double),
        ("angularVisionX", C.c_double),
        ("angularVisionY", C.c_double),
    ]


class EkfParams(C.Structure):
    _fields_ = [
        ("initInvDepthRho", C.c_double),
        ("initLinearAccelSD", C.c_double),
        ("initAngularAccelSD", C.c_double),
        ("linearAccelSD", C.c_double),
        ("angularAccelSD", C.c_double),
        ("inverseDepthRhoSD", C.c_double),
        ("matchingCompCoefSecondBestVSFirst", C.c_double),
        ("ransacThresholdPredictDistance", C.c_double),
        ("ransacAllInliersProbability", C.c_double),
        ("ransacChi2Threshold", C.c_double),
        ("goodFeatureMatchingPercent", C.c_double),
        ("inverseDepthLinearityIndexThreshold", C.c_double),
    ]


class EkfStepInfo(C.Structure):
    """OrcStepInfo (oracle) and EkfStepInfo (engine) share this layout."""

    _fields_ = [
        ("n_predicted", C.c_int32),
        ("n_matches", C.c_int32),
        ("n_hypotheses", C.c_int32),
        ("n_inliers", C.c_int32),
        ("n_outliers", C.c_int32),
        ("n_rescued", C.c_int32),
        ("status", C.c_int32),
        ("n_sweep_retries", C.c_int32),
    ]


class EkfMapPoint(C.Structure):
    """One landmark as a 3-D point (ekf_get_map_points); 216 bytes, no padding."""

    _fields_ = [
        ("xyz", C.c_double * 3),
        ("cov", C.c_double * 9),
        ("cam", C.c_double * 3),
        ("cov_cam", C.c_double * 9),
        ("linearity", C.c_double),
        ("type", C.c_int32),
        ("covpos", C.c_int32),
        ("times_predicted", C.c_uint32),
        ("times_matched", C.c_uint32),
    ]


PREDICTION_DTYPE = np.dtype(
    [("featureIndex", "<i4"), ("_pad", "<i4"), ("imagePos", "<f8", (2,)), ("covarianceMatrix", "<f8", (4,))]
)
MATCH_DTYPE = np.dtype(
    [("featureIndex", "<i4"), ("keypointIndex", "<i4"), ("imagePos", "<f8", (2,)), ("distance", "<f4"), ("_pad", "<f4")]
)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4")])
# numpy view of an EkfMapPoint array: same fields, the covariances as (3, 3)
MAP_POINT_DTYPE = np.dtype(
    [("xyz", "<f8", (3,)), ("cov", "<f8", (3, 3)), ("cam", "<f8", (3,)), ("cov_cam", "<f8", (3, 3)), ("linearity", "<f8"),
     ("type", "<i4"), ("covpos", "<i4"), ("times_predicted", "<u4"), ("times_matched", "<u4")]
)
assert MAP_POINT_DTYPE.itemsize == C.sizeof(EkfMapPoint) == 216
assert PREDICTION_DTYPE.itemsize == 56 and MATCH_DTYPE.itemsize == 32 and KEYPOINT_DTYPE.itemsize == 8
# EkfNccRival: what the NCC matcher's distinctiveness test found for one prediction (state 0 = no valid match, 1 = valid and no
# rival in the gate, 2 = rival and kept, 3 = rival and rejected)
NCC_RIVAL_DTYPE = np.dtype(
    [("featureIndex", "<i4"), ("state", "<i4"), ("rivalPos", "<f4", (2,)), ("distance", "<f4"), ("rivalDistance", "<f4")]
)
assert NCC_RIVAL_DTYPE.itemsize == 24



class EkfUpdateConsistency(C.Structure):
    """One covariance update with the consistency mode on (ekf_get_consistency); 24 bytes."""

    _fields_ = [("stage", C.c_int32), ("matches", C.c_int32), ("rows", C.c_int32), ("_pad", C.c_int32), ("nis", C.c_double)]


class EkfInnovation(C.Structure):
    """One match of such an update (ekf_get_innovations); 48 bytes, no padding."""

    _fields_ = [("featureIndex", C.c_int32), ("stage", C.c_int32), ("nu", C.c_double * 2), ("d2_marginal", C.c_double),
                ("nis_conditional", C.c_double), ("_reserved", C.c_double)]


# numpy views of the two: stage 0 = ekf_update, 1 = a step's first (LI) update, 2 = its second (HI) update
CONSISTENCY_DTYPE = np.dtype([("stage", "<i4"), ("matches", "<i4"), ("rows", "<i4"), ("_pad", "<i4"), ("nis", "<f8")])
INNOVATION_DTYPE = np.dtype([("featureIndex", "<i4"), ("stage", "<i4"), ("nu", "<f8", (2,)), ("d2_marginal", "<f8"),
                             ("nis_conditional", "<f8"), ("_reserved", "<f8")])
assert CONSISTENCY_DTYPE.itemsize == C.sizeof(EkfUpdateConsistency) == 24
assert INNOVATION_DTYPE.itemsize == C.sizeof(EkfInnovation) == 48


MAX_UPDATE_ITERATIONS = 8  # EKF_MAX_UPDATE_ITERATIONS
ITER_STOP_COUNT, ITER_STOP_TOL, ITER_STOP_FEATURE_LEFT, ITER_STOP_FAILED = 0, 1, 2, 3  # EKF_ITER_STOP_*


class EkfIterationRecord(C.Structure):
    """One iterated update of the last call (ekf_get_iteration_records); 80 bytes, no padding."""

    _fields_ = [("stage", C.c_int32), ("passes_run", C.c_int32), ("stop_reason", C.c_int32), ("_pad", C.c_int32),
                ("step", C.c_double * MAX_UPDATE_ITERATIONS)]


# step[i] = max_j |x_j^(i+1) - x_j^i| / sqrt(P_jj) over the prior's positive variances; 0 from passes_run on
ITERATION_RECORD_DTYPE = np.dtype([("stage", "<i4"), ("passes_run", "<i4"), ("stop_reason", "<i4"), ("_pad", "<i4"),
                                   ("step", "<f8", (MAX_UPDATE_ITERATIONS,))])
assert ITERATION_RECORD_DTYPE.itemsize == C.sizeof(EkfIterationRecord) == 80


class EkfMeasurementRank(C.Structure):
    """One predicted feature of a step with the measurement budget active (ekf_get_measurement_ranks); 32 bytes, no padding."""

    _fields_ = [("featureIndex", C.c_int32), ("rank", C.c_int32), ("selected", C.c_int32), ("_pad", C.c_int32), ("key", C.c_double),
                ("gain", C.c_double)]


# rank 0 = most informative; key = det(S_i), -1 when not positive; gain = 0.5 log(key / pixelErrorX^2), 0 when key = -1
MEASUREMENT_RANK_DTYPE = np.dtype([("featureIndex", "<i4"), ("rank", "<i4"), ("selected", "<i4"), ("_pad", "<i4"), ("key", "<f8"),
                                   ("gain", "<f8")])
assert MEASUREMENT_RANK_DTYPE.itemsize == C.sizeof(EkfMeasurementRank) == 32

EXT_MAX_ROWS, EXT_MAX_NNZ = 16, 32  # EKF_EXT_MAX_ROWS / EKF_EXT_MAX_NNZ: rows per external update, entries per row of H


class EkfExternalUpdate(C.Structure):
    """What ekf_update_external reports: the NIS, the whitened residual, its rows and whether the gate let it through; 144 bytes."""

    _fields_ = [("nis", C.c_double), ("z", C.c_double * EXT_MAX_ROWS), ("rows", C.c_int32), ("applied", C.c_int32)]


assert C.sizeof(EkfExternalUpdate) == 144



class EkfMapBlobInfo(C.Structure):
    """What the header of a map blob says (ekf_load_map / ekf_map_blob_info); 144 bytes, no padding."""

    _fields_ = [("version", C.c_uint32), ("N", C.c_int32), ("n", C.c_int32), ("p_elem_bytes", C.c_int32), ("p_layout", C.c_int32),
                ("desc_bytes", C.c_int32), ("desc_flags", C.c_int32), ("section_mask", C.c_uint32), ("total_bytes", C.c_uint64),
                ("cam", EkfCamera)]


assert C.sizeof(EkfMapBlobInfo) == 144

RELOC_MAX_HYPOTHESES = 4096  # EKF_RELOC_MAX_HYPOTHESES


class EkfRelocParams(C.Structure):
    """Parameters of ekf_relocalise; 72 bytes, no padding."""

    _fields_ = [("hypotheses", C.c_int32), ("min_inliers", C.c_int32), ("seed", C.c_uint64), ("max_distance", C.c_double),
                ("second_best_coef", C.c_double), ("inlier_px", C.c_double), ("max_rel_depth_sd", C.c_double),
                ("sigma_position", C.c_double), ("sigma_angle", C.c_double), ("install", C.c_int32), ("_pad", C.c_int32)]


class EkfRelocResult(C.Structure):
    """What ekf_relocalise reports; 96 bytes, no padding."""

    _fields_ = [("found", C.c_int32), ("installed", C.c_int32), ("n_features_used", C.c_int32), ("n_candidates", C.c_int32),
                ("n_hypotheses", C.c_int32), ("n_valid_hypotheses", C.c_int32), ("best_hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("rms_px", C.c_double), ("r", C.c_double * 3), ("q", C.c_double * 4)]


class EkfRelocHypothesis(C.Structure):
    """One hypothesis of the last ekf_relocalise (ekf_get_relocalise_hypotheses); 88 bytes, no padding."""

    _fields_ = [("cand", C.c_int32 * 3), ("n_solutions", C.c_int32), ("inliers", C.c_int32), ("_pad", C.c_int32),
                ("sse", C.c_double), ("r", C.c_double * 3), ("q", C.c_double * 4)]


RELOC_HYPOTHESIS_DTYPE = np.dtype([("cand", "<i4", (3,)), ("n_solutions", "<i4"), ("inliers", "<i4"), ("_pad", "<i4"), ("sse", "<f8"),
                                   ("r", "<f8", (3,)), ("q", "<f8", (4,))])
assert C.sizeof(EkfRelocParams) == 72 and C.sizeof(EkfRelocResult) == 96
assert RELOC_HYPOTHESIS_DTYPE.itemsize == C.sizeof(EkfRelocHypothesis) == 88

DESC_BYTES = 32
FEATURE_DEPTH = 1
FEATURE_INVERSE_DEPTH = 2

EKF_OK = 0
STATUS_NAMES = {
    0: "EKF_OK",
    1: "EKF_ERR_INVALID_ARG",
    2: "EKF_ERR_CAPACITY",
    3: "EKF_ERR_NOT_POSITIVE_DEFINITE",
    4: "EKF_ERR_NON_FINITE",
    5: "EKF_ERR_HIP",
    6: "EKF_ERR_NO_DEVICE",
    7: "EKF_ERR_COMM",
    8: "EKF_ERR_TIMEOUT",
}


def s3_camera(width=640, height=480):
    """Camera "S3" of the reference's shipped experiment (experiments/s3/config.yml:49-63), scaled to the
    frame size the way SURVEY.md section 8(d) prescribes: fx fy cx cy scale with width/640, the pixel pitch
    dx dy with its inverse, k1 k2 and the field of view are kept."""
    s = width / 640.0
    cam = EkfCamera()
    cam.pixelsX, cam.pixelsY = int(width), int(height)
    cam.fx = 525.060143149240389 * s
    cam.fy = 524.245488213640215 * s
    cam.k1 = -7.613e-003
    cam.k2 = 9.388e-004
    cam.cx = 308.649343121753361 * s
    cam.cy = 236.536005491807288 * s
    cam.dx = 0.007021618750000 / s
    cam.dy = 0.007027222916667 / s
    cam.pixelErrorX = 1.0
    cam.pixelErrorY = 1.0
    cam.angularVisionX = 62.720770890650357
    cam.angularVisionY = 49.163954709609868
    return cam


def s3_params():
    """EKF profile "EKF" of experiments/s3/config.yml:10-37."""
    p = EkfParams()
    p.initInvDepthRho = 1.0
    p.initLinearAccelSD = 0.001
    p.initAngularAccelSD = 0.004
    p.linearAccelSD = 0.0007
    p.angularAccelSD = 0.002
    p.inverseDepthRhoSD = 1.0
    p.matchingCompCoefSecondBestVSFirst = 1.0
    p.ransacThresholdPredictDistance = 1.0
    p.ransacAllInliersProbability = 0.99
    p.ransacChi2Threshold = 5.9915
    p.goodFeatureMatchingPercent = 0.5
    p.inverseDepthLinearityIndexThreshold = 0.1
    return p
