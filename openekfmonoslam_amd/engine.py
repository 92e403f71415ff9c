"""ctypes binding of libekf_engine.so (the HIP engine).  There is no CPU fallback: if the library is missing or
no MI355X is visible, construction fails loudly.

The names mirror the reference's stage functions (include/ekf_engine.h cites each reference file:line):
``predict`` = stateAndCovariancePrediction, ``predict_measurements`` = predictCameraMeasurements,
``match`` = matchPredictedFeatures (downstream of the detector), ``ransac``, ``update``, ``rescue``,
``step`` = EKF::step.
"""
import ctypes as C
import os

import numpy as np

from .ekftypes import (CONSISTENCY_DTYPE, DESC_BYTES, INNOVATION_DTYPE, ITERATION_RECORD_DTYPE, KEYPOINT_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE,
                       MEASUREMENT_RANK_DTYPE, NCC_RIVAL_DTYPE,
                       PREDICTION_DTYPE, RELOC_HYPOTHESIS_DTYPE, STATUS_NAMES, EkfCamera, EkfExternalUpdate, EkfMapBlobInfo, EkfMapPoint,
                       EkfParams, EkfRelocParams, EkfRelocResult, EkfStepInfo)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libekf_engine.so")
PRECISION_F64, PRECISION_F32, PRECISION_F32_EXACT, PRECISION_F64_EXACT, PRECISION_AUTO = 0, 1, 2, 3, 4
IMAGE_MATCHER_NCC, IMAGE_MATCHER_KEYPOINTS = 0, 1
MAP_TEMPLATES, MAP_WARP_SOURCES, MAP_PATCH_NORMALS, MAP_ALL = 1, 2, 4, 7  # EKF_MAP_*: optional sections of a map blob


class EkfEngineConfig(C.Structure):
    _fields_ = [
        ("cam", EkfCamera),
        ("par", EkfParams),
        ("max_features", C.c_int32),
        ("max_keypoints", C.c_int32),
        ("precision", C.c_int32),
        ("device", C.c_int32),
        ("ransac_batch", C.c_int32),
        ("flags", C.c_int32),
    ]


class EkfStageTimes(C.Structure):
    _fields_ = [
        ("prediction_ms", C.c_double),
        ("matching_ms", C.c_double),
        ("ransac_ms", C.c_double),
        ("update_li_ms", C.c_double),
        ("rescue_ms", C.c_double),
        ("update_hi_ms", C.c_double),
        ("p_update_kernel_ms", C.c_double),
        ("p_update_launches", C.c_int64),
        ("p_update_flops", C.c_double),
        ("p_update_bytes", C.c_double),
        ("steps", C.c_int64),
    ]


class EkfPatchNormal(C.Structure):
    """ekf_get_patch_normals: slope, information (00, 01, 11), world normal, update count; 72 bytes"""

    _fields_ = [
        ("pq", C.c_double * 2),
        ("info", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("updates", C.c_int32),
        ("pad", C.c_int32),
    ]


PATCH_NORMAL_DTYPE = np.dtype([("pq", "<f8", (2,)), ("info", "<f8", (3,)), ("normal", "<f8", (3,)), ("updates", "<i4"), ("_pad", "<i4")])
assert PATCH_NORMAL_DTYPE.itemsize == C.sizeof(EkfPatchNormal) == 72

# every symbol include/ekf_engine.h declares: name -> (restype, argtypes)
_vp, _i = C.c_void_p, C.c_int
ABI = {
    "ekf_engine_create": (_i, [C.POINTER(EkfEngineConfig), C.POINTER(_vp)]),
    "ekf_engine_destroy": (None, [_vp]),
    "ekf_last_error": (C.c_char_p, [_vp]),
    "ekf_abi_version": (_i, []),
    "ekf_device_count": (_i, []),
    "ekf_set_state": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ekf_get_state": (_i, [_vp, _vp, _vp, _vp]),
    "ekf_get_map_features": (_i, [_vp, _vp, _vp, _vp]),
    "ekf_map_blob_bytes": (_i, [_vp, _i, C.POINTER(C.c_size_t)]),
    "ekf_save_map": (_i, [_vp, _i, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ekf_load_map": (_i, [_vp, _vp, C.c_size_t, C.POINTER(EkfMapBlobInfo)]),
    "ekf_map_blob_info": (_i, [_vp, C.c_size_t, C.POINTER(EkfMapBlobInfo)]),
    "ekf_reset": (_i, [_vp]),
    "ekf_add_features": (_i, [_vp, _vp, _vp, _i]),
    "ekf_remove_features": (_i, [_vp, _vp, _i]),
    "ekf_remove_bad_features": (_i, [_vp, C.POINTER(_i)]),
    "ekf_convert_inverse_depth_to_depth": (_i, [_vp, C.POINTER(_i)]),
    "ekf_convert_all_inverse_depth_to_depth": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_get_feature_layout": (_i, [_vp, _vp, _vp]),
    "ekf_keep_step_predictions": (_i, [_vp, _i]),
    "ekf_get_step_predictions": (_i, [_vp, _vp, C.POINTER(_i)]),
    "ekf_get_camera_covariance": (_i, [_vp, _vp]),
    "ekf_get_map_points": (_i, [_vp, C.POINTER(EkfMapPoint), _i, C.POINTER(_i)]),
    "ekf_get_unseen_features": (_i, [_vp, _vp, C.POINTER(_i)]),
    "ekf_set_consistency": (_i, [_vp, _i]),
    "ekf_get_consistency": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_get_innovations": (_i, [_vp, _i, _vp, _i, C.POINTER(_i)]),
    "ekf_get_consistency_totals": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ekf_reset_consistency_totals": (_i, [_vp]),
    "ekf_set_measurement_budget": (_i, [_vp, _i]),
    "ekf_get_measurement_ranks": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_get_measurement_budget_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_state_dim": (_i, [_vp]),
    "ekf_descriptor_bytes": (_i, [_vp]),
    "ekf_num_features": (_i, [_vp]),
    "ekf_predict": (_i, [_vp]),
    "ekf_set_frame_interval": (_i, [_vp, C.c_double]),
    "ekf_get_frame_interval": (_i, [_vp, C.POINTER(C.c_double)]),
    "ekf_predict_dt": (_i, [_vp, C.c_double]),
    "ekf_set_staged_intervals": (_i, [_vp, _i, _vp]),
    "ekf_predict_camera_ahead": (_i, [_vp, C.c_double, _vp, _vp]),
    "ekf_predict_measurements": (_i, [_vp, _vp, _i, _vp, C.POINTER(_i), _vp, _vp]),
    "ekf_predict_measurement_state": (_i, [_vp, _vp, C.POINTER(_i)]),
    "ekf_match": (_i, [_vp, _vp, _vp, _i, _vp, C.POINTER(_i)]),
    "ekf_ransac": (_i, [_vp, _vp, _i, _vp, C.POINTER(_i)]),
    "ekf_update": (_i, [_vp, _vp, _i]),
    "ekf_update_only_state": (_i, [_vp, _vp, _i]),
    "ekf_update_external": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, C.POINTER(EkfExternalUpdate)]),
    "ekf_fuse_camera_position": (_i, [_vp, _vp, _vp, C.c_double, C.POINTER(EkfExternalUpdate)]),
    "ekf_fuse_feature_distance": (_i, [_vp, _i, _i, C.c_double, C.c_double, C.c_double, C.POINTER(EkfExternalUpdate)]),
    "ekf_update_fixed_map": (_i, [_vp, _vp, _i]),
    "ekf_set_fixed_map": (_i, [_vp, _i]),
    "ekf_get_fixed_map": (_i, [_vp, C.POINTER(_i), C.POINTER(C.c_int64)]),
    "ekf_relocalise": (_i, [_vp, _vp, _vp, _i, C.POINTER(EkfRelocParams), C.POINTER(EkfRelocResult)]),
    "ekf_relocalise_image": (_i, [_vp, C.c_double, C.POINTER(EkfRelocParams), C.POINTER(EkfRelocResult)]),
    "ekf_get_relocalise_candidates": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i)]),
    "ekf_get_relocalise_hypotheses": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_update_iterated": (_i, [_vp, _vp, _i, _i, C.c_double]),
    "ekf_set_update_iterations": (_i, [_vp, _i, C.c_double]),
    "ekf_get_update_iterations": (_i, [_vp, C.POINTER(_i), C.POINTER(C.c_double)]),
    "ekf_get_iteration_records": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_get_linearisation_point": (_i, [_vp, _vp, _vp]),
    "ekf_rescue": (_i, [_vp, _vp, _i, _vp]),
    "ekf_step": (_i, [_vp, _vp, _vp, _i, C.POINTER(EkfStepInfo)]),
    "ekf_frames_upload": (_i, [_vp, _i, _vp, _vp, _vp]),
    "ekf_step_frame": (_i, [_vp, _i, C.POINTER(EkfStepInfo)]),
    "ekf_set_async_errors": (_i, [_vp, _i]),
    "ekf_set_update_path": (_i, [_vp, _i]),
    "ekf_set_sweep_mode": (_i, [_vp, _i]),
    "ekf_get_precision": (_i, [_vp]),
    "ekf_image_upload": (_i, [_vp, _vp, _i, _i, _i, _i]),
    "ekf_get_image_level": (_i, [_vp, _i, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_capture_templates": (_i, [_vp, _vp, _vp, _i]),
    "ekf_match_ncc": (_i, [_vp, _vp, C.POINTER(_i)]),
    "ekf_set_template_warp": (_i, [_vp, _i]),
    "ekf_get_template_warp_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_get_match_templates": (_i, [_vp, _vp, _i, _vp]),
    "ekf_set_subpixel_matches": (_i, [_vp, _i]),
    "ekf_get_subpixel_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_set_ncc_wide_search": (_i, [_vp, _i]),
    "ekf_get_ncc_wide_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_set_ncc_distinct": (_i, [_vp, C.c_double]),
    "ekf_get_ncc_distinct_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_get_ncc_rivals": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ekf_set_patch_normals": (_i, [_vp, _i]),
    "ekf_refine_patch_normals": (_i, [_vp, _vp, _i]),
    "ekf_get_patch_normals": (_i, [_vp, _vp, _i, _vp]),
    "ekf_set_patch_normal": (_i, [_vp, _i, _vp, _vp]),
    "ekf_get_patch_normal_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_step_image": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(EkfStepInfo)]),
    "ekf_detect_new_features": (_i, [_vp, _i, _i, C.c_double, C.c_double, _vp, C.POINTER(_i)]),
    "ekf_images_upload": (_i, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ekf_select_staged_image": (_i, [_vp, _i]),
    "ekf_step_staged_image": (_i, [_vp, _i, C.POINTER(EkfStepInfo)]),
    "ekf_set_image_matcher": (_i, [_vp, _i, C.c_double]),
    "ekf_detect_keypoints": (_i, [_vp, C.c_double, _i, _vp, _vp, _i, C.POINTER(_i)]),
    "ekf_describe": (_i, [_vp, _vp, _i, _vp]),
    "ekf_get_step_keypoints": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_timing_enable": (_i, [_vp, _i]),
    "ekf_timing_reset": (_i, [_vp]),
    "ekf_timing_get": (_i, [_vp, C.POINTER(EkfStageTimes)]),
    "ekf_synchronize": (_i, [_vp]),
    "ekf_timing_p_update_launches": (_i, [_vp, _i, _vp, _vp, C.POINTER(_i)]),
    "ekf_timing_sweep": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                              C.POINTER(C.c_double)]),
    "ekf_timing_sweep_launches": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "ekf_round_covariance_to_f32": (_i, [_vp]),
    "ekf_get_sweep_retries": (_i, [_vp]),
    "ekf_shard_rows": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_engine_create_sharded": (_i, [C.POINTER(EkfEngineConfig), _i, _i, C.POINTER(_vp)]),
    "ekf_set_exchange": (_i, [_vp, _vp, _vp]),
    "ekf_comm_unique_id": (_i, [_vp]),
    "ekf_comm_init": (_i, [_vp, _vp]),
    "ekf_shard_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "ekf_shard_counters": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ekf_device_copy": (_i, [_vp, _vp, _vp, C.c_size_t]),
}

# include/ekf_test_hooks.h: fault injection for the tests, not part of the boundary
TEST_HOOKS = {
    "ekf_debug_stall_next_sweep": (_i, [_vp]),
    "ekf_debug_stall_sweep_after": (_i, [_vp, _i]),
    "ekf_debug_plane0_pieces": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "ekf_debug_dense_products": (_i, [_vp, _i]),
    "ekf_debug_get_hp_rows": (_i, [_vp, _vp, _i, _vp, _vp]),
}

# int fn(void *user, int what, void *device_base, size_t row_bytes, const int32_t *row_begin, int world, int rank)
EXCHANGE_FN = C.CFUNCTYPE(_i, _vp, _i, _vp, C.c_size_t, C.POINTER(C.c_int32), _i, _i)
XCHG_HP, XCHG_PRED_S = 0, 1

_lib = None


def load_library():
    """Loads libekf_engine.so.  torch (if installed) is imported first so that one HIP runtime serves both."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m openekfmonoslam_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback."
        )
    try:
        import torch  # noqa: F401  (pulls in torch's libamdhip64 before ours resolves the same SONAME)
    except Exception:
        pass
    override = os.environ.get("EKF_ENGINE_LIB")  # A/B timing of another build of the engine (scripts/build_variant.sh)
    L = C.CDLL(os.path.abspath(override) if override else LIB_PATH)
    for name, (rt, at) in list(ABI.items()) + list(TEST_HOOKS.items()):
        if override and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = rt
        fn.argtypes = at
    _lib = L
    return L


class EkfError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def shard_rows(n_features, world, rank):
    lo, hi = _i(0), _i(0)
    rc = load_library().ekf_shard_rows(n_features, world, rank, C.byref(lo), C.byref(hi))
    if rc:
        raise EkfError(rc)
    return lo.value, hi.value


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 of a sharded filter creates it, the host distributes it to every rank)."""
    buf = np.zeros(128, dtype=np.uint8)
    rc = load_library().ekf_comm_unique_id(_p(buf))
    if rc:
        raise EkfError(rc, "ekf_comm_unique_id (librccl.so.1 not loadable?)")
    return buf


def _blob_info_dict(info):
    d = {name: int(getattr(info, name)) for name, _ in EkfMapBlobInfo._fields_ if name != "cam"}
    d["cam"] = {name: getattr(info.cam, name) for name, _ in EkfCamera._fields_}
    return d


def map_blob_info(blob):
    """Validates a map blob on the host (no engine, no device; every checksum included) and returns its header as a dict."""
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    info = EkfMapBlobInfo()
    rc = load_library().ekf_map_blob_info(_p(b), b.size, C.byref(info))
    if rc:
        raise EkfError(rc, "not a valid map blob")
    return _blob_info_dict(info)


class EkfEngine:
    """One device-resident filter (state, covariance, map, per-frame tables) on one MI355X."""

    def __init__(self, cam, par, max_features, max_keypoints=0, precision=PRECISION_F64, device=-1, ransac_batch=0,
                 shard=None, descriptor_cols_f32=0):
        """shard = (rank, world) creates one rank of a row-sharded filter; install the exchange with
        set_exchange before the first prediction.  descriptor_cols_f32 > 0: CV_32F descriptors of that many floats
        matched by L2 distance (EKF_DESCRIPTOR_F32_L2) instead of 32-byte binary descriptors / Hamming."""
        self.L = load_library()
        cfg = EkfEngineConfig()
        cfg.cam, cfg.par = cam, par
        cfg.max_features, cfg.max_keypoints = int(max_features), int(max_keypoints)
        cfg.precision, cfg.device, cfg.ransac_batch = int(precision), int(device), int(ransac_batch)
        cfg.flags = (1 | (int(descriptor_cols_f32) << 8)) if descriptor_cols_f32 else 0
        h = _vp()
        if shard is None:
            rc = self.L.ekf_engine_create(C.byref(cfg), C.byref(h))
        else:
            rc = self.L.ekf_engine_create_sharded(C.byref(cfg), int(shard[0]), int(shard[1]), C.byref(h))
        self._xchg_ref = None
        if rc:
            raise EkfError(rc, "ekf_engine_create failed (no MI355X visible?)")
        self.h = h
        self.cap = int(max_features)
        self.precision = int(self.L.ekf_get_precision(self.h))  # (what PRECISION_AUTO resolved to)
        self.desc_bytes = self.L.ekf_descriptor_bytes(self.h)
        self.desc_dtype = np.float32 if descriptor_cols_f32 else np.uint8

    def _desc(self, desc):
        """descriptor matrix -> contiguous bytes, one row of desc_bytes per descriptor"""
        if desc is None:
            return None
        d = np.ascontiguousarray(desc, dtype=self.desc_dtype)
        return d.view(np.uint8).reshape(-1, self.desc_bytes)

    def set_exchange(self, fn):
        """fn(what, device_base, row_bytes, row_begin[world+1], world, rank) -> 0 on success; called by the engine
        (from C, with its stream idle) whenever a replicated per-feature table has to be completed across ranks."""
        def tramp(_user, what, base, row_bytes, rb, world, rank):
            try:
                return int(fn(int(what), int(base), int(row_bytes), [int(rb[i]) for i in range(world + 1)], int(world),
                              int(rank)) or 0)
            except Exception:  # an exception must not unwind through the C frames
                import traceback

                traceback.print_exc()
                return 1

        self._xchg_ref = EXCHANGE_FN(tramp)
        self._chk(self.L.ekf_set_exchange(self.h, C.cast(self._xchg_ref, _vp), None))

    def comm_init(self, unique_id):
        """collective over the ranks of a sharded filter: the engine's own RCCL communicator (in-stream exchange)"""
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        self._chk(self.L.ekf_comm_init(self.h, _p(uid)))

    def shard_info(self):
        r, w, lo, hi = _i(0), _i(1), _i(0), _i(0)
        self._chk(self.L.ekf_shard_info(self.h, C.byref(r), C.byref(w), C.byref(lo), C.byref(hi)))
        return r.value, w.value, lo.value, hi.value

    def shard_counters(self):
        """(bytes of digit planes received so far, first own column, one past the last own column) -- exact configuration"""
        b, c0, c1 = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.L.ekf_shard_counters(self.h, C.byref(b), C.byref(c0), C.byref(c1)))
        return b.value, c0.value, c1.value

    def device_copy(self, dst, src, nbytes):
        self._chk(self.L.ekf_device_copy(self.h, _vp(dst), _vp(src), nbytes))

    def close(self):
        if getattr(self, "h", None):
            self.L.ekf_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc, allow=()):
        if rc and rc not in allow:
            raise EkfError(rc, (self.L.ekf_last_error(self.h) or b"").decode())
        return rc

    # ---- state
    @property
    def n(self):
        return self.L.ekf_state_dim(self.h)

    @property
    def N(self):
        return self.L.ekf_num_features(self.h)

    def set_state(self, x13, feature_pos, feature_type, desc, P):
        x13 = np.ascontiguousarray(x13, dtype=np.float64)
        fp = np.ascontiguousarray(feature_pos, dtype=np.float64).reshape(-1, 6)
        ft = None if feature_type is None else np.ascontiguousarray(feature_type, dtype=np.int32)
        d = self._desc(desc)
        Pm = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        self._chk(self.L.ekf_set_state(self.h, _p(x13), len(fp), _p(fp), _p(ft), _p(d), _p(Pm)))

    def get_state(self, want_P=True, P_out=None):
        """P_out: an existing [n, n] float64 array to fill (a sharded engine writes only the rows it holds, so the
        ranks of a group can assemble the whole matrix in one buffer)."""
        x = np.zeros(13)
        fp = np.zeros((max(self.N, 1), 6))
        P = P_out if P_out is not None else (np.zeros((self.n, self.n)) if want_P else None)
        self._chk(self.L.ekf_get_state(self.h, _p(x), _p(fp), _p(P)))
        return x, fp[: self.N], P

    def map_blob_bytes(self, sections=MAP_ALL):
        """size of the blob save_map would return now"""
        nb = C.c_size_t(0)
        self._chk(self.L.ekf_map_blob_bytes(self.h, int(sections), C.byref(nb)))
        return nb.value

    def save_map(self, sections=MAP_ALL):
        """The whole filter and map as one blob (np.uint8): state, map, counters, P packed on the device, and with `sections` the
        NCC templates, the warp's source patches and capture poses, the patch normals.  Read-only."""
        blob = np.zeros(self.map_blob_bytes(sections), dtype=np.uint8)
        nb = C.c_size_t(0)
        self._chk(self.L.ekf_save_map(self.h, int(sections), _p(blob), blob.size, C.byref(nb)))
        assert nb.value == blob.size
        return blob

    def load_map(self, blob):
        """Replaces the filter and map by the blob's; a refused blob leaves the engine as it was.  Returns the blob's header."""
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        info = EkfMapBlobInfo()
        self._chk(self.L.ekf_load_map(self.h, _p(b), b.size, C.byref(info)))
        return _blob_info_dict(info)

    def camera_covariance(self):
        P = np.zeros((13, 13))
        self._chk(self.L.ekf_get_camera_covariance(self.h, _p(P)))
        return P

    def map_points(self):
        """The map as 3-D points, computed on the device: a structured array (MAP_POINT_DTYPE: xyz, cov (3, 3), cam,
        cov_cam (3, 3), linearity, type, covpos, times_predicted, times_matched) viewed on the ctypes buffer the
        library filled.  Read-only for the filter."""
        buf = (EkfMapPoint * max(self.N, 1))()
        n = _i(0)
        self._chk(self.L.ekf_get_map_points(self.h, buf, len(buf), C.byref(n)))
        return np.frombuffer(buf, dtype=MAP_POINT_DTYPE)[: n.value]

    # ---- external measurements
    @staticmethod
    def _external_result(out):
        return {"nis": out.nis, "z": np.array(out.z[: out.rows]), "rows": out.rows, "applied": bool(out.applied)}

    def update_external(self, H_rows, residual, R, gate_nis=0.0, allow_errors=()):
        """An EKF update with any linearised measurement, between steps: H_rows is a dense [m, n] array over the state indices
        (its non-zeros become the rows) or (row_start, col, val) in CSR form, residual = z - h(x), R the m x m measurement
        covariance (upper triangle read); m <= 16 rows of <= 32 entries.  gate_nis > 0: applied only if nis <= gate_nis.
        Returns {"nis", "z", "rows", "applied"}; with allow_errors, {"code": rc} for an allowed error code."""
        if isinstance(H_rows, tuple):
            row_start, col, val = H_rows
        else:
            H = np.atleast_2d(np.asarray(H_rows, dtype=np.float64))
            nz = [np.flatnonzero(r) for r in H]
            row_start = np.cumsum([0] + [len(k) for k in nz])
            col = np.concatenate(nz) if nz else np.zeros(0)
            val = np.concatenate([r[k] for r, k in zip(H, nz)]) if nz else np.zeros(0)
        row_start = np.ascontiguousarray(row_start, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        residual = np.ascontiguousarray(np.atleast_1d(residual), dtype=np.float64)
        m = len(row_start) - 1
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(-1)
        if m < 0 or len(residual) != m or R.size != m * m or len(col) != len(val) or len(col) < int(row_start[-1]):
            raise ValueError("update_external: row_start, col / val, residual and R do not describe the same m rows")
        out = EkfExternalUpdate()
        rc = self._chk(self.L.ekf_update_external(self.h, m, _p(row_start), _p(col), _p(val), _p(residual), _p(R), float(gate_nis),
                                                  C.byref(out)), allow_errors)
        return {"code": rc} if rc else self._external_result(out)

    def fuse_camera_position(self, r, R, gate_nis=0.0):
        """a fix r of the camera position with 3 x 3 covariance R"""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(3)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        out = EkfExternalUpdate()
        self._chk(self.L.ekf_fuse_camera_position(self.h, _p(r), _p(R), float(gate_nis), C.byref(out)))
        return self._external_result(out)

    def fuse_feature_distance(self, i, j, d, sigma, gate_nis=0.0):
        """a measured distance d (standard deviation sigma) between the world points of map features i and j"""
        out = EkfExternalUpdate()
        self._chk(self.L.ekf_fuse_feature_distance(self.h, int(i), int(j), float(d), float(sigma), float(gate_nis), C.byref(out)))
        return self._external_result(out)

    # ---- relocalisation on the map
    @staticmethod
    def _reloc_params(hypotheses=256, min_inliers=6, seed=1, max_distance=48.0, second_best_coef=0.8, inlier_px=3.0,
                      max_rel_depth_sd=0.0, sigma_position=0.05, sigma_angle=0.02, install=0):
        p = EkfRelocParams()
        p.hypotheses, p.min_inliers, p.seed = int(hypotheses), int(min_inliers), int(seed) & ((1 << 64) - 1)
        p.max_distance, p.second_best_coef, p.inlier_px = float(max_distance), float(second_best_coef), float(inlier_px)
        p.max_rel_depth_sd, p.sigma_position, p.sigma_angle = float(max_rel_depth_sd), float(sigma_position), float(sigma_angle)
        p.install = int(install)
        return p

    @staticmethod
    def _reloc_result(out):
        d = {name: int(getattr(out, name)) for name, _ in EkfRelocResult._fields_[:8]}
        d.update(rms_px=out.rms_px, r=np.array(out.r[:]), q=np.array(out.q[:]))
        return d

    def relocalise(self, kps, desc, allow_errors=(), **params):
        """Finds the camera pose from the map and one frame's keypoints (KEYPOINT_DTYPE [K], uint8 [K, 32]) alone: global descriptor
        match, P3P hypotheses, the filter's own projection as the score.  params: the fields of EkfRelocParams (hypotheses,
        min_inliers, seed, max_distance, second_best_coef, inlier_px, max_rel_depth_sd, sigma_position, sigma_angle, install).
        Returns the fields of EkfRelocResult as a dict; with install=1 a found pose replaces the camera state and the camera's rows
        and columns of P.  With allow_errors, {"code": rc} for an allowed error code."""
        kps = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(len(kps), -1) if len(kps) else np.zeros((0, DESC_BYTES), dtype=np.uint8)
        if desc.shape[1] != DESC_BYTES:
            raise ValueError("relocalise: 32-byte descriptors are needed")
        p, out = self._reloc_params(**params), EkfRelocResult()
        rc = self._chk(self.L.ekf_relocalise(self.h, _p(kps), _p(desc), len(kps), C.byref(p), C.byref(out)), allow_errors)
        return {"code": rc} if rc else self._reloc_result(out)

    def relocalise_image(self, min_response=1e9, allow_errors=(), **params):
        """relocalise on the keypoints the detector and BRIEF-32 find in the current image (upload_image), unmasked; they and their
        count stay on the device"""
        p, out = self._reloc_params(**params), EkfRelocResult()
        rc = self._chk(self.L.ekf_relocalise_image(self.h, float(min_response), C.byref(p), C.byref(out)), allow_errors)
        return {"code": rc} if rc else self._reloc_result(out)

    def relocalise_candidates(self):
        """(MATCH_DTYPE [C], uint8 [C]): the candidates of the last relocalise in ascending feature order, and which of them are
        inliers of its best hypothesis"""
        n = _i(0)
        self._chk(self.L.ekf_get_relocalise_candidates(self.h, None, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=MATCH_DTYPE)
        mask = np.zeros(max(n.value, 1), dtype=np.uint8)
        self._chk(self.L.ekf_get_relocalise_candidates(self.h, _p(out), _p(mask), len(out), C.byref(n)))
        return out[: n.value].copy(), mask[: n.value].copy()

    def relocalise_hypotheses(self):
        """RELOC_HYPOTHESIS_DTYPE [hypotheses of the last relocalise]: cand, n_solutions, inliers, sse, r, q"""
        n = _i(0)
        self._chk(self.L.ekf_get_relocalise_hypotheses(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=RELOC_HYPOTHESIS_DTYPE)
        self._chk(self.L.ekf_get_relocalise_hypotheses(self.h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    # ---- filter consistency
    def set_consistency(self, on=True):
        """every covariance update records its NIS and per-match innovations on the device; off (the default): no extra launch"""
        self._chk(self.L.ekf_set_consistency(self.h, 1 if on else 0))

    def consistency(self):
        """CONSISTENCY_DTYPE [0..2]: the updates recorded since the last step or update() began (stage, matches, rows, nis)"""
        out = np.zeros(2, dtype=CONSISTENCY_DTYPE)
        n = _i(0)
        self._chk(self.L.ekf_get_consistency(self.h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def innovations(self, which):
        """INNOVATION_DTYPE [matches of record `which`], in the update's order: nu, d2_marginal, nis_conditional"""
        out = np.zeros(max(self.cap, 1), dtype=INNOVATION_DTYPE)
        n = _i(0)
        self._chk(self.L.ekf_get_innovations(self.h, int(which), _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def consistency_totals(self):
        """(sum of nis, sum of rows, updates) over every update recorded since creation or the last reset"""
        s, r, u = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.ekf_get_consistency_totals(self.h, C.byref(s), C.byref(r), C.byref(u)))
        return s.value, r.value, u.value

    def reset_consistency_totals(self):
        self._chk(self.L.ekf_reset_consistency_totals(self.h))

    # ---- measurement budget
    def set_measurement_budget(self, K):
        """a step measures at most the K most informative of the features it predicts (largest det S_i); 0 (the default): off"""
        self._chk(self.L.ekf_set_measurement_budget(self.h, int(K)))

    def measurement_ranks(self):
        """MEASUREMENT_RANK_DTYPE [features the last step predicted], in feature order, if the budget was active in it; else empty"""
        n = _i(0)
        self._chk(self.L.ekf_get_measurement_ranks(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=MEASUREMENT_RANK_DTYPE)
        self._chk(self.L.ekf_get_measurement_ranks(self.h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def measurement_budget_counts(self):
        """(predicted, selected) of the last step's full prediction; equal when the budget did not bind"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_measurement_budget_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def unseen_features(self):
        idx = np.zeros(max(self.N, 1), dtype=np.int32)
        n = C.c_int(0)
        self._chk(self.L.ekf_get_unseen_features(self.h, _p(idx), C.byref(n)))
        return idx[: n.value].copy()

    def set_async_errors(self, on=True):
        """no read-back at the end of step(): a failed second update is reported by the next step instead"""
        if hasattr(self.L, "ekf_set_async_errors"):
            self._chk(self.L.ekf_set_async_errors(self.h, 1 if on else 0))

    @property
    def sweep_retries(self):
        """updates re-run on the launch-per-panel sweep because their persistent sweep timed out (ekf_get_sweep_retries)"""
        return int(self.L.ekf_get_sweep_retries(self.h))

    def stall_sweep(self, skip=0):
        """test hook (include/ekf_test_hooks.h): the persistent sweep after the next `skip` ones runs without its chain workgroup"""
        self._chk(self.L.ekf_debug_stall_sweep_after(self.h, int(skip)))

    def plane0_pieces(self):
        """test hook: (non-zero, all) 16 x 32 pieces of digit plane 0 of B in the last update (exact configurations)"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_debug_plane0_pieces(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dense_products(self, on=True):
        """test hook: the exact downdate / int8 GEMM multiply every digit product (the zero-piece tables are not consulted)"""
        self._chk(self.L.ekf_debug_dense_products(self.h, 1 if on else 0))

    def hp_rows(self, feat_idx):
        """test hook: (HP [k, 2, n], HPc [k, 2, 13]) -- the H P row pairs of the listed features as the last measurement prediction
        left them on the device, and the fp64 copy of their 13 camera columns"""
        idx = np.ascontiguousarray(feat_idx, dtype=np.int32)
        HP = np.zeros((max(len(idx), 1), 2, self.n))
        HPc = np.zeros((max(len(idx), 1), 2, 13))
        self._chk(self.L.ekf_debug_get_hp_rows(self.h, _p(idx), len(idx), _p(HP), _p(HPc)))
        return HP[: len(idx)], HPc[: len(idx)]

    def set_update_path(self, path):
        """0: by size, 1: B = inv(L) H P inside the Cholesky sweep, 2: explicit inverse + GEMM (ekf_engine.h)"""
        self._chk(self.L.ekf_set_update_path(self.h, int(path)))

    def set_sweep_mode(self, mode):
        """2: by size (default: ONE persistent launch per update on maps below 8192 state columns, launches per panel above),
        3: the persistent sweep wherever it is available, 4: launches per panel (1 / 0: one / two panels per launch); ekf_engine.h"""
        self._chk(self.L.ekf_set_sweep_mode(self.h, int(mode)))

    def keep_step_predictions(self, on=True):
        self._chk(self.L.ekf_keep_step_predictions(self.h, 1 if on else 0))

    def step_predictions(self):
        """predictions of the last step's full prediction, as they were before the updates (drawPrediction's input)"""
        from .ekftypes import PREDICTION_DTYPE

        n = C.c_int(0)
        self._chk(self.L.ekf_get_step_predictions(self.h, None, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=PREDICTION_DTYPE)
        self._chk(self.L.ekf_get_step_predictions(self.h, _p(out), C.byref(n)))
        return out[: n.value].copy()

    # ---- map management
    def reset(self):
        self._chk(self.L.ekf_reset(self.h))

    def add_features(self, uv, desc=None):
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        d = self._desc(desc)
        self._chk(self.L.ekf_add_features(self.h, _p(uv), _p(d), len(uv)))

    def remove_features(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._chk(self.L.ekf_remove_features(self.h, _p(idx), len(idx)))

    def remove_bad_features(self):
        k = _i(0)
        self._chk(self.L.ekf_remove_bad_features(self.h, C.byref(k)))
        return k.value

    def convert_inverse_depth_to_depth(self):
        k = _i(-1)
        self._chk(self.L.ekf_convert_inverse_depth_to_depth(self.h, C.byref(k)))
        return k.value

    def convert_all_inverse_depth_to_depth(self):
        """every inverse-depth feature below the linearity threshold, in one pass -> their indices, ascending (int32)"""
        idx = np.zeros(max(self.N, 1), dtype=np.int32)
        k = _i(0)
        self._chk(self.L.ekf_convert_all_inverse_depth_to_depth(self.h, _p(idx), self.N, C.byref(k)))
        return idx[: k.value].copy()

    def feature_layout(self):
        t = np.zeros(max(self.N, 1), dtype=np.int32)
        c = np.zeros(max(self.N, 1), dtype=np.int32)
        self._chk(self.L.ekf_get_feature_layout(self.h, _p(t), _p(c)))
        return t[: self.N], c[: self.N]

    def get_map_features(self):
        """(descriptors [N,32] u8, timesPredicted [N] u32, timesMatched [N] u32)."""
        N = max(self.N, 1)
        d = np.zeros((N, self.desc_bytes), dtype=np.uint8)
        tp = np.zeros(N, dtype=np.uint32)
        tm = np.zeros(N, dtype=np.uint32)
        self._chk(self.L.ekf_get_map_features(self.h, _p(d), _p(tp), _p(tm)))
        return d[: self.N].view(self.desc_dtype), tp[: self.N], tm[: self.N]

    # ---- stages
    def predict(self, dt=None):
        """One prediction over the set frame interval (ekf_predict), or -- dt given -- over dt, leaving the set interval alone
        (ekf_predict_dt)."""
        if dt is None:
            self._chk(self.L.ekf_predict(self.h))
        else:
            self._chk(self.L.ekf_predict_dt(self.h, float(dt)))

    def set_frame_interval(self, dt):
        """The interval predict() and every step use from now on, in units of the frame period the noise parameters were tuned for
        (default 1.0; a frame after k dropped ones: k + 1).  Not finite or not > 0: EkfError(EKF_ERR_INVALID_ARG), nothing changes."""
        self._chk(self.L.ekf_set_frame_interval(self.h, float(dt)))

    def frame_interval(self):
        dt = C.c_double(0.0)
        self._chk(self.L.ekf_get_frame_interval(self.h, C.byref(dt)))
        return dt.value

    def set_staged_intervals(self, dts):
        """Per-index intervals of a pre-staged sequence: step_frame(i) / step_staged_image(i) use dts[i] for i < len(dts), the set
        interval beyond; an empty list clears the table.  One bad entry refuses the whole table."""
        d = np.ascontiguousarray(dts, dtype=np.float64).reshape(-1)
        self._chk(self.L.ekf_set_staged_intervals(self.h, len(d), _p(d) if len(d) else None))

    def camera_ahead(self, tau):
        """Look-ahead (ekf_predict_camera_ahead): (x13, P13) -- the camera state and its 13 x 13 covariance F P_cc F' + G Q G' a
        prediction over tau would leave, computed on the device in fp64 without touching the filter."""
        x, P = np.zeros(13), np.zeros((13, 13))
        self._chk(self.L.ekf_predict_camera_ahead(self.h, float(tau), _p(x), _p(P)))
        return x, P

    def predict_measurements(self, feat_idx=None):
        idx = None if feat_idx is None else np.ascontiguousarray(feat_idx, dtype=np.int32)
        cnt = 0 if idx is None else len(idx)
        cap = self.N if idx is None else max(cnt, 1)
        preds = np.zeros(max(cap, 1), dtype=PREDICTION_DTYPE)
        Hs = np.zeros((max(cap, 1), 2, 13))
        Hf = np.zeros((max(cap, 1), 2, 6))
        k = _i(0)
        self._chk(self.L.ekf_predict_measurements(self.h, _p(idx), cnt, _p(preds), C.byref(k), _p(Hs), _p(Hf)))
        return preds[: k.value].copy(), Hs[: k.value].copy(), Hf[: k.value].copy()

    def predict_measurement_state(self):
        preds = np.zeros(max(self.N, 1), dtype=PREDICTION_DTYPE)
        k = _i(0)
        self._chk(self.L.ekf_predict_measurement_state(self.h, _p(preds), C.byref(k)))
        return preds[: k.value].copy()

    def match(self, kps, desc):
        kps = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        desc = self._desc(desc)
        out = np.zeros(max(self.N, 1), dtype=MATCH_DTYPE)
        k = _i(0)
        self._chk(self.L.ekf_match(self.h, _p(kps), _p(desc), len(kps), _p(out), C.byref(k)))
        return out[: k.value].copy()

    def ransac(self, matches):
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        mask = np.zeros(max(len(matches), 1), dtype=np.uint8)
        nh = _i(0)
        self._chk(self.L.ekf_ransac(self.h, _p(matches), len(matches), _p(mask), C.byref(nh)))
        return mask[: len(matches)].astype(bool), nh.value

    def update(self, matches, allow_errors=()):
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        return self._chk(self.L.ekf_update(self.h, _p(matches), len(matches)), allow_errors)

    def update_only_state(self, matches):
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        self._chk(self.L.ekf_update_only_state(self.h, _p(matches), len(matches)))

    def update_fixed_map(self, matches, allow_errors=()):
        """The Schmidt-Kalman update of a fixed map (ekf_update_fixed_map): the camera state and the camera's rows
        and columns of P move, the map block of P and the features keep their bits.  Arguments and errors as update()."""
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        return self._chk(self.L.ekf_update_fixed_map(self.h, _p(matches), len(matches)), allow_errors)

    def set_fixed_map(self, on=True):
        """on: both covariance updates of every step become fixed-map updates (ekf_set_fixed_map); update(), update_only_state(),
        update_external() and map management are not affected.  Refused on a sharded engine and in EKF_PRECISION_F32."""
        self._chk(self.L.ekf_set_fixed_map(self.h, 1 if on else 0))

    def fixed_map(self):
        """(mode on?, fixed-map updates applied since the engine was created); synchronises the stream"""
        on, k = _i(0), C.c_int64(0)
        self._chk(self.L.ekf_get_fixed_map(self.h, C.byref(on), C.byref(k)))
        return bool(on.value), int(k.value)

    # ---- iterated update
    def update_iterated(self, matches, iterations, tol=0.0, allow_errors=()):
        """The covariance update in up to `iterations` passes (ekf_update_iterated): the measurement is linearised again at every
        new estimate and the update solved again from the prior; iterations = 1 is update().  tol > 0: a pass that moved no state by
        tol prior standard deviations makes the next pass the last.  Arguments and errors as update()."""
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        return self._chk(self.L.ekf_update_iterated(self.h, _p(matches), len(matches), int(iterations), float(tol)), allow_errors)

    def set_update_iterations(self, iterations, tol=0.0):
        """both updates of every step run up to `iterations` passes (ekf_set_update_iterations); 1, the default: the plain updates.
        Refused on a sharded engine and, above 1, while the fixed-map mode is on."""
        self._chk(self.L.ekf_set_update_iterations(self.h, int(iterations), float(tol)))

    def update_iterations(self):
        """(iterations, tol) of the step functions"""
        k, t = _i(0), C.c_double(0.0)
        self._chk(self.L.ekf_get_update_iterations(self.h, C.byref(k), C.byref(t)))
        return int(k.value), float(t.value)

    def iteration_records(self):
        """ITERATION_RECORD_DTYPE [0..2]: the iterated updates of the last update_iterated() or step (stage, passes_run, stop_reason,
        step[8]); synchronises the stream"""
        out = np.zeros(2, dtype=ITERATION_RECORD_DTYPE)
        n = _i(0)
        self._chk(self.L.ekf_get_iteration_records(self.h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def linearisation_point(self):
        """(x13, feature_pos [N, 6]) at which the last iterated update linearised its covariance pass; synchronises the stream"""
        x, fp = np.zeros(13), np.zeros((max(self.N, 1), 6))
        self._chk(self.L.ekf_get_linearisation_point(self.h, _p(x), _p(fp)))
        return x, fp[: self.N].copy()

    def rescue(self, outliers):
        outliers = np.ascontiguousarray(outliers, dtype=MATCH_DTYPE)
        mask = np.zeros(max(len(outliers), 1), dtype=np.uint8)
        self._chk(self.L.ekf_rescue(self.h, _p(outliers), len(outliers), _p(mask)))
        return mask[: len(outliers)].astype(bool)

    def step(self, kps, desc):
        kps = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        desc = self._desc(desc)
        info = EkfStepInfo()
        self._chk(self.L.ekf_step(self.h, _p(kps), _p(desc), len(kps), C.byref(info)))
        return info

    # ---- staged sequences
    def upload_frames(self, frames):
        if len(frames) == 0:  # drops the staged frames
            self._chk(self.L.ekf_frames_upload(self.h, 0, None, None, None))
            return
        counts = np.array([len(k) for k, _ in frames], dtype=np.int32)
        kps = np.ascontiguousarray(np.concatenate([k for k, _ in frames]), dtype=KEYPOINT_DTYPE)
        desc = self._desc(np.concatenate([d for _, d in frames]))
        self._chk(self.L.ekf_frames_upload(self.h, len(frames), _p(counts), _p(kps), _p(desc)))

    def step_frame(self, i):
        info = EkfStepInfo()
        self._chk(self.L.ekf_step_frame(self.h, int(i), C.byref(info)))
        return info

    # ---- matcher mode B (image in)
    @staticmethod
    def _image_args(image):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.ndim == 2:
            h, w = img.shape
            ch = 1
        else:
            h, w, ch = img.shape
        return img, w, h, w * ch, ch

    def upload_image(self, image):
        img, w, h, stride, ch = self._image_args(image)
        self._chk(self.L.ekf_image_upload(self.h, _p(img), w, h, stride, ch))

    def image_level(self, level):
        w, h = C.c_int(0), C.c_int(0)
        self._chk(self.L.ekf_get_image_level(self.h, int(level), None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), dtype=np.uint8)
        self._chk(self.L.ekf_get_image_level(self.h, int(level), _p(out), C.byref(w), C.byref(h)))
        return out

    def capture_templates(self, feat_idx, uv):
        idx = np.ascontiguousarray(feat_idx, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        assert len(idx) == len(uv)
        self._chk(self.L.ekf_capture_templates(self.h, _p(idx), _p(uv), len(idx)))

    def match_ncc(self):
        out = np.zeros(max(self.N, 1), dtype=MATCH_DTYPE)
        n = C.c_int(0)
        self._chk(self.L.ekf_match_ncc(self.h, _p(out), C.byref(n)))
        return out[: n.value]

    def set_template_warp(self, on=True):
        """NCC templates re-rendered from the predicted viewpoint before every search; off: the stored ones"""
        self._chk(self.L.ekf_set_template_warp(self.h, 1 if on else 0))

    def template_warp_counts(self):
        """(levels warped, levels fallen back) in the last NCC match"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_template_warp_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def match_templates(self, feat_idx):
        """the templates the last NCC match compared for the listed features -> uint8 [k, 3, 11, 11]"""
        idx = np.ascontiguousarray(feat_idx, dtype=np.int32)
        out = np.zeros((max(len(idx), 1), 3, 11, 11), dtype=np.uint8)
        self._chk(self.L.ekf_get_match_templates(self.h, _p(idx), len(idx), _p(out)))
        return out[: len(idx)]

    def set_subpixel_matches(self, on=True):
        """NCC matches at the vertex of a parabola through the best pixel's and its neighbours' scores, per axis;
        off: integer pixels"""
        self._chk(self.L.ekf_set_subpixel_matches(self.h, 1 if on else 0))

    def subpixel_counts(self):
        """(axes moved by the fit, axes left at the integer) over the matches of the last NCC match"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_subpixel_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_ncc_wide_search(self, on=True):
        """NCC gates larger than the 43 x 43 coarse window (major semi-axis of 64 px or more) are searched whole;
        off: within 16 coarse pixels of the prediction"""
        self._chk(self.L.ekf_set_ncc_wide_search(self.h, 1 if on else 0))

    def ncc_wide_counts(self):
        """(predictions searched wide, coarse candidates evaluated for them) in the last NCC match"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_ncc_wide_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_ncc_distinct(self, coef):
        """NCC matches with a rival peak in the gate are kept only if distance < rival distance * coef, 0 < coef <= 1
        (DESIGN.md 4.10); 0: off"""
        self._chk(self.L.ekf_set_ncc_distinct(self.h, float(coef)))

    def ncc_distinct_counts(self):
        """(accepted matches that had a rival, those of them rejected) in the last NCC match"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_ncc_distinct_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ncc_rivals(self):
        """NCC_RIVAL_DTYPE [predictions of the last NCC match], in their order; empty with the mode off"""
        out = np.zeros(max(self.cap, 1), dtype=NCC_RIVAL_DTYPE)
        n = _i(0)
        self._chk(self.L.ekf_get_ncc_rivals(self.h, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def set_patch_normals(self, on=True):
        """the warp's patch planes get a normal estimated from the images, one estimator step per image step;
        needs set_template_warp(True); off: every plane faces the camera that captured it"""
        self._chk(self.L.ekf_set_patch_normals(self.h, 1 if on else 0))

    def refine_patch_normals(self, matches):
        """one estimator step on the current image and state for the features of `matches` (MATCH_DTYPE: featureIndex and the
        pixel the feature is seen at)"""
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        self._chk(self.L.ekf_refine_patch_normals(self.h, _p(m), len(m)))

    def patch_normals(self, feat_idx=None):
        """PATCH_NORMAL_DTYPE [k]: slope, information, world normal and update count of the listed features (default: all)"""
        idx = np.ascontiguousarray(np.arange(self.N) if feat_idx is None else feat_idx, dtype=np.int32)
        out = np.zeros(max(len(idx), 1), dtype=PATCH_NORMAL_DTYPE)
        self._chk(self.L.ekf_get_patch_normals(self.h, _p(idx), len(idx), _p(out)))
        return out[: len(idx)]

    def set_patch_normal(self, feat, pq, info=(1.0, 0.0, 1.0)):
        pq = np.ascontiguousarray(pq, dtype=np.float64).reshape(2)
        info = np.ascontiguousarray(info, dtype=np.float64).reshape(3)
        self._chk(self.L.ekf_set_patch_normal(self.h, int(feat), _p(pq), _p(info)))

    def patch_normal_counts(self):
        """(features updated, features left alone) by the last estimator run"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_patch_normal_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def step_image(self, image):
        img, w, h, stride, ch = self._image_args(image)
        info = EkfStepInfo()
        self._chk(self.L.ekf_step_image(self.h, _p(img), w, h, stride, ch, C.byref(info)))
        return info

    def detect_new_features(self, max_new, divide_times=2, mask_ellipse_size=10.0, min_response=1e9):
        """detectNewImageFeatures on the current image -> [k, 2] pixel positions (k <= max_new)."""
        out = np.zeros((max(int(max_new), 1), 2))
        n = C.c_int(0)
        self._chk(self.L.ekf_detect_new_features(self.h, int(max_new), int(divide_times), float(mask_ellipse_size),
                                                 float(min_response), _p(out), C.byref(n)))
        return out[: n.value].copy()

    # ---- image in, descriptor matcher (keypoint detector + BRIEF-32 on the device)
    def set_image_matcher(self, matcher, min_response=1e9):
        """IMAGE_MATCHER_NCC (default) or IMAGE_MATCHER_KEYPOINTS for step_image / step_staged_image; min_response =
        threshold of the keypoint detector on the integer corner measure"""
        self._chk(self.L.ekf_set_image_matcher(self.h, int(matcher), float(min_response)))

    def detect_keypoints(self, min_response=1e9, masked=False, capacity=None, descriptors=True):
        """keypoints of the current image in raster order -> (KEYPOINT_DTYPE [k], uint8 [k, 32]) with k = min(found,
        capacity); masked: only inside the gates of the last full prediction.  Also sets self.last_found."""
        n = _i(0)
        if capacity is None:
            self._chk(self.L.ekf_detect_keypoints(self.h, float(min_response), int(bool(masked)), None, None, 0, C.byref(n)))
            capacity = n.value
        kps = np.zeros(max(int(capacity), 1), dtype=KEYPOINT_DTYPE)
        desc = np.zeros((max(int(capacity), 1), DESC_BYTES), dtype=np.uint8)
        self._chk(self.L.ekf_detect_keypoints(self.h, float(min_response), int(bool(masked)), _p(kps),
                                              _p(desc) if descriptors else None, int(capacity), C.byref(n)))
        self.last_found = n.value
        k = min(n.value, int(capacity))
        return kps[:k].copy(), desc[:k].copy()

    def describe(self, uv):
        """BRIEF-32 of the current image at pixel positions uv [k, 2] (centre: floor(u + 0.5), floor(v + 0.5)) -> [k, 32] u8"""
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        out = np.zeros((max(len(uv), 1), DESC_BYTES), dtype=np.uint8)
        self._chk(self.L.ekf_describe(self.h, _p(uv), len(uv), _p(out)))
        return out[: len(uv)].copy()

    def step_keypoints(self):
        """(detected, kept) keypoints of the last KEYPOINTS-mode image step"""
        a, b = _i(0), _i(0)
        self._chk(self.L.ekf_get_step_keypoints(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def upload_images(self, images):
        arr = np.ascontiguousarray(np.stack(images), dtype=np.uint8)
        n = arr.shape[0]
        _, w, h, stride, ch = self._image_args(arr[0])
        self._chk(self.L.ekf_images_upload(self.h, n, _p(arr), w, h, stride, ch))

    def select_staged_image(self, i):
        self._chk(self.L.ekf_select_staged_image(self.h, int(i)))

    def step_staged_image(self, i):
        info = EkfStepInfo()
        self._chk(self.L.ekf_step_staged_image(self.h, int(i), C.byref(info)))
        return info

    # ---- instrumentation
    def timing(self, on=True):
        self._chk(self.L.ekf_timing_enable(self.h, 1 if on else 0))

    def timing_reset(self):
        self._chk(self.L.ekf_timing_reset(self.h))

    def timing_get(self):
        t = EkfStageTimes()
        self._chk(self.L.ekf_timing_get(self.h, C.byref(t)))
        return t

    def p_update_launches(self):
        """(m_rows[int32], ms[float32]) of every P-update launch since the last timing_reset."""
        k = _i(0)
        self._chk(self.L.ekf_timing_p_update_launches(self.h, 0, None, None, C.byref(k)))
        m = np.zeros(max(k.value, 1), dtype=np.int32)
        ms = np.zeros(max(k.value, 1), dtype=np.float32)
        self._chk(self.L.ekf_timing_p_update_launches(self.h, k.value, _p(m), _p(ms), C.byref(k)))
        return m[: k.value], ms[: k.value]

    def sweep_timing(self):
        """dict: HIP-event ms over the Cholesky sweep's launches, panels, updates, fp64 flops of the factorisations, flops of
        the rows of B formed in the same launches (since the last timing_reset)."""
        ms, fl64, flb = C.c_double(0), C.c_double(0), C.c_double(0)
        panels, updates = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.ekf_timing_sweep(self.h, C.byref(ms), C.byref(panels), C.byref(updates), C.byref(fl64), C.byref(flb)))
        launches, slice_ms = C.c_int64(0), C.c_double(0)
        self._chk(self.L.ekf_timing_sweep_launches(self.h, C.byref(launches), C.byref(slice_ms)))
        return {"ms": ms.value, "panels": panels.value, "updates": updates.value, "flops_fp64": fl64.value, "flops_b": flb.value,
                "launches": launches.value, "slice_ms": slice_ms.value}

    def round_covariance_to_f32(self):
        """fp64 engines: every entry of P to its nearest fp32 value, in place (storage-floor measurements)."""
        self._chk(self.L.ekf_round_covariance_to_f32(self.h))

    def synchronize(self):
        self._chk(self.L.ekf_synchronize(self.h))
