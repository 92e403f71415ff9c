// reloc_host.cpp -- relocalisation on the map behind the C ABI (see include/ekf_engine.h and DESIGN.md 4.17): argument checking, the
// per-call scratch, the read-back of the result and what an installed pose means for the host's bookkeeping.  The numbers come from
// the kernels in kernels_reloc.hip.
#include "engine_host.h"

#include <cmath>
#include <cstring>

using namespace ekf;

// null, or why the parameters are refused
static const char *reloc_params_refusal(const EkfRelocParams *p)
{
    if (p->hypotheses < 1 || p->hypotheses > RELOC_MAX_HYP) return "hypotheses is outside 1..4096";
    if (p->min_inliers < 4) return "min_inliers is below 4";
    if (!(p->max_distance >= 0.0)) return "max_distance is negative or not a number";
    if (!(p->second_best_coef == 0.0 || (p->second_best_coef > 0.0 && p->second_best_coef <= 1.0))) return "second_best_coef is neither 0 nor in (0, 1]";
    if (!(p->inlier_px > 0.0) || !std::isfinite(p->inlier_px)) return "inlier_px is not a positive number";
    if (!(p->max_rel_depth_sd >= 0.0)) return "max_rel_depth_sd is negative or not a number";
    if (!(p->sigma_position > 0.0) || !std::isfinite(p->sigma_position)) return "sigma_position is not a positive number";
    if (!(p->sigma_angle > 0.0) || !std::isfinite(p->sigma_angle)) return "sigma_angle is not a positive number";
    return nullptr;
}

// what both entry points refuse before anything is enqueued
static int reloc_refusal(EkfEngine *e, const char *who, const EkfRelocParams *p)
{
    const char *why = nullptr;
    if (e->shard_world > 1) why = "not available on a sharded engine";
    else if (e->desc_f32) why = "binary descriptors only: needs an EKF_DESCRIPTOR_U8_HAMMING engine";
    else why = reloc_params_refusal(p);
    if (!why) return EKF_OK;
    e->err = std::string(who) + ": " + why;
    return EKF_ERR_INVALID_ARG;
}

static int reloc_scratch(EkfEngine *e)
{
    if (e->d.reloc_ctl) return EKF_OK;
    const size_t cap = (size_t)e->cap;
    auto g = e->bufs.group();
    g.alloc(&e->d.reloc_ctl, 1);
    g.alloc(&e->d.reloc_X, 3 * cap);
    g.alloc(&e->d.reloc_flag, cap);
    g.alloc(&e->d.reloc_kp, cap);
    g.alloc(&e->d.reloc_dist, cap);
    g.alloc(&e->d.reloc_cand, cap);
    g.alloc(&e->d.reloc_cX, 3 * cap);
    g.alloc(&e->d.reloc_cf, 3 * cap);
    g.alloc(&e->d.reloc_mask, cap);
    g.alloc(&e->d.reloc_hyp, (size_t)RELOC_MAX_HYP);
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "relocalisation scratch");
    return EKF_OK;
}

// the launches, the read-back and the host's side of an installed pose; the stream is drained and no error is pending
static int reloc_run(EkfEngine *e, const RelocCall &call, EkfRelocResult *out)
{
    launch_relocalise(e, call);
    HIPCHK(hipGetLastError());
    RelocCtl ctl;
    HIPCHK(hipMemcpyAsync(&ctl, e->d.reloc_ctl, sizeof(ctl), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (ctl.res.installed) {
        // as after ekf_set_state, as far as the camera goes: no prediction stands and no earlier update is run again.  The map's
        // layout did not change, so the layout mirrors, the gates' snapshot and the linearisation point stay.
        e->n_pred = 0;
        e->match_gates_valid = false;
        e->last_update.persist = false;
        e->last_update.sym = e->p_exact_sym; // (the strip was written to both places of every pair: symmetry is as it was)
        HIPCHK(hipMemsetAsync(e->d.pred_vis, 0, (size_t)e->cap * sizeof(int), e->stream));
        HIPCHK(hipMemsetAsync(e->d.pred_vis_full, 0, (size_t)e->cap * sizeof(int), e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (out) *out = ctl.res;
    return EKF_OK;
}

int ekf_relocalise(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, const EkfRelocParams *params, EkfRelocResult *out)
{
    if (!e || !params) return EKF_ERR_INVALID_ARG;
    if (int rc = reloc_refusal(e, "ekf_relocalise", params)) return rc;
    if (n_kp < 0 || n_kp > e->kcap || (n_kp > 0 && (!kps || !desc32))) {
        e->err = "ekf_relocalise: n_kp = " + std::to_string(n_kp) + " is outside 0.." + std::to_string(e->kcap) + ", or a null keypoint table";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e); // as ekf_update_external: the failed update it reports is not this call's
    if (rc) return rc;
    if ((rc = reloc_scratch(e))) return rc;
    if (n_kp > 0) {
        HIPCHK(hipMemcpyAsync(e->d.kps, kps, (size_t)n_kp * sizeof(EkfKeypoint), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->d.kdesc, desc32, (size_t)n_kp * EKF_DESC_BYTES, hipMemcpyHostToDevice, e->stream));
    }
    RelocCall call;
    call.params = params;
    call.kps = e->d.kps;
    call.kdesc = e->d.kdesc;
    call.n_kp = n_kp;
    return reloc_run(e, call, out);
}

int ekf_relocalise_image(EkfEngine *e, double min_response, const EkfRelocParams *params, EkfRelocResult *out)
{
    if (!e || !params) return EKF_ERR_INVALID_ARG;
    if (int rc = reloc_refusal(e, "ekf_relocalise_image", params)) return rc;
    if (std::isnan(min_response) || !e->img.valid) {
        e->err = "ekf_relocalise_image: no image uploaded, or a NaN threshold";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e);
    if (rc) return rc;
    if ((rc = reloc_scratch(e))) return rc;
    if ((rc = detect_frame_keypoints(e, min_response, false))) return rc; // into d.kps / d.kdesc, the count stays on the device
    RelocCall call;
    call.params = params;
    call.kps = e->d.kps;
    call.kdesc = e->d.kdesc;
    call.n_kp = e->kcap;
    call.d_nkp = e->d.counts + CNT_KP_FOUND;
    return reloc_run(e, call, out);
}

// the counts of the last call (zeros before the first)
static int reloc_counts(EkfEngine *e, RelocCtl *ctl)
{
    std::memset(ctl, 0, sizeof(*ctl));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->d.reloc_ctl) HIPCHK(hipMemcpy(ctl, e->d.reloc_ctl, sizeof(*ctl), hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_get_relocalise_candidates(EkfEngine *e, EkfMatch *out, uint8_t *inlier_mask, int capacity, int *count)
{
    if (!e || !count || (out && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    RelocCtl ctl;
    if (int rc = reloc_counts(e, &ctl)) return rc;
    const int n = ctl.n_cand;
    *count = n;
    if (n == 0 || !out) return EKF_OK;
    if (capacity < n) {
        e->err = "ekf_get_relocalise_candidates: capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " candidates";
        return EKF_ERR_CAPACITY;
    }
    HIPCHK(hipMemcpy(out, e->d.reloc_cand, (size_t)n * sizeof(EkfMatch), hipMemcpyDeviceToHost));
    if (inlier_mask) HIPCHK(hipMemcpy(inlier_mask, e->d.reloc_mask, (size_t)n, hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_get_relocalise_hypotheses(EkfEngine *e, EkfRelocHypothesis *out, int capacity, int *count)
{
    if (!e || !count || (out && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    RelocCtl ctl;
    if (int rc = reloc_counts(e, &ctl)) return rc;
    const int n = ctl.res.n_hypotheses;
    *count = n;
    if (n == 0 || !out) return EKF_OK;
    if (capacity < n) {
        e->err = "ekf_get_relocalise_hypotheses: capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " hypotheses";
        return EKF_ERR_CAPACITY;
    }
    HIPCHK(hipMemcpy(out, e->d.reloc_hyp, (size_t)n * sizeof(EkfRelocHypothesis), hipMemcpyDeviceToHost));
    return EKF_OK;
}
