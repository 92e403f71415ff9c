// engine_host.h -- host helpers shared by engine.cpp (C ABI, argument checking, copies), map_host.cpp (the map's host side: state
// transfer, map blob, map management) and step.cpp (counter read-back, stage cores, EKF::step).  Internal: nothing here is part of
// the library's interface.
#pragma once
#include "engine.h"
#include "feature_tables.h"

#include <string>
#include <vector>

#define NOT_WHEN_SHARDED(e)                                                \
    if ((e)->shard_world > 1) {                                            \
        (e)->err = "map management is not available on a sharded engine";  \
        return EKF_ERR_INVALID_ARG;                                        \
    }

#define HIPCHK(call)                                                                                          \
    do {                                                                                                      \
        hipError_t _st = (call);                                                                              \
        if (_st != hipSuccess) {                                                                              \
            e->err = std::string(#call) + ": " + hipGetErrorString(_st);                                      \
            return EKF_ERR_HIP;                                                                               \
        }                                                                                                     \
    } while (0)

namespace ekf {
#pragma GCC visibility push(hidden)

// element size of H P and of its gathered rows (fp64 beside the exact downdate, else the covariance's)
inline size_t hp_elem_bytes(const EkfEngine *e) { return e->exact ? 8 : (e->f32 ? 4 : 8); }

// the patch-normal estimator's two counters, from a counter block just read back
inline void harvest_pn_counts(EkfEngine *e)
{
    e->pn_counts[0] = e->h_counts[CNT_PN_UPD];
    e->pn_counts[1] = e->h_counts[CNT_PN_SKIP];
}

// ---- engine.cpp
int check_async(EkfEngine *e);
// a failed allocation (DeviceBuffers, or a Group's status): the error text and the code of the call
int alloc_failed(EkfEngine *e, hipError_t st, const char *what);
int exchange_rows(EkfEngine *e, int what, void *base, size_t row_bytes, const std::vector<int32_t> &rb, const char *name);
int fixed_map_scratch(EkfEngine *e);
int match_ncc_dev(EkfEngine *e, int *n_matches);
int detect_step_keypoints(EkfEngine *e);
int detect_frame_keypoints(EkfEngine *e, double min_response, bool masked);

// ---- map_host.cpp: the optional per-feature tables (feature_tables.h), each group allocated whole and zeroed, or not at all.  Nothing
// when the group exists; the caller has set the device and drained the stream.
int ensure_warp_tables(EkfEngine *e);         // d.wsrc, d.wpose and the match's cache d.wtmpl (ekf_set_template_warp, ekf_load_map)
int ensure_patch_normal_tables(EkfEngine *e); // d.wnorm and d.pn_list (ekf_set_patch_normals, ekf_load_map)

// ---- step.cpp
int read_counts(EkfEngine *e); // the device counter block -> e->h_counts
int validate_matches(const EkfEngine *e, const EkfMatch *m, int M);
int finish_update(EkfEngine *e);
// With ekf_set_async_errors a step does not read the error flag of its last update back; the flag is sticky on the
// device and is reported (and cleared) by the next step, by ekf_synchronize or by ekf_get_state, whichever comes first.
inline int take_pending_error(EkfEngine *e) { return e->async_errors ? finish_update(e) : EKF_OK; }
// body of ekf_update, ekf_update_only_state and ekf_update_fixed_map: one update of kind UPDATE_* with a caller's match list
int update_stage(EkfEngine *e, const EkfMatch *matches, int M, int kind);
void harvest_pu_events(EkfEngine *e);

// what a step matches its predictions against
enum StepSource {
    STEP_KEYPOINTS,        // keypoints and descriptors already on the device (uploaded or staged)
    STEP_DETECT_KEYPOINTS, // detected and described on the device from the loaded image, into d.kps / d.kdesc (n_kp: their capacity)
    STEP_NCC               // the NCC matcher on the loaded image: no keypoints
};
struct StepInput {
    StepSource source = STEP_KEYPOINTS;
    const EkfKeypoint *d_kps = nullptr;
    const uint8_t *d_desc = nullptr;
    int n_kp = 0;
};
// EKF::step (EKF.cpp:242-556) over the interval e->step_dt
int run_step(EkfEngine *e, const StepInput &in, EkfStepInfo *info);

#pragma GCC visibility pop
} // namespace ekf
