// engine_host.h -- host helpers shared by engine.cpp (C ABI, argument checking, copies) and step.cpp (counter read-back, stage
// cores, EKF::step).  Internal: nothing here is part of the library's interface.
#pragma once
#include "engine.h"

#include <string>
#include <vector>

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
int exchange_rows(EkfEngine *e, int what, void *base, size_t row_bytes, const std::vector<int32_t> &rb, const char *name);
int fixed_map_scratch(EkfEngine *e);
int match_ncc_dev(EkfEngine *e, int *n_matches);
int detect_step_keypoints(EkfEngine *e);

// ---- step.cpp
int read_counts(EkfEngine *e); // the device counter block -> e->h_counts
int validate_matches(const EkfEngine *e, const EkfMatch *m, int M);
int finish_update(EkfEngine *e);
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
