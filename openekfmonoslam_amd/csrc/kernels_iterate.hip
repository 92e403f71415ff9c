// kernels_iterate.hip -- the glue of the iterated EKF update (ekf_update_iterated / ekf_set_update_iterations).
//
// The passes themselves are the engine's own launches: the sub-list prediction (k_predict_features, k_hp_rows) at the current
// estimate x^i and launch_update from the prior x^ (step.cpp: iterated_update_dev).  What is new sits between them:
//   k_iter_snapshot       x^ (state block and every feature), diag(P) of the prior, the matched features as a prediction sub-list
//   k_iter_step           the normalised step of the pass just finished, and x^i into a buffer of its own
//   k_iter_shift_restore  iter_uv = pred_uv + Hs (x^_cam - x^i_cam) + Hf (x^_f - x^i_f) per match, and the live state back to x^
//   k_iter_load           the live state back to an earlier linearisation point (a matched feature left the image)
// A "state image" is ITER_X doubles of the state block (x13 at ST_X, R(q) at ST_R) followed by the 6 N feature parameters.
// The hazard of the shift -- it needs x^i while the restore overwrites it -- does not arise: x^i was copied into its own image by
// k_iter_step, one launch earlier, and no thread of k_iter_shift_restore reads the live state.
// All of them are latency-bound (a few thousand doubles); none uses an atomic.
#include "engine.h"

#include <algorithm>

namespace ekf {

// thread t of the grid owns entry t of the state image
template <typename T>
__global__ void __launch_bounds__(256)
k_iter_snapshot(const double *st, const double *feat_pos, int N, const T *P, int ld, int n, const EkfMatch *matches, int M,
                double *snap, double *lin0, double *diag, int *idx, double *steps)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ITER_X + 6 * N) {
        const double v = t < ITER_X ? st[t] : feat_pos[t - ITER_X];
        snap[t] = v;
        lin0[t] = v;
    }
    if (t < n) diag[t] = (double)P[(size_t)t * ld + t];
    if (t < M) idx[t] = matches[t].featureIndex;
    if (t < EKF_MAX_UPDATE_ITERATIONS) steps[t] = 0.0;
}

// ONE workgroup: the maximum over the state columns j with P_jj > 0 of |x_j - prev_j| / sqrt(P_jj), x the live state.  Lane-local
// over t, t + 1024, ..., down a wavefront by shuffles, across the 16 wavefronts through LDS: a maximum, so the order is immaterial.
// cur != nullptr: the live state is also copied into the image cur, and the tolerance flag is left in the counter block, where
// the read-back of the prediction that follows finds it.
__global__ void __launch_bounds__(1024)
k_iter_step(const double *st, const double *feat_pos, const int *feat_type, const int *feat_covpos, int N, const double *prev,
            double *cur, const double *diag, double *step_out, double tol, int *counts)
{
    __shared__ double wmax[16];
    double mx = 0.0;
    for (int t = threadIdx.x; t < ITER_X + 6 * N; t += 1024) {
        const double v = t < ITER_X ? st[t] : feat_pos[t - ITER_X];
        if (cur) cur[t] = v;
        int j = -1; // the state column of this entry (R(q) and the unused parameters of an XYZ feature have none)
        if (t < 13) j = t;
        else if (t >= ITER_X) {
            const int f = (t - ITER_X) / 6, a = (t - ITER_X) % 6;
            if (a < feat_dim(feat_type[f])) j = feat_covpos[f] + a;
        }
        if (j >= 0) {
            const double d = diag[j];
            if (d > 0.0) mx = fmax(mx, fabs(v - prev[t]) / sqrt(d));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) mx = fmax(mx, wmax[w]);
        *step_out = mx;
        if (cur) counts[CNT_ITER_SMALL] = tol > 0.0 && mx < tol ? 1 : 0;
    }
}

// thread t: match t's two entries of iter_uv (sums in ascending column order: 7 live camera columns, then the feature's 3 or 6),
// and entry t of the state image back into the live state
__global__ void __launch_bounds__(256)
k_iter_shift_restore(const EkfMatch *matches, int M, const double *uv_tab, const double *Hs_tab, const double *Hf_tab, const int *feat_type,
                     const double *snap, const double *lin, double *iter_uv, double *st, double *feat_pos, int N, const int *counts)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < M) {
        const int f = matches[t].featureIndex;
        const int dim = feat_dim(feat_type[f]);
        double dc[7], df[6];
#pragma unroll
        for (int c = 0; c < 7; ++c) dc[c] = snap[ST_X + c] - lin[ST_X + c];
#pragma unroll
        for (int a = 0; a < 6; ++a) df[a] = a < dim ? snap[ITER_X + 6 * f + a] - lin[ITER_X + 6 * f + a] : 0.0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 7; ++c) acc += Hs_tab[14 * f + 7 * r + c] * dc[c];
            for (int a = 0; a < dim; ++a) acc += Hf_tab[12 * f + 6 * r + a] * df[a];
            iter_uv[2 * f + r] = uv_tab[2 * f + r] + acc;
        }
    }
    if (filter_frozen(counts)) return; // a pass failed: x is x^ already and stays so (engine.h)
    if (t < ST_R + 9) st[t] = snap[t];
    else if (t >= ITER_X && t < ITER_X + 6 * N) feat_pos[t - ITER_X] = snap[t];
}

__global__ void __launch_bounds__(256) k_iter_load(const double *img, double *st, double *feat_pos, int N, const int *counts)
{
    if (filter_frozen(counts)) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ST_R + 9) st[t] = img[t];
    else if (t >= ITER_X && t < ITER_X + 6 * N) feat_pos[t - ITER_X] = img[t];
}

static double *lin_image(const EkfEngine *e, int which) { return e->d.iter_lin + (size_t)which * (ITER_X + 6 * (size_t)e->cap); }

void launch_iter_snapshot(EkfEngine *e, const EkfMatch *matches, int M, double *steps)
{
    const int nt = std::max(std::max(ITER_X + 6 * e->N, e->n), std::max(M, EKF_MAX_UPDATE_ITERATIONS));
    const int nb = (nt + 255) / 256;
#define SNAP_ARGS e->ldP, e->n, matches, M, e->d.iter_snap, lin_image(e, 0), e->d.iter_diag, e->d.iter_idx, steps
    if (e->f32) k_iter_snapshot<float><<<nb, 256, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->N, (const float *)e->d.P, SNAP_ARGS);
    else k_iter_snapshot<double><<<nb, 256, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->N, (const double *)e->d.P, SNAP_ARGS);
#undef SNAP_ARGS
}

void launch_iter_step(EkfEngine *e, int prev, int cur, double *step_out, double tol)
{
    k_iter_step<<<1, 1024, 0, e->stream>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos, e->N, lin_image(e, prev),
                                          cur >= 0 ? lin_image(e, cur) : nullptr, e->d.iter_diag, step_out, tol, e->d.counts);
}

// even_frozen: the host is rebuilding the tables of a failed pass in front of its retry (step.cpp) and moves the state itself
void launch_iter_shift_restore(EkfEngine *e, const EkfMatch *matches, int M, int lin, bool even_frozen)
{
    const int nt = std::max(ITER_X + 6 * e->N, M);
    k_iter_shift_restore<<<(nt + 255) / 256, 256, 0, e->stream>>>(matches, M, e->d.pred_uv, e->d.Hs, e->d.Hf, e->d.feat_type, e->d.iter_snap,
                                                                 lin_image(e, lin), e->d.iter_uv, e->d.state, e->d.feat_pos, e->N,
                                                                 even_frozen ? nullptr : e->d.counts);
}

void launch_iter_load(EkfEngine *e, int lin, bool even_frozen)
{
    const int nt = ITER_X + 6 * e->N;
    k_iter_load<<<(nt + 255) / 256, 256, 0, e->stream>>>(lin_image(e, lin), e->d.state, e->d.feat_pos, e->N, even_frozen ? nullptr : e->d.counts);
}

} // namespace ekf
