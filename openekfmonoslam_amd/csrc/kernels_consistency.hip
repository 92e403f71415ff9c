// kernels_consistency.hip -- filter consistency (ekf_set_consistency): the normalised innovation squared of a
// covariance update and, per match, the innovation, its marginal Mahalanobis distance and its conditional share of the NIS.
//
// Every sweep of kernels_update.hip leaves z = inv(L) nu in d.zvec (L the Cholesky factor of S = H P H' + R): NIS = |z|^2 costs
// one pass over 2 M doubles, and z_2i^2 + z_2i+1^2 is what match i adds given the matches before it.  The marginal distance of a
// match needs its own 2 x 2 block of S only, which the prediction that every update follows has left in the prediction table
// (pred_S = H_i P H_i' + I, formed from the same H P rows the update gathers; kernels_ransac.hip reads it the same way).
// The innovation is formed again exactly as gather_body forms it: the sweep consumes d.nu.
#include "engine.h"

namespace ekf {

// One workgroup: m <= 2 cap rows, a few microseconds of latency like k_map_points.  The sum runs in ONE order -- lane-local over
// i = t, t + 256, ..., down the 64 lanes of a wavefront by shuffles, then the four wavefronts' partials from LDS as
// (p0 + p1) + (p2 + p3) -- and thread 0 alone writes the header and adds to the totals, in stream order: two runs give the same
// bits.  Writes d.cons_ctl / d.cons_recs only; with the error flag set (S not positive definite, a row of B not finite, a
// persistent sweep that timed out and will be run again) it writes nothing, and the retry's own launch records the update.
__global__ void __launch_bounds__(256)
k_consistency(const double *zvec, const EkfMatch *matches, int M, const double *uv_tab, const double *S_tab, double pixel_err,
              const int *counts, int stage, int epoch, int slot_stride, ConsCtl *ctl, EkfInnovation *recs)
{
    if (counts[CNT_ERR] != 0) return;
    __shared__ double part[4];
    __shared__ int s_slot;
    const int t = threadIdx.x;
    if (t == 0) s_slot = ctl->epoch == epoch ? ctl->count : 0;
    __syncthreads();
    const int slot = s_slot;
    if (slot >= CONS_SLOTS) return; // (a third covered update in one epoch does not exist; the tables hold two)
    EkfInnovation *out = recs + (size_t)slot * slot_stride;
    double acc = 0.0;
    for (int i = t; i < M; i += 256) {
        const EkfMatch mt = matches[i];
        const int fi = mt.featureIndex;
        double nu[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double a = mt.imagePos[c] - uv_tab[2 * fi + c];
            nu[c] = fabs(a) > EKF_DELTA ? a : 0.0;
        }
        // S_i = H_i P H_i' + R with R = I * pixelErrorX; the table holds H_i P H_i' + I
        const double s00 = S_tab[4 * fi] - 1.0 + pixel_err, s01 = S_tab[4 * fi + 1], s10 = S_tab[4 * fi + 2],
                     s11 = S_tab[4 * fi + 3] - 1.0 + pixel_err;
        const double det = s00 * s11 - s01 * s10;
        const double z0 = zvec[2 * i], z1 = zvec[2 * i + 1];
        const double ci = z0 * z0 + z1 * z1;
        EkfInnovation r;
        r.featureIndex = fi;
        r.stage = stage;
        r.nu[0] = nu[0];
        r.nu[1] = nu[1];
        r.d2_marginal = det > 0.0 ? (nu[0] * (s11 * nu[0] - s01 * nu[1]) + nu[1] * (s00 * nu[1] - s10 * nu[0])) / det : 1e300;
        r.nis_conditional = ci;
        r._reserved = 0.0;
        out[i] = r;
        acc += ci;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((t & 63) == 0) part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const double nis = (part[0] + part[1]) + (part[2] + part[3]);
        EkfUpdateConsistency h;
        h.stage = stage;
        h.matches = M;
        h.rows = 2 * M;
        h._pad = 0;
        h.nis = nis;
        ctl->rec[slot] = h;
        ctl->epoch = epoch;
        ctl->count = slot + 1;
        ctl->nis_sum += nis;
        ctl->rows_sum += 2 * M;
        ctl->updates += 1;
    }
}

void launch_consistency(EkfEngine *e, const EkfMatch *matches, int M, int stage, const double *uv_tab)
{
    if (M <= 0 || M > e->cap || !e->d.cons_ctl || !e->d.cons_recs) return;
    k_consistency<<<1, 256, 0, e->stream>>>(e->d.zvec, matches, M, uv_tab, e->d.pred_S, e->cfg.cam.pixelErrorX, e->d.counts,
                                           stage, e->cons_epoch, e->cap, e->d.cons_ctl, e->d.cons_recs);
}

} // namespace ekf
