// kernels_budget.hip -- measurement budget (ekf_set_measurement_budget): of the np features a step's full prediction
// sees, the K whose measurement carries most information about the state go on to the H P pass, the matcher and the updates.  The
// information of feature i is 0.5 ln(det S_i / det R); with R = pixelErrorX I for every feature the ranking is that of det S_i, and
// S_i needs 13 x 13 entries of P, not the feature's rows of H P.  No counterpart in the reference.
//
//   k_budget_score  one wavefront per predicted feature: S_i = H_i P H_i' + I into pred_S, key_i = det(S_i - I + r I)
//   k_budget_rank   one thread per predicted feature: rank_i = #{j : key_j > key_i, or equal and feature j < feature i}, the selected
//                   flag and the EkfMeasurementRank record
//   k_compact       (kernels_predict.hip) flags -> the predicted list handed on, in feature order
//
// Compiled without FMA contraction like k_hp_rows, whose chunk 0 forms the same S_i with the same operations in the same order.
#include "engine.h"

namespace ekf {

constexpr int SCORE_WAVES = 4; // predicted features per workgroup of k_budget_score
constexpr int SCORE_W = 13;    // columns / rows of P one feature touches at most: 7 of the camera, 6 of its own
constexpr int RANK_BLOCK = 256;

// The gathered block of P is held as k_hp_rows holds a column's operands: rows 0..d-1 the feature's own rows pos..pos+d-1, rows
// d..d+6 the camera rows 0..6; columns 0..6 the camera's, 7..7+d-1 the feature's own.
template <typename T>
__global__ void __launch_bounds__(SCORE_WAVES * 64)
k_budget_score(const T *P, int ld, const int *plist, int np, const int *feat_type, const int *feat_covpos, const double *Hs_tab,
               const double *Hf_tab, double pixel_err, double *S_tab, double *key, const int *counts)
{
    if (filter_frozen(counts)) return;
    __shared__ double sP[SCORE_WAVES][SCORE_W * SCORE_W];
    __shared__ double sH[SCORE_WAVES][26];     // Hs (2x7) then Hf (2x6)
    __shared__ double sHP[SCORE_WAVES][2][13]; // fp64 H P at columns 0..6 and pos..pos+d-1
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slot = (int)blockIdx.x * SCORE_WAVES + wv;
    const bool live = slot < np;
    int fi = 0, d = 0, pos = 0;
    if (live) {
        fi = plist[slot];
        d = feat_dim(feat_type[fi]);
        pos = feat_covpos[fi];
    }
    const int w = 7 + d;
    if (live) {
        for (int i = lane; i < w * w; i += 64) {
            const int a = i / w, c = i - a * w;
            const int row = a < d ? pos + a : a - d;
            const int col = c < 7 ? c : pos + (c - 7);
            sP[wv][a * SCORE_W + c] = (double)P[(size_t)row * ld + col];
        }
        if (lane < 14) sH[wv][lane] = Hs_tab[14 * fi + lane];
        else if (lane < 26) sH[wv][lane] = Hf_tab[12 * fi + lane - 14];
    }
    __syncthreads();
    if (live && lane < w) { // one lane per column: a0 + b0 as in k_hp_rows
        const double *h = sH[wv], *p = sP[wv] + lane;
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        for (int a = 0; a < d; ++a) {
            a0 += h[14 + a] * p[a * SCORE_W];
            a1 += h[20 + a] * p[a * SCORE_W];
        }
        for (int a = 0; a < 7; ++a) {
            b0 += h[a] * p[(d + a) * SCORE_W];
            b1 += h[7 + a] * p[(d + a) * SCORE_W];
        }
        sHP[wv][0][lane] = a0 + b0;
        sHP[wv][1][lane] = a1 + b1;
    }
    __syncthreads();
    double s = 0.0;
    if (live && lane < 4) { // s1 + s2 + 1 as in k_hp_rows
        const int r = lane >> 1, c = lane & 1;
        double s1 = 0.0, s2 = 0.0;
        for (int a = 0; a < 7; ++a) s1 += sHP[wv][r][a] * sH[wv][c * 7 + a];
        for (int a = 0; a < d; ++a) s2 += sHP[wv][r][7 + a] * sH[wv][14 + c * 6 + a];
        s = s1 + s2 + (r == c ? 1.0 : 0.0);
        S_tab[4 * fi + lane] = s;
    }
    const double s00 = __shfl(s, 0, 64), s01 = __shfl(s, 1, 64), s10 = __shfl(s, 2, 64), s11 = __shfl(s, 3, 64);
    if (live && lane == 0) { // the determinant of the S the filter uses: R = pixelErrorX I, as k_ransac_hyp reads the table
        double k = (s00 - 1.0 + pixel_err) * (s11 - 1.0 + pixel_err) - s01 * s10;
        if (!(k > 0.0)) k = -1.0; // NaN or not positive: ranks last
        key[slot] = k;
    }
}

// All keys stream through LDS in tiles of the block size; every thread counts the ones that beat its own.  The count is exact: no
// floating-point sum, no atomics, nothing that depends on the order workgroups run in.
// The list of a full prediction is in ascending feature order (k_predict_features' work item w is feature w and the compaction
// keeps the order), so "featureIndex_j < featureIndex_i" is "j before i in the list": an entry of a tile in front of the
// workgroup's own beats with >=, one of a tile behind it with >, and only the own tile compares positions.  One comparison per
// entry; the feature indices never enter LDS.
// A frozen filter (filter_frozen) is not ranked: the first K of the list pass, so that the compaction behind this launch still
// writes a list of this prediction's features.
template <int MODE> // 0: tile in front of the own one, 1: behind it, 2: the own tile
__device__ __forceinline__ int rank_tile(const double *skey, double ki, int tid)
{
    int rank = 0;
    // every lane reads the same address (a broadcast).  Eight entries are read before they are compared, without a branch, so that
    // their reads are in flight together: one wavefront per SIMD has nothing else to hide the latency behind
    for (int t0 = 0; t0 < RANK_BLOCK; t0 += 8) {
        double kj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) kj[u] = skey[t0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            rank += MODE == 0 ? (int)(kj[u] >= ki) : MODE == 1 ? (int)(kj[u] > ki) : ((int)(kj[u] > ki) | ((int)(kj[u] == ki) & (int)(t0 + u < tid)));
    }
    return rank;
}

__global__ void __launch_bounds__(RANK_BLOCK)
k_budget_rank(const double *key, const int *plist, int np, int K, double pixel_err, int *all, int *flag, EkfMeasurementRank *recs,
              const int *counts)
{
    __shared__ double skey[RANK_BLOCK];
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x * RANK_BLOCK + tid;
    const bool live = slot < np;
    const int fi = live ? plist[slot] : 0;
    if (filter_frozen(counts)) {
        if (live) {
            all[slot] = fi;
            flag[slot] = slot < K ? 1 : 0;
        }
        return;
    }
    const double ki = live ? key[slot] : 0.0;
    int rank = 0;
    for (int tile = 0; tile * RANK_BLOCK < np; ++tile) {
        const int j = tile * RANK_BLOCK + tid;
        skey[tid] = j < np ? key[j] : -2.0; // past the end (the last tile: the own one or one behind it): below every key, the least is -1
        __syncthreads();
        if (tile < (int)blockIdx.x) rank += rank_tile<0>(skey, ki, tid);
        else if (tile > (int)blockIdx.x) rank += rank_tile<1>(skey, ki, tid);
        else rank += rank_tile<2>(skey, ki, tid);
        __syncthreads();
    }
    if (!live) return;
    const int sel = (np <= K || rank < K) ? 1 : 0;
    all[slot] = fi;
    flag[slot] = sel;
    EkfMeasurementRank r;
    r.featureIndex = fi;
    r.rank = rank;
    r.selected = sel;
    r._pad = 0;
    r.key = ki;
    r.gain = ki > 0.0 ? 0.5 * log(ki / (pixel_err * pixel_err)) : 0.0;
    recs[slot] = r;
}

// d.plist (np predicted features, feature order) -> S_i of all of them in d.pred_S, d.bud_key, d.bud_recs, the selected flags in
// d.bud_flag and a copy of the list in d.bud_all (the compaction writes d.plist itself)
void launch_budget_select(EkfEngine *e, int np, int K)
{
    e->match_gates_valid = false; // pred_S is rewritten here
    if (np <= 0) return;
    const int gs = (np + SCORE_WAVES - 1) / SCORE_WAVES;
#define SCORE_ARGS e->ldP, e->d.plist, np, e->d.feat_type, e->d.feat_covpos, e->d.Hs, e->d.Hf, e->cfg.cam.pixelErrorX, e->d.pred_S, e->d.bud_key, e->d.counts
    if (e->f32) k_budget_score<float><<<gs, SCORE_WAVES * 64, 0, e->stream>>>((const float *)e->d.P, SCORE_ARGS);
    else k_budget_score<double><<<gs, SCORE_WAVES * 64, 0, e->stream>>>((const double *)e->d.P, SCORE_ARGS);
#undef SCORE_ARGS
    k_budget_rank<<<(np + RANK_BLOCK - 1) / RANK_BLOCK, RANK_BLOCK, 0, e->stream>>>(e->d.bud_key, e->d.plist, np, K, e->cfg.cam.pixelErrorX,
                                                                                  e->d.bud_all, e->d.bud_flag, e->d.bud_recs, e->d.counts);
}

} // namespace ekf
