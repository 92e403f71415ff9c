// engine.h -- internal layout of the device-resident filter and the kernel launchers (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ekf_engine.h"
#include "device_buffers.h"
#include "device_math.h"
#include "map_blob.h" // the per-feature row sizes
#include "patch_normal.h"
#include "update_route.h" // NB, LD_ALIGN, B_SWEEP_MAX, round_up and the route of an update

namespace ekf {

constexpr int DX_SPLIT = 16;    // k-splits of the dx = B' z reduction
constexpr int RANSAC_WIDE_FACTOR = 8; // hypotheses per launch behind a frame's first batch, in units of cfg.ransac_batch (engine.cpp)
#ifndef PX_S_VALUE
#define PX_S_VALUE 5
#endif
constexpr int PX_S = PX_S_VALUE; // EKF_PRECISION_F32_EXACT: balanced base-256 digits per element of B (kernels_pexact.hip)
// rows of B up to which the int32 level sums of the exact downdate cannot wrap: PX_S products of |d d'| <= 2^14 per level and row
constexpr int PX_MAX_ROWS = ((1 << 17) / PX_S) / 32 * 32; // 26208 at PX_S = 5

// Row storage of P.  A rank keeps the 13 camera rows (replicated on every rank) at local rows 0..12 and the
// global rows [r0, r1) it owns from local row `base` on; every row holds ALL n columns.  Unsharded engine:
// r0 = base = 13, r1 = n, i.e. the identity.  Sharded: base = SHARD_BASE so that the owned block
// starts on a tile boundary of the downdate kernel.
constexpr int SHARD_BASE = 128;
struct RowMap {
    int r0, r1, base;
};
__host__ __device__ inline int local_row(const RowMap &m, int i) { return i < 13 ? i : m.base + (i - m.r0); }
__host__ __device__ inline bool owns_row(const RowMap &m, int i) { return i < 13 || (i >= m.r0 && i < m.r1); }

// distinctiveness test of the NCC matcher: what it found for one prediction slot
struct NccRivalRec {
    int state;  // 0 = not a valid match, 1 = valid and no rival, 2 = rival and kept, 3 = rival and rejected
    int rx, ry; // level-0 pixel of the refined rival (states 2, 3; else 0)
    float d1;   // 1 - sqrt(key) of the best (states 1, 2, 3; else 0)
    float d2;   // ... and of the rival (states 2, 3; else 0)
};

// integer slots of the device counter block
enum {
    CNT_NPRED = 0,    // predictions of the last full prediction
    CNT_NPRED_SUB,    // predictions of the last subset prediction
    CNT_NMATCH,       // matches produced by k_match
    CNT_ERR,          // sticky error flag (Cholesky breakdown, ...)
    CNT_RS_BEST,      // RANSAC: best support size
    CNT_RS_BESTH,     // RANSAC: hypothesis index of the best
    CNT_RS_NHYP,      // RANSAC: adaptive hypothesis bound
    CNT_RS_NEXT,      // RANSAC: next hypothesis to examine
    CNT_RS_DONE,      // RANSAC: loop finished
    CNT_NRESC,        // rescued count
    CNT_KP_FOUND,     // keypoints the detector found in the current image (k_kp_compact)
    CNT_SUBPIX_INT,   // sub-pixel NCC matches: axes of valid matches left at the integer by the last NCC match (k_ncc_match<true>)
    CNT_SHARD0,       // sharded filter: CNT_SHARD0 + r = first entry of a feature-sorted match list that rank r owns
                      // (r = 0 .. world, at most 16 ranks: slots 12 .. 28; k_shard_bounds)
    CNT_WARP_OK = 29, // template warp: levels re-rendered for the last NCC match (k_ncc_warp)
    CNT_WARP_FB,      // ... and levels that fell back to the stored template
    CNT_SUBPIX_FIT,   // sub-pixel NCC matches: axes of valid matches moved by the parabola fit (the others: CNT_SUBPIX_INT)
    CNT_WIDE_SLOTS,   // wide search: prediction slots whose gate exceeds the 43 x 43 window in the last NCC match (k_ncc_wide_classify)
    CNT_WIDE_CANDS,   // ... and the coarse candidates evaluated for them, saturating at INT_MAX (k_ncc_wide_finish)
    CNT_PN_UPD,       // patch normals: features whose estimate the last estimator launch updated (k_ncc_normal)
    CNT_PN_SKIP,      // ... and listed features it left alone (no source patch, no usable level, solve not finite)
    CNT_RIVAL_WITH,   // distinctiveness test: accepted matches of the last NCC match that had a rival in the gate (k_ncc_match<.., true>)
    CNT_RIVAL_REJ,    // ... and those of them the test rejected
    CNT_ITER_SMALL,   // iterated update: the normalised step of the pass just finished is below the call's tolerance (k_iter_step)
    CNT_COUNT = 40    // (publish_counts_block / k_publish_counts copy with the lanes t < 64; the mirror page holds 64 ints)
};
constexpr int MAX_SHARD_WORLD = 16;

// filter consistency (ekf_set_consistency): the device-resident control block of k_consistency.  A step or an
// ekf_update begins a new epoch on the host; the first record written under a new epoch takes slot 0.
constexpr int CONS_SLOTS = 2; // covered updates of one epoch: a step's first (LI) and second (HI) update
struct ConsCtl {
    int epoch;                          // epoch of the records below
    int count;                          // records of that epoch, 0 .. CONS_SLOTS
    double nis_sum;                     // running totals since the last ekf_reset_consistency_totals, added in stream order
    long long rows_sum, updates;
    EkfUpdateConsistency rec[CONS_SLOTS];
};

// doubles in the device state block
enum { ST_X = 0, ST_R = 13, ST_F = 32, ST_GQG = 32 + 169, ST_JN = 32 + 338, ST_COUNT = 32 + 338 + 16 };

// external measurement update (ekf_update_external): what a call uploads, and the record its solve kernel leaves
constexpr int EXT_ROWS = EKF_EXT_MAX_ROWS, EXT_NNZ = EKF_EXT_MAX_NNZ, EXT_ENTRIES = EXT_ROWS * EXT_NNZ;
enum { EXT_APPLIED = 0, EXT_GATED = 1, EXT_NOT_PD = 2 }; // ExtResult::verdict; the kernels behind the solve return unless APPLIED
struct ExtCtl {
    double val[EXT_ENTRIES];      // H in CSR form over state indices, rows one behind the other
    double R[EXT_ROWS * EXT_ROWS]; // leading dimension EXT_ROWS; the upper triangle is read
    double residual[EXT_ROWS];
    double gate_nis;              // 0: no gate
    int col[EXT_ENTRIES];
    int row_start[EXT_ROWS + 1];
    int m;
};
struct ExtResult {
    EkfExternalUpdate out;
    int verdict, pad;
};

// iterated update: doubles of the state block in front of the feature parameters of a state image; updates of one
// call that keep a record (a step's two)
constexpr int ITER_X = ST_F, ITER_SLOTS = 2;

// fixed-map update: x_save is written by the strip kernel for the tail, whose workgroups each need the camera state
// as it was while one of them rewrites it; updates is incremented by the tail of every update that was applied
constexpr int FM_LD = 16; // leading dimension of the m x 13 tables B_c and K_c'
struct FmCtl {
    double x_save[13];
    long long updates;
};

// map blob (ekf_save_map / ekf_load_map): what the kernels of kernels_mapblob.hip accumulate over a P section
struct MapBlobCtl {
    unsigned long long sum; // the section's checksum (map_blob.h)
    unsigned non_finite;    // entries that are not finite (k_map_check)
    unsigned bad_diag;      // diagonal entries that are not > 0 (k_map_check)
    unsigned asym, pad;     // entries above the diagonal whose bits differ from their mirror's (k_map_asym)
};

// relocalisation (ekf_relocalise): the counts its kernels hand on, and the result its last kernel leaves
constexpr int RELOC_MAX_HYP = EKF_RELOC_MAX_HYPOTHESES;
struct RelocCtl {
    int n_used, n_cand; // features that took part / candidates (k_reloc_compact)
    int pad[2];
    EkfRelocResult res; // k_reloc_select
};

// 1-point RANSAC: what a hypothesis needs of one match, gathered once per frame by the launch that writes the feature -> match index
// (k_match_compact on the step path, k_match_index behind an arbitrary list) so that the hypotheses' workgroups read ONE contiguous
// record per match instead of chasing match -> feature -> type / position / parameters through four tables each
struct RansacRec {
    double fp[6];  // the feature's parameters
    double img[2]; // the matched image position
    int f;         // feature index, -1: outside the map (such a match supports nothing)
    int type, pos; // feature type, covariance position
    int pad;
};

struct DeviceArrays {
    // map + state
    double *state = nullptr;    // ST_COUNT doubles: x13, R, F, GQG, Jnorm
    double *feat_pos = nullptr; // 6 per feature
    int *feat_type = nullptr;
    int *feat_covpos = nullptr;
    uint8_t *feat_desc = nullptr;
    unsigned *feat_times_predicted = nullptr; // MapFeature::timesPredicted / timesMatched (EKF/MapFeature.h:72-73)
    unsigned *feat_times_matched = nullptr;
    void *P = nullptr; // T [ncap x ldP]
    void *P2 = nullptr; // second buffer of the same size, allocated by the first out-of-place pass (compaction, batch conversion: its target)
    double *mm_scratch = nullptr; // map management scratch: Jpo/Jhr of a batch, 3 x ldP conversion rows, N linearity values
    int *mm_index = nullptr;      // new2old row map (ncap ints)
    // batch conversion (ekf_convert_all_inverse_depth_to_depth; allocated by its first conversion)
    int *ca_rows = nullptr;       // per row u of the new matrix: first source row s(u), then row 3 k + a of ca_J or -1 for a kept row (2 x ncap ints)
    double *ca_J = nullptr;       // the 3 x 6 Jacobian of the k-th converted feature, in ascending feature order (18 x cap doubles)
    int *ca_sel = nullptr;        // the converted feature indices, ascending (cap ints)
    double *cam_ahead = nullptr;  // ekf_predict_camera_ahead: 13 + 169 doubles, the only thing its kernel writes
    EkfMapPoint *map_points = nullptr; // ekf_get_map_points: cap records, allocated by its first call
    // prediction tables, keyed by feature index
    int *pred_vis = nullptr;      // visibility per feature, latest prediction (full or subset)
    int *pred_vis_full = nullptr; // visibility per feature, last FULL prediction (the step's unseenFeatures)
    EkfPrediction *step_preds = nullptr; // snapshot of the last full prediction (ekf_keep_step_predictions)
    double *pred_uv = nullptr; // 2 per feature
    int *pred_vis2 = nullptr;    // scratch copies for state-only predictions
    double *pred_uv2 = nullptr;
    double *pred_S = nullptr;  // 4 per feature
    double *match_gates = nullptr; // 5 per feature: the descriptor matcher's Gate (gate.h) of the last full prediction, see match_gates_valid
    double *Hs = nullptr;      // 2x7 per feature
    double *Hf = nullptr;      // 2x6 per feature
    void *HP = nullptr;        // T [2*cap x ldP]: rows 2f, 2f+1 = H_f P   (fp64 in EKF_PRECISION_F32_EXACT)
    // work lists
    int *work_idx = nullptr;   // input feature indices of a subset prediction
    int *work_flag = nullptr;  // per work item: predicted?
    int *plist = nullptr;      // compacted feature indices, full prediction
    int *plist_sub = nullptr;  // compacted feature indices, subset prediction
    int *counts = nullptr;     // CNT_COUNT ints
    int *shard_feat = nullptr; // sharded filter: first feature of every rank, world + 1 ints
    // keypoints of the current frame
    EkfKeypoint *kps = nullptr;
    uint8_t *kdesc = nullptr;
    // matching
    int *mt_valid = nullptr;  // per prediction slot
    int *mt_kp = nullptr;
    float *mt_dist = nullptr;
    EkfKeypoint *mt_xy = nullptr; // NCC matcher: matched pixel per prediction slot
    NccRivalRec *mt_rival = nullptr; // NCC matcher, distinctiveness test (ekf_set_ncc_distinct): per prediction slot
    uint8_t *tmpl = nullptr;      // NCC matcher: 3 levels x 121 bytes per feature
    // template warp (ekf_set_template_warp; allocated by its first call)
    uint8_t *wsrc = nullptr;      // 3 levels x 41 x 41 source bytes per feature
    double *wpose = nullptr;      // 9 per feature: capture position r0, quaternion q0 (all zero: no source patch), capture pixel
    uint8_t *wtmpl = nullptr;     // the templates the match compares with the mode on: same layout as tmpl
    // patch normals (ekf_set_patch_normals; allocated by its first call)
    PatchNormalRec *wnorm = nullptr; // one record per feature, beside wpose (all zero: no estimate)
    EkfMatch *pn_list = nullptr;     // the matches the estimator is handed: a frame's inliers, then its rescued (cap records)
    // wide search (ekf_set_ncc_wide_search; allocated by its first match)
    void *wide_list = nullptr;    // WideSlot per wide prediction slot, slot order (kernels_ncc.hip), cap records + one WideTotals
    void *wide_part = nullptr;    // WidePartial per (wide slot, tile of the coarse level): cap x wide_tiles records
    double *gates = nullptr;      // new-feature detector: gate + centre + radius (8 doubles) per prediction of the last full prediction
    unsigned long long *kp_rowmask = nullptr; // keypoint detector: one bit per pixel of the frame, 64-pixel row segments
    EkfKeypoint *det_kps = nullptr;  // ekf_detect_keypoints / ekf_describe: output staging (det_cap entries)
    uint8_t *det_desc = nullptr;
    int *det_centres = nullptr;      // ekf_describe: integer centres
    long long *cell_resp = nullptr; // detector: best response per 16x16 cell
    int *cell_xy = nullptr;         // detector: its pixel
    EkfMatch *matches = nullptr; // compacted matches (prediction order) / uploaded matches
    EkfMatch *msel = nullptr;    // matches selected for an update (inliers / rescued), update order
    EkfMatch *mout = nullptr;    // outlier matches
    EkfPrediction *preds_out = nullptr; // staging for prediction downloads
    int *match_of_feat = nullptr;
    // RANSAC
    RansacRec *ransac_rec = nullptr; // mcap records, one per match of the list match_of_feat indexes
    int *hyp_count = nullptr;
    uint8_t *hyp_flags = nullptr;  // batch x mcap
    uint8_t *best_flags = nullptr; // mcap
    // update
    void *G = nullptr;   // T [(mcap + 1) x ldP] : rows of H P gathered for the selected matches
    void *A = nullptr;   // T [(mcap + 1) x ldP] : B = inv(L) G  (k-major operand of the downdate)
    double *S = nullptr;  // (mcap + slack) x ldS: lower triangle of S, updated in place by the sweep
    double *LL = nullptr; // same shape: L below the 32x32 diagonal blocks and L' mirrored above them
    float *LLf = nullptr; // fp32 covariance: the mirrored part (L') again in fp32, the A operand of the rows of B
    double *Tbuf = nullptr; // [mw x ldW] scratch of the doubling steps (T = L21 X11)
    double *nu = nullptr;
    double *Dinv = nullptr; // V = inv(L), row-major [mw x ldW], built up from 32x32 diagonal blocks by doubling
    double *W = nullptr;    // W = inv(L)' (upper triangular), row-major [mw x ldW]: the k-major operand of B = W' G
    float *Wf = nullptr;    // fp32 copy of W (fp32 configuration)
    double *mHs = nullptr;  // per selected match
    double *mHf = nullptr;
    int *mpos = nullptr;
    int *mdim = nullptr;
    double *dx_part = nullptr; // DX_SPLIT x ldP (+ 4: the quaternion as it was before the update)
    double *sq_part = nullptr; // DX_SPLIT x ldP: partial sums of squares of the columns of B (fp64 diagonal of B'B)
    double *diag_save = nullptr; // ldP: diagonal of P before a downdate
    double *cam_part = nullptr;  // DX_SPLIT x 13 x ldP: partial sums of the camera rows of B'B (fp64): the fast fp32 configuration's repair,
                                 // and the fixed-map update's strip (never both: that configuration refuses the fixed-map update)
    double *cam_save = nullptr;  // 13 x ldP: camera rows of P before a downdate
    double *HPc = nullptr;       // [2 cap x 16]: fp64 camera columns of the H P rows
    double *Gc = nullptr;        // [(mcap + slack) x 16]: those of the gathered rows (working right-hand sides of the sweep)
    double *Bc = nullptr;        // [(mcap + slack) x 16]: inv(L) Gc, the fp64 camera columns of B
    double *zvec = nullptr;      // [mcap + slack]: z = inv(L) nu (nu itself is the sweep's working vector)
    double *yvec = nullptr;      // [mcap + slack]: y = inv(L)' z = inv(S) nu (fp32 configuration: dx = (H P)' y)
    uint8_t *mask = nullptr;   // generic byte mask output (rescue)
    void *pu_tilemap = nullptr; // int2 (ti, tj) per upper-triangle tile, XCD-friendly order
    void *sweep_ctl = nullptr;  // flags of the persistent Cholesky sweep (chol_persist.h), zeroed once
    int8_t *Bq = nullptr;       // EKF_PRECISION_F32_EXACT: PX_S digit planes of B, each [bq_rows / 16][ldP][16] bytes (kernels_pexact.hip)
    int *Bexp = nullptr;        // its column scales (biased exponents), ldP ints
    uint8_t *Bz = nullptr;      // ... and which 16-row x 32-column pieces of digit plane 0 hold anything but zeros: [column / 32][bz_stride] bytes
                                // (written with the planes' last reader before the downdate, k_dx_planes / k_slice_B; read by k_p_update_i8p)
    uint8_t *Wz = nullptr, *Gz = nullptr; // the same tables for the planes of inv(L)' and of G (B = inv(L) G above B_SWEEP_MAX rows)
    int8_t *Lq = nullptr;       // digit planes of L for the rows of B formed from planes (chol_bplanes.h): PX_S x lq_nbk^2 KB
    int *Lexp = nullptr;        // row scales of L (biased exponents)
    int *Grow = nullptr;        // row of the H P table behind every gathered row (k_gather without the copy)
    int8_t *Wq = nullptr, *Gq = nullptr; // digit planes of inv(L)' and of G for B = inv(L) G on the int8 MFMA (updates above B_SWEEP_MAX rows)
    int *Wexp = nullptr, *Gexp = nullptr; // their column scales
    // external measurement update (ekf_update_external; one group, allocated by its first call)
    double *ext_A = nullptr;      // (EXT_ROWS + 1) x ldP: A = H P, overwritten by B = inv(L) A; the row behind them is dx = B' z
    double *ext_sel = nullptr;    // EXT_ROWS x EXT_ENTRIES: A[i, col_e] for every entry e of H, what S = A H' + R reads
    ExtCtl *ext_ctl = nullptr;
    ExtResult *ext_res = nullptr;
    // fixed-map update (ekf_update_fixed_map / ekf_set_fixed_map; one group, allocated by the first use)
    FmCtl *fm_ctl = nullptr;      // the camera state as it was before the update, and the count of updates applied
    double *fm_gain = nullptr;    // 2 x [mw x FM_LD]: B_c = inv(L) G[:, 0:13] and K_c' = inv(L)' B_c (updates whose route forms no rows of B)
    ConsCtl *cons_ctl = nullptr;        // filter consistency (ekf_set_consistency; allocated by its first call)
    EkfInnovation *cons_recs = nullptr; // CONS_SLOTS x cap records: the matches of record s from s * cap on, update order
    // measurement budget (ekf_set_measurement_budget; allocated by its first call with K > 0): per slot of the full
    // predicted list
    double *bud_key = nullptr;             // det(S_i - I + pixelErrorX I), -1 when not positive
    int *bud_all = nullptr;                // the list before the selection (the compaction writes d.plist from it)
    int *bud_flag = nullptr;               // selected?
    EkfMeasurementRank *bud_recs = nullptr; // ekf_get_measurement_ranks
    // iterated update (ekf_update_iterated / ekf_set_update_iterations; one group, allocated by the first use).  A state
    // image is ITER_X doubles of the state block (x13, R) followed by the 6 N feature parameters
    double *iter_uv = nullptr;    // 2 per feature: pred_uv + H_i (x^ - x^i) of the matched features, the table a pass i >= 1 forms nu from
    double *iter_snap = nullptr;  // x^: the state image as it was before the update
    double *iter_lin = nullptr;   // two state images used in turn: the linearisation points x^(i-1) and x^i
    double *iter_diag = nullptr;  // diag(P) before the update, by state index (ncap doubles)
    double *iter_step = nullptr;  // ITER_SLOTS x EKF_MAX_UPDATE_ITERATIONS: the normalised step of every pass of an update of the last call
    int *iter_idx = nullptr;      // the matched features, update order: the sub-list of a pass's prediction
    MapBlobCtl *mb_ctl = nullptr; // map blob (ekf_save_map / ekf_load_map; allocated by the first of them)
    // relocalisation (ekf_relocalise; one group of per-call scratch, allocated by the first call).  Not per-feature
    // tables: nothing here outlives a call but the records the two getters read
    RelocCtl *reloc_ctl = nullptr;
    double *reloc_X = nullptr;     // 3 per feature: its world point
    int *reloc_flag = nullptr;     // per feature: 0 takes no part, 1 takes part, 2 candidate
    int *reloc_kp = nullptr;       // ... the candidate's keypoint
    int *reloc_dist = nullptr;     // ... and its Hamming distance
    EkfMatch *reloc_cand = nullptr; // the candidates, ascending feature order (cap records)
    double *reloc_cX = nullptr;    // 3 per candidate: world point
    double *reloc_cf = nullptr;    // 3 per candidate: bearing
    uint8_t *reloc_mask = nullptr; // per candidate: inlier of the best hypothesis
    EkfRelocHypothesis *reloc_hyp = nullptr; // RELOC_MAX_HYP records
    float *Pdiag = nullptr;     // sharded exact configuration: diagonal of P, n floats, completed by an exchange
    int8_t *Bstage = nullptr;   // ... and the digit planes of B in the exchange layout [column][plane][k / 16][16]
};

// current frame of the NCC matcher: gray pyramid (level 0 = full resolution) + the raw upload staging buffer
struct Image {
    uint8_t *px[3] = {nullptr, nullptr, nullptr};
    uint8_t *px2[3] = {nullptr, nullptr, nullptr}; // second pyramid: the NEXT staged frame is reduced into it on stream2
    int prefetched = -1;                           // staged frame whose pyramid sits (or is being built) in px2
    int w[3] = {0, 0, 0}, h[3] = {0, 0, 0};
    uint8_t *raw = nullptr;
    size_t raw_cap = 0;
    bool valid = false;
    // staged sequence (ekf_images_upload)
    uint8_t *seq = nullptr;
    int seq_n = 0, seq_w = 0, seq_h = 0, seq_stride = 0, seq_channels = 0;
};

// Persistent Cholesky sweeps (chol_persist.h) need ALL their workgroups resident at once; two of them in flight on one device, each
// only partly resident, would wait for each other's workgroups until the watchdog ends both.  Engines of one process that share a
// device therefore share one registry (held by shared_ptr: it lives exactly as long as its engines): with more than one member every
// persistent launch is ordered behind the last persistent launch of any OTHER member by an event.  (Other processes on the device
// cannot be ordered; the watchdog and the automatic retry on the launch-per-panel sweep cover them.)
struct SweepRegistry {
    std::mutex mu;
    int device = 0;
    int members = 0;                  // engines attached
    hipEvent_t last = nullptr;        // end of the most recent persistent sweep recorded here
    const void *owner = nullptr;      // the engine that recorded it
    ~SweepRegistry()
    {
        if (last) (void)hipEventDestroy(last);
    }
};
std::shared_ptr<SweepRegistry> sweep_registry_attach(int device); // kernels_update.hip
void sweep_registry_detach(const std::shared_ptr<SweepRegistry> &reg, const void *engine);

struct Frames {
    int n = 0;
    std::vector<int> offset, count;
    EkfKeypoint *kps = nullptr;
    uint8_t *desc = nullptr;
};

// one bracket of the covariance downdate's kernel (launch_p_update, launch_p_update_exact, the external update), not yet harvested
struct PuBracket {
    hipEvent_t first, second;
    double work; // n^2 m of the launch
    int m;
};
// one bracket of the Cholesky sweep's launches of one update
struct SweepBracket {
    hipEvent_t first, second;
    int m;        // rows of S; negative: the rows of B were not formed in these launches
    int launches; // (pair launches cover two panels)
};

} // namespace ekf

struct EkfEngine {
    EkfEngineConfig cfg;
    ekf::CamD cam;
    ekf::ParD par;
    int device = 0;
    int cap = 0, ncap = 0, mcap = 0, kcap = 0;
    int ldP = 0, ldS = 0, ldW = 0;
    int N = 0, n = 0;
    bool f32 = false;   // P stored in fp32 (and, unless `exact`, H P, its gathered rows and B)
    bool exact = false; // EKF_PRECISION_F32_EXACT: P in fp32; H P, G and B in fp64; downdate with exact accumulation (kernels_pexact.hip)
    int desc_bytes = EKF_DESC_BYTES; // bytes per descriptor row
    bool desc_f32 = false;           // CV_32F descriptors / L2 distance (Matching.cpp:60-73) instead of CV_8U / Hamming
    // row sharding: world == 1 means the whole matrix lives here
    int shard_rank = 0, shard_world = 1;
    int p_rows_cap = 0;                  // rows allocated for P
    ekf::RowMap rm{13, 13, 13};          // refreshed by set_state / map management
    std::vector<int> shard_feat_begin;   // [world + 1] first feature of each rank
    EkfExchangeFn xchg = nullptr;        // all-gather of per-feature row blocks between the ranks
    void *comm = nullptr;                // ncclComm_t of the in-engine transport (ekf_comm_init), or null
    bool hp_complete = true;             // sharded: the H.P table holds EVERY rank's rows since the last prediction
    // the row-block exchange of engine.cpp (RCCL send / recv or the host callback), callable from the update's launcher
    int (*exchange_hook)(EkfEngine *, int what, void *base, size_t row_bytes, const std::vector<int32_t> &rb, const char *name) = nullptr;
    std::vector<int32_t> shard_row_begin; // [world + 1] first state row of each rank's share (0 for rank 0: it also holds the camera's), n at the end
    long long xchg_bytes_planes = 0;      // bytes of digit planes this rank received (tests assert them against the model)
    std::vector<int32_t> shard_rb;       // row boundaries of the gathered rows by owner (from CNT_SHARD0..)
    std::vector<int32_t> slot_rb;        // sharded step: prediction slots of the last full prediction by owner (from CNT_SHARD0..)
    std::vector<int32_t> last_col_rb;    // column shares of the planes of B used by the last sharded update (ekf_shard_counters)
    void *xchg_user = nullptr;
    int n_cus = 256;           // compute units of the device (launch-shape decisions)
    int b_path = 0;            // ekf_set_update_path: 0 by size (B_SWEEP_MAX), 1 B in the sweep, 2 inverse + GEMM
    int sweep_mode = 2;        // ekf_set_sweep_mode: EKF_SWEEP_* (2 AUTO: one persistent launch per update where it applies, chol_persist.h)
    unsigned ps_epoch = 0;                // persistent sweep: epoch of its flags
    int ps_fault = 0;                     // include/ekf_test_hooks.h: countdown; the persistent sweep that takes it to zero runs without its chain workgroup
    std::shared_ptr<ekf::SweepRegistry> ps_reg; // the device's registry of persistent sweeps (shared with the other engines on it)
    // automatic retry of an update whose persistent sweep timed out (EKF_ERR_TIMEOUT): the kernels behind a failed sweep leave the
    // filter untouched (filter_frozen), so the update is run again from the same P on the launch-per-panel sweep
    int sweep_retries = 0;                // updates re-run this way since the engine was created (ekf_get_sweep_retries)
    // back-off (EKF_SWEEP_AUTO only): a device that another process shares makes persistent sweeps time out again and again, 5 ms each;
    // after a time-out the next ps_backoff updates take the launch-per-panel sweep, twice as many after every further time-out (64 ..
    // 4096), and 256 persistent sweeps in a row without one forget the history
    int ps_backoff = 0, ps_backoff_len = 0, ps_ok_streak = 0;
    // the last update enqueued: a retry issues ekf::retry_of(call), its list is still in d.msel
    struct {
        ekf::UpdateCall call;
        bool sym = false;     // p_exact_sym as it was before that update
        bool persist = false; // that update's sweep was the persistent launch
    } last_update;
    // d.match_gates holds the gates of the predictions now in pred_S / pred_uv: set by the launch_hp_rows that wrote them, cleared by
    // everything else that rewrites those tables or the map under them
    bool match_gates_valid = false;
    int ps_cap[2] = {0, 0};    // resident workgroups of k_chol_persist<false / true> on this device (0: not asked yet, -1: unusable)
    bool async_errors = false; // ekf_set_async_errors: no read-back at the end of a step
    bool err_unread = false;   // the last step returned without reading the error flag back (cleared by recover_failed_update)
    bool p_exact_sym = false; // P known to be bitwise symmetric (engine-maintained invariant)
    int n_pred = 0;           // predictions of the last full prediction
    int n_gates = 0;          // gates snapshotted for the new-feature detector
    bool keep_step_preds = false; // snapshot every full prediction for ekf_get_step_predictions
    int n_step_preds = 0;
    int cells_cap = 0;        // detector cell buffers allocated for this many cells
    int image_matcher = EKF_IMAGE_MATCHER_NCC; // ekf_set_image_matcher: how image steps match
    bool warp_on = false;          // ekf_set_template_warp: NCC templates re-rendered from the predicted pose before every search
    bool last_match_warped = false; // the last NCC match compared d.wtmpl (else d.tmpl)
    int warp_counts[2] = {0, 0};   // levels warped / fallen back in the last NCC match
    bool subpix_on = false;        // ekf_set_subpixel_matches: NCC matches carry the parabola-fitted position
    int subpix_counts[2] = {0, 0}; // axes fitted / left at the integer over the valid matches of the last NCC match
    bool wide_on = false;          // ekf_set_ncc_wide_search: gates beyond the 43 x 43 coarse window are searched whole
    int wide_counts[2] = {0, 0};   // wide slots / coarse candidates evaluated for them in the last NCC match
    bool pn_on = false;            // ekf_set_patch_normals: patch normals estimated per frame and used by the warp
    int pn_counts[2] = {0, 0};     // features updated / skipped by the last estimator launch
    int wide_tiles = 0;            // tiles per slot d.wide_part was allocated for (the coarse level's tile count)
    int wide_parts = 0;            // partial tables d.wide_part holds, one behind the other: 1, or 2 for the rival pass
    double distinct_coef = 0.0;    // ekf_set_ncc_distinct: 0 = off, else an NCC match with a rival peak is kept when d1 < d2 * coef
    int distinct_counts[2] = {0, 0}; // accepted matches with a rival / rejected by the test in the last NCC match
    int rival_slots = 0;           // prediction slots of the last NCC match that ran with the test on (records of d.mt_rival)
    bool fixed_map = false;        // ekf_set_fixed_map: the covariance updates of the step functions are fixed-map updates
    int fm_rows = 0;               // rows of each of the two tables in d.fm_gain
    bool consistency = false;      // ekf_set_consistency: every covariance update is followed by k_consistency
    int cons_epoch = 0;            // bumped when a step or an ekf_update begins with the mode on (ConsCtl::epoch)
    int update_iterations = 1;     // ekf_set_update_iterations: passes of both updates of the step functions; 1: the plain update
    double update_iter_tol = 0.0;  // ... and the normalised step below which the next pass is the last (0: by count alone)
    std::vector<EkfIterationRecord> iter_records; // the iterated updates of the last call (their steps are in d.iter_step until asked for)
    int iter_lin_sel = -1;         // which image of d.iter_lin the last iterated update linearised its covariance pass at (-1: none yet)
    int iter_lin_N = 0;            // ... and the features it holds
    double frame_interval = 1.0;   // ekf_set_frame_interval: the dt of ekf_predict and of every step function
    double step_dt = 1.0;          // the interval of the step being run: frame_interval, or the staged table's entry of its frame
    std::vector<double> staged_dt; // ekf_set_staged_intervals: per index of a pre-staged sequence, kept on the host (the value is a kernel argument)
    int budget_K = 0;              // ekf_set_measurement_budget: 0 = off, else a step measures at most this many features
    int bud_recs_n = 0;            // records in d.bud_recs: predicted features of the last step if the budget was active in it, else 0
    int bud_predicted = 0, bud_selected = 0; // the last step's full prediction: features predicted / handed on (equal when the budget did not bind)
    double kp_min_response = 0.0;              // ... and the keypoint detector's threshold there
    int step_kp_detected = 0, step_kp_kept = 0; // keypoints of the last KEYPOINTS-mode image step
    size_t rowmask_cap = 0;   // words of d.kp_rowmask
    int det_cap = 0;          // entries of d.det_kps / det_desc / det_centres
    int n_kp = 0;
    long long pu_tilemap_nt = -1;
    std::map<long long, std::pair<void *, int>> pu_tables; // built work lists of the downdate: key -> (device list, units per XCD)
    int pu_per_xcd = 0;
    int bq_rows = 0;          // rows of B a digit plane holds (multiple of 64)
    int bz_stride = 0;        // 16-row groups per column block of d.Bz (= bq_rows / 16)
    bool px_dense = false;    // include/ekf_test_hooks.h: the downdate and the int8 GEMM multiply every digit product (the tables are not consulted)
    int px_scale_shift = 0;   // bits of head-room added to the a-priori column scales of B (exponent of sqrt(P_jj)); EKF_PX_SCALE_SHIFT in the
                              // environment sets it (a measurement knob).  With 1 / 2 bits digit plane 0 is 82 / 95-97 % zero pieces on converged
                              // maps too and the downdate skips their products: 1187 -> 1266 updates/s at N = 1000 -- but the 38-bit integers are
                              // then 37- / 36-bit ones, and the far features' inverse depths need every bit: one bit puts one of the five
                              // N = 1000 scenes at 1.12e-5 component-wise, two bits N = 2000 at 1.9e-5 (profiles/r06_scale_shift.txt).  Left at 0.
    int lq_nbk = 0;           // 32-row blocks per side of the digit planes of L
    int bstage_rows = 0;      // rows of B the exchange image of the planes holds (sharded exact configuration)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> px_events; // exact configuration: end of the sweep -> start of the downdate (inverse, GEMM, digit planes, dx, state)
    hipEvent_t px_mid = nullptr;                               // recorded after the sweep's last launch (timing only)
    int pu_slots = 0;         // resident workgroups of the downdate kernel on this device (0: not asked yet, -1: unknown): launch_p_update's query
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;             // image-only work of the next frame, overlapped with the update
    hipEvent_t ev_main = nullptr, ev_prefetch = nullptr;
    // owner of every device allocation below (d, frames, img, pu_tables): allocate and free through it alone (device_buffers.h)
    ekf::DeviceBuffers bufs{ekf::DeviceAllocApi{hipMalloc, hipMemset, hipFree}};
    ekf::DeviceArrays d;
    ekf::Frames frames;
    ekf::Image img;
    std::string err;
    // timing
    bool timing = false;
    EkfStageTimes times{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<ekf::PuBracket> pu_events;                     // P-update kernel brackets not yet harvested
    std::vector<std::pair<int, float>> pu_log;                 // harvested (m, ms) per launch
    std::vector<ekf::SweepBracket> sw_events;                  // brackets of the Cholesky sweeps not yet harvested
    double sweep_ms = 0.0, sweep_flops_f64 = 0.0, sweep_flops_b = 0.0; // harvested totals (ekf_timing_sweep)
    long long sweep_panels = 0, sweep_updates = 0, sweep_launches = 0;
    double slice_ms = 0.0;                                     // exact configuration: sweep end -> downdate start (harvested)
    // host scratch
    std::vector<int> h_counts;
    int *h_mirror = nullptr, *d_mirror = nullptr; // GPU-writable host page: counters + sequence number (read_counts)
    int mirror_seq = 0;
    std::vector<int> h_type, h_covpos; // host mirror of the map layout (type, covariance position per feature)
};

namespace ekf {

// C[i][j] = alpha sum_k X[k][i] Y[k][j] (kernels_gemm.hip); batch element b adds b * (xb, yb, cb, ctb) elements
struct XtyArgs {
    const void *X; int ldx; long long xb;
    const void *Y; int ldy; long long yb;
    void *C; int ldc; long long cb;       // may be null
    void *Ct; int ldct; long long ctb;    // transposed copy in fp64, may be null
    float *Ctf;                           // transposed copy in fp32 (same layout as Ct), may be null
    int M, N, K;                          // output rows / columns / k-depth per batch element
    int row0_first, row0_stride, m_lim;   // rows of element b that exist: min(M, m_lim - (row0_first + b row0_stride))
    int tri;                              // 0: all k; 1: Y[k][j] = 0 for k < j; 2: X[k][i] = 0 for k > i
    int tiles_i, tiles_j;                 // row tiles / column tiles
    int tj0;                              // first column tile (row-sharded engines form their own columns of B only)
    int n_split;                          // bottom row tiles cut into two half units (tri == 2, batch 1 only)
    double alpha;
};
void launch_xty(EkfEngine *e, const XtyArgs &a, int batch, bool f32, hipStream_t stream);

// A failed factorisation of S (EKF_ERR_NOT_POSITIVE_DEFINITE) or a timed-out persistent sweep (EKF_ERR_TIMEOUT) leaves its code in
// counts[CNT_ERR] until the host has read it.  While it is set the filter is FROZEN: the kernels that write the state, the covariance
// or the map's bookkeeping return at once (the downdate and the state update of the failed update itself, and whatever of the
// following stages was enqueued before the host looked), so the host finds x, P and the map exactly as they were before the failed
// update and can run it again (time-out) or go on without it (S not positive definite: the reference's cv::invert returns zeros
// there, i.e. K = 0 and an unchanged filter, EKF/Update.cpp:101-108).  counts == nullptr: no guard (stage calls that synchronise).
#ifdef __HIPCC__
__device__ __forceinline__ bool filter_frozen(const int *counts) { return counts != nullptr && counts[CNT_ERR] != 0; }

// the RANSAC record of a match of feature f at pixel (u, v): see RansacRec
__device__ __forceinline__ RansacRec load_ransac_rec(int f, int N, const double *feat_pos, const int *feat_type, const int *feat_covpos,
                                                     double u, double v)
{
    RansacRec r;
    const bool in_map = f >= 0 && f < N;
#pragma unroll
    for (int a = 0; a < 6; ++a) r.fp[a] = in_map ? feat_pos[6 * f + a] : 0.0;
    r.img[0] = u;
    r.img[1] = v;
    r.f = in_map ? f : -1;
    r.type = in_map ? feat_type[f] : 0;
    r.pos = in_map ? feat_covpos[f] : 0;
    r.pad = 0;
    return r;
}

// quaternion normalisation and its Jacobian (Update.cpp:45-62, 303-312), one thread: J from the un-normalised q, then q /= |q|
// and R(q)
// (q: the un-normalised quaternion in, the normalised one out; J: the 4 x 4 Jacobian of the normalisation; R: the rotation of the result)
__device__ inline void quat_norm_parts(double *q, double *J, double *R)
{
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    const double nrm = sqrt(r * r + x * x + y * y + z * z);
    const double a = 1.0 / (nrm * nrm * nrm);
    const double M[16] = {x * x + y * y + z * z, -r * x, -r * y, -r * z,
                          -x * r, r * r + y * y + z * z, -x * y, -x * z,
                          -y * r, -y * x, r * r + x * x + z * z, -y * z,
                          -z * r, -z * x, -z * y, r * r + x * x + y * y};
    for (int i = 0; i < 16; ++i) J[i] = M[i] * a;
    q[0] = r / nrm; q[1] = x / nrm; q[2] = y / nrm; q[3] = z / nrm;
    quat_to_rot(q, R);
}
__device__ inline void quat_norm_dev(double *st) { quat_norm_parts(st + ST_X + 3, st + ST_JN, st + ST_R); }
#endif

// Exclusive prefix sum of one int per thread over a 1024-thread workgroup (and the total): inside a wavefront by shuffles,
// across the 16 wavefronts through LDS -- one barrier, where a Hillis-Steele scan in LDS needs twenty.  Device code only.
#ifdef __HIPCC__
__device__ __forceinline__ int block_exclusive_scan_1024(int c, int *wtot /* __shared__ int[16] */, int *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wv] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int t = wtot[w];
        base += w < wv ? t : 0;
        tot += t;
    }
    *total = tot;
    return base + x - c;
}
#endif

// ---- launchers (kernels_*.hip) ; T selected by e->f32 ----------------------------------------------------
void launch_predict(EkfEngine *e, double dt); // one prediction over the interval dt (> 0, finite: the ABI checks)
void launch_camera_ahead(const EkfEngine *e, double tau, double *d_out); // read-only: x13 and the camera corner at horizon tau -> 13 + 169 doubles
// full (idx == nullptr) or subset prediction; fills tables, compacted list and CNT_NPRED / CNT_NPRED_SUB
bool launch_predict_features(EkfEngine *e, const int *d_idx, int count, bool state_only, bool defer_compact = false);
bool launch_predict_with_features(EkfEngine *e, int count, double dt); // step path: prepare, then covariance strips + all features in one launch
// the H P rows and S_i of the features in d_list (kernels_predict.hip has the details of from_flags and gates)
struct HpRowsCall {
    const int *d_list = nullptr;
    int n_list = 0;
    bool count_predicted = false; // timesPredicted++ of the listed features (EKF.cpp:572)
    const int *d_count = nullptr; // not null: n_list is an upper bound, the list's length is read on the device
    bool from_flags = false;      // the compaction of the predicted list was left to this launch (launch_predict_*'s return value)
    bool gates = false;           // also write the descriptor matcher's gates (a full prediction)
};
void launch_hp_rows(EkfEngine *e, const HpRowsCall &c);
// descriptor matching of the predictions in d.plist against the keypoints kps / kdesc
struct MatchCall {
    const EkfKeypoint *kps = nullptr;
    const uint8_t *kdesc = nullptr;
    int n_pred = 0, n_kp = 0;
    const int *d_npred = nullptr;  // not null: n_pred is an upper bound, the number of predictions is read on the device
    const int *d_nkp = nullptr;    // likewise for n_kp (keypoints detected on the device)
    bool with_ransac_init = false; // the compaction also sets the RANSAC loop state, the feature -> match index and the records
};
void launch_match(EkfEngine *e, const MatchCall &c);
// The two stable partitions of a step (k_partition, kernels_match.hip).  After RANSAC: d.matches by d.best_flags into the inliers
// (d.msel; timesMatched++ and the map descriptor replaced by the keypoint's, MapManagement.cpp:88-113) and the outliers (d.mout,
// their features into d.work_idx: the work list of the re-prediction).
struct RansacPartition {
    int M = 0;                     // matches
    const int *d_M = nullptr;      // not null: M is an upper bound for the launch, the kernel reads the count
    bool behind_ransac = false;    // enqueued behind the first batch of hypotheses, before the host has seen its outcome: does
                                   // nothing unless that batch ended the loop (k_partition)
    const uint8_t *d_kdesc = nullptr; // the frame's keypoint descriptors (null: NCC matches have none)
};
void launch_ransac_partition(EkfEngine *e, const RansacPartition &c);
// After the outliers' re-prediction: d.mout by the rescue mask d.mask into d.msel, the count into counts[CNT_NRESC], the same
// bookkeeping for the rescued.
struct RescuePartition {
    int n_outliers = 0;
    const uint8_t *d_kdesc = nullptr;
    bool fused_rescue = false; // the launch computes the mask itself (rescueOutliers, EKF.cpp:84-97) instead of reading launch_rescue's
    int publish_seq = 0;       // > 0: the launch also publishes the counter block under this sequence number (publish_counts_block)
};
void launch_rescue_partition(EkfEngine *e, const RescuePartition &c);
void launch_outlier_idx(EkfEngine *e, const EkfMatch *src, int M, int *idx);
// d_M != nullptr (RANSAC launchers): M is an upper bound, the number of matches is read on the device
void launch_match_index(EkfEngine *e, int M, const int *d_M = nullptr);
// sharded filter: per-rank boundaries of a feature-sorted match list -> counts[CNT_SHARD0 ..]
void launch_shard_bounds(EkfEngine *e, const EkfMatch *list, int count);
void launch_shard_bounds_idx(EkfEngine *e, const int *list, const int *d_count); // ... of a feature-index list whose length is on the device
// sharded filter: matching and RANSAC hypotheses divided by feature ownership (kernels_match.hip, kernels_ncc.hip, kernels_ransac.hip)
void launch_match_slots(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *kdesc, int n_kp, int s_lo, int s_hi);
void launch_match_ncc_slots(EkfEngine *e, int s_lo, int s_hi, bool subpix);
void launch_match_compact(EkfEngine *e, const EkfKeypoint *kps, int n_pred);
void launch_match_compact_slots(EkfEngine *e, int n_pred, const EkfKeypoint *d_slot_xy);
void launch_ransac_hyp(EkfEngine *e, int M, int h0, int batch, const int *d_M, int h_lo, int h_hi);
void launch_ransac_select(EkfEngine *e, int M, int h0, int batch, const int *d_M, int publish_seq);
// publish_seq > 0: the batch's bookkeeping kernel also publishes the counter block (see publish_counts_block)
void launch_ransac_batch(EkfEngine *e, int M, int h0, int batch, const int *d_M = nullptr, int publish_seq = 0);
void launch_ransac_init(EkfEngine *e, int M);
// enqueues the update (update_route.h: UpdateCall, UPDATE_*); EKF_OK, or the code of the stage that ended it with e->err set
int launch_update(EkfEngine *e, const UpdateCall &call);
// the merged gather / assembly launch of an update of the matches in d.msel whose count (at most M_max) is still on the device at
// d_M; launched == false: the route does not allow it, nothing was enqueued (kernels_update.hip)
EarlyGather launch_early_gather(EkfEngine *e, int M_max, const int *d_M, int kind);
// fixed-map update (kernels_fixedmap.hip), fp64 arithmetic, unsharded engines.  _gain: where the route forms no rows of B, behind the inverse of
// L -- B_c = W' G[:, 0:13] and K_c' = W B_c into d.fm_gain.  _strip: the partial sums of the 13 x n strip Y' X (Y = B[:, 0:13] and
// X = B, m rows in d.A; or from_gain: Y = K_c' and X = G) into d.cam_part, then the tail: strip downdate, camera state, normalisation
void launch_fixed_map_gain(EkfEngine *e, int m, const double *G);
void launch_fixed_map_strip(EkfEngine *e, int m, const double *X, bool from_gain);
int launch_p_update_exact(EkfEngine *e, int m, bool use_bc, bool exps_ready = false, bool planes_ready = false); // kernels_pexact.hip; EKF_OK or the error
void launch_round_P_f32(EkfEngine *e);                        // kernels_map.hip
void launch_diag_extract(EkfEngine *e, float *diag);          // kernels_pexact.hip: sharded exact configuration
void launch_planes_move(EkfEngine *e, bool pack, int m_k, int c_lo, int c_hi, int skip_lo, int skip_hi);
void launch_dx_planes(EkfEngine *e, int m_k);
void launch_slice_columns(EkfEngine *e, int m, int c_lo, int c_hi);
int launch_b_gemm_planes(EkfEngine *e, int m, int c_lo, int c_hi); // EKF_OK or the error
void launch_rescue(EkfEngine *e, const EkfMatch *matches, int M);
void launch_state_only_predict(EkfEngine *e, EkfPrediction *d_out); // predictMeasurementState on current state
void launch_add_features(EkfEngine *e, const double *d_uv, int count, double *d_Jpo, double *d_Jhr);
void launch_compact_P(EkfEngine *e, int n_new, const int *d_new2old);
void launch_linearity(EkfEngine *e, double *d_out);
void launch_convert(EkfEngine *e, int fi, int pos, double *d_J, double *d_T3);
// k_convert_all_P: tiles of CA_TILE x CA_TILE entries of the new matrix; the old columns one tile's columns read fit CA_CW (22 converted
// features at most: 1 + 20 x 3 + 3 new columns), which the host checks on the row table it builds
constexpr int CA_TILE = 64, CA_CW = 132;
// batch conversion: X, J and the type of the `count` features in d.ca_sel, then P' = R P R' from d.P into d.P2 by the row table in
// d.ca_rows (n_new rows), and the swap of the two buffers
void launch_convert_all(EkfEngine *e, int count, int n_new);
void launch_map_points(EkfEngine *e, EkfMapPoint *d_out); // read-only: state, map tables and P -> N records
// relocalisation (kernels_reloc.hip): the four kernels of DESIGN.md 4.17 over the keypoints kps / kdesc, into the d.reloc_* scratch;
// the last one writes the state and the camera strip of P when the pose is found and params->install is set
struct RelocCall {
    const EkfRelocParams *params = nullptr; // validated by the caller
    const EkfKeypoint *kps = nullptr;
    const uint8_t *kdesc = nullptr;
    int n_kp = 0;
    const int *d_nkp = nullptr; // not null: n_kp is the capacity, the number of keypoints is read on the device
};
void launch_relocalise(EkfEngine *e, const RelocCall &c);
// map blob (kernels_mapblob.hip; layout: mapblob::P_TRIANGLE / P_FULL of map_blob.h).  _pack: the engine's P -> the flat section in
// `staging`, its checksum -> *d_ctl (zeroed first).  _check: read-only pass over an uploaded section of n rows and elem_bytes per
// element -> *d_ctl (zeroed first).  _unpack: such a section -> the engine's P (rows and columns below n; both triangles)
// _asym: read-only pass over the engine's P, counts the pairs (i, j > i) that are not bitwise equal -> d_ctl->asym (zeroed first)
void launch_map_asym(EkfEngine *e, MapBlobCtl *d_ctl);
void launch_map_pack(EkfEngine *e, int layout, void *staging, MapBlobCtl *d_ctl);
void launch_map_check(EkfEngine *e, const void *staging, int n, int elem_bytes, int layout, MapBlobCtl *d_ctl);
void launch_map_unpack(EkfEngine *e, const void *staging, int n, int elem_bytes, int layout);
// external measurement update (kernels_external.hip): the call's ExtCtl is in d.ext_ctl; enqueues A = H P, the solve, the state
// update, the downdate and the normalisation of the covariance, and leaves the record in d.ext_res
void launch_external_update(EkfEngine *e, int m);
// filter consistency (kernels_consistency.hip): NIS and the per-match innovations of the update whose sweep was just enqueued, from
// d.zvec, the M matches and the prediction tables -> d.cons_ctl / d.cons_recs, recorded under `stage`; does nothing when the error flag is set
// uv_tab: the prediction table the update formed nu from (UpdateCall::pred_uv, or d.pred_uv)
void launch_consistency(EkfEngine *e, const EkfMatch *matches, int M, int stage, const double *uv_tab);
// iterated update (kernels_iterate.hip); a state image: engine.h DeviceArrays::iter_snap
// _snapshot: the state -> d.iter_snap and image 0 of d.iter_lin, diag(P) -> d.iter_diag, the matches' features -> d.iter_idx, steps[0..8) = 0
// _step: max_j |x_j - prev_j| / sqrt(P_jj) over the state columns with P_jj > 0 -> *step_out, x being the live state and prev image
//   `prev` of d.iter_lin; cur >= 0: the live state -> image cur, and counts[CNT_ITER_SMALL] = (tol > 0 and the step is below it)
// _shift_restore: d.iter_uv of the M matches from the prediction tables, x^ and image `lin`; then the live state <- x^ (all features)
// _load: the live state <- image `lin`.  The two that write the state leave it alone while the filter is frozen, unless even_frozen
// (the host rebuilds the tables of a failed pass in front of its retry and puts x^ back itself).
void launch_iter_snapshot(EkfEngine *e, const EkfMatch *matches, int M, double *steps);
void launch_iter_step(EkfEngine *e, int prev, int cur, double *step_out, double tol);
void launch_iter_shift_restore(EkfEngine *e, const EkfMatch *matches, int M, int lin, bool even_frozen = false);
void launch_iter_load(EkfEngine *e, int lin, bool even_frozen = false);
// measurement budget (kernels_budget.hip): S_i of the np features in d.plist -> d.pred_S, their keys, ranks, records and selected flags
// (rank < K, or all when np <= K) -> d.bud_*; launch_compact (k_compact) then turns flags into a list
void launch_budget_select(EkfEngine *e, int np, int K);
void launch_compact(EkfEngine *e, const int *flag, const int *idx, int count, int *list, int *out_count);
void launch_ncc_pyramid(EkfEngine *e, const uint8_t *d_raw, int stride, int channels);
void launch_ncc_pyramid_on(EkfEngine *e, hipStream_t stream, uint8_t *const px[3], const uint8_t *d_raw, int stride, int channels);
void launch_ncc_capture(EkfEngine *e, const int *d_idx, const double *d_uv, int count);
// template warp: source patches + capture pose of the listed features (keep = false: marks them "no source patch")
void launch_ncc_warp_capture(EkfEngine *e, const int *d_idx, const double *d_uv, int count, bool keep);
// patch normals: one estimator step for the features of the M matches in d.pn_list against the current image and state; zeroes and
// then counts CNT_PN_UPD / CNT_PN_SKIP
void launch_ncc_normal(EkfEngine *e, int M);
// subpix: k_ncc_match<true>, positions refined by the fit of DESIGN.md 4.7; wide: the slots whose gate exceeds the coarse window go
// through the three kernels of DESIGN.md 4.8 instead (d.wide_list / d.wide_part sized for the current frame: engine.cpp)
// coef > 0: the distinctiveness test of DESIGN.md 4.10 (d.mt_rival, CNT_RIVAL_WITH / CNT_RIVAL_REJ; with wide, d.wide_part holds two tables)
void launch_match_ncc(EkfEngine *e, int n_pred, bool subpix, bool wide, double coef);
// (the per-feature row sizes are stated once, in map_blob.h)
constexpr int NCC_TT = mapblob::TEMPLATE_LEVEL_BYTES; // bytes of one 11 x 11 template; d.tmpl / d.wtmpl hold 3 levels per feature
constexpr int WARP_S = mapblob::WARP_SOURCE_SIDE, WARP_SS = WARP_S * WARP_S; // template warp: side and bytes of one source patch; d.wsrc holds 3 per feature
constexpr int WPOSE_DOUBLES = mapblob::WARP_POSE_DOUBLES; // ... and its capture pose record in d.wpose: r0 (3), q0 (4), capture pixel (2)
static_assert(sizeof(PatchNormalRec) == mapblob::PATCH_NORMAL_BYTES, "a row of d.wnorm is a row of the PATCH_NORMALS section");
constexpr int NCC_WIDE_TILE = 32;          // coarse candidates per tile side
constexpr int NCC_WIDE_SLOT_BYTES = 80;    // sizeof(WideSlot), kernels_ncc.hip
constexpr int NCC_WIDE_PARTIAL_BYTES = 16; // sizeof(WidePartial)
constexpr int NCC_WIDE_TOTALS_BYTES = 16;  // sizeof(WideTotals): one record behind the list
inline int ncc_wide_tiles(int w2, int h2) { return ((w2 + NCC_WIDE_TILE - 1) / NCC_WIDE_TILE) * ((h2 + NCC_WIDE_TILE - 1) / NCC_WIDE_TILE); }
void launch_gate_snapshot(EkfEngine *e, int n_pred);
void launch_detect_cells(EkfEngine *e, int n_gates, int cells_x, int cells_y, long long *d_resp, int *d_xy);
// keypoints of the current image (kernels_detect.hip): the first `cap` in raster order -> out, all of them -> *d_found;
// masked: inside the gates of the last full prediction.  rowmask: kp_rowmask_words(w, h) words of scratch
void launch_kp_detect(EkfEngine *e, long long thr, bool masked, unsigned long long *rowmask, EkfKeypoint *out, int cap, int *d_found);
size_t kp_rowmask_words(int w, int h);
// BRIEF-32 of the keypoints' pixels (centres == nullptr) or of integer centres; d_n != nullptr: n is a bound, count on the device
void launch_brief(EkfEngine *e, const EkfKeypoint *kps, const int *centres, int n, const int *d_n, uint8_t *desc);
void launch_publish_counts(EkfEngine *e, int *d_mirror, int seq);
// The same publication from inside a kernel that ends a stage (saves the separate launch): called by EVERY thread of a
// block after the block's last write to `counts`; the lanes below CNT_COUNT copy the counters to the GPU-writable host page, lane 0
// then releases the sequence number the host polls.
__device__ __forceinline__ void publish_counts_block(const int *counts, int *mirror, int seq)
{
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 64) { // first wavefront
        if (t < CNT_COUNT) __hip_atomic_store(&mirror[t], counts[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __builtin_amdgcn_wave_barrier();
        if (t == 0) {
            __threadfence_system();
            __hip_atomic_store(&mirror[CNT_COUNT], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
void launch_pack_predictions(EkfEngine *e, const int *d_list, int n, EkfPrediction *d_out);

} // namespace ekf
