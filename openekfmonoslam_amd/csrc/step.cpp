// step.cpp -- EKF::step on the device: the counter read-back, the cores of the stages with their C ABI functions, and the two
// schedules of a step (step_device_counts, step_host_counts).  Host orchestration only, like engine.cpp.
#include "engine_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

using namespace ekf;

// ------------------------------------------------------------------------------------------- counter read-back
// The device counter block is mirrored into a page of host memory the GPU can write (hipHostMallocMapped, coherent):
// a one-wavefront kernel copies the 16 ints and then a sequence number, the host polls the sequence number.  The
// per-frame control flow needs ~6 of these round trips (how many predictions / matches / inliers / rescued decide the
// next launches); a memcpy + stream synchronise costs ~20 us each, the poll a few.
constexpr int POLL_SECONDS = 20; // bound of a host poll in wall time (not in iterations: their rate depends on the host); then the plain path

// polls the mirror page for sequence number seq; true: it arrived and the block is in h_counts.  false: the stream drained
// without the write, or the time bound passed -- the caller takes the plain path
static bool poll_mirror(EkfEngine *e, int seq)
{
    volatile int *m = e->h_mirror;
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(POLL_SECONDS);
    for (long spin = 0;; ++spin) {
        if (m[CNT_COUNT] == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            for (int i = 0; i < CNT_COUNT; ++i) e->h_counts[i] = m[i];
            return true;
        }
        if ((spin & 0xfffff) == 0xfffff && // every ~1e6 polls
            ((hipStreamQuery(e->stream) == hipSuccess && m[CNT_COUNT] != seq) || std::chrono::steady_clock::now() > t_end)) return false;
#if defined(__x86_64__)
        __builtin_ia32_pause(); // the caller's thread polls one cache line; leave the core's other thread its issue slots
#endif
    }
}

int ekf::read_counts(EkfEngine *e)
{
    if (e->h_mirror) { // (optional: without the page, memcpy + synchronise)
        const int seq = ++e->mirror_seq;
        launch_publish_counts(e, e->d_mirror, seq);
        if (poll_mirror(e, seq)) return EKF_OK;
    }
    HIPCHK(hipMemcpyAsync(e->h_counts.data(), e->d.counts, CNT_COUNT * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return EKF_OK;
}

// read_counts for a stage whose last kernel published the counter block itself (publish_counts_block, sequence number
// taken with next_publish_seq before that launch): poll only
static int next_publish_seq(EkfEngine *e) { return e->h_mirror ? ++e->mirror_seq : 0; }

static int wait_counts(EkfEngine *e, int seq)
{
    if (seq > 0 && poll_mirror(e, seq)) return EKF_OK;
    return read_counts(e); // no page, or the poll gave up: the plain path
}

// ---------------------------------------------------------------------------------------------------- stages
// Sharded filter: the FULL exchange of the H.P table (2N x ldP: 192 MB at N = 2000, 1.2 GB at N = 5000 in fp32) and of its
// fp64 camera columns -- what rounds 1-2 did after every prediction.  EKF::step no longer needs it (see `lean` below); the
// stateless stage calls of the ABI (ekf_ransac / ekf_update / ... on a caller-ordered match list) still do.
static int complete_hp_table(EkfEngine *e)
{
    if (e->shard_world <= 1 || e->hp_complete) return EKF_OK;
    int rc;
    std::vector<int32_t> rb(e->shard_world + 1);
    for (int r = 0; r <= e->shard_world; ++r) rb[r] = 2 * e->shard_feat_begin[r];
    if ((rc = exchange_rows(e, EKF_XCHG_HP, e->d.HP, (size_t)e->ldP * hp_elem_bytes(e), rb, "the H.P row blocks"))) return rc;
    if (e->f32 && !e->exact && (rc = exchange_rows(e, EKF_XCHG_HPC, e->d.HPc, 16 * sizeof(double), rb, "the fp64 camera columns of H.P"))) return rc;
    e->hp_complete = true;
    return EKF_OK;
}

struct PredictCall {
    const int *d_idx = nullptr;   // the features to predict (count of them); null: the whole map
    int count = 0;
    bool count_predicted = false; // timesPredicted++ (a step's full prediction)
    bool lean = false;
    int budget = 0;
};

// device-side core of predictCameraMeasurements; leaves the count in h_counts.
// lean (sharded EKF::step): only the 2x2 innovation blocks S_i travel after a prediction (32 bytes per feature; every rank
// gates and matches all predictions).  The H.P rows stay with their owners until somebody consumes them: the rows of a
// RANSAC batch's hypotheses (ransac_dev) and the rows of the matches an update selects (the gather stage of a lean update) -- 2M of
// the 2N rows, and for the outlier re-prediction nothing but the S_i (missing 2a / EKF.cpp:473).
// budget > 0 (a step's full prediction with the measurement budget active): the predicted features are scored and
// ranked before the H P pass and the `budget` most informative go on; what describes the whole prediction -- the kept step
// predictions and the gate snapshot -- is taken from all of them first, with the S_i the selector formed.
static int predict_measurements_dev(EkfEngine *e, const PredictCall &c, int *n_out)
{
    const int *d_idx = c.d_idx;
    const bool lean = c.lean;
    const int budget = c.budget;
    launch_predict_features(e, d_idx, d_idx ? c.count : e->N, /*state_only*/ false);
    const bool slots = lean && !d_idx && e->shard_world > 1; // sharded step: where each rank's run of the predicted list starts (matching by owner)
    if (slots) launch_shard_bounds_idx(e, e->d.plist, e->d.counts + CNT_NPRED);
    int rc = read_counts(e);
    if (rc) return rc;
    int np = e->h_counts[d_idx ? CNT_NPRED_SUB : CNT_NPRED];
    const bool budgeted = budget > 0 && !d_idx;
    if (budgeted) {
        const int np_all = np;
        launch_budget_select(e, np_all, budget);
        if (e->keep_step_preds) {
            launch_pack_predictions(e, e->d.plist, np_all, e->d.step_preds);
            e->n_step_preds = np_all;
        }
        if (e->img.valid) {
            launch_gate_snapshot(e, np_all);
            e->n_gates = np_all;
        }
        if (np_all > 0) launch_compact(e, e->d.bud_flag, e->d.bud_all, np_all, e->d.plist, e->d.counts + CNT_NPRED);
        np = std::min(np_all, budget);
        e->bud_recs_n = e->bud_predicted = np_all;
        e->bud_selected = np;
    }
    if (slots) {
        e->slot_rb.assign(e->shard_world + 1, 0);
        for (int r = 0; r <= e->shard_world; ++r) e->slot_rb[r] = e->h_counts[CNT_SHARD0 + r];
    } else if (!d_idx) e->slot_rb.clear();
    // (the whole map, all of its predictions: the matcher's gates ride along)
    HpRowsCall rows;
    rows.d_list = d_idx ? e->d.plist_sub : e->d.plist; rows.n_list = np;
    rows.count_predicted = c.count_predicted; rows.gates = !d_idx && !budgeted;
    launch_hp_rows(e, rows);
    if (!d_idx) e->n_pred = np;
    *n_out = np;
    if (e->shard_world > 1 && np > 0) {
        // every rank wrote the H.P rows and S_i of the features it owns
        e->hp_complete = false;
        if (!lean && (rc = complete_hp_table(e))) return rc;
        std::vector<int32_t> rb(e->shard_world + 1);
        for (int r = 0; r <= e->shard_world; ++r) rb[r] = e->shard_feat_begin[r];
        if ((rc = exchange_rows(e, EKF_XCHG_PRED_S, e->d.pred_S, 4 * sizeof(double), rb, "the innovation covariance blocks"))) return rc;
    }
    if (!d_idx && !budgeted && e->keep_step_preds) { // EKF.cpp:294-305 draws the step's predictions as they were BEFORE the updates
        launch_pack_predictions(e, e->d.plist, np, e->d.step_preds);
        e->n_step_preds = np;
    }
    if (!d_idx && !budgeted && e->img.valid) { // image mode: keep the gates of this prediction for detectNewImageFeatures' mask
        launch_gate_snapshot(e, np);
        e->n_gates = np;
    }
    return check_async(e);
}

static int download_predictions(EkfEngine *e, const int *d_list, int np, EkfPrediction *preds, double *Hs, double *Hf)
{
    if (np <= 0) return EKF_OK;
    const int N = e->N;
    std::vector<int> list(np);
    std::vector<double> uv(2 * (size_t)N), S(4 * (size_t)N), hs(14 * (size_t)N), hf(12 * (size_t)N);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(list.data(), d_list, np * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(uv.data(), e->d.pred_uv, uv.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(S.data(), e->d.pred_S, S.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hs.data(), e->d.Hs, hs.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hf.data(), e->d.Hf, hf.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < np; ++k) {
        const int fi = list[k];
        if (preds) {
            preds[k].featureIndex = fi;
            preds[k]._pad = 0;
            preds[k].imagePos[0] = uv[2 * fi];
            preds[k].imagePos[1] = uv[2 * fi + 1];
            for (int i = 0; i < 4; ++i) preds[k].covarianceMatrix[i] = S[4 * fi + i];
        }
        if (Hs)
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 13; ++c) Hs[(size_t)26 * k + r * 13 + c] = c < 7 ? hs[14 * fi + r * 7 + c] : 0.0;
        if (Hf)
            for (int i = 0; i < 12; ++i) Hf[(size_t)12 * k + i] = hf[12 * fi + i];
    }
    return EKF_OK;
}

int ekf_predict_measurements(EkfEngine *e, const int32_t *feat_idx, int count, EkfPrediction *preds, int *n_preds,
                             double *Hs, double *Hf)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    const bool sub = feat_idx && count > 0;
    if (sub) {
        if (count > e->cap) return EKF_ERR_CAPACITY;
        for (int i = 0; i < count; ++i)
            if (feat_idx[i] < 0 || feat_idx[i] >= e->N) return EKF_ERR_INVALID_ARG;
        HIPCHK(hipMemcpyAsync(e->d.work_idx, feat_idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    int np = 0;
    PredictCall call;
    if (sub) { call.d_idx = e->d.work_idx; call.count = count; }
    int rc = predict_measurements_dev(e, call, &np);
    if (rc) return rc;
    if (n_preds) *n_preds = np;
    if (preds || Hs || Hf) return download_predictions(e, sub ? e->d.plist_sub : e->d.plist, np, preds, Hs, Hf);
    return EKF_OK;
}

static int upload_keypoints(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp)
{
    if (n_kp > e->kcap) return EKF_ERR_CAPACITY;
    if (n_kp > 0) {
        HIPCHK(hipMemcpyAsync(e->d.kps, kps, (size_t)n_kp * sizeof(EkfKeypoint), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->d.kdesc, desc32, (size_t)n_kp * e->desc_bytes, hipMemcpyHostToDevice, e->stream));
    }
    e->n_kp = n_kp;
    return EKF_OK;
}

// the keypoints of `call` against the e->n_pred predictions of the last full prediction
static int match_dev(EkfEngine *e, MatchCall call, int *n_matches)
{
    call.n_pred = e->n_pred;
    launch_match(e, call);
    int rc = read_counts(e);
    if (rc) return rc;
    *n_matches = e->h_counts[CNT_NMATCH];
    return check_async(e);
}

// Sharded EKF::step ("Matching: features/ellipses independent => shard by feature; image replicated; all-gather match
// lists"): every rank gates and matches the predictions of the features it OWNS -- one run of slots of the feature-ordered
// predicted list (slot_rb, predict_measurements_dev) -- with either matcher, the per-slot tables (valid flag, keypoint index or
// matched pixel, distance) are all-gathered, and every rank compacts the same tables into the same match list
// (Matching.cpp:217-262 divided by the ranks; the list is identical to the unsharded one, which the tests assert).
static int match_sharded_dev(EkfEngine *e, bool use_ncc, const EkfKeypoint *d_kps, const uint8_t *d_desc, int n_kp, int *n_matches)
{
    const int W = e->shard_world, me = e->shard_rank, np = e->n_pred;
    if ((int)e->slot_rb.size() != W + 1 || e->slot_rb[0] != 0 || e->slot_rb[W] != np) {
        e->err = "sharded matching: the predicted list is not in feature order";
        return EKF_ERR_INVALID_ARG;
    }
    if (use_ncc && !e->img.valid) {
        e->err = "NCC matcher: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    int rc = EKF_OK;
    if (np > 0) {
        if (use_ncc) launch_match_ncc_slots(e, e->slot_rb[me], e->slot_rb[me + 1], e->subpix_on);
        else launch_match_slots(e, d_kps, d_desc, n_kp, e->slot_rb[me], e->slot_rb[me + 1]);
        rc = exchange_rows(e, EKF_XCHG_MATCH_VALID, e->d.mt_valid, sizeof(int), e->slot_rb, "the match flags");
        if (!rc) rc = use_ncc ? exchange_rows(e, EKF_XCHG_MATCH_XY, e->d.mt_xy, sizeof(EkfKeypoint), e->slot_rb, "the matched pixels")
                              : exchange_rows(e, EKF_XCHG_MATCH_KP, e->d.mt_kp, sizeof(int), e->slot_rb, "the matched keypoint indices");
        if (!rc) rc = exchange_rows(e, EKF_XCHG_MATCH_DIST, e->d.mt_dist, sizeof(float), e->slot_rb, "the match distances");
    }
    if (!rc) {
        if (use_ncc) {
            if (np > 0) launch_match_compact_slots(e, np, e->d.mt_xy);
            else HIPCHK(hipMemsetAsync(e->d.counts + CNT_NMATCH, 0, sizeof(int), e->stream));
        } else launch_match_compact(e, d_kps, np);
    }
    if (rc) return rc;
    if ((rc = read_counts(e))) return rc;
    *n_matches = e->h_counts[CNT_NMATCH];
    return check_async(e);
}

int ekf_match(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, EkfMatch *matches,
              int *n_matches)
{
    if (!e || n_kp < 0 || (n_kp > 0 && (!kps || !desc32))) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int rc = upload_keypoints(e, kps, desc32, n_kp);
    if (rc) return rc;
    int M = 0;
    MatchCall call;
    call.kps = e->d.kps; call.kdesc = e->d.kdesc; call.n_kp = n_kp;
    rc = match_dev(e, call, &M);
    if (rc) return rc;
    if (n_matches) *n_matches = M;
    if (matches && M > 0) HIPCHK(hipMemcpy(matches, e->d.matches, (size_t)M * sizeof(EkfMatch), hipMemcpyDeviceToHost));
    return EKF_OK;
}

// RANSAC over e->d.matches[0..M); on return best_flags holds the inlier mask, h_counts the loop state.
// lean (sharded EKF::step, feature-ordered match list): the hypotheses are divided by feature ownership, see below.
static int ransac_dev(EkfEngine *e, int M, bool lean)
{
    launch_ransac_init(e, M);
    launch_match_index(e, M);
    const int batch = e->cfg.ransac_batch;
    const int W = e->shard_world, me = e->shard_rank;
    // Sharded EKF::step ("RANSAC: hypotheses are independent => shard hypotheses across GPUs, all-gather the support
    // counts"): hypothesis h uses the H.P rows of ITS feature as gain columns, and those rows are with the feature's owner -- so every
    // rank evaluates the hypotheses of the features it owns (one run [mb[me], mb[me + 1]) of the feature-ordered match list: no row of
    // H.P travels) and the ranks all-gather a batch's support counts (4 bytes per hypothesis) and inlier masks (M bytes per
    // hypothesis) before the sequential bookkeeping, which every rank then replays identically (1PointRansac.cpp:125-180).
    const bool by_owner = lean && W > 1 && !e->hp_complete;
    std::vector<int32_t> mb, rb;
    if (by_owner) {
        launch_shard_bounds(e, e->d.matches, M);
        int rc = read_counts(e);
        if (rc) return rc;
        mb.assign(W + 1, 0);
        for (int r = 0; r <= W; ++r) mb[r] = e->h_counts[CNT_SHARD0 + r];
        if (mb[0] != 0 || mb[W] != M) {
            e->err = "sharded RANSAC: the match list is not in feature order";
            return EKF_ERR_INVALID_ARG;
        }
        rb.assign(W + 1, 0);
    }
    for (int h0 = 0, nb = batch; h0 < M; h0 += nb, nb = batch * RANSAC_WIDE_FACTOR) {
        const int batch = nb; // (this batch's width: the first one narrow -- a converged filter ends inside it --, the others wide)
        if (by_owner) {
            const int h1 = std::min(M, h0 + batch);
            launch_ransac_hyp(e, M, h0, batch, /*d_M*/ nullptr, mb[me], mb[me + 1]);
            for (int r = 0; r <= W; ++r) rb[r] = std::min(std::max(mb[r], h0), h1) - h0; // rows of the batch's tables by owner
            int rc;
            if ((rc = exchange_rows(e, EKF_XCHG_HYP_COUNT, e->d.hyp_count, sizeof(int), rb, "the support counts of a RANSAC batch"))) return rc;
            if ((rc = exchange_rows(e, EKF_XCHG_HYP_FLAGS, e->d.hyp_flags, (size_t)e->mcap, rb, "the inlier masks of a RANSAC batch"))) return rc;
            launch_ransac_select(e, M, h0, batch, /*d_M*/ nullptr, /*publish_seq*/ 0);
        } else {
            launch_ransac_batch(e, M, h0, batch);
        }
        int rc = read_counts(e);
        if (rc) return rc;
        if (e->h_counts[CNT_RS_DONE]) break;
    }
    return check_async(e);
}

// The device code keys predictions, Jacobians and H.P rows by featureIndex: one match per feature (what the matcher
// produces, Matching.cpp:217-262).  A list with a repeated featureIndex is rejected instead of being half-processed.
int ekf::validate_matches(const EkfEngine *e, const EkfMatch *m, int M)
{
    if (M < 0 || M > e->cap || (M > 0 && !m)) return EKF_ERR_INVALID_ARG;
    std::vector<uint8_t> seen((size_t)e->N, 0);
    for (int i = 0; i < M; ++i) {
        const int f = m[i].featureIndex;
        if (f < 0 || f >= e->N || seen[f]) return EKF_ERR_INVALID_ARG;
        seen[f] = 1;
    }
    return EKF_OK;
}

int ekf_ransac(EkfEngine *e, const EkfMatch *matches, int M, uint8_t *inlier_mask, int *n_hypotheses)
{
    if (!e || !inlier_mask) return EKF_ERR_INVALID_ARG;
    int rc = validate_matches(e, matches, M);
    if (rc) return rc;
    if (n_hypotheses) *n_hypotheses = 0;
    if (M == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->d.matches, matches, (size_t)M * sizeof(EkfMatch), hipMemcpyHostToDevice, e->stream));
    if ((rc = complete_hp_table(e))) return rc; // a sharded step leaves the H.P table with the owners' rows only
    rc = ransac_dev(e, M, /*lean*/ false);
    if (rc) return rc;
    HIPCHK(hipMemcpy(inlier_mask, e->d.best_flags, (size_t)M, hipMemcpyDeviceToHost));
    if (n_hypotheses) *n_hypotheses = e->h_counts[CNT_RS_NEXT];
    return EKF_OK;
}

// update with the matches in e->d.msel[0..M), recorded as `stage` (UpdateCall); lean: a sharded step, whose H.P table holds the
// owners' rows only -- the gather stage completes the gathered rows by an exchange (kernels_update.hip); early: launch_early_gather
static int update_dev(EkfEngine *e, int M, int kind, int stage, bool lean, const EarlyGather &early)
{
    if (M <= 0) return EKF_OK; // Update.cpp:292
    lean = lean && e->shard_world > 1 && !e->hp_complete;
    if (lean) { // where each rank's run of the (feature-ordered) selected matches starts
        launch_shard_bounds(e, e->d.msel, M);
        int rc = read_counts(e);
        if (rc) return rc;
        e->shard_rb.assign(e->shard_world + 1, 0);
        for (int r = 0; r <= e->shard_world; ++r) e->shard_rb[r] = 2 * e->h_counts[CNT_SHARD0 + r];
        if (e->shard_rb[0] != 0 || e->shard_rb[e->shard_world] != 2 * M) {
            e->err = "sharded update: the match list is not in feature order";
            return EKF_ERR_INVALID_ARG;
        }
    }
    UpdateCall call;
    call.matches = e->d.msel; call.M = M; call.kind = kind; call.stage = stage;
    call.lean = lean; call.early = early;
    const int rc = launch_update(e, call);
    return rc ? rc : check_async(e);
}

// e->h_counts[CNT_ERR] != 0 was read back: the last update enqueued failed and, with everything enqueued behind it, left the filter
// as it was (filter_frozen, engine.h).  Clears the flag.  A persistent sweep that timed out (another process's kernels on the
// device, a partition that could not hold the grid: chol_persist.h) is not the caller's problem: the SAME update -- its match list
// is still in d.msel -- runs again on the launch-per-panel sweep, which has no cross-workgroup waits, from the untouched P
// (S, nu and the gathered rows are formed again); *status stays EKF_OK when that succeeds and the engine counts the retry.
// Anything else (S not positive definite) goes to *status: that update is skipped, as the reference skips it (cv::invert
// returns zeros, K = 0: EKF/Update.cpp:101-108).  Returns a hard error (HIP, exchange) or EKF_OK.  Called right after a read-back,
// so a step's unread flag (err_unread) has been read and is handled here.
static int recover_failed_update(EkfEngine *e, int *status)
{
    e->err_unread = false;
    const int code = e->h_counts[CNT_ERR];
    if (!code) return EKF_OK;
    HIPCHK(hipMemsetAsync(e->d.counts + CNT_ERR, 0, sizeof(int), e->stream));
    e->h_counts[CNT_ERR] = 0;
    e->p_exact_sym = e->last_update.sym; // (the frozen downdate did not symmetrise an uploaded P)
    if (code == EKF_ERR_TIMEOUT && e->last_update.persist && e->last_update.call.M > 0) {
        e->ps_backoff_len = std::min(std::max(64, 2 * e->ps_backoff_len), 4096); // see engine.h
        e->ps_backoff = e->ps_backoff_len;
        e->ps_ok_streak = 0;
        // (filter consistency: the retry records the stage of the update it repeats)
        int rc = launch_update(e, retry_of(e->last_update.call));
        if (!rc) rc = check_async(e);
        ++e->sweep_retries;
        if (rc) return rc;
        if ((rc = read_counts(e))) return rc;
        if (!e->h_counts[CNT_ERR]) return EKF_OK;
        const int code2 = e->h_counts[CNT_ERR]; // the retry's own outcome (it cannot time out)
        HIPCHK(hipMemsetAsync(e->d.counts + CNT_ERR, 0, sizeof(int), e->stream));
        e->h_counts[CNT_ERR] = 0;
        e->p_exact_sym = e->last_update.sym;
        *status = code2;
    } else {
        *status = code;
    }
    e->err = *status == EKF_ERR_TIMEOUT ? "the persistent Cholesky sweep timed out"
             : (*status == EKF_ERR_NON_FINITE ? "a row of B = inv(L) H P does not fit its a-priori column scale (covariance not positive semi-definite, or not finite)"
                                              : "S = H P H' + R is not positive definite");
    return EKF_OK;
}

// --------------------------------------------------------------------------------- iterated update
// the mode's scratch, on its first use (DeviceArrays::iter_*)
static int iterate_scratch(EkfEngine *e)
{
    if (e->d.iter_uv) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    const size_t image = ITER_X + 6 * (size_t)e->cap;
    auto g = e->bufs.group();
    g.alloc(&e->d.iter_uv, 2 * (size_t)e->cap);
    g.alloc(&e->d.iter_snap, image);
    g.alloc(&e->d.iter_lin, 2 * image);
    g.alloc(&e->d.iter_diag, (size_t)e->ncap);
    g.alloc(&e->d.iter_step, (size_t)ITER_SLOTS * EKF_MAX_UPDATE_ITERATIONS);
    g.alloc(&e->d.iter_idx, (size_t)e->cap);
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "iterated update scratch");
    return EKF_OK;
}

// why an update of `iterations` passes is not available on this engine, or null
static const char *iterations_refusal(const EkfEngine *e, int iterations, double tol)
{
    if (iterations < 1 || iterations > EKF_MAX_UPDATE_ITERATIONS) return "iterations must be 1 .. 8";
    if (!(tol >= 0.0) || !std::isfinite(tol)) return "tol must be finite and not negative";
    if (e->shard_world > 1) return "not available on a sharded engine";
    if (iterations > 1 && e->fixed_map) return "more than one pass is not available while the fixed-map mode is on";
    return nullptr;
}

// The covariance update with the matches in e->d.msel[0..M) in up to K passes, recorded as `stage`; the record goes to
// e->iter_records, its steps to slot iter_records.size() of d.iter_step.  Pass 0 is today's update from the tables of the caller's
// prediction; pass i >= 1 predicts the matched features again at x^i (a sub-list prediction: no counter of the map moves), shifts
// the predictions to the prior (k_iter_shift_restore) and runs the update from x^ with that table.  Two launches per extra pass
// beside the prediction's and the update's own, and no read-back but the prediction's -- which also brings the tolerance flag, the
// number predicted and the error flag of the pass before.  *status: as recover_failed_update (a pass whose S is not positive
// definite: x and P are those before the update, the remaining passes are not run); returns a hard error or EKF_OK.
static int iterated_update_dev(EkfEngine *e, int M, int stage, int K, double tol, int *status)
{
    if (M <= 0) return EKF_OK; // Update.cpp:292
    int rc;
    if ((rc = iterate_scratch(e))) return rc;
    const int slot = (int)e->iter_records.size();
    if (slot >= ITER_SLOTS) {
        e->err = "more iterated updates in one call than records";
        return EKF_ERR_INVALID_ARG;
    }
    EkfIterationRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    rec.stage = stage;
    rec.stop_reason = EKF_ITER_STOP_COUNT;
    double *steps = e->d.iter_step + (size_t)slot * EKF_MAX_UPDATE_ITERATIONS;
    launch_iter_snapshot(e, e->d.msel, M, steps);
    int lin = 0; // the image of d.iter_lin that holds the linearisation point of the pass about to run
    bool last = K == 1;
    for (int i = 0;; ++i) {
        if (i >= 1) { // the live state is x^i
            int np = 0;
            PredictCall sub;
            sub.d_idx = e->d.iter_idx; sub.count = M;
            for (int attempt = 0; attempt < 2; ++attempt) {
                launch_iter_step(e, lin, lin ^ 1, steps + (i - 1), tol);
                if ((rc = predict_measurements_dev(e, sub, &np))) return rc;
                if (!e->h_counts[CNT_ERR]) break;
                // pass i - 1 failed (seen at this read-back; everything behind it left x = x^ alone): run it again or give up
                // (recover_failed_update), then this pass's preamble again.  The prediction above ran at x^ and overwrote the tables
                // of pass i - 1, which its retry gathers from: they are formed again at x^(i-1) first, and x^ is put back
                if (i >= 2) {
                    launch_iter_load(e, lin, /*even_frozen*/ true);
                    if ((rc = predict_measurements_dev(e, sub, &np))) return rc;
                    launch_iter_shift_restore(e, e->d.msel, M, lin, /*even_frozen*/ true);
                }
                int st = EKF_OK;
                if ((rc = recover_failed_update(e, &st))) return rc;
                if (st) {
                    rec.passes_run = i - 1;
                    rec.stop_reason = EKF_ITER_STOP_FAILED;
                    e->iter_records.push_back(rec);
                    *status = st;
                    return EKF_OK;
                }
            }
            if (np < M) {
                // a matched feature is not predicted at x^i: finish from x^(i-1), where all of them were, by predicting there again
                rec.stop_reason = EKF_ITER_STOP_FEATURE_LEFT;
                last = true;
                launch_iter_load(e, lin);
                if ((rc = predict_measurements_dev(e, sub, &np))) return rc;
            } else {
                lin ^= 1;
                if (tol > 0.0 && e->h_counts[CNT_ITER_SMALL]) {
                    rec.stop_reason = EKF_ITER_STOP_TOL;
                    last = true;
                }
                if (i == K - 1) last = true;
            }
            launch_iter_shift_restore(e, e->d.msel, M, lin);
        }
        UpdateCall call;
        call.matches = e->d.msel; call.M = M; call.kind = last ? UPDATE_COV : UPDATE_STATE_ONLY; call.stage = stage;
        call.pred_uv = i >= 1 ? e->d.iter_uv : nullptr;
        if ((rc = launch_update(e, call)) || (rc = check_async(e))) return rc;
        if (last) {
            rec.passes_run = rec.stop_reason == EKF_ITER_STOP_FEATURE_LEFT ? i : i + 1;
            break;
        }
    }
    launch_iter_step(e, lin, -1, steps + (rec.passes_run - 1), 0.0); // the last pass's step, to the normalised state
    e->iter_lin_sel = lin;
    e->iter_lin_N = e->N;
    e->iter_records.push_back(rec);
    return EKF_OK;
}

int ekf_update_iterated(EkfEngine *e, const EkfMatch *matches, int M, int iterations, double tol)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (const char *why = iterations_refusal(e, iterations, tol)) {
        e->err = std::string("ekf_update_iterated: ") + why;
        return EKF_ERR_INVALID_ARG;
    }
    int rc = validate_matches(e, matches, M);
    if (rc) return rc;
    e->iter_records.clear();
    if (M == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->d.msel, matches, (size_t)M * sizeof(EkfMatch), hipMemcpyHostToDevice, e->stream));
    if (e->consistency) ++e->cons_epoch; // the record of this call: the covariance pass
    int status = EKF_OK;
    const int retries0 = e->sweep_retries;
    if ((rc = iterated_update_dev(e, M, /*stage*/ 0, iterations, tol, &status))) return rc;
    if (status) return status;
    rc = finish_update(e);
    EkfIterationRecord &rec = e->iter_records.back();
    if (rc == EKF_ERR_NOT_POSITIVE_DEFINITE || rc == EKF_ERR_NON_FINITE || rc == EKF_ERR_TIMEOUT) {
        rec.stop_reason = EKF_ITER_STOP_FAILED; // the covariance pass: x and P are those before the call
        rec.passes_run -= 1;                    // ... and the passes before it are all that ran
    } else if (!rc && e->sweep_retries != retries0) {
        // the covariance pass timed out and was run again: its step was taken from the frozen state, take it again
        launch_iter_step(e, e->iter_lin_sel, -1, e->d.iter_step + (rec.passes_run - 1), 0.0);
    }
    return rc;
}

int ekf_set_update_iterations(EkfEngine *e, int iterations, double tol)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (const char *why = iterations_refusal(e, iterations, tol)) {
        e->err = std::string("ekf_set_update_iterations: ") + why;
        return EKF_ERR_INVALID_ARG;
    }
    e->update_iterations = iterations;
    e->update_iter_tol = tol;
    return EKF_OK;
}

int ekf_get_update_iterations(const EkfEngine *e, int *iterations, double *tol)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (iterations) *iterations = e->update_iterations;
    if (tol) *tol = e->update_iter_tol;
    return EKF_OK;
}

int ekf_get_iteration_records(EkfEngine *e, EkfIterationRecord *out, int capacity, int *count)
{
    if (!e || !count || capacity < 0) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e);
    if (rc) return rc;
    const int n = (int)e->iter_records.size();
    *count = n;
    if (!out || n == 0) return EKF_OK;
    if (capacity < n) return EKF_ERR_CAPACITY;
    for (int k = 0; k < n; ++k) {
        out[k] = e->iter_records[k];
        HIPCHK(hipMemcpy(out[k].step, e->d.iter_step + (size_t)k * EKF_MAX_UPDATE_ITERATIONS, sizeof(out[k].step), hipMemcpyDeviceToHost));
        for (int i = std::max(0, out[k].passes_run); i < EKF_MAX_UPDATE_ITERATIONS; ++i) out[k].step[i] = 0.0;
    }
    return EKF_OK;
}

int ekf_get_linearisation_point(EkfEngine *e, double x13[13], double *feature_pos)
{
    if (!e || !x13) return EKF_ERR_INVALID_ARG;
    // (the map's host side clears iter_lin_sel wherever the map is replaced or its layout changes; the count is checked all the same:
    // feature_pos is sized by the caller from the map as it is now)
    if (e->iter_lin_sel < 0 || !e->d.iter_lin || e->iter_lin_N != e->N) {
        e->err = "ekf_get_linearisation_point: no iterated update has run on this map";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const double *img = e->d.iter_lin + (size_t)e->iter_lin_sel * (ITER_X + 6 * (size_t)e->cap);
    HIPCHK(hipMemcpy(x13, img + ST_X, 13 * sizeof(double), hipMemcpyDeviceToHost));
    if (feature_pos && e->iter_lin_N > 0) HIPCHK(hipMemcpy(feature_pos, img + ITER_X, (size_t)e->iter_lin_N * 6 * sizeof(double), hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf::finish_update(EkfEngine *e)
{
    int rc = read_counts(e);
    if (rc) return rc;
    int status = EKF_OK;
    if ((rc = recover_failed_update(e, &status))) return rc;
    return status;
}

int ekf::update_stage(EkfEngine *e, const EkfMatch *matches, int M, int kind)
{
    int rc = validate_matches(e, matches, M);
    if (rc) return rc;
    if (M == 0) return EKF_OK;
    if (kind == UPDATE_FIXED_MAP && (rc = fixed_map_scratch(e))) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->d.msel, matches, (size_t)M * sizeof(EkfMatch), hipMemcpyHostToDevice, e->stream));
    if ((rc = complete_hp_table(e))) return rc; // (a fixed-map engine is not sharded: nothing to complete)
    if (kind != UPDATE_STATE_ONLY && e->consistency) ++e->cons_epoch; // the records of this call: DESIGN.md 4.11
    if ((rc = update_dev(e, M, kind, /*stage*/ 0, /*lean*/ false, EarlyGather()))) return rc;
    return finish_update(e);
}

int ekf_update(EkfEngine *e, const EkfMatch *matches, int M) { return e ? update_stage(e, matches, M, UPDATE_COV) : EKF_ERR_INVALID_ARG; }

int ekf_update_only_state(EkfEngine *e, const EkfMatch *matches, int M)
{
    return e ? update_stage(e, matches, M, UPDATE_STATE_ONLY) : EKF_ERR_INVALID_ARG;
}

// ------------------------------------------------------------------------------------------------------ step
void ekf::harvest_pu_events(EkfEngine *e)
{
    for (auto &pr : e->px_events) { // exact downdate: the column-scale + digit-plane kernels (their end event is the downdate's start event, destroyed below)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) e->slice_ms += ms;
        (void)hipEventDestroy(pr.first);
    }
    e->px_events.clear();
    for (const PuBracket &b : e->pu_events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, b.first, b.second) == hipSuccess) {
            e->times.p_update_kernel_ms += ms;
            e->times.p_update_launches += 1;
            e->times.p_update_flops += b.work;
            e->times.p_update_bytes += 2.0 * (double)e->n * (double)e->n * (e->f32 ? 4.0 : 8.0);
            e->pu_log.emplace_back(b.m, ms);
        }
        (void)hipEventDestroy(b.first);
        (void)hipEventDestroy(b.second);
    }
    e->pu_events.clear();
    for (const SweepBracket &b : e->sw_events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, b.first, b.second) == hipSuccess) {
            const double m = std::abs(b.m);
            e->sweep_ms += ms;
            e->sweep_panels += ((long long)m + NB - 1) / NB;
            e->sweep_launches += b.launches;
            e->sweep_updates += 1;
            e->sweep_flops_f64 += m * m * m / 3.0;                  // Cholesky of S
            if (b.m > 0) e->sweep_flops_b += m * m * (double)e->n;  // B = inv(L) (H P): forward substitution, m^2 n
        }
        (void)hipEventDestroy(b.first);
        (void)hipEventDestroy(b.second);
    }
    e->sw_events.clear();
}

namespace {
struct StageTimer {
    EkfEngine *e;
    std::vector<hipEvent_t> evs;
    explicit StageTimer(EkfEngine *eng) : e(eng) {}
    ~StageTimer() // early returns of a step skip finish(): the events recorded so far are released here
    {
        for (auto ev : evs) (void)hipEventDestroy(ev);
    }
    void mark()
    {
        if (!e->timing) return;
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        (void)hipEventRecord(ev, e->stream);
        evs.push_back(ev);
    }
    void finish()
    {
        if (!e->timing || evs.size() < 7) return;
        (void)hipStreamSynchronize(e->stream);
        double *dst[6] = {&e->times.prediction_ms, &e->times.matching_ms, &e->times.ransac_ms,
                          &e->times.update_li_ms,  &e->times.rescue_ms,   &e->times.update_hi_ms};
        for (int i = 0; i < 6; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, evs[i], evs[i + 1]) == hipSuccess) *dst[i] += ms;
        }
        for (auto ev : evs) (void)hipEventDestroy(ev);
        evs.clear();
        e->times.steps += 1;
        harvest_pu_events(e);
    }
};
} // namespace

namespace {
// The running values of one step: what its schedule has decided and counted so far.
struct StepRun {
    EkfEngine *e;
    int kind;           // of both updates: UPDATE_COV, or UPDATE_FIXED_MAP (ekf_set_fixed_map: they move the camera alone)
    bool lean = false;  // sharded: rows of H.P travel when consumed, not after every prediction
    int budget = 0;     // measurement budget K where it can bind, else 0
    bool normals = false, detect = false; // what the last read-back also carries: the patch-normal and the keypoint counters
    int iterations = 1; // passes of both updates (ekf_set_update_iterations; > 1 on the host-count schedule only)
    double iter_tol = 0.0;
    int np = 0, M = 0, ni = 0, no = 0, nr = 0; // predicted, matches, inliers, outliers, rescued
    EkfStepInfo li;
    int status;         // of the step: EKF_OK, or why an update was skipped (recover_failed_update)
    int retries0;       // e->sweep_retries when the step began
    StageTimer tm;
    StepRun(EkfEngine *eng, int kind_, int status0, int retries) : e(eng), kind(kind_), status(status0), retries0(retries), tm(eng)
    {
        std::memset(&li, 0, sizeof(li));
    }
};
} // namespace

// the RANSAC loop has ended and its counters are in h_counts (np and M are set): what the step records of it
static void take_ransac_result(StepRun &s)
{
    EkfEngine *e = s.e;
    s.li.n_predicted = s.np;
    s.li.n_matches = s.M;
    if (!s.budget) { // measurement budget counts of a step it did not bind in
        e->bud_recs_n = 0;
        e->bud_predicted = e->bud_selected = s.np;
    }
    if (s.M > 0) {
        s.li.n_hypotheses = e->h_counts[CNT_RS_NEXT];
        s.ni = e->h_counts[CNT_RS_BEST];
        s.no = s.M - s.ni;
    }
    s.li.n_inliers = s.ni;
    s.li.n_outliers = s.no;
}

// 7. low-innovation update (:430), with the inliers in d.msel
static int low_innovation_update(StepRun &s)
{
    s.tm.mark();
    const int rc = s.iterations > 1 ? iterated_update_dev(s.e, s.ni, /*stage*/ 1, s.iterations, s.iter_tol, &s.status)
                                    : update_dev(s.e, s.ni, s.kind, /*stage*/ 1, s.lean, EarlyGather());
    s.tm.mark();
    return rc;
}

// 10. high-innovation update (:529-532), with the rescued in d.msel (this update's route decides whether the early launch
// serves it: launch_update)
static int high_innovation_update(StepRun &s, const EarlyGather &early)
{
    s.li.n_rescued = s.nr;
    const int rc = s.iterations > 1 ? iterated_update_dev(s.e, s.nr, /*stage*/ 2, s.iterations, s.iter_tol, &s.status)
                                    : update_dev(s.e, s.nr, s.kind, /*stage*/ 2, s.lean, early);
    s.tm.mark();
    return rc;
}

// the end of a step whose last read-back is done or left to the next call
static int close_step(StepRun &s, EkfStepInfo *info)
{
    s.tm.finish();
    s.li.status = s.status;
    s.li.n_sweep_retries = s.e->sweep_retries - s.retries0;
    if (info) *info = s.li;
    return s.status;
}

// the step's last read-back: the error flag of the second update, and the counters that travel with it
static int finish_step(StepRun &s, EkfStepInfo *info)
{
    EkfEngine *e = s.e;
    int rc;
    if ((rc = read_counts(e))) return rc;
    if (s.normals) harvest_pn_counts(e);
    if (s.detect) {
        e->step_kp_detected = e->h_counts[CNT_KP_FOUND];
        e->step_kp_kept = std::min(e->step_kp_detected, e->kcap);
    }
    if ((rc = recover_failed_update(e, &s.status))) return rc;
    return close_step(s, info);
}

// what step_device_counts returns, besides the codes of the ABI, when its first read-back shows the error flag of the PREVIOUS
// step's last update, left unread (err_unread): nothing this run enqueued has touched the filter (filter_frozen, engine.h)
constexpr int STEP_FOUND_UNREAD_FAILURE = -1;

// EKF::step on the device-count schedule.  How many features were predicted, how many matches there are and how many outliers
// were re-predicted only decide launch sizes, so the launches use upper bounds (N, N, the outlier count) and the kernels read the
// counts on the device.  What the host still needs to know -- the RANSAC result (loop state and inlier count: the size of the first
// update), the rescued count (the size of the second), the error flag -- comes from three read-backs instead of six (two with
// ekf_set_async_errors).  A read-back idles the GPU for as long as the host needs to see the counters and enqueue the next
// launch, a few us; behind the first two the next stage's first launch is therefore enqueued BEFORE the poll, sized by an upper
// bound and reading its count on the device: the low-innovation partition behind the first RANSAC batch (28.2 against 36.0 us
// per frame in ransac_ms) and the second update's gather / assembly behind the rescue partition (2-3 us per frame; DESIGN.md
// 4.2).  What follows them -- the sweeps, whose grid layout the host decides from the size -- still waits.
// may_find_unread: this is the step's first run, see STEP_FOUND_UNREAD_FAILURE.
static int step_device_counts(StepRun &s, const StepInput &in, bool may_find_unread, EkfStepInfo *info)
{
    EkfEngine *e = s.e;
    int *cnt = e->d.counts;
    int rc;
    if (e->consistency) ++e->cons_epoch; // filter consistency: the records of this step
    s.tm.mark();
    // 1-2. prediction (:273-284), timesPredicted++ (EKF.cpp:572): covariance strips and pixel predictions in one launch; with more
    // than 256 features the compaction of the predicted list rides in the launch of the H P rows, as do the matcher's gates
    HpRowsCall rows;
    rows.d_list = e->d.plist; rows.n_list = e->N; rows.d_count = cnt + CNT_NPRED;
    rows.count_predicted = true; rows.gates = true;
    rows.from_flags = launch_predict_with_features(e, e->N, e->step_dt);
    launch_hp_rows(e, rows);
    s.tm.mark();
    // 4. matching (:337), + the RANSAC loop state and the feature -> match index
    MatchCall match;
    match.kps = in.d_kps; match.kdesc = in.d_desc; match.n_kp = in.n_kp;
    match.n_pred = e->N; match.d_npred = cnt + CNT_NPRED;
    match.with_ransac_init = true;
    launch_match(e, match);
    s.tm.mark();
    // 6. 1-point RANSAC (:402); predictions/Jacobians are looked up by featureIndex (:368-392).  The first batch is launched
    // before anything is known on the host
    const int batch = e->cfg.ransac_batch;
    const int seq_r = next_publish_seq(e);
    launch_ransac_batch(e, e->N, 0, batch, cnt + CNT_NMATCH, seq_r);
    // The partition behind the loop is enqueued before the host polls for the batch's outcome, so the GPU does not wait for the
    // host between the two: sized by N, it reads the match count on the device and does nothing unless this batch ended the loop
    // and the filter is not frozen (k_partition: behind_ransac) -- a second run of the step sees no side effect.
    RansacPartition part;
    part.d_kdesc = in.d_desc;
    const bool early_partition = e->N > 0;
    if (early_partition) {
        part.M = e->N; part.d_M = cnt + CNT_NMATCH; part.behind_ransac = true;
        launch_ransac_partition(e, part);
    }
    if ((rc = wait_counts(e, seq_r))) return rc;
    if (e->h_counts[CNT_ERR] && may_find_unread) return STEP_FOUND_UNREAD_FAILURE;
    s.np = e->n_pred = e->h_counts[CNT_NPRED];
    s.M = e->h_counts[CNT_NMATCH];
    const bool partitioned = early_partition && e->h_counts[CNT_RS_DONE] && !e->h_counts[CNT_ERR]; // what the early launch saw (same counter block)
    for (int h0 = batch, nb = batch * RANSAC_WIDE_FACTOR; !e->h_counts[CNT_RS_DONE] && h0 < s.M; h0 += nb) {
        launch_ransac_batch(e, s.M, h0, nb); // (wide batches behind the first: see ransac_dev)
        if ((rc = read_counts(e))) return rc;
    }
    take_ransac_result(s);
    // + updateMapFeatures for the low-innovation inliers (MapManagement.cpp:88-113), same launch -- unless the first batch ended
    // the loop: the launch enqueued behind that batch has done this
    if (s.M > 0 && !partitioned) {
        part.M = s.M; part.d_M = nullptr; part.behind_ransac = false;
        launch_ransac_partition(e, part);
    }
    if ((rc = low_innovation_update(s))) return rc;
    // 8-9. re-predict the outliers with the updated state / covariance, rescue (:473-506): rescued matches join the inliers
    // (EKF.cpp:552-556).  An outlier that is not re-predicted has pred_vis = 0 and is not rescued.
    EarlyGather early; // the second update's gather / assembly, where it is already enqueued for the count this stage left on the device
    if (s.no > 0) {
        for (int attempt = 0; attempt < 2; ++attempt) {
            launch_predict_features(e, e->d.work_idx, s.no, /*state_only*/ false);
            HpRowsCall sub;
            sub.d_list = e->d.plist_sub; sub.n_list = s.no; sub.d_count = cnt + CNT_NPRED_SUB;
            launch_hp_rows(e, sub);
            // rescueOutliers (EKF.cpp:84-97) and the partition it feeds in one launch
            RescuePartition resc;
            resc.n_outliers = s.no; resc.d_kdesc = in.d_desc;
            resc.fused_rescue = true; resc.publish_seq = next_publish_seq(e);
            launch_rescue_partition(e, resc);
            // The second update's first launch goes behind the partition before the host polls for the rescued count, so the GPU
            // does not wait for the host between the two: sized by the outlier count, it reads the rescued count on the device
            // and writes update scratch only -- nothing at all behind a failed first update, where this stage runs again below.
            // (Only where the partition publishes the counters itself: a copy of the counter block made behind this launch could show
            // the error flag of the SECOND update's first diagonal block as if the first update had failed.)
            early = resc.publish_seq > 0 ? launch_early_gather(e, s.no, cnt + CNT_NRESC, s.kind) : EarlyGather();
            if ((rc = wait_counts(e, resc.publish_seq))) return rc;
            if (!e->h_counts[CNT_ERR]) break;
            // the first update failed (seen at this stage's read-back; everything behind it was frozen, the fused partition did
            // nothing and the inliers are still in d.msel): run it again or skip it (recover_failed_update), then this stage again
            early = EarlyGather();
            if ((rc = recover_failed_update(e, &s.status))) return rc;
        }
        s.nr = e->h_counts[CNT_NRESC];
    }
    s.tm.mark();
    if ((rc = high_innovation_update(s, early))) return rc;
    if (e->async_errors) {
        e->err_unread = true; // reported by the next step, ekf_synchronize or ekf_get_state
        return close_step(s, info);
    }
    return finish_step(s, info);
}

// EKF::step on the host-count schedule: the counts are read back after each stage, because the host sizes or records launches
// by them -- with an image loaded the prediction's gates are snapshotted for the detectors (n_gates), kept predictions are packed
// for ekf_get_step_predictions, the NCC matcher is launched per prediction, a sharded engine divides predictions, matches and
// updates between the ranks by owner, and the measurement budget ranks the predictions before the H P pass.
// STEP_DETECT_KEYPOINTS: the keypoints of this frame are detected and described on the device between the prediction and the
// matching (ekf_set_image_matcher(EKF_IMAGE_MATCHER_KEYPOINTS)).
static int step_host_counts(StepRun &s, const StepInput &in, EkfStepInfo *info)
{
    EkfEngine *e = s.e;
    const bool use_ncc = in.source == STEP_NCC;
    int rc;
    // A failed update is seen at the next read-back; until then everything enqueued behind it has left the filter alone
    // (filter_frozen, engine.h).  The previous step's last update can still be unread (err_unread, ekf_set_async_errors): this
    // schedule reads it before it launches anything, and that update runs again or is skipped and reported here.
    if (e->err_unread) {
        if ((rc = read_counts(e))) return rc;
        if ((rc = recover_failed_update(e, &s.status))) return rc;
    }
    if (e->consistency) ++e->cons_epoch; // filter consistency: the records of this step
    s.tm.mark();
    // 1-2. prediction (:273-284), timesPredicted++ (EKF.cpp:572)
    launch_predict(e, e->step_dt);
    PredictCall full;
    full.count_predicted = true; full.lean = s.lean; full.budget = s.budget;
    if ((rc = predict_measurements_dev(e, full, &s.np))) return rc;
    s.tm.mark();
    // 4. matching (:337); keypoints from images: detector + descriptor inside the gates of this prediction (Matching.cpp:188-210)
    if (s.detect && (rc = detect_step_keypoints(e))) return rc;
    if (s.lean) { // every rank matches the predictions of its own features
        rc = match_sharded_dev(e, use_ncc, in.d_kps, in.d_desc, in.n_kp, &s.M);
    } else if (use_ncc) {
        rc = match_ncc_dev(e, &s.M);
    } else {
        MatchCall match;
        match.kps = in.d_kps; match.kdesc = in.d_desc; match.n_kp = in.n_kp;
        if (s.detect) match.d_nkp = e->d.counts + CNT_KP_FOUND; // n_kp is the capacity, the count is read by the kernel
        rc = match_dev(e, match, &s.M);
    }
    if (rc) return rc;
    s.tm.mark();
    // 6. 1-point RANSAC (:402); predictions/Jacobians are looked up by featureIndex (:368-392)
    if (s.M > 0 && (rc = ransac_dev(e, s.M, s.lean))) return rc;
    take_ransac_result(s);
    if (s.M > 0) { // + updateMapFeatures for the low-innovation inliers (MapManagement.cpp:88-113), same launch
        RansacPartition part;
        part.M = s.M; part.d_kdesc = in.d_desc;
        launch_ransac_partition(e, part);
    }
    // patch normals: the estimator runs behind the frame's last update on the inliers and the rescued; d.msel is
    // overwritten by the rescue, so each list is copied behind its partition
    if (s.normals && s.ni > 0)
        HIPCHK(hipMemcpyAsync(e->d.pn_list, e->d.msel, (size_t)s.ni * sizeof(EkfMatch), hipMemcpyDeviceToDevice, e->stream));
    if ((rc = low_innovation_update(s))) return rc;
    // 8-9. re-predict the outliers with the updated state / covariance, rescue (:473-506): rescued matches join the inliers
    // (EKF.cpp:552-556).  An outlier that is not re-predicted has pred_vis = 0 and is not rescued.
    if (s.no > 0) {
        int nop = 0;
        PredictCall outliers;
        outliers.d_idx = e->d.work_idx; outliers.count = s.no; outliers.lean = s.lean;
        for (int attempt = 0; attempt < 2; ++attempt) {
            if ((rc = predict_measurements_dev(e, outliers, &nop))) return rc;
            if (!e->h_counts[CNT_ERR]) break;
            // the first update failed (seen at this stage's read-back; everything behind it was frozen and the inliers are still
            // in d.msel): run it again or skip it (recover_failed_update), then this stage again
            if ((rc = recover_failed_update(e, &s.status))) return rc;
        }
        if (nop > 0) {
            launch_rescue(e, e->d.mout, s.no);
            RescuePartition resc;
            resc.n_outliers = s.no; resc.d_kdesc = in.d_desc;
            launch_rescue_partition(e, resc);
            if ((rc = read_counts(e))) return rc;
            s.nr = e->h_counts[CNT_NRESC];
        }
    }
    s.tm.mark();
    if (s.normals && s.nr > 0)
        HIPCHK(hipMemcpyAsync(e->d.pn_list + s.ni, e->d.msel, (size_t)s.nr * sizeof(EkfMatch), hipMemcpyDeviceToDevice, e->stream));
    if ((rc = high_innovation_update(s, EarlyGather()))) return rc;
    if (s.normals) launch_ncc_normal(e, s.ni + s.nr); // its two counters travel with the step's last read-back
    return finish_step(s, info);
}

// Whether a step can leave its counts on the device: descriptor matcher on keypoints the host supplied, no image loaded, no kept
// predictions, one GPU, no binding measurement budget, plain (un-iterated) updates.  Everything else needs a count on the host between two stages
// (step_host_counts says what for).
static bool counts_stay_on_device(const EkfEngine *e, const StepInput &in, bool budget_active)
{
    return in.source == STEP_KEYPOINTS && !e->img.valid && !e->keep_step_preds && e->shard_world == 1 && !budget_active &&
           e->update_iterations == 1;
}

int ekf::run_step(EkfEngine *e, const StepInput &in, EkfStepInfo *info)
{
    const bool budget_active = e->budget_K > 0 && e->budget_K < e->N; // measurement budget: with K >= N it cannot bind
    const int kind = e->fixed_map ? UPDATE_FIXED_MAP : UPDATE_COV;
    const int retries0 = e->sweep_retries;
    e->iter_records.clear();
    if (e->update_iterations > 1 && e->fixed_map) { // (the setters refuse the combination: nothing reaches this)
        e->err = "iterated updates are not available while the fixed-map mode is on";
        return EKF_ERR_INVALID_ARG;
    }
    if (!counts_stay_on_device(e, in, budget_active)) {
        StepRun s(e, kind, EKF_OK, retries0);
        s.iterations = e->update_iterations;
        s.iter_tol = e->update_iter_tol;
        s.lean = e->shard_world > 1;
        s.budget = budget_active ? e->budget_K : 0;
        s.normals = in.source == STEP_NCC && e->pn_on;
        s.detect = in.source == STEP_DETECT_KEYPOINTS;
        return step_host_counts(s, in, info);
    }
    int rc;
    {
        StepRun s(e, kind, EKF_OK, retries0);
        if ((rc = step_device_counts(s, in, /*may_find_unread*/ true, info)) != STEP_FOUND_UNREAD_FAILURE) return rc;
    }
    // the previous step's last update failed and its final read-back was skipped: recover (that update again, or skipped and
    // reported by this step), then this step from its start -- once: a flag still set then is this step's to handle
    int status = EKF_OK;
    if ((rc = recover_failed_update(e, &status))) return rc;
    StepRun again(e, kind, status, retries0);
    return step_device_counts(again, in, /*may_find_unread*/ false, info);
}

int ekf_step(EkfEngine *e, const EkfKeypoint *kps, const uint8_t *desc32, int n_kp, EkfStepInfo *info)
{
    if (!e || n_kp < 0 || (n_kp > 0 && (!kps || !desc32))) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int rc = upload_keypoints(e, kps, desc32, n_kp);
    if (rc) return rc;
    e->step_dt = e->frame_interval;
    StepInput in;
    in.d_kps = e->d.kps; in.d_desc = e->d.kdesc; in.n_kp = n_kp;
    return run_step(e, in, info);
}

