// update_route.h -- which kernels an EKF update launches (kernels_update.hip: update_impl), decided in ONE place: plain values in,
// plain values out, no HIP and no side effects (tests/cpp/update_route_check.cpp compiles it with g++).  DESIGN.md 4.3.1 has the table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ekf_engine.h"

namespace ekf {

constexpr int NB = 32;          // Cholesky panel width
constexpr int LD_ALIGN = 128;   // leading dimensions are multiples of this many elements
constexpr int B_SWEEP_MAX = 2048; // rows of S up to which B = inv(L) G is formed inside the sweep's launches

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// grid layout of the persistent sweep (chol_persist.h): block order [chain][B workers][tile workers], layout_cus != 0: block
// layout_cus -- which in-order dispatch would put on the chain workgroup's CU -- is an empty spacer
struct PsLayout {
    int nbk, n_b, n_t, grid, layout_cus;
};

// kind of an update: the state alone (updateOnlyState), state and covariance, or the Schmidt-Kalman update of a fixed map (state
// and covariance strip of the camera alone)
enum { UPDATE_STATE_ONLY = 0, UPDATE_COV = 1, UPDATE_FIXED_MAP = 2 };

// the gather / assembly launch a step enqueued ahead of its second update (launch_early_gather): whether anything was enqueued
// and what it assumed of the route.  The step hands it to that one update in its UpdateCall.
struct EarlyGather {
    bool launched = false;
    bool planes_b = false, apriori = false, persist = false, b_in_sweep = false;
};

// One update, as its caller asks for it (launch_update): everything the launcher is told, nothing it has to find in the engine.
struct UpdateCall {
    const EkfMatch *matches = nullptr; // the match list, on the device
    int M = 0;
    int kind = UPDATE_COV;       // UPDATE_*
    int stage = 0;               // what the consistency record says: 0 ekf_update, 1 a step's first update, 2 its second
    bool lean = false;           // sharded step: each rank gathered the rows of the matches it owns, an exchange completes them
    bool force_launches = false; // the launch-per-panel sweep whatever sweep_mode says (the retry of a timed-out persistent sweep)
    EarlyGather early;           // this update's merged gather / assembly launch may be enqueued already
    const double *pred_uv = nullptr; // the prediction table nu = z - uv is formed from, 2 per feature; null: the engine's d.pred_uv.  A pass
                                     // of the iterated update hands in the predictions shifted by H (x^ - x^i)
};

struct UpdateRouteIn {
    int M = 0, n = 0; // matches (two rows each), state columns
    bool update_cov = true;
    bool fixed_map = false; // Schmidt-Kalman update (ekf_update_fixed_map): the camera's strip of P alone; update_cov is not read
    bool b_fp32 = false; // sizeof(TB) == 4: H P, G and B = inv(L) G in fp32 (the fast fp32 configuration)
    bool p_fp32 = false; // sizeof(T) == 4: P stored in fp32
    bool exact = false;  // EKF_PRECISION_F32_EXACT / _F64_EXACT
    int b_path = EKF_UPDATE_PATH_AUTO, sweep_mode = EKF_SWEEP_AUTO;
    bool force_launches = false; // UpdateCall::force_launches: the retry of a timed-out persistent sweep
    bool ps_backoff = false;     // ps_backoff > 0: recent time-outs (a shared device), engine.h
    int shard_world = 1, shard_rank = 0;
    const int32_t *shard_row_begin = nullptr;
    size_t n_shard_row_begin = 0;
    bool Lq = false, Wq = false, Bstage = false, W = false, Tbuf = false, sweep_ctl = false; // which optional tables exist
    int bstage_rows = 0;
    bool exchange_hook = false;
    bool after_gather = false; // UpdateCall::lean: the gathered rows are completed by an exchange behind the gather
    bool shard_rb_ok = false; // shard_rb has world + 1 entries
    int n_cus = 256;
    int ps_cap[2] = {0, 0}; // resident workgroups of k_chol_persist<false / true> (-1: unusable)
};

struct UpdateRoute {
    const char *refusal = nullptr; // not null: the update is refused with this message (EKF_ERR_INVALID_ARG), nothing else is set
    int M = 0, n = 0, m = 0, m_pad = 0, n_pad = 0;
    bool update_cov = false, b_fp32 = false;
    bool fixed_map = false;    // the 13 x n strip of the camera instead of the downdate (kernels_fixedmap.hip); update_cov is false then.
                               // need_inverse with it: inv(L) is formed but NOT the GEMM -- the camera's gain columns come from W alone
    bool b_in_sweep = false;   // row block k of B = inv(L) G is formed inside the launch of panel k
    bool sharded = false;
    bool shard_cols = false;   // every rank forms its own columns of B
    bool planes_b = false;     // the rows of B come from int8 digit planes inside the sweep (chol_bplanes.h)
    bool apriori = false;      // column scales of B from diag(P)
    bool gemm_own = false;     // sharded, above B_SWEEP_MAX rows: the int8 GEMM over the rank's own column tiles
    bool sym_g = false;        // sharded: G by symmetry and S by columns (k_g_cols) instead of the exchange of the rows of G
    bool persist = false;      // ONE persistent launch for the whole sweep (chol_persist.h)
    bool consumed_backoff = false; // the sweep would have been persistent but for ps_backoff: the caller decrements it
    bool merged_ga = false;    // gather and the assembly of S in one launch
    bool need_inverse = false; // inv(L) is formed explicitly behind the sweep
    bool gemm_planes = false;  // B = inv(L) G on the int8 MFMA, straight into the digit planes of B (kernels_pexact.hip)
    bool merged_tail = false;  // the state update shares a launch with the normalisation of the covariance (k_apply_normalize)
    bool fix = false;          // the fast fp32 configuration's fp64 repair of the diagonal / camera rows is collected by k_dx_partial
    bool fix_diag = false;     // ... and applied by its own tail (k_fix_normalize)
    int lmode = EKF_SWEEP_AUTO; // mode of the launch-per-panel sweep: EKF_SWEEP_PAIRS, _SINGLE or _AUTO
    int cb0 = 0, cb1 = 0;      // this rank forms the 32-column blocks [cb0, cb1) of B in the sweep
    int n_bblocks = 0;         // ... their number, 0 when B is not formed in the sweep
    int c_live0 = 0, n_live = 0; // planes_b: the columns the saturation check of the cut covers
    int n_cus = 0;
    std::vector<int32_t> col_rb; // sharded with planes_b || shard_cols: column boundaries of the ranks' shares of the planes
    PsLayout ps{};
};

// tile workers of a persistent sweep: at least one per 64 tiles; then the grid and its spacer
inline void ps_set_tile_workers(PsLayout &L, int n_t, int n_cus)
{
    const int ntiles = (L.nbk + 1) * (L.nbk + 2) / 2 - 1;
    L.n_t = std::max(n_t, (ntiles + 63) / 64);
    const bool spacer = 1 + L.n_b + L.n_t > n_cus;
    L.grid = 1 + L.n_b + L.n_t + (spacer ? 1 : 0);
    L.layout_cus = spacer ? n_cus : 0;
}

// layout of the persistent sweep of an update of m rows with n_bcols 32-column blocks of B on cap resident workgroups; false: it
// does not fit the device (decided BEFORE the gather / assembly launch, which skips the first block's factorisation for it)
inline bool persist_layout(int cap, int n_cus, bool sweep_ctl, int m, int n_bcols, PsLayout &L)
{
    const int nbk = (m + NB - 1) / NB;
    if (cap < 64 || nbk > B_SWEEP_MAX / NB || !sweep_ctl) return false;
    const int ntiles = (nbk + 1) * (nbk + 2) / 2 - 1;
    // One B worker per 32-column block (at most 3/5 of the slots), the rest tile workers: with one or two tiles each they react to
    // a published inverse within ~3 us, which the chain needs in its first panels (the band of two tiles it applies itself covers
    // the rest).  Measured at N = 1000 (profiles/r05_persist_layout.txt): 134 tile workers beside B workers with CUs of their own
    // 10.4 us per panel, 200 / 322 tile workers sharing the B workers' CUs 9.4 / 9.0.
    L.nbk = nbk;
    L.n_b = std::max(1, std::min(n_bcols, (cap - 2) * 3 / 5));
    ps_set_tile_workers(L, std::min(ntiles, cap - 2 - L.n_b), n_cus);
    return 1 + L.n_b + L.n_t + 1 <= cap;
}

inline UpdateRoute choose_update_route(const UpdateRouteIn &in)
{
    UpdateRoute r;
    // fixed map: fp64 rows of B (or of G) in a one-GPU engine -- the fast fp32 configuration's fp32 rows of B with their fp64 repair
    // of the camera rows, and a row-sharded P, are separate designs
    if (in.fixed_map && in.shard_world > 1) {
        r.refusal = "the fixed-map update is not available on a sharded engine";
        return r;
    }
    if (in.fixed_map && in.b_fp32) {
        r.refusal = "the fixed-map update is not available in EKF_PRECISION_F32";
        return r;
    }
    // the stages in front of the strip are those of a state-only update: nothing of the downdate's machinery (digit planes, a-priori
    // column scales, the fp64 repair, the merged tail) is chosen
    const bool update_cov = in.update_cov && !in.fixed_map;
    const int m = 2 * in.M, m_pad = round_up(m, NB), n_pad = round_up(in.n, LD_ALIGN);
    // B = inv(L) G: up to B_SWEEP_MAX rows, row block k is formed inside the launch of panel k (forward substitution beside the
    // look-ahead factorisation: no explicit inverse, no GEMM launch); above it the per-launch row block becomes longer than the
    // factorisation it hides behind, and the explicit inverse + one big-tile GEMM is the better use of the MFMA pipe.
    // Fixed map: the strip needs the 13 camera columns of the gain, not B.  Below 8192 state columns the rows of B ride behind the
    // latency-bound chain of the persistent sweep and cost nothing (N = 1000: 0.73 ms per frame against 0.98 through the inverse);
    // from there on -- where the sweep leaves the persistent launch and the rows of B are its longest role -- the m^2 n flops of B
    // are the frame, and the inverse with the two m x 13 tables is taken at every size (N = 2000: 2.25 against 3.07 ms)
    const bool fm_no_b = in.fixed_map && n_pad >= 8192;
    const bool b_in_sweep = in.b_path == EKF_UPDATE_PATH_SWEEP || (in.b_path == EKF_UPDATE_PATH_AUTO && m_pad <= B_SWEEP_MAX && !fm_no_b);
    if (in.b_fp32 && b_in_sweep && m_pad > B_SWEEP_MAX) {
        // fp32 forward substitution over more than 64 panels changes the filter's decisions (measured at N = 5000, DESIGN.md
        // section 6): the size switch to inverse + GEMM is an accuracy boundary -- EKF_UPDATE_PATH_SWEEP is refused there
        r.refusal = "EKF_UPDATE_PATH_SWEEP with more than 2048 measurement rows in the fp32 configuration";
        return r;
    }
    r.M = in.M; r.n = in.n; r.m = m; r.m_pad = m_pad; r.n_pad = n_pad;
    r.update_cov = update_cov; r.fixed_map = in.fixed_map; r.b_fp32 = in.b_fp32; r.n_cus = in.n_cus;
    r.b_in_sweep = b_in_sweep; r.need_inverse = !b_in_sweep; r.sharded = in.shard_world > 1;
    const bool exact_cov = in.exact && update_cov;
    r.shard_cols = exact_cov && r.sharded && in.exchange_hook && in.Bstage && m_pad + NB <= in.bstage_rows &&
                   (int)in.n_shard_row_begin == in.shard_world + 1;
    // exact configuration, B in the sweep: its rows are formed from int8 digit planes, in single-panel launches (the planes of L
    // cover B_SWEEP_MAX rows; a sharded rank does not know the diagonal of the rows it does not own)
    r.planes_b = exact_cov && b_in_sweep && m_pad <= B_SWEEP_MAX && in.Lq && (!r.sharded || r.shard_cols);
    // exact configuration above B_SWEEP_MAX rows: the GEMM on the int8 MFMA, straight into the digit planes of B
    const bool gemm_i8 = exact_cov && !b_in_sweep && in.Wq;
    r.gemm_planes = gemm_i8 && (!r.sharded || r.shard_cols);
    r.gemm_own = gemm_i8 && r.shard_cols;
    r.apriori = r.planes_b || r.shard_cols || gemm_i8;
    // (no rows of G travel at any size: above 2048 rows B = inv(L) G is the int8 GEMM over the rank's own column tiles)
    r.sym_g = r.shard_cols && (r.planes_b || r.gemm_own) && in.after_gather && in.shard_rb_ok && in.W && in.Tbuf;
    r.merged_ga = !r.sharded && !r.sym_g && !in.after_gather;
    // covariance updates of the exact and the fp64 configuration: the state update waits behind the downdate and shares a launch
    // with the normalisation of the covariance; the fast fp32 configuration keeps its own tail (k_fix_normalize)
    r.fix_diag = in.p_fp32 && !in.exact; // (the exact downdate needs no fp64 repair of the diagonal / camera rows)
    r.fix = update_cov && r.fix_diag;
    r.merged_tail = update_cov && !r.fix_diag;
    // sharded: this rank forms the column blocks [cb0, cb1) of B -- the blocks whose first column lies in its share of the state
    // rows (rank 0: from column 0) -- and receives the others' digit planes afterwards (the B role divided by the ranks)
    r.cb1 = n_pad / NB;
    if (r.planes_b) r.n_live = in.n;
    if (r.sharded && (r.planes_b || r.shard_cols)) {
        const int W = in.shard_world;
        r.col_rb.assign(W + 1, 0);
        // (G by symmetry: a rank can only form the columns of the rows it holds, so the shares end exactly at the ownership
        // boundaries and the 32-column block that straddles one is formed by both neighbours, each valid in its own columns)
        for (int k = 1; k < W; ++k) r.col_rb[k] = std::min(n_pad, r.sym_g ? in.shard_row_begin[k] : round_up(in.shard_row_begin[k], NB));
        r.col_rb[W] = n_pad;
        if (r.planes_b) {
            r.cb0 = r.col_rb[in.shard_rank] / NB;
            r.cb1 = (r.col_rb[in.shard_rank + 1] + NB - 1) / NB;
            r.c_live0 = r.col_rb[in.shard_rank]; // (this rank's own columns)
            r.n_live = std::min(in.n, (int)r.col_rb[in.shard_rank + 1]);
        }
    }
    r.n_bblocks = b_in_sweep ? r.cb1 - r.cb0 : 0;
    // ONE persistent launch for the whole sweep where it applies: B inside the sweep, at most B_SWEEP_MAX rows, one GPU, fp64
    // arithmetic of B (the fp64 and the exact configurations); otherwise the launch-per-panel sweep
    const int sweep_mode = in.force_launches ? EKF_SWEEP_LAUNCHES : in.sweep_mode;
    r.lmode = (sweep_mode == EKF_SWEEP_PERSISTENT || sweep_mode == EKF_SWEEP_LAUNCHES) ? EKF_SWEEP_AUTO : sweep_mode;
    r.persist = (sweep_mode == EKF_SWEEP_AUTO || sweep_mode == EKF_SWEEP_PERSISTENT) && b_in_sweep && m_pad <= B_SWEEP_MAX && !r.sharded &&
                !in.b_fp32 && in.sweep_ctl;
    // by size: one B worker per block of 32 columns is what the persistent sweep is laid out for; on wider maps (from 8192 state
    // columns on, where the launch-per-panel sweep switches to two panels per launch) its B workers take several blocks each and it
    // loses: N = 2000, 20.4 against 14.0 us per panel (profiles/r05_bench_n2000_f32x_persistent.json)
    if (r.persist && sweep_mode == EKF_SWEEP_AUTO && n_pad >= 8192) r.persist = false;
    if (r.persist && sweep_mode == EKF_SWEEP_AUTO && in.ps_backoff) {
        r.consumed_backoff = true;
        r.persist = false;
    }
    // its grid must fit the device's resident workgroups (a device partition with few CUs: the launch-per-panel sweep instead)
    if (r.persist) r.persist = persist_layout(in.ps_cap[r.planes_b ? 1 : 0], in.n_cus, in.sweep_ctl, m, r.planes_b ? r.cb1 - r.cb0 : n_pad / NB, r.ps);
    return r;
}

// Everything the merged gather / assembly launch takes from the route besides the number of matches: which tables it writes
// (planes_b: row map and row scales of L; b_in_sweep: no transposed inverse), where the column scales come from (apriori) and
// whether it factorises the first diagonal block (not for a persistent sweep).  Two routes that agree here differ, for that
// launch, in the count alone -- a launch that reads the count on the device serves both.
inline bool same_gather_launch(const UpdateRoute &a, const UpdateRoute &b)
{
    return !a.refusal && !b.refusal && a.merged_ga == b.merged_ga && a.planes_b == b.planes_b && a.apriori == b.apriori &&
           a.persist == b.persist && a.b_in_sweep == b.b_in_sweep && a.sharded == b.sharded && a.sym_g == b.sym_g &&
           a.b_fp32 == b.b_fp32 && a.n == b.n && a.n_pad == b.n_pad;
}

// what a call decides of the route's input (the rest is read of the engine: kernels_update.hip route_input)
inline void route_input_of_call(UpdateRouteIn &in, const UpdateCall &c)
{
    in.M = c.M; in.update_cov = c.kind == UPDATE_COV; in.fixed_map = c.kind == UPDATE_FIXED_MAP;
    in.after_gather = c.lean; in.force_launches = c.force_launches;
}

// whether the launch recorded in g is the merged gather / assembly launch of an update on route r: that update skips its own
inline bool early_gather_serves(const EarlyGather &g, const UpdateRoute &r)
{
    return g.launched && r.merged_ga && r.planes_b == g.planes_b && r.apriori == g.apriori &&
           r.persist == g.persist && r.b_in_sweep == g.b_in_sweep;
}

// the retry of an update whose persistent sweep timed out: the same update on the launch-per-panel sweep, every launch its own
// (no lean exchange -- a sharded update's sweep is never persistent -- and no early gather; the same prediction table: the retry
// of a pass of the iterated update repeats THAT pass)
inline UpdateCall retry_of(const UpdateCall &c)
{
    UpdateCall r;
    r.matches = c.matches; r.M = c.M; r.kind = c.kind; r.stage = c.stage;
    r.pred_uv = c.pred_uv;
    r.force_launches = true;
    return r;
}

// One launch of the launch-per-panel sweep, panels from row k0 on; have_pair: an earlier launch of this sweep was a pair launch
// (once the 64 x 64 look-ahead inverse exists the sweep stays in pairs).
// One panel per launch (k_chol_step) while the launch is as long as its look-ahead workgroup; two panels per launch (chol_pair.h)
// once the rows of B are the longest role -- a pair launch reads the finished rows of B once for both panels (the left-looking
// sum re-reads ALL of them every launch: at n = 12013 that traffic, not the factorisation, sets the pace).  Measured: N = 1000
// 9.1 us per panel in single launches against 9.55 in pairs; N = 2000 19.2 against 16.7.  A launch of the pair kernel with
// kbB = 0 eliminates one panel and prepares the first pair (it is also how a sweep in EKF_SWEEP_PAIRS mode starts).
struct PairStep {
    bool pair_launch;
    int kbB;     // rows of the second panel of a pair launch (0: the launch that prepares the first pair)
    bool b_wide; // pair launches of a large fp32 map: 64 columns of B per workgroup (chol_pair.h, b_pair_rows_wide)
};
inline PairStep choose_pair_step(const UpdateRoute &r, int k0, bool have_pair)
{
    // (panels before this one) x n_pad from which a launch is in pairs.  Maps whose rows of B are more 32-column blocks than the
    // chip has CUs (n_pad > 8192; they get the 64-column B role of chol_pair.h) run in pairs from the first launch -- N = 2000:
    // 14.0 us per panel from the start, 14.2 from 120 k, 14.5 from 195 k (single launches: 19.2); smaller maps stay in single
    // launches up to 195 k, i.e. N = 1000 (<= 190 k) always: 9.1 against 9.55 us per panel in pairs.
    const long long PAIR_FROM = r.n_bblocks > r.n_cus ? 0 : 195000;
    // rows of the trailing matrix from which a sweep without the B role starts in pairs: it is bound by streaming the fp64
    // trailing matrix once per launch, 2 x 8 m^2 bytes; pairs stream it once per two panels (N = 5000, m = 3000-4500: 16.6 -> 15.4
    // us per panel)
    constexpr int PAIR_ROWS = 3072;
    const bool want_pairs = r.lmode == EKF_SWEEP_PAIRS ||
                            (r.lmode == EKF_SWEEP_AUTO && (r.b_in_sweep ? (long long)(k0 / NB) * r.n_pad >= PAIR_FROM : r.m - k0 >= PAIR_ROWS));
    // rows of B from digit planes (chol_bplanes.h b_pair_rows_planes): two panels per launch halve the re-reads of the finished
    // planes and the rounds of workgroups of a wide map -- N = 2000: 15.4 -> 13.3 us per panel; N = 1000: 9.9 either way, so AUTO
    // takes pairs from 8192 state columns on (profiles/r04_sweep_pairs_planes.txt)
    const bool want_pairs_pl = r.lmode == EKF_SWEEP_PAIRS || (r.lmode == EKF_SWEEP_AUTO && r.n_pad >= 8192);
    PairStep p;
    p.pair_launch = have_pair || (r.planes_b ? want_pairs_pl : want_pairs);
    p.kbB = have_pair ? std::max(0, std::min(NB, r.m - k0 - NB)) : 0;
    p.b_wide = p.pair_launch && p.kbB > 0 && r.b_fp32 && r.n_bblocks > r.n_cus;
    return p;
}

} // namespace ekf
