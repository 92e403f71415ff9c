// The route of an EKF update (openekfmonoslam_amd/csrc/update_route.h) against a table written out by hand from the rules of
// every decision at both sides of its boundary.  Plain C++, no HIP (tests/test_update_route_host.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../openekfmonoslam_amd/csrc/update_route.h"

using namespace ekf;

static int n_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("line %d: %s\n", __LINE__, #c);                 \
            ++n_failed;                                                 \
        }                                                               \
    } while (0)

enum Cfg { F64, F32, F32X, F64X }; // the four precision configurations: (T, TB, EXACT) of update_impl
static const Cfg ALL[4] = {F64, F32, F32X, F64X};
static bool is_exact(Cfg c) { return c == F32X || c == F64X; }

// one GPU, every optional table present, 256 CUs with two resident workgroups of the persistent sweep each
static UpdateRouteIn make(Cfg c, int M, int n)
{
    UpdateRouteIn in;
    in.M = M; in.n = n;
    in.b_fp32 = c == F32; in.p_fp32 = c == F32 || c == F32X; in.exact = is_exact(c);
    in.Lq = in.Wq = in.Bstage = in.W = in.Tbuf = in.sweep_ctl = true;
    in.n_cus = 256;
    in.ps_cap[0] = in.ps_cap[1] = 512;
    return in;
}

static void auto_path_boundary()
{
    for (Cfg c : ALL) {
        const bool x = is_exact(c);
        UpdateRoute r = choose_update_route(make(c, 1024, 613)); // 2048 rows: the last size with B in the sweep
        CHECK(!r.refusal && r.m == 2048 && r.m_pad == 2048 && r.n_pad == 640);
        CHECK(r.b_in_sweep && !r.need_inverse && !r.gemm_planes && !r.gemm_own);
        CHECK(r.planes_b == x && r.apriori == x);
        CHECK(r.n_bblocks == 20 && r.cb0 == 0 && r.cb1 == 20);
        CHECK(r.persist == (c != F32)); // 64 panels, 20 B workers, 490 tile workers, chain and spacer: exactly the 512 slots
        if (r.persist) CHECK(r.ps.nbk == 64 && r.ps.n_b == 20 && r.ps.n_t == 490 && r.ps.grid == 512 && r.ps.layout_cus == 256);
        CHECK(r.merged_ga && !r.sharded && !r.shard_cols && !r.sym_g && r.col_rb.empty());
        CHECK(r.merged_tail == (c != F32) && r.fix == (c == F32) && r.fix_diag == (c == F32));
        if (x) CHECK(r.n_live == 613 && r.c_live0 == 0);

        r = choose_update_route(make(c, 1025, 613)); // 2050 rows in 2080: inverse + GEMM
        CHECK(!r.refusal && r.m == 2050 && r.m_pad == 2080);
        CHECK(!r.b_in_sweep && r.need_inverse && !r.planes_b && !r.persist && r.n_bblocks == 0);
        CHECK(r.gemm_planes == x && r.apriori == x && !r.gemm_own);

        UpdateRouteIn in = make(c, 1025, 613);
        in.Wq = false; // no digit planes of inv(L)': the plain GEMM
        r = choose_update_route(in);
        CHECK(r.need_inverse && !r.gemm_planes && !r.apriori && !r.planes_b);

        in = make(c, 1024, 613);
        in.Lq = false; // no digit planes of L: fp64 rows of B in the sweep
        r = choose_update_route(in);
        CHECK(r.b_in_sweep && !r.planes_b && !r.apriori);

        for (int M : {1024, 1025}) { // update_cov false: the exact machinery serves the downdate alone
            in = make(c, M, 613);
            in.update_cov = false;
            r = choose_update_route(in);
            CHECK(!r.planes_b && !r.apriori && !r.gemm_planes && !r.merged_tail && !r.fix && !r.update_cov);
            CHECK(r.fix_diag == (c == F32) && r.b_in_sweep == (M == 1024));
        }
    }
}

static void forced_path()
{
    for (Cfg c : ALL) {
        UpdateRouteIn in = make(c, 1025, 613);
        in.b_path = EKF_UPDATE_PATH_SWEEP;
        UpdateRoute r = choose_update_route(in);
        if (c == F32) CHECK(r.refusal && !std::strcmp(r.refusal, "EKF_UPDATE_PATH_SWEEP with more than 2048 measurement rows in the fp32 configuration"));
        else CHECK(!r.refusal && r.b_in_sweep && !r.planes_b && !r.persist && !r.gemm_planes && r.n_bblocks == 20); // (the planes of L end at 2048 rows)
        in.M = 1024;
        r = choose_update_route(in);
        CHECK(!r.refusal && r.b_in_sweep && r.planes_b == is_exact(c));
        in.b_path = EKF_UPDATE_PATH_GEMM;
        r = choose_update_route(in);
        CHECK(!r.refusal && !r.b_in_sweep && r.need_inverse && !r.planes_b && r.gemm_planes == is_exact(c) && !r.persist);
    }
}

static void sweep_modes()
{
    const int32_t rb2[3] = {0, 301, 613};
    // who can take the persistent sweep at all: fp64 arithmetic of B, one GPU, the flag block present
    for (int who = 0; who < 5; ++who) {
        const Cfg c = who == 1 ? F32 : who == 4 ? F32X : F64;
        const bool can = who == 0 || who == 4;
        auto base = [&](int n) {
            UpdateRouteIn in = make(c, 16, n);
            if (who == 2) { in.shard_world = 2; in.shard_row_begin = rb2; in.n_shard_row_begin = 3; }
            if (who == 3) in.sweep_ctl = false;
            return in;
        };
        for (int mode : {EKF_SWEEP_PAIRS, EKF_SWEEP_SINGLE, EKF_SWEEP_AUTO, EKF_SWEEP_PERSISTENT, EKF_SWEEP_LAUNCHES}) {
            UpdateRouteIn in = base(613);
            in.sweep_mode = mode;
            UpdateRoute r = choose_update_route(in);
            const bool pm = mode == EKF_SWEEP_AUTO || mode == EKF_SWEEP_PERSISTENT;
            CHECK(r.persist == (can && pm) && !r.consumed_backoff);
            CHECK(r.lmode == (mode == EKF_SWEEP_PAIRS || mode == EKF_SWEEP_SINGLE ? mode : EKF_SWEEP_AUTO));
            in.force_launches = true; // the retry: launch-per-panel sweep by the size rule whatever the mode
            r = choose_update_route(in);
            CHECK(!r.persist && r.lmode == EKF_SWEEP_AUTO && !r.consumed_backoff);
        }
        UpdateRouteIn in = base(8051); // 8064 state columns: the widest map AUTO sweeps persistently
        UpdateRoute r = choose_update_route(in);
        CHECK(r.n_pad == 8064 && r.persist == can);
        in.ps_backoff = true;
        r = choose_update_route(in);
        CHECK(!r.persist && r.consumed_backoff == can);
        in = base(8077); // 8192
        r = choose_update_route(in);
        CHECK(r.n_pad == 8192 && !r.persist && !r.consumed_backoff);
        in.ps_backoff = true; // nothing to back off from: the count stays
        r = choose_update_route(in);
        CHECK(!r.persist && !r.consumed_backoff);
        in.sweep_mode = EKF_SWEEP_PERSISTENT; // asked for by name: neither the size rule nor the back-off
        r = choose_update_route(in);
        CHECK(r.persist == can && !r.consumed_backoff && r.lmode == EKF_SWEEP_AUTO);
        if (r.persist) CHECK(r.ps.n_b == 256 && r.ps.n_t == 2 && r.ps.grid == 260 && r.ps.layout_cus == 256);
    }
}

static void persistent_layout()
{
    PsLayout L{};
    // a partition of 32 CUs: 64 resident workgroups is the least the sweep takes
    UpdateRouteIn in = make(F64, 16, 613);
    in.n_cus = 32;
    in.ps_cap[0] = 64;
    UpdateRoute r = choose_update_route(in);
    CHECK(r.persist && r.ps.nbk == 1 && r.ps.n_b == 20 && r.ps.n_t == 2 && r.ps.grid == 23 && r.ps.layout_cus == 0);
    in.ps_cap[0] = 63;
    CHECK(!choose_update_route(in).persist);
    in.ps_cap[0] = -1; // the occupancy query failed
    CHECK(!choose_update_route(in).persist);
    in = make(F32X, 16, 613); // the exact configuration asks the capacity of the kernel with planes
    in.ps_cap[0] = 0;
    CHECK(choose_update_route(in).persist);
    in.ps_cap[0] = 512; in.ps_cap[1] = 0;
    CHECK(!choose_update_route(in).persist);
    // ... and a big update on a wide map does not fit it: 37 B workers (3/5 of 62), 2144 tiles need 34 tile workers, 73 > 64
    in = make(F64, 1024, 8051);
    in.n_cus = 32;
    in.ps_cap[0] = 64;
    r = choose_update_route(in);
    CHECK(!r.persist && r.b_in_sweep && r.lmode == EKF_SWEEP_AUTO && !r.consumed_backoff);
    // the same update: 0.4 (cap - 2) slots for tile workers against their floor of 34 -- 85 = 1 + 49 + 34 + 1 fits, 84 (49 + 33 left) not
    in.n_cus = 256;
    in.ps_cap[0] = 85;
    r = choose_update_route(in);
    CHECK(r.persist && r.ps.n_b == 49 && r.ps.n_t == 34 && r.ps.grid == 84 && r.ps.layout_cus == 0);
    in.ps_cap[0] = 84;
    CHECK(!choose_update_route(in).persist);
    // 64 panels of 32 rows at most
    CHECK(persist_layout(512, 256, true, 2048, 20, L) && L.nbk == 64);
    CHECK(!persist_layout(512, 256, true, 2049, 20, L));
    CHECK(!persist_layout(512, 256, false, 2048, 20, L));
    // the spacer: exactly when chain + B workers + tile workers exceed the CUs (one panel: 2 tiles)
    CHECK(persist_layout(512, 256, true, 32, 253, L) && L.n_b == 253 && L.n_t == 2 && L.grid == 256 && L.layout_cus == 0);
    CHECK(persist_layout(512, 256, true, 32, 254, L) && L.n_b == 254 && L.n_t == 2 && L.grid == 258 && L.layout_cus == 256);
    // B workers: at most 3/5 of the slots beside chain and spacer
    CHECK(persist_layout(512, 256, true, 32, 400, L) && L.n_b == 306 && L.n_t == 2);
    r = choose_update_route(make(F64, 32, 8051)); // two panels: 5 tiles, 1 + 252 + 5 = 258 > 256
    CHECK(r.persist && r.ps.nbk == 2 && r.ps.n_b == 252 && r.ps.n_t == 5 && r.ps.grid == 259 && r.ps.layout_cus == 256);
    r = choose_update_route(make(F64, 16, 8051)); // one panel: 255
    CHECK(r.persist && r.ps.grid == 255 && r.ps.layout_cus == 0);
}

static void sharded_exact()
{
    const int n = 8051;
    const int32_t rb[4] = {0, 397, 781, n};
    auto base = [&](int M) {
        UpdateRouteIn in = make(F32X, M, n);
        in.shard_world = 3; in.shard_rank = 1;
        in.shard_row_begin = rb; in.n_shard_row_begin = 4;
        in.exchange_hook = in.after_gather = in.shard_rb_ok = true;
        in.bstage_rows = 64;
        return in;
    };
    UpdateRoute r = choose_update_route(base(16)); // 32 rows + one block = the 64 rows of the exchange image
    CHECK(r.sharded && r.shard_cols && r.planes_b && r.apriori && r.sym_g && !r.merged_ga && !r.persist && !r.gemm_own);
    CHECK((r.col_rb == std::vector<int32_t>{0, 397, 781, 8064})); // G by symmetry: the shares end at the ownership boundaries
    CHECK(r.cb0 == 12 && r.cb1 == 25 && r.n_bblocks == 13 && r.c_live0 == 397 && r.n_live == 781);
    r = choose_update_route(base(17)); // 64 rows + one block > 64
    CHECK(r.sharded && !r.shard_cols && !r.planes_b && !r.apriori && !r.sym_g && r.col_rb.empty() && !r.merged_ga);
    CHECK(r.cb0 == 0 && r.cb1 == 252 && r.n_bblocks == 252 && r.b_in_sweep);
    for (int miss = 0; miss < 4; ++miss) { // every rank forms its own columns only with the hook, the image and all the boundaries
        UpdateRouteIn in = base(16);
        if (miss == 0) in.exchange_hook = false;
        if (miss == 1) in.Bstage = false;
        if (miss == 2) in.n_shard_row_begin = 3;
        if (miss == 3) in.update_cov = false;
        r = choose_update_route(in);
        CHECK(!r.shard_cols && !r.planes_b && !r.sym_g && r.col_rb.empty() && !r.merged_ga);
    }
    for (int miss = 0; miss < 4; ++miss) { // G by the exchange of its rows: the shares are whole 32-column blocks
        UpdateRouteIn in = base(16);
        if (miss == 0) in.after_gather = false;
        if (miss == 1) in.shard_rb_ok = false;
        if (miss == 2) in.W = false;
        if (miss == 3) in.Tbuf = false;
        r = choose_update_route(in);
        CHECK(r.shard_cols && r.planes_b && !r.sym_g && !r.merged_ga);
        CHECK((r.col_rb == std::vector<int32_t>{0, 416, 800, 8064}));
        CHECK(r.cb0 == 13 && r.cb1 == 25 && r.c_live0 == 416 && r.n_live == 800);
    }
    UpdateRouteIn in = base(16); // the last rank's share ends with the live columns
    in.shard_rank = 2;
    r = choose_update_route(in);
    CHECK(r.cb0 == 24 && r.cb1 == 252 && r.c_live0 == 781 && r.n_live == 8051);
    in = base(1025); // above 2048 rows: the int8 GEMM over the rank's own column tiles
    in.bstage_rows = 2112;
    r = choose_update_route(in);
    CHECK(r.shard_cols && !r.planes_b && r.gemm_planes && r.gemm_own && r.sym_g && r.apriori && r.need_inverse);
    CHECK((r.col_rb == std::vector<int32_t>{0, 397, 781, 8064}) && r.cb0 == 0 && r.cb1 == 252 && r.n_bblocks == 0);
    in.bstage_rows = 2111;
    r = choose_update_route(in);
    CHECK(!r.shard_cols && !r.gemm_planes && !r.gemm_own && !r.sym_g && r.apriori && r.col_rb.empty()); // (the scales still come from diag(P))
    in = make(F32X, 16, n); // one GPU with the hook of a sharded step set: gather and assembly stay apart
    in.after_gather = true;
    r = choose_update_route(in);
    CHECK(!r.sharded && !r.merged_ga && r.planes_b && r.persist);
}

static void pair_steps()
{
    auto launches = [](Cfg c, int M, int n, int mode = EKF_SWEEP_LAUNCHES, int path = EKF_UPDATE_PATH_AUTO) {
        UpdateRouteIn in = make(c, M, n);
        in.sweep_mode = mode; in.b_path = path;
        return choose_update_route(in);
    };
    // up to 256 blocks of B (8192 columns): single launches until (panels done) x n_pad reaches 195000 -- 23 x 8192 = 188416, 24 x 8192 = 196608
    UpdateRoute r = launches(F64, 512, 8077);
    CHECK(r.n_bblocks == 256 && !r.persist && !r.planes_b);
    CHECK(!choose_pair_step(r, 0, false).pair_launch && !choose_pair_step(r, 736, false).pair_launch);
    PairStep p = choose_pair_step(r, 768, false);
    CHECK(p.pair_launch && p.kbB == 0 && !p.b_wide); // (the launch that prepares the first pair)
    p = choose_pair_step(r, 64, true); // sticky: the 64 x 64 inverse exists
    CHECK(p.pair_launch && p.kbB == 32 && !p.b_wide);
    r = launches(F32, 512, 8077);
    CHECK(!choose_pair_step(r, 736, false).pair_launch && choose_pair_step(r, 768, false).pair_launch);
    CHECK(!choose_pair_step(r, 800, true).b_wide); // fp32 B, but no more blocks than CUs
    // more blocks than CUs: pairs from the first launch, fp32 B 64 columns wide once a launch has a second panel
    for (Cfg c : {F64, F32}) {
        r = launches(c, 64, 12013);
        CHECK(r.n_bblocks == 376);
        p = choose_pair_step(r, 0, false);
        CHECK(p.pair_launch && p.kbB == 0 && !p.b_wide);
        p = choose_pair_step(r, 32, true);
        CHECK(p.pair_launch && p.kbB == 32 && p.b_wide == (c == F32));
    }
    r = launches(F32, 40, 12013); // 80 rows: the last pair is 32 + 16 rows, then nothing is left for a second panel
    CHECK(choose_pair_step(r, 32, true).kbB == 16 && choose_pair_step(r, 32, true).b_wide);
    p = choose_pair_step(r, 64, true);
    CHECK(p.pair_launch && p.kbB == 0 && !p.b_wide);
    // without the B role: pairs while 3072 rows or more are left
    r = launches(F64, 2000, 613, EKF_SWEEP_LAUNCHES, EKF_UPDATE_PATH_GEMM);
    CHECK(!r.b_in_sweep && r.n_bblocks == 0 && r.m == 4000);
    CHECK(choose_pair_step(r, 0, false).pair_launch && choose_pair_step(r, 928, false).pair_launch && !choose_pair_step(r, 960, false).pair_launch);
    CHECK(choose_pair_step(r, 960, true).pair_launch);
    // rows of B from digit planes: by the width of the map alone
    r = launches(F32X, 512, 8051);
    CHECK(r.planes_b && r.n_pad == 8064 && !choose_pair_step(r, 0, false).pair_launch && !choose_pair_step(r, 800, false).pair_launch);
    CHECK(choose_pair_step(r, 800, true).pair_launch);
    r = launches(F32X, 512, 8077);
    CHECK(r.planes_b && r.n_pad == 8192 && choose_pair_step(r, 0, false).pair_launch);
    // the modes by name
    for (Cfg c : {F64, F32, F32X}) {
        r = launches(c, 512, 613, EKF_SWEEP_PAIRS);
        CHECK(!r.persist && choose_pair_step(r, 0, false).pair_launch);
        r = launches(c, 512, 12013, EKF_SWEEP_SINGLE);
        CHECK(!r.persist && !choose_pair_step(r, 0, false).pair_launch && !choose_pair_step(r, 992, false).pair_launch);
        CHECK(choose_pair_step(r, 0, true).pair_launch);
    }
}

// a route with the four fields the merged gather / assembly launch depends on (same_gather_launch), merged_ga as given
static UpdateRoute route_with(bool planes_b, bool apriori, bool persist, bool b_in_sweep, bool merged_ga)
{
    UpdateRoute r;
    r.planes_b = planes_b; r.apriori = apriori; r.persist = persist; r.b_in_sweep = b_in_sweep; r.merged_ga = merged_ga;
    return r;
}

static void early_gather()
{
    CHECK(!EarlyGather().launched);
    CHECK(!early_gather_serves(EarlyGather(), route_with(false, false, false, false, true))); // nothing was enqueued
    for (int bits = 0; bits < 16; ++bits) { // every value of the four fields
        const bool pb = bits & 1, ap = bits & 2, ps = bits & 4, bs = bits & 8;
        EarlyGather g;
        g.launched = true;
        g.planes_b = pb; g.apriori = ap; g.persist = ps; g.b_in_sweep = bs;
        CHECK(early_gather_serves(g, route_with(pb, ap, ps, bs, true)));
        CHECK(!early_gather_serves(g, route_with(!pb, ap, ps, bs, true))); // any one of the four differs
        CHECK(!early_gather_serves(g, route_with(pb, !ap, ps, bs, true)));
        CHECK(!early_gather_serves(g, route_with(pb, ap, !ps, bs, true)));
        CHECK(!early_gather_serves(g, route_with(pb, ap, ps, !bs, true)));
        CHECK(!early_gather_serves(g, route_with(pb, ap, ps, bs, false))); // gather and assembly apart: the early launch is not this update's
        g.launched = false;
        CHECK(!early_gather_serves(g, route_with(pb, ap, ps, bs, true)));
    }
    // on real routes: what launch_early_gather records of one serves the same route, and not its launch-per-panel retry
    for (Cfg c : ALL) {
        const UpdateRoute r = choose_update_route(make(c, 16, 613));
        EarlyGather g;
        g.launched = true;
        g.planes_b = r.planes_b; g.apriori = r.apriori; g.persist = r.persist; g.b_in_sweep = r.b_in_sweep;
        CHECK(early_gather_serves(g, r));
        UpdateRouteIn in = make(c, 16, 613);
        in.force_launches = true;
        CHECK(early_gather_serves(g, choose_update_route(in)) == !r.persist);
    }
}

static void retries()
{
    static const EkfMatch list[2] = {};
    for (int kind : {UPDATE_STATE_ONLY, UPDATE_COV, UPDATE_FIXED_MAP})
        for (int stage : {0, 1, 2})
            for (int flags = 0; flags < 8; ++flags) {
                UpdateCall c;
                c.matches = list + (stage & 1); c.M = 17 + stage; c.kind = kind; c.stage = stage;
                c.lean = flags & 1; c.force_launches = flags & 2;
                if (flags & 4) {
                    c.early.launched = true;
                    c.early.planes_b = c.early.apriori = c.early.persist = c.early.b_in_sweep = true;
                }
                const UpdateCall t = retry_of(c);
                CHECK(t.matches == c.matches && t.M == c.M && t.kind == kind && t.stage == stage);
                CHECK(t.force_launches && !t.lean);
                CHECK(!t.early.launched && !t.early.planes_b && !t.early.apriori && !t.early.persist && !t.early.b_in_sweep);
                CHECK(!early_gather_serves(t.early, route_with(false, false, false, false, true)));
            }
}

// the route's input as a call fills it: force_launches and lean, both sides of each
static void calls()
{
    for (int mode : {EKF_SWEEP_PAIRS, EKF_SWEEP_SINGLE, EKF_SWEEP_AUTO, EKF_SWEEP_PERSISTENT, EKF_SWEEP_LAUNCHES})
        for (Cfg c : {F64, F32X})
            for (int force = 0; force < 2; ++force) {
                UpdateCall call;
                call.M = 16; call.force_launches = force != 0;
                UpdateRouteIn in = make(c, 1, 613);
                in.sweep_mode = mode;
                route_input_of_call(in, call);
                const UpdateRoute r = choose_update_route(in);
                const bool pm = mode == EKF_SWEEP_AUTO || mode == EKF_SWEEP_PERSISTENT;
                CHECK(r.M == 16 && r.update_cov && !r.fixed_map);
                CHECK(r.persist == (pm && !force));
                // (the retry: the launch-per-panel sweep by the size rule whatever the mode)
                CHECK(r.lmode == (!force && (mode == EKF_SWEEP_PAIRS || mode == EKF_SWEEP_SINGLE) ? mode : EKF_SWEEP_AUTO));
            }
    for (Cfg c : ALL)
        for (int lean = 0; lean < 2; ++lean) {
            UpdateCall call;
            call.M = 16; call.lean = lean != 0;
            UpdateRouteIn in = make(c, 1, 613);
            route_input_of_call(in, call);
            CHECK(choose_update_route(in).merged_ga == !lean); // one GPU: gather and assembly in one launch unless rows are exchanged between them
            CHECK(!choose_update_route(in).sym_g);
        }
    for (int kind : {UPDATE_STATE_ONLY, UPDATE_COV, UPDATE_FIXED_MAP}) {
        UpdateCall call;
        call.M = 16; call.kind = kind;
        UpdateRouteIn in = make(F64, 1, 613);
        route_input_of_call(in, call);
        CHECK(in.update_cov == (kind == UPDATE_COV) && in.fixed_map == (kind == UPDATE_FIXED_MAP));
        const UpdateRoute r = choose_update_route(in);
        CHECK(r.update_cov == (kind == UPDATE_COV) && r.fixed_map == (kind == UPDATE_FIXED_MAP));
    }
    // the retry of a call, end to end: never persistent, never lean
    UpdateCall call;
    call.M = 16; call.lean = true;
    UpdateRouteIn in = make(F64, 1, 613);
    route_input_of_call(in, retry_of(call));
    CHECK(!choose_update_route(in).persist && choose_update_route(in).merged_ga);
}

int main()
{
    auto_path_boundary();
    forced_path();
    sweep_modes();
    persistent_layout();
    sharded_exact();
    pair_steps();
    early_gather();
    retries();
    calls();
    if (n_failed) {
        std::printf("update_route_check: %d checks failed\n", n_failed);
        return 1;
    }
    std::printf("update_route_check: ok\n");
    return 0;
}
