// The route of a fixed-map update (openekfmonoslam_amd/csrc/update_route.h with UpdateRouteIn::fixed_map) at both
// sides of the B_SWEEP_MAX boundary, its refusals, and that the input's default leaves every other route as it was.  Plain C++, no
// HIP (tests/test_fixed_map_route_host.py).
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

static bool same_route(const UpdateRoute &a, const UpdateRoute &b)
{
    const bool same_refusal = (a.refusal == nullptr) == (b.refusal == nullptr) && (!a.refusal || !std::strcmp(a.refusal, b.refusal));
    return same_refusal && a.M == b.M && a.n == b.n && a.m == b.m && a.m_pad == b.m_pad && a.n_pad == b.n_pad && a.update_cov == b.update_cov &&
           a.b_fp32 == b.b_fp32 && a.fixed_map == b.fixed_map && a.b_in_sweep == b.b_in_sweep && a.sharded == b.sharded &&
           a.shard_cols == b.shard_cols && a.planes_b == b.planes_b && a.apriori == b.apriori && a.gemm_own == b.gemm_own &&
           a.sym_g == b.sym_g && a.persist == b.persist && a.consumed_backoff == b.consumed_backoff && a.merged_ga == b.merged_ga &&
           a.need_inverse == b.need_inverse && a.gemm_planes == b.gemm_planes && a.merged_tail == b.merged_tail && a.fix == b.fix &&
           a.fix_diag == b.fix_diag && a.lmode == b.lmode && a.cb0 == b.cb0 && a.cb1 == b.cb1 && a.n_bblocks == b.n_bblocks &&
           a.c_live0 == b.c_live0 && a.n_live == b.n_live && a.n_cus == b.n_cus && a.col_rb == b.col_rb && a.ps.nbk == b.ps.nbk &&
           a.ps.n_b == b.ps.n_b && a.ps.n_t == b.ps.n_t && a.ps.grid == b.ps.grid && a.ps.layout_cus == b.ps.layout_cus;
}

// the stages in front of the strip are those of a state-only update; the route says fixed_map and never update_cov
static void boundary()
{
    for (Cfg c : {F64, F32X, F64X}) {
        UpdateRouteIn in = make(c, 1024, 613); // m_pad = 2048: the rows of B in the sweep, fp64, one persistent launch
        in.fixed_map = true;
        UpdateRoute r = choose_update_route(in);
        CHECK(!r.refusal && r.fixed_map && !r.update_cov && r.m == 2048 && r.m_pad == 2048 && r.n_pad == 640);
        CHECK(r.b_in_sweep && !r.need_inverse && r.n_bblocks == 20 && r.cb0 == 0 && r.cb1 == 20);
        CHECK(!r.planes_b && !r.gemm_planes && !r.gemm_own && !r.apriori);
        CHECK(!r.merged_tail && !r.fix && !r.fix_diag && r.merged_ga && !r.sharded && r.col_rb.empty());
        CHECK(r.persist && r.ps.nbk == 64 && r.ps.n_b == 20 && r.ps.grid == 512);
        in.update_cov = false; // not read with fixed_map
        CHECK(same_route(r, choose_update_route(in)));
        // ... which is the route of the state-only update but for the flag
        UpdateRouteIn so = make(c, 1024, 613);
        so.update_cov = false;
        UpdateRoute rs = choose_update_route(so);
        rs.fixed_map = true;
        CHECK(same_route(r, rs));

        in = make(c, 1025, 613); // m_pad = 2080: inv(L) is formed, and NO digit-plane or fp64 GEMM is chosen by the route
        in.fixed_map = true;
        r = choose_update_route(in);
        CHECK(!r.refusal && r.fixed_map && !r.update_cov && r.m == 2050 && r.m_pad == 2080);
        CHECK(!r.b_in_sweep && r.need_inverse && r.n_bblocks == 0 && !r.persist);
        CHECK(!r.planes_b && !r.gemm_planes && !r.gemm_own && !r.apriori && !r.merged_tail && !r.fix && !r.fix_diag);

        in.b_path = EKF_UPDATE_PATH_SWEEP; // the knob reaches the route: fp64 rows of B in the sweep above the boundary too
        r = choose_update_route(in);
        CHECK(!r.refusal && r.fixed_map && r.b_in_sweep && !r.need_inverse && !r.persist && !r.planes_b && !r.gemm_planes);
        in = make(c, 8, 613);
        in.fixed_map = true;
        in.b_path = EKF_UPDATE_PATH_GEMM; // ... and the inverse below it
        r = choose_update_route(in);
        CHECK(!r.refusal && r.fixed_map && !r.b_in_sweep && r.need_inverse && !r.persist && !r.planes_b && !r.gemm_planes);
        // by size, maps from 8192 state columns on: no rows of B at any number of measurement rows (the inverse and the gain tables)
        for (int M : {8, 1024}) {
            UpdateRouteIn wide = make(c, M, 8051); // n_pad = 8064: still the rows of B in the sweep
            wide.fixed_map = true;
            r = choose_update_route(wide);
            CHECK(r.n_pad == 8064 && r.fixed_map && r.b_in_sweep && !r.need_inverse && r.persist);
            wide = make(c, M, 8077); // n_pad = 8192
            wide.fixed_map = true;
            r = choose_update_route(wide);
            CHECK(r.n_pad == 8192 && r.fixed_map && !r.b_in_sweep && r.need_inverse && !r.persist && r.n_bblocks == 0 && !r.planes_b && !r.gemm_planes);
            wide.b_path = EKF_UPDATE_PATH_SWEEP; // (the knob still forces them)
            r = choose_update_route(wide);
            CHECK(r.fixed_map && r.b_in_sweep && !r.need_inverse);
            wide.fixed_map = false; wide.b_path = EKF_UPDATE_PATH_AUTO; // the full update of the same map is not affected
            r = choose_update_route(wide);
            CHECK(r.b_in_sweep && !r.need_inverse && !r.fixed_map);
        }
        in.b_path = EKF_UPDATE_PATH_AUTO;
        in.sweep_mode = EKF_SWEEP_LAUNCHES;
        r = choose_update_route(in);
        CHECK(r.fixed_map && r.b_in_sweep && !r.persist);
        in.sweep_mode = EKF_SWEEP_AUTO;
        in.force_launches = true; // the retry of a timed-out persistent sweep
        r = choose_update_route(in);
        CHECK(r.fixed_map && r.b_in_sweep && !r.persist);
    }
}

static void refusals()
{
    for (int M : {8, 1024, 1025}) {
        UpdateRouteIn in = make(F32, M, 613); // the fast fp32 configuration
        in.fixed_map = true;
        UpdateRoute r = choose_update_route(in);
        CHECK(r.refusal && std::strstr(r.refusal, "EKF_PRECISION_F32") && !r.fixed_map && r.m == 0);
        const int32_t rb[3] = {0, 301, 613};
        for (Cfg c : {F64, F32, F32X, F64X}) { // sharded
            in = make(c, M, 613);
            in.fixed_map = true;
            in.shard_world = 2; in.shard_rank = 1;
            in.shard_row_begin = rb; in.n_shard_row_begin = 3;
            in.exchange_hook = in.after_gather = in.shard_rb_ok = true;
            in.bstage_rows = 4096;
            r = choose_update_route(in);
            CHECK(r.refusal && std::strstr(r.refusal, "sharded") && !r.fixed_map && r.m == 0);
        }
    }
}

// fixed_map false (the default): a sample of the inputs of update_route_check.cpp, each against itself with the field written
static void default_changes_nothing()
{
    int n_routes = 0;
    for (Cfg c : {F64, F32, F32X, F64X})
        for (int M : {1, 16, 17, 1024, 1025, 2000})
            for (int n : {613, 8051, 8077, 12013})
                for (int cov = 0; cov < 2; ++cov)
                    for (int path : {EKF_UPDATE_PATH_AUTO, EKF_UPDATE_PATH_SWEEP, EKF_UPDATE_PATH_GEMM})
                        for (int mode : {EKF_SWEEP_PAIRS, EKF_SWEEP_SINGLE, EKF_SWEEP_AUTO, EKF_SWEEP_PERSISTENT, EKF_SWEEP_LAUNCHES}) {
                            UpdateRouteIn in = make(c, M, n);
                            in.update_cov = cov != 0; in.b_path = path; in.sweep_mode = mode;
                            CHECK(!in.fixed_map); // the default
                            const UpdateRoute a = choose_update_route(in);
                            CHECK(!a.fixed_map && (a.refusal || a.update_cov == in.update_cov));
                            in.fixed_map = false;
                            CHECK(same_route(a, choose_update_route(in)));
                            ++n_routes;
                        }
    CHECK(n_routes == 4 * 6 * 4 * 2 * 3 * 5);
    // rows of the existing table, restated: the default route still chooses what it chose
    UpdateRoute r = choose_update_route(make(F32X, 1024, 613));
    CHECK(r.planes_b && r.apriori && r.merged_tail && r.update_cov && r.persist && !r.fixed_map);
    r = choose_update_route(make(F64X, 1025, 613));
    CHECK(r.gemm_planes && r.apriori && r.need_inverse && r.update_cov && !r.fixed_map);
    r = choose_update_route(make(F32, 1024, 613));
    CHECK(r.fix && r.fix_diag && !r.merged_tail && !r.persist && !r.fixed_map);
    r = choose_update_route(make(F64, 1024, 613));
    CHECK(r.merged_tail && !r.planes_b && r.persist && r.ps.n_t == 490 && !r.fixed_map);
    const int32_t rb[4] = {0, 397, 781, 8051};
    UpdateRouteIn in = make(F32X, 16, 8051);
    in.shard_world = 3; in.shard_rank = 1;
    in.shard_row_begin = rb; in.n_shard_row_begin = 4;
    in.exchange_hook = in.after_gather = in.shard_rb_ok = true;
    in.bstage_rows = 64;
    r = choose_update_route(in);
    CHECK(!r.refusal && r.sharded && r.shard_cols && r.planes_b && r.sym_g && r.cb0 == 12 && r.cb1 == 25 && !r.fixed_map);
}

int main()
{
    boundary();
    refusals();
    default_changes_nothing();
    if (n_failed) {
        std::printf("fixed_map_route_check: %d checks failed\n", n_failed);
        return 1;
    }
    std::printf("fixed_map_route_check: ok\n");
    return 0;
}
