// feature_tables_check.cpp -- the list of per-feature tables, the compaction plan and the row gather of
// openekfmonoslam_amd/csrc/feature_tables.h, on the host alone: built with -fsanitize=address,undefined and without HIP
// (tests/test_feature_tables_host.py).  Exits non-zero on a miss.
#include "../../openekfmonoslam_amd/csrc/feature_tables.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace ekf;

static int g_misses = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_misses <= 20) std::printf("MISS %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static const int DEPTH = EKF_FEATURE_DEPTH, INVERSE = EKF_FEATURE_INVERSE_DEPTH;

// ---------------------------------------------------------------------------------------------- the compaction plan
// The reference works on row ownership, not on sums of dimensions: every old row of P is the camera's (-1) or one feature's; a new
// row is an old row that is not dropped; a kept feature's new position is where its first old row went.
struct Ref {
    std::vector<int> keep, covpos, new2old;
    int n_new;
};
static Ref reference(const std::vector<int> &old_covpos, int n_old, const std::vector<uint8_t> &df, const std::vector<uint8_t> &dr)
{
    Ref r;
    std::vector<int> new_of_old(n_old, -1);
    for (int i = 0; i < n_old; ++i)
        if (!dr[i]) {
            new_of_old[i] = (int)r.new2old.size();
            r.new2old.push_back(i);
        }
    r.n_new = (int)r.new2old.size();
    for (size_t f = 0; f < old_covpos.size(); ++f)
        if (!df[f]) {
            r.keep.push_back((int)f);
            r.covpos.push_back(new_of_old[old_covpos[f]]);
        }
    return r;
}

static std::vector<int> positions(const std::vector<int> &type, int *n)
{
    std::vector<int> c(type.size());
    int pos = 13;
    for (size_t i = 0; i < type.size(); ++i) {
        c[i] = pos;
        pos += type[i] == INVERSE ? 6 : 3;
    }
    *n = pos;
    return c;
}

static void check_plan(const CompactionPlan &p, const Ref &r)
{
    CHECK(p.ok);
    CHECK(p.n_new == r.n_new);
    CHECK(p.new2old == r.new2old);
    CHECK(p.keep == r.keep);
    CHECK(p.covpos == r.covpos);
}

// features `df` removed from the map of these types, rows flagged as ekf_remove_features flags them
static void removal_case(const std::vector<int> &type, const std::vector<uint8_t> &df)
{
    int n = 0;
    const std::vector<int> covpos = positions(type, &n);
    std::vector<uint8_t> dr(n, 0);
    for (size_t f = 0; f < type.size(); ++f)
        if (df[f])
            for (int k = 0; k < feature_dims(type[f]); ++k) dr[covpos[f] + k] = 1;
    check_plan(plan_compaction(type, df, dr), reference(covpos, n, df, dr));
}

static void plan_checks()
{
    for (int N = 0; N <= 7; ++N) // every mix of 3-row and 6-row features, every drop subset
        for (int mix = 0; mix < (1 << N); ++mix)
            for (int sub = 0; sub < (1 << N); ++sub) {
                std::vector<int> type(N);
                std::vector<uint8_t> df(N);
                for (int i = 0; i < N; ++i) {
                    type[i] = (mix >> i & 1) ? INVERSE : DEPTH;
                    df[i] = (uint8_t)(sub >> i & 1);
                }
                removal_case(type, df);
            }
    std::mt19937 rng(20240607u);
    {
        const int N = 200;
        std::vector<int> type(N);
        for (int &t : type) t = (rng() & 1) ? INVERSE : DEPTH;
        for (int s = 0; s < 50; ++s) {
            std::vector<uint8_t> df(N);
            const unsigned density = 1 + rng() % 7; // from sparse to most of the map
            for (uint8_t &d : df) d = (uint8_t)(rng() % 8 < density);
            removal_case(type, df);
        }
    }
    // a single conversion: rows pos + 3 .. pos + 5 of the converted feature dropped, no feature dropped, and the type mirror already
    // says DEPTH -- every position of every mix at 5 features
    for (int mix = 1; mix < (1 << 5); ++mix)
        for (int fi = 0; fi < 5; ++fi) {
            if (!(mix >> fi & 1)) continue;
            std::vector<int> type(5);
            for (int i = 0; i < 5; ++i) type[i] = (mix >> i & 1) ? INVERSE : DEPTH;
            int n = 0;
            const std::vector<int> covpos = positions(type, &n);
            std::vector<uint8_t> df(5, 0), dr(n, 0);
            dr[covpos[fi] + 3] = dr[covpos[fi] + 4] = dr[covpos[fi] + 5] = 1;
            type[fi] = DEPTH;
            const CompactionPlan p = plan_compaction(type, df, dr);
            check_plan(p, reference(covpos, n, df, dr));
            CHECK(p.n_new == n - 3 && (int)p.keep.size() == 5);
            const int next = fi + 1 < 5 ? p.covpos[fi + 1] : p.n_new;
            CHECK(next - p.covpos[fi] == 3); // the converted feature has 3 rows
            CHECK(p.covpos[fi] == covpos[fi]);
        }
    // the row flags disagree with the types
    {
        const std::vector<int> type = {INVERSE, DEPTH, INVERSE};
        int n = 0;
        const std::vector<int> covpos = positions(type, &n);
        std::vector<uint8_t> df = {0, 1, 0}, dr(n, 0);
        CHECK(!plan_compaction(type, df, dr).ok); // a feature dropped, its rows kept
        df = {0, 0, 0};
        dr[covpos[1]] = dr[covpos[1] + 1] = dr[covpos[1] + 2] = 1;
        CHECK(!plan_compaction(type, df, dr).ok); // rows dropped, their feature kept
        df = {1, 0, 0};
        dr.assign(n, 0);
        for (int k = 0; k < 3; ++k) dr[covpos[0] + k] = 1;
        CHECK(!plan_compaction(type, df, dr).ok); // a 6-row feature dropped with 3 rows
        dr.assign(n, 0);
        dr[covpos[2] + 3] = dr[covpos[2] + 4] = dr[covpos[2] + 5] = 1;
        df = {0, 0, 0};
        CHECK(!plan_compaction(type, df, dr).ok); // a conversion's rows dropped, the mirror still INVERSE_DEPTH
    }
}

// -------------------------------------------------------------------------------------------------- the row gather
static void gather_checks()
{
    const size_t widths[] = {1, 4, 48, 363, 5043};
    const int N = 9;
    std::vector<std::vector<int>> keeps(5);
    for (int i = 0; i < N; ++i) keeps[0].push_back(i); // all
    // keeps[1]: none
    keeps[2] = {0};
    keeps[3] = {N - 1};
    for (int i = 1; i < N; i += 2) keeps[4].push_back(i); // alternating
    std::vector<int> alt0;
    for (int i = 0; i < N; i += 2) alt0.push_back(i);
    keeps.push_back(alt0);
    std::mt19937 rng(7u);
    for (size_t rb : widths)
        for (const std::vector<int> &keep : keeps) {
            uint8_t *buf = static_cast<uint8_t *>(std::malloc(N * rb)); // exactly N rows: one byte too far is ASan's
            std::vector<uint8_t> orig(N * rb);
            for (uint8_t &b : orig) b = (uint8_t)rng();
            std::memcpy(buf, orig.data(), N * rb);
            gather_rows(buf, rb, keep);
            std::vector<uint8_t> want(orig); // copy-out reference: the kept rows in order, the rows behind them untouched
            for (size_t w = 0; w < keep.size(); ++w) std::memcpy(&want[w * rb], &orig[(size_t)keep[w] * rb], rb);
            CHECK(std::memcmp(buf, want.data(), N * rb) == 0);
            std::free(buf);
        }
    gather_rows(nullptr, 48, {}); // an empty map
}

// ----------------------------------------------------------------------------------------------------- the list
struct FakeArrays {
    double *feat_pos, *wpose;
    int *feat_type, *feat_covpos;
    uint8_t *feat_desc, *tmpl, *wsrc;
    unsigned *feat_times_predicted, *feat_times_matched;
    struct Rec { char b[48]; } *wnorm;
};
struct FakeEngine {
    FakeArrays d;
    int desc_bytes;
};

static void list_checks()
{
    static double dbl[2];
    static int ints[2];
    static uint8_t bytes[3];
    static unsigned counts[2];
    static FakeArrays::Rec rec;
    for (int desc_bytes : {32, 128}) {
        FakeEngine e;
        e.d = FakeArrays{&dbl[0], &dbl[1], &ints[0], &ints[1], &bytes[0], &bytes[1], &bytes[2], &counts[0], &counts[1], &rec};
        e.desc_bytes = desc_bytes;
        const FeatureTables T = feature_tables(e);
        const void *member[N_FEATURE_TABLES] = {e.d.feat_pos, e.d.feat_type, e.d.feat_covpos, e.d.feat_desc, e.d.feat_times_predicted, e.d.feat_times_matched,
                                                e.d.tmpl, e.d.wsrc, e.d.wpose, e.d.wnorm};
        int seen[mapblob::N_SECTIONS] = {};
        for (int i = 0; i < N_FEATURE_TABLES; ++i) {
            CHECK(T[i].id == i && T[i].rows == member[i] && T[i].row_bytes > 0);
            CHECK(T[i].optional == (i == FT_WSRC || i == FT_WPOSE || i == FT_WNORM));
            if (T[i].section != NO_SECTION) {
                CHECK(T[i].section >= 0 && T[i].section < mapblob::N_SECTIONS);
                ++seen[T[i].section];
            }
        }
        CHECK(T[FT_COVPOS].section == NO_SECTION);
        for (int N : {0, 1, 5}) {
            mapblob::Shape s, s0;
            s.N = N;
            s.n = s0.n = 13 + 6 * 5; // the same n throughout: only what is sized per FEATURE changes with N
            s.desc_bytes = s0.desc_bytes = desc_bytes;
            s.mask = s0.mask = mapblob::MASK_ALL;
            s0.N = 0;
            mapblob::Shape s1 = s0;
            s1.N = 1;
            const mapblob::Layout L = mapblob::layout_of(s), L0 = mapblob::layout_of(s0), L1 = mapblob::layout_of(s1);
            int per_feature = 0;
            for (int id = 0; id < mapblob::N_SECTIONS; ++id) {
                const bool sized_per_feature = L0.bytes[id] != L1.bytes[id];
                per_feature += sized_per_feature;
                CHECK(seen[id] == (sized_per_feature ? 1 : 0)); // each such section exactly once, no other section at all
            }
            CHECK(per_feature == N_FEATURE_TABLES - 1);
            for (const FeatureTable &t : T)
                if (t.section != NO_SECTION) CHECK((uint64_t)t.row_bytes * (uint64_t)N == L.bytes[t.section]);
        }
    }
    CHECK(feature_dims(DEPTH) == 3 && feature_dims(INVERSE) == 6);
}

int main()
{
    plan_checks();
    gather_checks();
    list_checks();
    if (g_misses) {
        std::printf("feature_tables_check: %d misses\n", g_misses);
        return 1;
    }
    std::printf("feature_tables_check: ok\n");
    return 0;
}
