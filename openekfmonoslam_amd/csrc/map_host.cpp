// map_host.cpp -- the map's host side behind the C ABI (see include/ekf_engine.h): state transfer, the map blob, the map readers and
// map management.  Whatever one of them does to a feature's rows it does as a loop over the list of per-feature
// tables in feature_tables.h; the numbers come from the kernels in kernels_map.hip and kernels_mapblob.hip.
#include "engine_host.h"

#include <algorithm>
#include <cstring>

using namespace ekf;

static_assert(sizeof(int) == sizeof(int32_t), "the type and covpos mirrors (std::vector<int>) are rows of 4-byte tables");

// `bytes` bytes of a device table from the host, or zeros (src == nullptr): on the engine's stream, or with the synchronous calls
static hipError_t fill_rows(EkfEngine *e, void *dst, const void *src, size_t bytes, bool async)
{
    if (async) return src ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream) : hipMemsetAsync(dst, 0, bytes, e->stream);
    return src ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : hipMemset(dst, 0, bytes);
}

// The per-feature part of a map replacement by N features, each table by its policy (feature_tables.h).  given[id]: the N rows the
// replacement brings for a table, or null.  ekf_set_state: synchronous calls, and a table it brings nothing for keeps its policy's
// "leave"; from_blob (ekf_load_map): on the stream, and such a table is treated as its on_absent says.
static int replace_feature_tables(EkfEngine *e, int N, const void *const given[N_FEATURE_TABLES], bool from_blob)
{
    const FeatureTables tables = feature_tables(*e);
    for (const FeatureTable &t : tables) // (the fills first, then the copies: on a stream the two kinds do not alternate)
        if (t.rows && t.on_replace == REPLACE_ZERO_ALL) HIPCHK(fill_rows(e, t.rows, nullptr, (size_t)e->cap * t.row_bytes, from_blob));
    for (const FeatureTable &t : tables) {
        const bool zeros = t.on_replace == REPLACE_ROWS || (from_blob && t.on_absent == ABSENT_ZERO_ROWS);
        if (t.rows && N > 0 && (given[t.id] || zeros)) HIPCHK(fill_rows(e, t.rows, given[t.id], (size_t)N * t.row_bytes, from_blob));
    }
    return EKF_OK;
}

int ekf::ensure_warp_tables(EkfEngine *e)
{
    if (e->d.wpose) return EKF_OK;
    const size_t cap = (size_t)e->cap;
    auto g = e->bufs.group();
    g.alloc(&e->d.wsrc, cap * mapblob::WARP_SOURCE_BYTES);
    g.alloc(&e->d.wtmpl, cap * mapblob::TEMPLATE_BYTES);
    g.alloc(&e->d.wpose, cap * WPOSE_DOUBLES); // zeroed: no feature has a source patch yet
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "template warp tables");
    return EKF_OK;
}

int ekf::ensure_patch_normal_tables(EkfEngine *e)
{
    if (e->d.wnorm) return EKF_OK;
    auto g = e->bufs.group();
    g.alloc(&e->d.wnorm, (size_t)e->cap); // zeroed: no feature has an estimate yet
    g.alloc(&e->d.pn_list, (size_t)e->cap);
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "patch normal tables");
    return EKF_OK;
}

static void refresh_row_map(EkfEngine *e);

// The map was replaced (ekf_set_state, ekf_load_map); e->N, e->n and the layout mirrors hold the new one.  Whatever was predicted,
// gated, snapshotted or ranked describes the map that was, and d.wtmpl belongs to the map the last match saw.  Left alone: p_exact_sym
// and the retry record e->last_update, which the two callers set differently (see there), and the counts of the last match or
// estimator run (warp_counts, pn_counts, ...), which describe a call and not the map.
static void map_replaced(EkfEngine *e)
{
    e->n_pred = 0;
    e->n_gates = 0;
    e->n_step_preds = 0;
    e->bud_recs_n = e->bud_predicted = e->bud_selected = 0; // measurement budget: the records belong to the map they were made on
    e->last_match_warped = false;
    e->iter_lin_sel = -1; // iterated update: the linearisation point was one of the map that was (ekf_get_linearisation_point)
    refresh_row_map(e);
}

// The map's layout changed under the same filter (ekf_add_features, compact_map, the batch conversion): no prediction stands, and
// d.wtmpl has no rows for new features and is not compacted (until the next match ekf_get_match_templates shows the stored
// templates).  Left alone, unlike map_replaced: n_gates, n_step_preds and the three budget counts, so the last step's gates,
// prediction snapshot and ranks stay readable with the feature indices of the map that step saw.  That is today's behaviour; nothing
// records whether the difference is meant, and it is kept as it is.
static void map_layout_changed(EkfEngine *e)
{
    e->n_pred = 0;
    e->last_match_warped = false;
    e->iter_lin_sel = -1; // iterated update: the linearisation point has the features and the order of the layout that was
    refresh_row_map(e);
}

// feature partition of a sharded engine (same arithmetic as ekf_shard_rows) and the row map that follows from it
static void refresh_row_map(EkfEngine *e)
{
    const int W = e->shard_world, N = e->N;
    e->match_gates_valid = false; // set_state, reset and map management end here: the matcher's gate table describes the map before them
    if (W == 1) {
        e->rm = RowMap{13, e->n, 13};
        e->shard_feat_begin.assign(2, 0);
        e->shard_feat_begin[1] = N;
        e->shard_row_begin = {0, e->n};
        return;
    }
    const int per = N / W, extra = N % W;
    for (int r = 0; r <= W; ++r) e->shard_feat_begin[r] = r * per + (r < extra ? r : extra);
    const int f0 = e->shard_feat_begin[e->shard_rank], f1 = e->shard_feat_begin[e->shard_rank + 1];
    auto row_of = [&](int f) { return f < N ? e->h_covpos[f] : e->n; };
    e->rm = RowMap{row_of(f0), row_of(f1), SHARD_BASE};
    e->shard_row_begin.assign(W + 1, 0);
    for (int r = 1; r <= W; ++r) e->shard_row_begin[r] = row_of(e->shard_feat_begin[r]);
    (void)hipMemcpyAsync(e->d.shard_feat, e->shard_feat_begin.data(), (size_t)(W + 1) * sizeof(int), hipMemcpyHostToDevice, e->stream);
    (void)hipStreamSynchronize(e->stream); // the host vector may be reassigned before the copy would otherwise run
}

int ekf_get_map_features(EkfEngine *e, uint8_t *desc32, uint32_t *times_predicted, uint32_t *times_matched)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t N = (size_t)e->N;
    if (N == 0) return EKF_OK;
    if (desc32) HIPCHK(hipMemcpy(desc32, e->d.feat_desc, N * e->desc_bytes, hipMemcpyDeviceToHost));
    if (times_predicted) HIPCHK(hipMemcpy(times_predicted, e->d.feat_times_predicted, N * 4, hipMemcpyDeviceToHost));
    if (times_matched) HIPCHK(hipMemcpy(times_matched, e->d.feat_times_matched, N * 4, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// ------------------------------------------------------------------------------------------- state transfer
int ekf_set_state(EkfEngine *e, const double x13[13], int n_features, const double *feature_pos,
                  const int32_t *feature_type, const uint8_t *desc32, const double *P)
{
    if (!e || !x13 || n_features < 0 || (n_features > 0 && !feature_pos)) return EKF_ERR_INVALID_ARG;
    if (n_features > e->cap) return EKF_ERR_CAPACITY;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<int> type(n_features), covpos(n_features);
    int pos = 13;
    for (int i = 0; i < n_features; ++i) {
        const int t = feature_type ? feature_type[i] : EKF_FEATURE_INVERSE_DEPTH;
        if (t != EKF_FEATURE_DEPTH && t != EKF_FEATURE_INVERSE_DEPTH) return EKF_ERR_INVALID_ARG;
        type[i] = t;
        covpos[i] = pos;
        pos += (t == EKF_FEATURE_INVERSE_DEPTH) ? 6 : 3;
    }
    const int n = pos;
    double st[ST_R + 9];
    std::memcpy(st, x13, 13 * sizeof(double));
    {
        const double r = x13[3], x = x13[4], y = x13[5], z = x13[6];
        double *M = st + ST_R;
        M[0] = r * r + x * x - y * y - z * z; M[1] = 2 * (x * y - r * z); M[2] = 2 * (z * x + r * y);
        M[3] = 2 * (x * y + r * z); M[4] = r * r - x * x + y * y - z * z; M[5] = 2 * (y * z - r * x);
        M[6] = 2 * (z * x - r * y); M[7] = 2 * (y * z + r * x); M[8] = r * r - x * x - y * y + z * z;
    }
    HIPCHK(hipMemcpy(e->d.state, st, sizeof(st), hipMemcpyHostToDevice));
    // the per-feature tables: counters, capture poses and normals start from zero over the whole capacity, and the templates and
    // source patches of the map that was stay where they are (feature_tables.h)
    const void *given[N_FEATURE_TABLES] = {};
    given[FT_POS] = feature_pos;
    given[FT_TYPE] = type.data();
    given[FT_COVPOS] = covpos.data();
    given[FT_DESC] = desc32;
    if (const int rc = replace_feature_tables(e, n_features, given, false)) return rc;
    e->N = n_features;
    e->n = n;
    e->h_type = type;
    e->h_covpos = covpos;
    map_replaced(e);
    if (e->shard_world > 1 && SHARD_BASE + (e->rm.r1 - e->rm.r0) > e->p_rows_cap) return EKF_ERR_CAPACITY;
    if (P) {
        const size_t w = e->f32 ? 4 : 8;
        HIPCHK(hipMemset(e->d.P, 0, (size_t)e->p_rows_cap * e->ldP * w));
        const bool sharded = e->shard_world > 1;
        // row blocks to upload: (first global row, count, first local row)
        const int blocks[2][3] = {{0, sharded ? 13 : n, 0}, {e->rm.r0, sharded ? e->rm.r1 - e->rm.r0 : 0, e->rm.base}};
        std::vector<float> tmp;
        std::vector<double> sym;
        for (const auto &b : blocks) {
            const int g0 = b[0], cnt = b[1], l0 = b[2];
            if (cnt <= 0) continue;
            const double *src = P + (size_t)g0 * n;
            if (sharded) { // no cross-rank averaging pass exists: symmetrise on the way in, in T arithmetic
                sym.resize((size_t)cnt * n);
                for (int i = 0; i < cnt; ++i)
                    for (int j = 0; j < n; ++j) {
                        const double a = P[(size_t)(g0 + i) * n + j], c = P[(size_t)j * n + g0 + i];
                        sym[(size_t)i * n + j] = e->f32 ? (double)(0.5f * (float)a + 0.5f * (float)c) : 0.5 * a + 0.5 * c;
                    }
                src = sym.data();
            }
            uint8_t *dst = (uint8_t *)e->d.P + (size_t)l0 * e->ldP * w;
            if (e->f32) {
                tmp.resize((size_t)cnt * n);
                for (size_t i = 0; i < (size_t)cnt * n; ++i) tmp[i] = (float)src[i];
                HIPCHK(hipMemcpy2D(dst, (size_t)e->ldP * 4, tmp.data(), (size_t)n * 4, (size_t)n * 4, cnt, hipMemcpyHostToDevice));
            } else {
                HIPCHK(hipMemcpy2D(dst, (size_t)e->ldP * 8, src, (size_t)n * 8, (size_t)n * 8, cnt, hipMemcpyHostToDevice));
            }
        }
        e->p_exact_sym = sharded;
    }
    HIPCHK(hipMemset(e->d.pred_vis, 0, (size_t)e->cap * sizeof(int)));
    HIPCHK(hipMemset(e->d.pred_vis_full, 0, (size_t)e->cap * sizeof(int)));
    // an update still unread (ekf_set_async_errors) belongs to the map that was: if it is found timed out it is reported, not run
    // again on this one.  (ekf_load_map resets the whole record instead; the difference is kept as it is.)
    e->last_update.persist = false;
    e->last_update.sym = e->p_exact_sym;
    return EKF_OK;
}

int ekf_get_state(EkfEngine *e, double x13[13], double *feature_pos, double *P)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int pending = take_pending_error(e); // the state is still copied out: the caller sees what the failed update left
    if (x13) HIPCHK(hipMemcpy(x13, e->d.state, 13 * sizeof(double), hipMemcpyDeviceToHost));
    if (feature_pos && e->N > 0)
        HIPCHK(hipMemcpy(feature_pos, e->d.feat_pos, (size_t)6 * e->N * sizeof(double), hipMemcpyDeviceToHost));
    if (P) {
        const int n = e->n;
        const size_t w = e->f32 ? 4 : 8;
        const bool sharded = e->shard_world > 1;
        const int blocks[2][3] = {{0, sharded ? 13 : n, 0}, {e->rm.r0, sharded ? e->rm.r1 - e->rm.r0 : 0, e->rm.base}};
        std::vector<float> tmp;
        for (const auto &b : blocks) { // a sharded engine fills the rows it holds and leaves the others untouched
            const int g0 = b[0], cnt = b[1], l0 = b[2];
            if (cnt <= 0) continue;
            const uint8_t *src = (const uint8_t *)e->d.P + (size_t)l0 * e->ldP * w;
            double *dst = P + (size_t)g0 * n;
            if (e->f32) {
                tmp.resize((size_t)cnt * n);
                HIPCHK(hipMemcpy2D(tmp.data(), (size_t)n * 4, src, (size_t)e->ldP * 4, (size_t)n * 4, cnt, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < (size_t)cnt * n; ++i) dst[i] = (double)tmp[i];
            } else {
                HIPCHK(hipMemcpy2D(dst, (size_t)n * 8, src, (size_t)e->ldP * 8, (size_t)n * 8, cnt, hipMemcpyDeviceToHost));
            }
        }
    }
    return pending;
}

// ------------------------------------------------------------------------------------------------ map blob
// (the format and the host-side validation: map_blob.h, the P section: kernels_mapblob.hip)
static int second_P(EkfEngine *e);

static int map_blob_refusal(EkfEngine *e, const char *who)
{
    if (e->shard_world > 1) {
        e->err = std::string(who) + ": not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    return EKF_OK;
}

static int map_blob_ctl(EkfEngine *e)
{
    if (e->d.mb_ctl) return EKF_OK;
    const hipError_t st = e->bufs.alloc(&e->d.mb_ctl, 1);
    if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc map blob control record");
    return EKF_OK;
}

// The shape of the blob the engine would write now.  The packed triangle needs a bitwise symmetric P: where the engine does not
// know it symmetric already (p_exact_sym: every covariance update leaves it so), a read-only pass on the device finds out -- a
// predicted covariance is, an uploaded one or the map block a fixed-map update leaves alone need not be.
static int map_blob_shape(EkfEngine *e, int sections, mapblob::Shape *out)
{
    mapblob::Shape s;
    s.N = e->N;
    s.n = e->n;
    s.p_elem_bytes = e->f32 ? 4 : 8;
    bool sym = e->p_exact_sym;
    if (!sym) {
        if (const int rc = map_blob_ctl(e)) return rc;
        launch_map_asym(e, e->d.mb_ctl);
        HIPCHK(hipGetLastError());
        MapBlobCtl ctl;
        HIPCHK(hipMemcpyAsync(&ctl, e->d.mb_ctl, sizeof(ctl), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        sym = ctl.asym == 0;
    }
    s.p_layout = sym ? mapblob::P_TRIANGLE : mapblob::P_FULL;
    s.desc_bytes = e->desc_bytes;
    s.desc_flags = e->cfg.flags;
    s.mask = (uint32_t)sections & mapblob::MASK_TEMPLATES;
    if ((sections & EKF_MAP_WARP_SOURCES) && e->d.wsrc && e->d.wpose) s.mask |= mapblob::MASK_WARP_SOURCES;
    if ((sections & EKF_MAP_PATCH_NORMALS) && e->d.wnorm) s.mask |= mapblob::MASK_PATCH_NORMALS;
    *out = s;
    return EKF_OK;
}

int ekf_map_blob_bytes(EkfEngine *e, int sections, size_t *bytes)
{
    if (!e || !bytes || (sections & ~EKF_MAP_ALL)) return EKF_ERR_INVALID_ARG;
    if (const int rc = map_blob_refusal(e, "ekf_map_blob_bytes")) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    mapblob::Shape s;
    if (const int rc = map_blob_shape(e, sections, &s)) return rc;
    *bytes = (size_t)mapblob::layout_of(s).total;
    return EKF_OK;
}

int ekf_save_map(EkfEngine *e, int sections, void *blob_, size_t capacity, size_t *bytes)
{
    if (!e || !bytes || (sections & ~EKF_MAP_ALL)) return EKF_ERR_INVALID_ARG;
    if (const int rc = map_blob_refusal(e, "ekf_save_map")) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e); // as ekf_update_external: the failed update it reports is not this call's
    if (rc) return rc;
    mapblob::Shape s;
    if ((rc = map_blob_shape(e, sections, &s))) return rc;
    const mapblob::Layout L = mapblob::layout_of(s);
    *bytes = (size_t)L.total;
    if (!blob_ || capacity < L.total) {
        e->err = "ekf_save_map: the buffer holds " + std::to_string(capacity) + " bytes, the blob needs " + std::to_string(L.total);
        return blob_ ? EKF_ERR_CAPACITY : EKF_ERR_INVALID_ARG;
    }
    if ((rc = second_P(e))) return rc; // the staging buffer of the P section
    if ((rc = map_blob_ctl(e))) return rc;
    uint8_t *blob = (uint8_t *)blob_;
    mapblob::zero_gaps(blob, L);
    launch_map_pack(e, s.p_layout, e->d.P2, e->d.mb_ctl);
    HIPCHK(hipGetLastError());
    MapBlobCtl ctl;
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(&ctl, e->d.mb_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(blob + L.offset[mapblob::SEC_P], e->d.P2, (size_t)L.bytes[mapblob::SEC_P], hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(blob + L.offset[mapblob::SEC_X13], e->d.state, (size_t)L.bytes[mapblob::SEC_X13], hipMemcpyDeviceToHost, st));
    // the per-feature tables are contiguous in map order: plain copies
    for (const FeatureTable &t : feature_tables(*e))
        if (t.rows && t.section != NO_SECTION && L.present[t.section] && L.bytes[t.section] > 0)
            HIPCHK(hipMemcpyAsync(blob + L.offset[t.section], t.rows, (size_t)L.bytes[t.section], hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(blob + L.offset[mapblob::SEC_CAMERA], &e->cfg.cam, sizeof(EkfCamera));
    uint64_t sums[mapblob::N_SECTIONS];
    for (int id = 0; id < mapblob::N_SECTIONS; ++id)
        sums[id] = !L.present[id] ? 0 : (id == mapblob::SEC_P ? (uint64_t)ctl.sum : mapblob::checksum(blob + L.offset[id], L.bytes[id]));
    mapblob::write_header(blob, s, L, sums);
    return EKF_OK;
}

int ekf_map_blob_info(const void *blob, size_t bytes, EkfMapBlobInfo *info)
{
    mapblob::Parsed p;
    if (!mapblob::parse(blob, bytes, true, &p, nullptr)) return EKF_ERR_INVALID_ARG;
    if (info) *info = mapblob::info_of(p);
    return EKF_OK;
}

int ekf_load_map(EkfEngine *e, const void *blob_, size_t bytes, EkfMapBlobInfo *info)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (const int rc = map_blob_refusal(e, "ekf_load_map")) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e); // as ekf_save_map
    if (rc) return rc;
    // 1. everything the host can check
    mapblob::Parsed p;
    if (!mapblob::parse(blob_, bytes, false, &p, &e->err)) return EKF_ERR_INVALID_ARG;
    const uint8_t *blob = (const uint8_t *)blob_;
    const mapblob::Shape &s = p.shape;
    const mapblob::Layout &L = p.layout;
    if (s.desc_bytes != e->desc_bytes || s.desc_flags != e->cfg.flags) {
        e->err = "map blob: desc_bytes / desc_flags " + std::to_string(s.desc_bytes) + " / " + std::to_string(s.desc_flags) +
                 " are not the engine's descriptor format " + std::to_string(e->desc_bytes) + " / " + std::to_string(e->cfg.flags);
        return EKF_ERR_INVALID_ARG;
    }
    if (s.N > e->cap) {
        e->err = "map blob: N = " + std::to_string(s.N) + " exceeds the engine's max_features = " + std::to_string(e->cap);
        return EKF_ERR_CAPACITY;
    }
    const int N = s.N, n = s.n;
    // 2. tables the blob needs and the engine lacks (zeroed; the modes stay as they are).  The normals are read beside the capture poses
    const bool has_warp = L.present[mapblob::SEC_WARP_SOURCES], has_norm = L.present[mapblob::SEC_PATCH_NORMALS];
    if ((has_warp || has_norm) && (rc = ensure_warp_tables(e))) return rc;
    if (has_norm && (rc = ensure_patch_normal_tables(e))) return rc;
    if ((rc = map_blob_ctl(e))) return rc;
    // 3. P goes up into a staging buffer and is checked there: d.P2 where the section fits (always when the element sizes agree),
    // else a buffer of this call's
    const size_t p_bytes = (size_t)L.bytes[mapblob::SEC_P];
    const size_t p2_bytes = (size_t)round_up(e->ncap, LD_ALIGN) * e->ldP * (e->f32 ? 4 : 8);
    void *staging = nullptr, *own = nullptr;
    if (p_bytes <= p2_bytes) {
        if ((rc = second_P(e))) return rc;
        staging = e->d.P2;
    } else {
        const hipError_t st = hipMalloc(&own, p_bytes);
        if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc map blob staging");
        staging = own;
    }
    hipStream_t st = e->stream;
    MapBlobCtl ctl;
    auto staged = [&]() -> int {
        HIPCHK(hipMemcpyAsync(staging, blob + L.offset[mapblob::SEC_P], p_bytes, hipMemcpyHostToDevice, st));
        launch_map_check(e, staging, n, s.p_elem_bytes, s.p_layout, e->d.mb_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&ctl, e->d.mb_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if ((uint64_t)ctl.sum != p.sums[mapblob::SEC_P]) {
            e->err = "map blob: section P: checksum does not match its bytes";
            return EKF_ERR_INVALID_ARG;
        }
        if (ctl.non_finite || ctl.bad_diag) {
            e->err = "map blob: section P: " + std::to_string(ctl.non_finite) + " entries are not finite, " + std::to_string(ctl.bad_diag) +
                     " diagonal entries are not > 0";
            return EKF_ERR_NON_FINITE;
        }
        // 4. only now is anything written
        double stt[ST_R + 9];
        std::memcpy(stt, blob + L.offset[mapblob::SEC_X13], 13 * sizeof(double));
        quat_to_rot(stt + 3, stt + ST_R);
        HIPCHK(hipMemcpyAsync(e->d.state, stt, sizeof(stt), hipMemcpyHostToDevice, st));
        std::vector<int> type(N), covpos(N);
        if (N > 0) std::memcpy(type.data(), blob + L.offset[mapblob::SEC_FEAT_TYPE], (size_t)N * 4);
        for (int i = 0, pos = 13; i < N; ++i) {
            covpos[i] = pos;
            pos += type[i] == EKF_FEATURE_INVERSE_DEPTH ? 6 : 3;
        }
        const size_t cap = (size_t)e->cap;
        // the per-feature tables: whole tables as ekf_set_state leaves them, then the blob's rows for the features 0 .. N - 1, and
        // zeros in those rows of a table whose section the blob lacks (feature_tables.h)
        const void *given[N_FEATURE_TABLES] = {};
        given[FT_COVPOS] = covpos.data();
        for (const FeatureTable &t : feature_tables(*e))
            if (t.section != NO_SECTION && L.present[t.section]) given[t.id] = blob + L.offset[t.section];
        if (const int rc_tables = replace_feature_tables(e, N, given, true)) return rc_tables;
        HIPCHK(hipMemsetAsync(e->d.P, 0, (size_t)e->p_rows_cap * e->ldP * (e->f32 ? 4 : 8), st));
        launch_map_unpack(e, staging, n, s.p_elem_bytes, s.p_layout);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(e->d.pred_vis, 0, cap * sizeof(int), st));
        HIPCHK(hipMemsetAsync(e->d.pred_vis_full, 0, cap * sizeof(int), st));
        HIPCHK(hipStreamSynchronize(st)); // (the copies above read this call's vectors and the caller's blob)
        e->N = N;
        e->n = n;
        e->h_type = type;
        e->h_covpos = covpos;
        map_replaced(e);
        e->p_exact_sym = s.p_layout == mapblob::P_TRIANGLE;
        // no update of the map that was is run again on this one (the whole record, where ekf_set_state clears `persist` alone)
        e->last_update = decltype(e->last_update)();
        e->last_update.sym = e->p_exact_sym;
        return EKF_OK;
    };
    rc = staged();
    if (rc != EKF_OK && rc != EKF_ERR_HIP && !own) (void)hipMemsetAsync(staging, 0, p_bytes, st); // a refused section does not stay in d.P2
    (void)hipStreamSynchronize(st);
    if (own) (void)hipFree(own);
    if (rc == EKF_OK && info) *info = mapblob::info_of(p);
    return rc;
}


// ------------------------------------------------------------------------------------------ map management
int ekf_reset(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    // initState + initCovariance, EKF/CommonFunctions.cpp:39-80
    double x[13] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, EKF_EPSILON, EKF_EPSILON, EKF_EPSILON};
    double P[169];
    std::memset(P, 0, sizeof(P));
    for (int i = 0; i < 7; ++i) P[i * 13 + i] = EKF_EPSILON;
    for (int i = 0; i < 3; ++i) {
        P[(i + 7) * 13 + i + 7] = e->cfg.par.initLinearAccelSD * e->cfg.par.initLinearAccelSD;
        P[(i + 10) * 13 + i + 10] = e->cfg.par.initAngularAccelSD * e->cfg.par.initAngularAccelSD;
    }
    return ekf_set_state(e, x, 0, nullptr, nullptr, nullptr, P);
}

int ekf_get_camera_covariance(EkfEngine *e, double P13[169])
{
    if (!e || !P13) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->f32) {
        float tmp[169];
        HIPCHK(hipMemcpy2D(tmp, 13 * 4, e->d.P, (size_t)e->ldP * 4, 13 * 4, 13, hipMemcpyDeviceToHost));
        for (int i = 0; i < 169; ++i) P13[i] = (double)tmp[i];
    } else {
        HIPCHK(hipMemcpy2D(P13, 13 * 8, e->d.P, (size_t)e->ldP * 8, 13 * 8, 13, hipMemcpyDeviceToHost));
    }
    return EKF_OK;
}

int ekf_get_map_points(EkfEngine *e, EkfMapPoint *points, int capacity, int *count)
{
    if (!e || !count || (points && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    NOT_WHEN_SHARDED(e)
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int pending = take_pending_error(e); // as ekf_get_state: the points are still produced from what the failed update left
    const int N = e->N;
    *count = N;
    if (N == 0 || !points) return pending;
    if (capacity < N) {
        e->err = "ekf_get_map_points: capacity " + std::to_string(capacity) + " < " + std::to_string(N) + " features";
        return EKF_ERR_CAPACITY;
    }
    if (!e->d.map_points) {
        const hipError_t st = e->bufs.alloc(&e->d.map_points, (size_t)e->cap);
        if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc map_points");
    }
    launch_map_points(e, e->d.map_points);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(points, e->d.map_points, (size_t)N * sizeof(EkfMapPoint), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return pending;
}

int ekf_get_unseen_features(EkfEngine *e, int32_t *feat_idx, int *count)
{
    if (!e || !count) return EKF_ERR_INVALID_ARG;
    *count = 0;
    if (e->N == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<int> vis(e->N);
    HIPCHK(hipMemcpy(vis.data(), e->d.pred_vis_full, (size_t)e->N * sizeof(int), hipMemcpyDeviceToHost));
    int k = 0;
    for (int i = 0; i < e->N; ++i)
        if (!vis[i]) {
            if (feat_idx) feat_idx[k] = i;
            ++k;
        }
    *count = k;
    return EKF_OK;
}

int ekf_get_feature_layout(EkfEngine *e, int32_t *type, int32_t *covpos)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    for (int i = 0; i < e->N; ++i) {
        if (type) type[i] = e->h_type[i];
        if (covpos) covpos[i] = e->h_covpos[i];
    }
    return EKF_OK;
}

int ekf_add_features(EkfEngine *e, const double *uv, const uint8_t *desc32, int count)
{
    if (!e || count < 0 || (count > 0 && !uv)) return EKF_ERR_INVALID_ARG;
    if (count == 0) return EKF_OK;
    NOT_WHEN_SHARDED(e)
    if (e->N + count > e->cap) return EKF_ERR_CAPACITY;
    HIPCHK(hipSetDevice(e->device));
    double *d_uv = e->d.mm_scratch, *d_Jpo = d_uv + 2 * (size_t)e->cap, *d_Jhr = d_Jpo + 42 * (size_t)count;
    HIPCHK(hipMemcpyAsync(d_uv, uv, (size_t)2 * count * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // the new rows of the per-feature tables: zeroed, the caller's (the descriptors are the only rows a caller gives), or left to the
    // kernel -- and those of the templates and source patches left unwritten until ekf_capture_templates (feature_tables.h)
    for (const FeatureTable &t : feature_tables(*e)) {
        if (!t.rows || t.on_add == ADD_LEAVE) continue;
        uint8_t *rows = static_cast<uint8_t *>(t.rows) + (size_t)e->N * t.row_bytes;
        HIPCHK(fill_rows(e, rows, t.on_add == ADD_GIVEN ? desc32 : nullptr, (size_t)count * t.row_bytes, true));
    }
    launch_add_features(e, d_uv, count, d_Jpo, d_Jhr);
    for (int j = 0; j < count; ++j) {
        e->h_type.push_back(EKF_FEATURE_INVERSE_DEPTH);
        e->h_covpos.push_back(e->n + 6 * j);
    }
    e->N += count;
    e->n += 6 * count;
    map_layout_changed(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_async(e);
}

// the out-of-place passes over P (compaction, batch conversion) write d.P2, allocated by the first of them
static int second_P(EkfEngine *e)
{
    if (e->d.P2) return EKF_OK;
    const size_t bytes = (size_t)round_up(e->ncap, LD_ALIGN) * e->ldP * (e->f32 ? 4 : 8);
    const hipError_t st = e->bufs.alloc_bytes(&e->d.P2, bytes); // zeroed, or not kept
    if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc P2");
    return EKF_OK;
}

// drop the listed rows (sorted row flags) from P and the listed features from the per-feature tables
static int compact_map(EkfEngine *e, const std::vector<uint8_t> &drop_feature, const std::vector<uint8_t> &drop_row)
{
    NOT_WHEN_SHARDED(e)
    const int N = e->N;
    if (const int rc = second_P(e)) return rc;
    const CompactionPlan plan = plan_compaction(e->h_type, drop_feature, drop_row);
    if (!plan.ok) { // (found before anything is enqueued)
        e->err = "map compaction: layout mismatch";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipMemcpyAsync(e->d.mm_index, plan.new2old.data(), (size_t)plan.n_new * sizeof(int), hipMemcpyHostToDevice, e->stream));
    launch_compact_P(e, plan.n_new, e->d.mm_index);
    // the per-feature tables: small, compacted through the host, every row behind its feature (feature_tables.h).  The covariance
    // positions are not moved but written anew from the plan.
    const FeatureTables tables = feature_tables(*e);
    std::vector<uint8_t> rows[N_FEATURE_TABLES];
    HIPCHK(hipStreamSynchronize(e->stream));
    for (const FeatureTable &t : tables) {
        if (!t.rows || t.id == FT_COVPOS) continue;
        rows[t.id].resize((size_t)N * t.row_bytes);
        HIPCHK(hipMemcpy(rows[t.id].data(), t.rows, rows[t.id].size(), hipMemcpyDeviceToHost));
        gather_rows(rows[t.id].data(), t.row_bytes, plan.keep);
    }
    const size_t w = plan.keep.size();
    e->h_type.resize(w); // the mirror follows the device's types: conversions change types
    if (w > 0) std::memcpy(e->h_type.data(), rows[FT_TYPE].data(), w * sizeof(int));
    e->h_covpos = plan.covpos;
    for (const FeatureTable &t : tables)
        if (t.rows && w > 0)
            HIPCHK(hipMemcpy(t.rows, t.id == FT_COVPOS ? (const void *)plan.covpos.data() : rows[t.id].data(), w * t.row_bytes, hipMemcpyHostToDevice));
    e->N = (int)w;
    e->n = plan.n_new;
    map_layout_changed(e);
    return check_async(e);
}

int ekf_remove_features(EkfEngine *e, const int32_t *feat_idx, int count)
{
    if (!e || count < 0 || (count > 0 && !feat_idx)) return EKF_ERR_INVALID_ARG;
    if (count == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    std::vector<uint8_t> df(e->N, 0), dr(e->n, 0);
    for (int i = 0; i < count; ++i) {
        const int f = feat_idx[i];
        if (f < 0 || f >= e->N || (i > 0 && feat_idx[i] <= feat_idx[i - 1])) return EKF_ERR_INVALID_ARG;
        df[f] = 1;
        for (int k = 0; k < feature_dims(e->h_type[f]); ++k) dr[e->h_covpos[f] + k] = 1;
    }
    return compact_map(e, df, dr);
}

int ekf_remove_bad_features(EkfEngine *e, int *n_removed)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int N = e->N;
    std::vector<unsigned> tp(N), tm(N);
    if (N > 0) {
        HIPCHK(hipMemcpy(tp.data(), e->d.feat_times_predicted, (size_t)N * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(tm.data(), e->d.feat_times_matched, (size_t)N * 4, hipMemcpyDeviceToHost));
    }
    std::vector<int32_t> idx;
    for (int i = 0; i < N; ++i) { // EKF/MapManagement.cpp:291-302 (float ratio, 0/0 = NaN keeps the feature)
        const float pct = static_cast<float>(tm[i]) / static_cast<float>(tp[i]);
        if (pct < e->cfg.par.goodFeatureMatchingPercent) idx.push_back(i);
    }
    if (n_removed) *n_removed = (int)idx.size();
    return ekf_remove_features(e, idx.data(), (int)idx.size());
}

int ekf_convert_inverse_depth_to_depth(EkfEngine *e, int *converted_index)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (converted_index) *converted_index = -1;
    if (e->N == 0) return EKF_OK;
    NOT_WHEN_SHARDED(e)
    HIPCHK(hipSetDevice(e->device));
    double *d_li = e->d.mm_scratch;
    launch_linearity(e, d_li);
    std::vector<double> li(e->N);
    HIPCHK(hipMemcpyAsync(li.data(), d_li, (size_t)e->N * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int fi = -1;
    for (int i = 0; i < e->N; ++i) // first inverse-depth feature in map order below the threshold, one per call (:494-521)
        if (e->h_type[i] == EKF_FEATURE_INVERSE_DEPTH && li[i] < e->cfg.par.inverseDepthLinearityIndexThreshold) {
            fi = i;
            break;
        }
    if (fi < 0) return EKF_OK;
    const int pos = e->h_covpos[fi];
    double *d_J = e->d.mm_scratch + e->cap, *d_T3 = d_J + 32;
    launch_convert(e, fi, pos, d_J, d_T3);
    e->h_type[fi] = EKF_FEATURE_DEPTH;
    std::vector<uint8_t> df(e->N, 0), dr(e->n, 0);
    dr[pos + 3] = dr[pos + 4] = dr[pos + 5] = 1;
    if (converted_index) *converted_index = fi;
    return compact_map(e, df, dr);
}

// Every inverse-depth feature below the threshold in one pass.  No feature index changes, so the tables keyed by
// feature index stay where they are: only types, positions, covpos and P are rewritten.
int ekf_convert_all_inverse_depth_to_depth(EkfEngine *e, int32_t *converted_idx, int capacity, int *count)
{
    if (!e || !count || capacity < 0) return EKF_ERR_INVALID_ARG;
    *count = 0;
    NOT_WHEN_SHARDED(e)
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e); // as ekf_update_external: the failed update it reports is not this call's
    if (rc) return rc;
    const int N = e->N;
    if (N == 0) return EKF_OK;
    double *d_li = e->d.mm_scratch;
    launch_linearity(e, d_li);
    std::vector<double> li(N);
    HIPCHK(hipMemcpyAsync(li.data(), d_li, (size_t)N * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<int> sel;
    for (int i = 0; i < N; ++i) // the comparison of the single conversion (:494-521), without its "first one only"
        if (e->h_type[i] == EKF_FEATURE_INVERSE_DEPTH && li[i] < e->cfg.par.inverseDepthLinearityIndexThreshold) sel.push_back(i);
    const int K = (int)sel.size();
    if (K == 0) return EKF_OK;
    if ((rc = second_P(e))) return rc;
    if (!e->d.ca_rows) {
        auto g = e->bufs.group();
        g.alloc(&e->d.ca_rows, (size_t)2 * e->ncap);
        g.alloc(&e->d.ca_J, (size_t)18 * e->cap);
        g.alloc(&e->d.ca_sel, (size_t)e->cap);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "batch conversion tables");
    }
    // the row table of the new matrix and the new layout, from the host mirrors
    std::vector<int> rows, covpos(N);
    rows.reserve(2 * (size_t)e->n);
    for (int i = 0; i < 13; ++i) {
        rows.push_back(i);
        rows.push_back(-1);
    }
    for (int f = 0, k = 0; f < N; ++f) {
        covpos[f] = (int)(rows.size() / 2);
        const bool conv = k < K && sel[k] == f;
        const int d = conv ? 3 : feature_dims(e->h_type[f]);
        for (int a = 0; a < d; ++a) {
            rows.push_back(conv ? e->h_covpos[f] : e->h_covpos[f] + a);
            rows.push_back(conv ? 3 * k + a : -1);
        }
        if (conv) ++k;
    }
    const int n_new = (int)(rows.size() / 2);
    if (n_new != e->n - 3 * K) {
        e->err = "batch conversion: layout mismatch";
        return EKF_ERR_INVALID_ARG;
    }
    for (int v0 = 0; v0 < n_new; v0 += CA_TILE) { // the old columns a tile of the kernel reads must fit its LDS rows
        const int vl = std::min(v0 + CA_TILE, n_new) - 1;
        if (rows[2 * vl] + (rows[2 * vl + 1] >= 0 ? 6 : 1) - rows[2 * v0] > CA_CW) {
            e->err = "batch conversion: a tile spans more old columns than the kernel holds";
            return EKF_ERR_INVALID_ARG;
        }
    }
    HIPCHK(hipMemcpyAsync(e->d.ca_sel, sel.data(), (size_t)K * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.ca_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.feat_covpos, covpos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, e->stream));
    launch_convert_all(e, K, n_new);
    HIPCHK(hipStreamSynchronize(e->stream)); // (the host vectors above are the sources of the copies)
    for (int k = 0; k < K; ++k) e->h_type[sel[k]] = EKF_FEATURE_DEPTH;
    e->h_covpos = covpos;
    e->n = n_new;
    map_layout_changed(e);
    *count = K;
    if (converted_idx)
        for (int k = 0; k < K && k < capacity; ++k) converted_idx[k] = sel[k];
    return check_async(e);
}
