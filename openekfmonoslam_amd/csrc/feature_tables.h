// feature_tables.h -- the one list of the per-feature tables, and the host arithmetic of a map compaction.  Host
// only: nothing of HIP, nothing of the engine but the names of its members, so that it compiles and is tested on its own
// (tests/cpp/feature_tables_check.cpp).
//
// A feature owns one row in each of these tables.  Every operation that adds, moves, replaces, saves or loads a feature's rows
// (map_host.cpp: ekf_add_features, compact_map, ekf_set_state, ekf_save_map, ekf_load_map) is a loop over this list, and what it does
// to a table is the table's policy below: a new per-feature table is one more record here.
//
// d.wtmpl is NOT in the list although it is sized per feature: it is a cache of the templates the last NCC match compared, valid only
// while e->last_match_warped is set, and every operation over this list clears that flag instead of moving the cache's rows.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "map_blob.h"

namespace ekf {

enum FeatureTableId { FT_POS = 0, FT_TYPE, FT_COVPOS, FT_DESC, FT_TIMES_PREDICTED, FT_TIMES_MATCHED, FT_TMPL, FT_WSRC, FT_WPOSE, FT_WNORM,
                      N_FEATURE_TABLES };
constexpr int NO_SECTION = -1;

// rows count features N_old .. N_old + count - 1 of ekf_add_features
enum OnAdd {
    ADD_LEAVE, // not written by the host: the kernel fills them (pos, type, covpos), or nothing does until ekf_capture_templates (tmpl, wsrc)
    ADD_ZERO,  // zeroed
    ADD_GIVEN  // the caller's rows, zeroed where the caller gives none
};
// a map replacement (ekf_set_state, ekf_load_map) of N features in a table of `cap` rows
enum OnReplace {
    REPLACE_LEAVE,    // untouched unless the replacement brings rows for it: ekf_set_state brings none for tmpl and wsrc and so leaves
                      // the old map's templates and source patches in place (today's behaviour, pinned by test_gpu_feature_tables.py)
    REPLACE_ZERO_ALL, // all `cap` rows zeroed, then the rows the replacement brings (ekf_load_map) written over rows 0 .. N - 1
    REPLACE_ROWS      // rows 0 .. N - 1 overwritten: the replacement's rows, zeros where it gives none (desc); the rest untouched
};
// ekf_load_map of a blob that lacks the table's section, into an engine that has the table
enum OnAbsent {
    ABSENT_LEAVE,    // nothing more than the replacement did (the section is never absent, or REPLACE_ZERO_ALL has zeroed the table)
    ABSENT_ZERO_ROWS // rows 0 .. N - 1 zeroed: no feature of the loaded map has a template / a source patch
};

struct FeatureTable {
    FeatureTableId id;
    void *rows;       // the DeviceArrays member's value; null: an optional table whose mode never allocated it
    size_t row_bytes; // per feature
    bool optional;    // allocated by a mode (ensure_warp_tables, ensure_patch_normal_tables), not by the engine's creation
    int section;      // mapblob::SEC_*, or NO_SECTION: derived from the types (covpos), never stored
    OnAdd on_add;
    OnReplace on_replace;
    OnAbsent on_absent;
};
using FeatureTables = std::array<FeatureTable, N_FEATURE_TABLES>;

// The list for an engine (anything with the members d.* and desc_bytes), in FeatureTableId order.  The row sizes are those of
// map_blob.h, which engine.h's constants are defined from.
template <class Engine>
inline FeatureTables feature_tables(const Engine &e)
{
    using namespace mapblob;
    const auto &d = e.d;
    return {{
        {FT_POS, d.feat_pos, 6 * sizeof(double), false, SEC_FEAT_POS, ADD_LEAVE, REPLACE_ROWS, ABSENT_LEAVE},
        {FT_TYPE, d.feat_type, sizeof(int32_t), false, SEC_FEAT_TYPE, ADD_LEAVE, REPLACE_ROWS, ABSENT_LEAVE},
        {FT_COVPOS, d.feat_covpos, sizeof(int32_t), false, NO_SECTION, ADD_LEAVE, REPLACE_ROWS, ABSENT_LEAVE},
        {FT_DESC, d.feat_desc, (size_t)e.desc_bytes, false, SEC_DESC, ADD_GIVEN, REPLACE_ROWS, ABSENT_LEAVE},
        {FT_TIMES_PREDICTED, d.feat_times_predicted, sizeof(uint32_t), false, SEC_TIMES_PREDICTED, ADD_ZERO, REPLACE_ZERO_ALL, ABSENT_LEAVE},
        {FT_TIMES_MATCHED, d.feat_times_matched, sizeof(uint32_t), false, SEC_TIMES_MATCHED, ADD_ZERO, REPLACE_ZERO_ALL, ABSENT_LEAVE},
        {FT_TMPL, d.tmpl, TEMPLATE_BYTES, false, SEC_TEMPLATES, ADD_LEAVE, REPLACE_LEAVE, ABSENT_ZERO_ROWS},
        {FT_WSRC, d.wsrc, WARP_SOURCE_BYTES, true, SEC_WARP_SOURCES, ADD_LEAVE, REPLACE_LEAVE, ABSENT_ZERO_ROWS},
        {FT_WPOSE, d.wpose, WARP_POSE_DOUBLES * sizeof(double), true, SEC_WARP_POSES, ADD_ZERO, REPLACE_ZERO_ALL, ABSENT_LEAVE},
        {FT_WNORM, d.wnorm, PATCH_NORMAL_BYTES, true, SEC_PATCH_NORMALS, ADD_ZERO, REPLACE_ZERO_ALL, ABSENT_LEAVE},
    }};
}

inline int feature_dims(int type) { return type == EKF_FEATURE_INVERSE_DEPTH ? 6 : 3; }

// What a compaction keeps: features (ascending, old indices), their new covariance positions, and the old row of every new row of P.
struct CompactionPlan {
    std::vector<int> keep, covpos, new2old;
    int n_new = 0;
    bool ok = false; // false: the row flags keep another number of rows than the kept features' types add up to
};

// type: the host mirror of the feature types as they are to be AFTER the compaction (a single conversion has already written DEPTH
// for the feature whose rows pos + 3 .. pos + 5 it drops); drop_feature: one flag per feature; drop_row: one flag per row of P.
// The old covariance positions do not enter: the kept rows close up in order, so the new positions follow from the types alone.
inline CompactionPlan plan_compaction(const std::vector<int> &type, const std::vector<uint8_t> &drop_feature, const std::vector<uint8_t> &drop_row)
{
    CompactionPlan p;
    for (size_t i = 0; i < drop_row.size(); ++i)
        if (!drop_row[i]) p.new2old.push_back((int)i);
    p.n_new = (int)p.new2old.size();
    int pos = 13;
    for (size_t i = 0; i < type.size(); ++i) {
        if (drop_feature[i]) continue;
        p.keep.push_back((int)i);
        p.covpos.push_back(pos);
        pos += feature_dims(type[i]);
    }
    p.ok = pos == p.n_new;
    return p;
}

// Compacts a host buffer of row_bytes-wide rows in place: row keep[w] moves to row w.  keep is ascending, so a row only ever moves
// towards the front, onto rows already moved or dropped.  The rows behind keep.size() are left as they are.
inline void gather_rows(void *buf, size_t row_bytes, const std::vector<int> &keep)
{
    uint8_t *b = static_cast<uint8_t *>(buf);
    for (size_t w = 0; w < keep.size(); ++w)
        if ((size_t)keep[w] != w) std::memmove(b + w * row_bytes, b + (size_t)keep[w] * row_bytes, row_bytes);
}

} // namespace ekf
