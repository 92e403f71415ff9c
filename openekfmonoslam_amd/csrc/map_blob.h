// map_blob.h -- the map blob of ekf_save_map / ekf_load_map: its layout, the writer of its header and the parser
// that validates an untrusted one.  Host only: no HIP, nothing but the C++ library and ekf_types.h, so that it compiles and is
// tested on its own (tests/cpp/map_blob_check.cpp).  The parser never reads outside [blob, blob + bytes), whatever the bytes say.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/ekf_types.h"

namespace ekf {
namespace mapblob {

constexpr uint32_t VERSION = 1;
constexpr int N_SECTIONS = 12, FIXED_BYTES = 64, ENTRY_BYTES = 32;
constexpr uint32_t HEADER_BYTES = FIXED_BYTES + N_SECTIONS * ENTRY_BYTES; // 448
constexpr uint64_t ALIGN = 64;                                            // every section starts on a multiple of it
constexpr char MAGIC[9] = "EKFMAP01";
// section ids, in the order they lie in the blob
enum { SEC_X13 = 0, SEC_FEAT_POS, SEC_FEAT_TYPE, SEC_DESC, SEC_TIMES_PREDICTED, SEC_TIMES_MATCHED, SEC_P, SEC_TEMPLATES,
       SEC_WARP_SOURCES, SEC_WARP_POSES, SEC_PATCH_NORMALS, SEC_CAMERA };
enum { P_TRIANGLE = 0, P_FULL = 1 };
// bits of section_mask (EKF_MAP_* of ekf_engine.h)
constexpr uint32_t MASK_TEMPLATES = 1, MASK_WARP_SOURCES = 2, MASK_PATCH_NORMALS = 4, MASK_ALL = 7;
// A feature's row in the optional sections.  The one place these sizes are stated: engine.h defines NCC_TT, WARP_S and WPOSE_DOUBLES
// from them and ties sizeof(PatchNormalRec) to the last; feature_tables.h sizes the device tables by them.
constexpr int TEMPLATE_LEVELS = 3;                                                       // pyramid levels of a template and of a source patch
constexpr int TEMPLATE_LEVEL_BYTES = 11 * 11, TEMPLATE_BYTES = TEMPLATE_LEVELS * TEMPLATE_LEVEL_BYTES; // 363
constexpr int WARP_SOURCE_SIDE = 41, WARP_SOURCE_BYTES = TEMPLATE_LEVELS * WARP_SOURCE_SIDE * WARP_SOURCE_SIDE; // 3 x 1681
constexpr int WARP_POSE_DOUBLES = 9, PATCH_NORMAL_BYTES = 48;
constexpr int32_t MAX_N = 1 << 24, MAX_DESC_BYTES = 4096; // what the size arithmetic below is safe for in 64 bits
static_assert(sizeof(EkfCamera) == 104, "the CAMERA section is the bytes of EkfCamera");

// byte offsets of the fixed header's fields
enum { H_MAGIC = 0, H_VERSION = 8, H_HEADER_BYTES = 12, H_TOTAL = 16, H_N = 24, H_n = 28, H_P_ELEM = 32, H_P_LAYOUT = 36,
       H_DESC_BYTES = 40, H_DESC_FLAGS = 44, H_MASK = 48, H_ZERO = 52, H_CHECKSUM = 56 };
// ... and of a directory entry's
enum { E_ID = 0, E_ELEM = 4, E_OFFSET = 8, E_BYTES = 16, E_CHECKSUM = 24 };

inline uint32_t get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t get64(const uint8_t *p) { return (uint64_t)get32(p) | (uint64_t)get32(p + 4) << 32; }
inline void put32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline void put64(uint8_t *p, uint64_t v)
{
    put32(p, (uint32_t)v);
    put32(p + 4, (uint32_t)(v >> 32));
}

// sum of w_k (2 k + 1) mod 2^64 over the little-endian 32-bit words w_k of the bytes, zero-padded to a multiple of four:
// commutative (any order of summation gives it), and sensitive to where a word stands
inline uint64_t checksum(const uint8_t *p, uint64_t bytes)
{
    uint64_t s = 0, k = 0;
    for (; 4 * k + 4 <= bytes; ++k) s += (uint64_t)get32(p + 4 * k) * (2 * k + 1);
    if (4 * k < bytes) {
        uint8_t last[4] = {0, 0, 0, 0};
        std::memcpy(last, p + 4 * k, (size_t)(bytes - 4 * k));
        s += (uint64_t)get32(last) * (2 * k + 1);
    }
    return s;
}

// what fixes every size in the blob
struct Shape {
    int32_t N = 0, n = 13;
    int32_t p_elem_bytes = 8, p_layout = P_TRIANGLE;
    int32_t desc_bytes = EKF_DESC_BYTES, desc_flags = 0;
    uint32_t mask = 0;
};

struct Layout {
    bool present[N_SECTIONS];
    uint32_t elem[N_SECTIONS];
    uint64_t offset[N_SECTIONS], bytes[N_SECTIONS];
    uint64_t total;
};

// elements of the P section: the packed upper triangle, row-major (row i starts at element i n - i (i - 1) / 2), or the square
inline uint64_t p_elements(int32_t n, int32_t layout)
{
    const uint64_t m = (uint64_t)n;
    return layout == P_TRIANGLE ? m * (m + 1) / 2 : m * m;
}

// the canonical layout of a blob of this shape (the shape's fields within the parser's limits)
inline Layout layout_of(const Shape &s)
{
    Layout L;
    const uint64_t N = (uint64_t)s.N;
    const bool warp = (s.mask & MASK_WARP_SOURCES) != 0;
    const bool pres[N_SECTIONS] = {true, true, true, true, true, true, true, (s.mask & MASK_TEMPLATES) != 0, warp, warp,
                                   (s.mask & MASK_PATCH_NORMALS) != 0, true};
    const uint32_t elem[N_SECTIONS] = {8, 8, 4, 1, 4, 4, (uint32_t)s.p_elem_bytes, 1, 1, 8, PATCH_NORMAL_BYTES, (uint32_t)sizeof(EkfCamera)};
    const uint64_t bytes[N_SECTIONS] = {13 * 8, 6 * N * 8, N * 4, N * (uint64_t)s.desc_bytes, N * 4, N * 4,
                                        p_elements(s.n, s.p_layout) * (uint64_t)s.p_elem_bytes, N * TEMPLATE_BYTES, N * WARP_SOURCE_BYTES,
                                        N * WARP_POSE_DOUBLES * 8, N * PATCH_NORMAL_BYTES, sizeof(EkfCamera)};
    uint64_t at = HEADER_BYTES;
    for (int id = 0; id < N_SECTIONS; ++id) {
        L.present[id] = pres[id];
        L.elem[id] = pres[id] ? elem[id] : 0;
        L.bytes[id] = pres[id] ? bytes[id] : 0;
        L.offset[id] = 0;
        if (!pres[id]) continue;
        at = (at + ALIGN - 1) / ALIGN * ALIGN;
        L.offset[id] = at;
        at += bytes[id];
    }
    L.total = at; // the blob ends with its last section (CAMERA)
    return L;
}

// writes the 448 header bytes of a blob of this shape; sums[id]: the checksum of every present section's bytes
inline void write_header(uint8_t *blob, const Shape &s, const Layout &L, const uint64_t sums[N_SECTIONS])
{
    std::memset(blob, 0, HEADER_BYTES);
    std::memcpy(blob + H_MAGIC, MAGIC, 8);
    put32(blob + H_VERSION, VERSION);
    put32(blob + H_HEADER_BYTES, HEADER_BYTES);
    put64(blob + H_TOTAL, L.total);
    put32(blob + H_N, (uint32_t)s.N);
    put32(blob + H_n, (uint32_t)s.n);
    put32(blob + H_P_ELEM, (uint32_t)s.p_elem_bytes);
    put32(blob + H_P_LAYOUT, (uint32_t)s.p_layout);
    put32(blob + H_DESC_BYTES, (uint32_t)s.desc_bytes);
    put32(blob + H_DESC_FLAGS, (uint32_t)s.desc_flags);
    put32(blob + H_MASK, s.mask);
    for (int id = 0; id < N_SECTIONS; ++id) {
        uint8_t *en = blob + FIXED_BYTES + ENTRY_BYTES * id;
        put32(en + E_ID, (uint32_t)id);
        if (!L.present[id]) continue;
        put32(en + E_ELEM, L.elem[id]);
        put64(en + E_OFFSET, L.offset[id]);
        put64(en + E_BYTES, L.bytes[id]);
        put64(en + E_CHECKSUM, sums[id]);
    }
    put64(blob + H_CHECKSUM, checksum(blob, HEADER_BYTES)); // (taken with the field still zero)
}

// zeroes the gaps between the header and the sections of a blob laid out as L (a writer that fills the sections in place)
inline void zero_gaps(uint8_t *blob, const Layout &L)
{
    uint64_t at = HEADER_BYTES;
    for (int id = 0; id < N_SECTIONS; ++id) {
        if (!L.present[id]) continue;
        std::memset(blob + at, 0, (size_t)(L.offset[id] - at));
        at = L.offset[id] + L.bytes[id];
    }
}

// a validated blob: its shape, where its sections lie, and the checksum its directory states for each
struct Parsed {
    Shape shape;
    Layout layout;
    uint64_t sums[N_SECTIONS];
    EkfCamera cam;
};

inline EkfMapBlobInfo info_of(const Parsed &p)
{
    EkfMapBlobInfo o;
    std::memset(&o, 0, sizeof(o));
    o.version = VERSION;
    o.N = p.shape.N;
    o.n = p.shape.n;
    o.p_elem_bytes = p.shape.p_elem_bytes;
    o.p_layout = p.shape.p_layout;
    o.desc_bytes = p.shape.desc_bytes;
    o.desc_flags = p.shape.desc_flags;
    o.section_mask = p.shape.mask;
    o.total_bytes = p.layout.total;
    o.cam = p.cam;
    return o;
}

inline bool fail(std::string *err, const std::string &what)
{
    if (err) *err = "map blob: " + what;
    return false;
}

// Validates everything the host can: the header and its checksum, the directory against the canonical layout of the header's shape
// (so every section is inside the blob, aligned, in order, of exactly the demanded size), zero gaps, the checksum of every section
// (that of P only with check_p: the engine leaves it to the device, k_map_check), the feature types against n, and finite x13 and
// feature parameters with a non-zero quaternion.  True, or false with a message that names the field.
inline bool parse(const void *blob_, size_t bytes, bool check_p, Parsed *out, std::string *err)
{
    static const char *const names[N_SECTIONS] = {"X13", "FEAT_POS", "FEAT_TYPE", "DESC", "TIMES_PREDICTED", "TIMES_MATCHED", "P", "TEMPLATES",
                                                  "WARP_SOURCES", "WARP_POSES", "PATCH_NORMALS", "CAMERA"};
    const uint8_t *blob = (const uint8_t *)blob_;
    if (!blob || bytes < HEADER_BYTES) return fail(err, "truncated: " + std::to_string(bytes) + " bytes hold no header (448 bytes)");
    if (std::memcmp(blob + H_MAGIC, MAGIC, 8) != 0) return fail(err, "magic is not EKFMAP01");
    if (get32(blob + H_VERSION) != VERSION) return fail(err, "version " + std::to_string(get32(blob + H_VERSION)) + " is not 1");
    if (get32(blob + H_HEADER_BYTES) != HEADER_BYTES) return fail(err, "header_bytes is not 448");
    {
        uint8_t h[HEADER_BYTES];
        std::memcpy(h, blob, HEADER_BYTES);
        put64(h + H_CHECKSUM, 0);
        if (checksum(h, HEADER_BYTES) != get64(blob + H_CHECKSUM)) return fail(err, "header_checksum does not match the header");
    }
    if (get64(blob + H_TOTAL) != (uint64_t)bytes)
        return fail(err, "total_bytes " + std::to_string(get64(blob + H_TOTAL)) + " is not the " + std::to_string(bytes) + " bytes given (truncated?)");
    Parsed p;
    Shape &s = p.shape;
    s.N = (int32_t)get32(blob + H_N);
    s.n = (int32_t)get32(blob + H_n);
    s.p_elem_bytes = (int32_t)get32(blob + H_P_ELEM);
    s.p_layout = (int32_t)get32(blob + H_P_LAYOUT);
    s.desc_bytes = (int32_t)get32(blob + H_DESC_BYTES);
    s.desc_flags = (int32_t)get32(blob + H_DESC_FLAGS);
    s.mask = get32(blob + H_MASK);
    if (s.N < 0 || s.N > MAX_N) return fail(err, "N out of range");
    if (s.n < 13 + 3 * (int64_t)s.N || s.n > 13 + 6 * (int64_t)s.N) return fail(err, "n is impossible for N features");
    if (s.p_elem_bytes != 4 && s.p_elem_bytes != 8) return fail(err, "p_elem_bytes is neither 4 nor 8");
    if (s.p_layout != P_TRIANGLE && s.p_layout != P_FULL) return fail(err, "p_layout is neither 0 nor 1");
    if (s.desc_bytes < 1 || s.desc_bytes > MAX_DESC_BYTES) return fail(err, "desc_bytes out of range");
    if (s.mask & ~MASK_ALL) return fail(err, "section_mask has unknown bits");
    if (get32(blob + H_ZERO) != 0) return fail(err, "reserved header word is not zero");
    const Layout L = layout_of(s);
    if (L.total != (uint64_t)bytes) return fail(err, "total_bytes is not what N, n and the header demand");
    uint64_t at = HEADER_BYTES;
    for (int id = 0; id < N_SECTIONS; ++id) {
        const uint8_t *en = blob + FIXED_BYTES + ENTRY_BYTES * id;
        const std::string nm = names[id];
        if (get32(en + E_ID) != (uint32_t)id) return fail(err, "directory entry " + std::to_string(id) + " has the wrong id");
        p.sums[id] = get64(en + E_CHECKSUM);
        if (get32(en + E_ELEM) != L.elem[id]) return fail(err, "section " + nm + ": elem_bytes (or its presence) contradicts the header");
        if (get64(en + E_BYTES) != L.bytes[id]) return fail(err, "section " + nm + ": size is not what N, n and the header demand");
        if (get64(en + E_OFFSET) != L.offset[id]) return fail(err, "section " + nm + ": offset is not the next multiple of 64");
        if (!L.present[id]) {
            if (p.sums[id] != 0) return fail(err, "section " + nm + ": absent, but its entry is not zero");
            continue;
        }
        // (L.offset + L.bytes <= L.total == bytes: everything read below is inside the blob)
        for (uint64_t g = at; g < L.offset[id]; ++g)
            if (blob[g] != 0) return fail(err, "gap before section " + nm + " is not zero");
        at = L.offset[id] + L.bytes[id];
        if ((id != SEC_P || check_p) && checksum(blob + L.offset[id], L.bytes[id]) != p.sums[id])
            return fail(err, "section " + nm + ": checksum does not match its bytes");
    }
    p.layout = L;
    std::memcpy(&p.cam, blob + L.offset[SEC_CAMERA], sizeof(EkfCamera));
    int64_t dims = 13;
    for (int32_t i = 0; i < s.N; ++i) {
        const uint32_t t = get32(blob + L.offset[SEC_FEAT_TYPE] + 4 * (uint64_t)i);
        if (t != EKF_FEATURE_DEPTH && t != EKF_FEATURE_INVERSE_DEPTH)
            return fail(err, "FEAT_TYPE of feature " + std::to_string(i) + " is " + std::to_string(t));
        dims += t == EKF_FEATURE_INVERSE_DEPTH ? 6 : 3;
    }
    if (dims != s.n) return fail(err, "n = " + std::to_string(s.n) + " but the FEAT_TYPE section sums to " + std::to_string(dims));
    auto f64_at = [&](uint64_t off) {
        const uint64_t u = get64(blob + off);
        double d;
        std::memcpy(&d, &u, 8);
        return d;
    };
    double qq = 0.0;
    for (int i = 0; i < 13; ++i) {
        const double v = f64_at(L.offset[SEC_X13] + 8 * (uint64_t)i);
        if (!std::isfinite(v)) return fail(err, "X13 is not finite");
        if (i >= 3 && i < 7) qq += v * v;
    }
    if (!(qq > 0.0)) return fail(err, "X13: the quaternion is zero");
    for (uint64_t i = 0; i < 6 * (uint64_t)s.N; ++i)
        if (!std::isfinite(f64_at(L.offset[SEC_FEAT_POS] + 8 * i))) return fail(err, "FEAT_POS is not finite (feature " + std::to_string(i / 6) + ")");
    if (out) *out = p;
    return true;
}

} // namespace mapblob
} // namespace ekf
