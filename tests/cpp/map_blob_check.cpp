// map_blob_check.cpp -- openekfmonoslam_amd/csrc/map_blob.h alone, on the host (tests/test_map_blob_host.py builds it under
// AddressSanitizer and UBSan): a small valid blob is built and parsed back, then every prefix of it, every single-byte corruption
// of its 448 header bytes and a few thousand seeded multi-byte corruptions are handed to the parser in a heap buffer of exactly the
// stated size -- a read outside [blob, blob + bytes) is a sanitizer report.  Each case must be refused or accepted, nothing else.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../openekfmonoslam_amd/csrc/map_blob.h"

using namespace ekf::mapblob;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);        \
            return 1;                                                 \
        }                                                             \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// parse a copy that lives in a heap block of exactly `bytes` bytes
static bool parse_exact(const uint8_t *data, size_t bytes, bool check_p, Parsed *out, std::string *err)
{
    uint8_t *copy = (uint8_t *)std::malloc(bytes ? bytes : 1);
    if (bytes) std::memcpy(copy, data, bytes);
    const bool ok = parse(bytes ? copy : copy, bytes, check_p, out, err);
    std::free(copy);
    return ok;
}

static std::vector<uint8_t> make_blob(const Shape &s, EkfCamera *cam_out)
{
    const Layout L = layout_of(s);
    std::vector<uint8_t> b((size_t)L.total, 0xcd);
    zero_gaps(b.data(), L);
    for (int id = 0; id < N_SECTIONS; ++id)
        if (L.present[id])
            for (uint64_t k = 0; k < L.bytes[id]; ++k) b[(size_t)(L.offset[id] + k)] = (uint8_t)rnd();
    double x13[13] = {0.1, 0.2, 0.3, 1, 0, 0, 0, 0, 0, 0, 1e-3, 1e-3, 1e-3};
    std::memcpy(&b[(size_t)L.offset[SEC_X13]], x13, sizeof(x13));
    int left = s.n - 13;
    for (int i = 0; i < s.N; ++i) {
        const int rest = s.N - 1 - i;
        const int32_t t = left - 6 >= 3 * rest ? EKF_FEATURE_INVERSE_DEPTH : EKF_FEATURE_DEPTH;
        left -= t == EKF_FEATURE_INVERSE_DEPTH ? 6 : 3;
        put32(&b[(size_t)L.offset[SEC_FEAT_TYPE] + 4 * (size_t)i], (uint32_t)t);
        for (int k = 0; k < 6; ++k) {
            const double v = 0.25 * (double)(i + k);
            std::memcpy(&b[(size_t)L.offset[SEC_FEAT_POS] + 8 * (size_t)(6 * i + k)], &v, 8);
        }
    }
    EkfCamera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.pixelsX = 640;
    cam.pixelsY = 480;
    cam.fx = 525.0;
    cam.fy = 524.0;
    std::memcpy(&b[(size_t)L.offset[SEC_CAMERA]], &cam, sizeof(cam));
    if (cam_out) *cam_out = cam;
    uint64_t sums[N_SECTIONS];
    for (int id = 0; id < N_SECTIONS; ++id) sums[id] = L.present[id] ? checksum(&b[(size_t)L.offset[id]], L.bytes[id]) : 0;
    write_header(b.data(), s, L, sums);
    return b;
}

int main()
{
    // the checksum's definition on a range that is no multiple of four bytes
    {
        const uint8_t d[7] = {1, 0, 0, 0, 2, 3, 4};
        CHECK(checksum(d, 7) == 1ull * 1 + (2ull | 3ull << 8 | 4ull << 16) * 3);
        CHECK(checksum(d, 0) == 0);
    }
    long refused = 0, accepted = 0;
    for (int variant = 0; variant < 3; ++variant) {
        Shape s;
        s.N = variant == 2 ? 0 : 5;
        s.n = variant == 2 ? 13 : 13 + 6 * 3 + 3 * 2;
        s.p_elem_bytes = variant == 0 ? 4 : 8;
        s.p_layout = variant == 0 ? P_TRIANGLE : P_FULL;
        s.desc_flags = 0;
        s.mask = variant == 0 ? MASK_ALL : (variant == 1 ? MASK_TEMPLATES : 0);
        EkfCamera cam;
        const std::vector<uint8_t> blob = make_blob(s, &cam);
        const size_t B = blob.size();
        CHECK(B % 1 == 0 && B > HEADER_BYTES);
        Parsed p;
        std::string err;
        CHECK(parse_exact(blob.data(), B, true, &p, &err));
        CHECK(p.shape.N == s.N && p.shape.n == s.n && p.shape.p_elem_bytes == s.p_elem_bytes && p.shape.p_layout == s.p_layout);
        CHECK(p.shape.desc_bytes == s.desc_bytes && p.shape.desc_flags == s.desc_flags && p.shape.mask == s.mask);
        CHECK(p.layout.total == B && std::memcmp(&p.cam, &cam, sizeof(cam)) == 0);
        const EkfMapBlobInfo info = info_of(p);
        CHECK(info.version == 1 && info.N == s.N && info.n == s.n && info.total_bytes == B && info.section_mask == s.mask);
        for (int id = 0; id < N_SECTIONS; ++id) {
            CHECK(p.layout.offset[id] % ALIGN == 0);
            CHECK(!p.layout.present[id] || p.layout.offset[id] + p.layout.bytes[id] <= B);
        }
        CHECK(p.layout.bytes[SEC_P] == p_elements(s.n, s.p_layout) * (uint64_t)s.p_elem_bytes);
        // every prefix is refused, and says so
        for (size_t len = 0; len < B; ++len) {
            err.clear();
            CHECK(!parse_exact(blob.data(), len, true, nullptr, &err));
            CHECK(!err.empty());
            ++refused;
        }
        // every single-byte corruption of the header is refused (the header checksum covers all 448 bytes)
        std::vector<uint8_t> bad;
        for (size_t at = 0; at < HEADER_BYTES; ++at)
            for (int k = 0; k < 3; ++k) {
                bad = blob;
                const uint8_t v = k == 0 ? (uint8_t)(bad[at] ^ 0xff) : (k == 1 ? (uint8_t)(bad[at] + 1) : (uint8_t)rnd());
                if (v == bad[at]) continue;
                bad[at] = v;
                CHECK(!parse_exact(bad.data(), B, true, nullptr, &err));
                ++refused;
            }
        // the same with the header checksum made right again: the field itself has to be caught (or be harmless)
        for (size_t at = 0; at < H_CHECKSUM; ++at) {
            bad = blob;
            bad[at] = (uint8_t)(bad[at] ^ (1u << (rnd() % 8)));
            put64(&bad[H_CHECKSUM], 0);
            put64(&bad[H_CHECKSUM], checksum(bad.data(), HEADER_BYTES));
            const bool ok = parse_exact(bad.data(), B, true, nullptr, &err);
            // desc_flags alone is free, and desc_bytes where an empty map has no descriptor rows: the engine compares both with its own
            CHECK(!ok || (at >= H_DESC_FLAGS && at < H_MASK) || (s.N == 0 && at >= H_DESC_BYTES && at < H_DESC_FLAGS));
            ok ? ++accepted : ++refused;
        }
        // seeded multi-byte corruptions anywhere, half of them with the header checksum recomputed, at the true and at wrong lengths
        for (int it = 0; it < 4000; ++it) {
            bad = blob;
            const int hits = 1 + (int)(rnd() % 6);
            for (int h = 0; h < hits; ++h) {
                const size_t at = (rnd() & 1) ? rnd() % HEADER_BYTES : rnd() % B;
                bad[at] = (uint8_t)rnd();
            }
            if (it & 1) {
                put64(&bad[H_CHECKSUM], 0);
                put64(&bad[H_CHECKSUM], checksum(bad.data(), HEADER_BYTES));
            }
            const size_t len = it % 7 == 0 ? rnd() % (B + 1) : B;
            const bool ok = parse_exact(bad.data(), len, (it & 2) != 0, nullptr, &err);
            ok ? ++accepted : ++refused;
        }
        // a flipped bit in every present section but P is caught by its checksum; in P only with check_p
        for (int id = 0; id < N_SECTIONS; ++id) {
            if (!p.layout.present[id] || p.layout.bytes[id] == 0) continue;
            bad = blob;
            bad[(size_t)(p.layout.offset[id] + p.layout.bytes[id] / 2)] ^= 0x04;
            CHECK(!parse_exact(bad.data(), B, true, nullptr, &err));
            CHECK(parse_exact(bad.data(), B, false, nullptr, &err) == (id == SEC_P));
        }
    }
    std::printf("map_blob_check: ok (%ld refused, %ld accepted)\n", refused, accepted);
    return 0;
}
