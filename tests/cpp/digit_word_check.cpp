// The digit word of the exact downdate as a double (openekfmonoslam_amd/csrc/digit_planes.h: px_word_value) against the 64-bit integer
// path it replaces in k_dx_planes (X = X * 256 + (signed char) digit, most significant first, then (double)X): bit for bit, for every
// top byte crossed with the corner low words and 10^5 seeded random ones, and the round trip px_digit_word -> double for the largest
// integers, +-1 and 0.  Plain C++, no HIP (tests/test_digit_word_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../openekfmonoslam_amd/csrc/digit_planes.h"

using namespace ekf;

static int n_failed = 0;

static uint64_t bits(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// the integer of a digit word as k_dx_planes formed it before px_word_value: a signed-byte Horner chain in long long
static double reference(unsigned long long W)
{
    long long X = 0;
    for (int s = 0; s < PX_S; ++s) X = X * 256 + (long long)(signed char)px_digit_byte(W, s);
    return (double)X;
}

static void check_word(unsigned long long W)
{
    const double want = reference(W), got = px_word_value((unsigned)(W >> 32), (unsigned)W);
    if (bits(want) != bits(got)) {
        if (n_failed < 20) std::printf("word %012llx: want %.17g (%016llx), got %.17g (%016llx)\n", W, want, (unsigned long long)bits(want), got,
                                       (unsigned long long)bits(got));
        ++n_failed;
    }
}

static void check_round_trip(double v, int sh, double want)
{
    const unsigned long long W = px_digit_word(v, sh);
    const double got = px_word_value((unsigned)(W >> 32), (unsigned)W);
    if (bits(got) != bits(want) || bits(reference(W)) != bits(want)) {
        std::printf("round trip of %.17g, shift %d: want %.17g, got %.17g (integer path %.17g)\n", v, sh, want, got, reference(W));
        ++n_failed;
    }
}

int main()
{
    static_assert(PX_S == 5, "the cases below are written for five digits");
    const unsigned corners[5] = {0u, 0x80808080u, 0x7F7F7F7Fu, 0xFFFFFFFFu, 0x00000001u};
    uint64_t rng = 0x9E3779B97F4A7C15ull; // (xorshift64*, fixed seed)
    static unsigned random_lo[100000];
    for (unsigned &r : random_lo) {
        rng ^= rng >> 12;
        rng ^= rng << 25;
        rng ^= rng >> 27;
        r = (unsigned)((rng * 0x2545F4914F6CDD1Dull) >> 32);
    }
    long long n_words = 0;
    for (unsigned top = 0; top < 256; ++top) {
        for (unsigned lo : corners) check_word(((unsigned long long)top << 32) | lo), ++n_words;
        for (unsigned lo : random_lo) check_word(((unsigned long long)top << 32) | lo), ++n_words;
    }
    // bits of the word above the PX_S digits are not part of it
    if (bits(px_word_value(0xFFFFFF00u, 0u)) != bits(0.0) || bits(px_word_value(0xABCDEF01u, 0u)) != bits(4294967296.0)) {
        std::printf("bits above the top digit changed the value\n");
        ++n_failed;
    }

    const double big = 274877906943.0; // 2^38 - 1
    check_round_trip(big, 0, big);
    check_round_trip(-big, 0, -big);
    check_round_trip(1.0, 0, 1.0);
    check_round_trip(-1.0, 0, -1.0);
    check_round_trip(0.0, 0, 0.0);
    // ... and through a scale, as k_slice_B cuts them: v 2^sh is the integer
    check_round_trip(big / 1024.0, 10, big);
    check_round_trip(-big * 8.0, -3, -big);
    check_round_trip(0.25, 2, 1.0);
    check_round_trip(-0.5, 1, -1.0);
    check_round_trip(0.0, 17, 0.0);

    if (n_failed) {
        std::printf("digit_word_check: %d FAILED\n", n_failed);
        return 1;
    }
    std::printf("digit_word_check: ok (%lld words)\n", n_words);
    return 0;
}
