// digit_planes.h -- cutting a scaled fp64 value into PX_S balanced base-256 digits (EKF_PRECISION_F32_EXACT; kernels_pexact.hip,
// chol_bplanes.h).  X = rint(v 2^sh), |X| <= 2^(8 PX_S - 2), is wanted as X = sum_s d_s 256^(PX_S - 1 - s) with every d_s in
// [-128, 127] (int8 operands of v_mfma_i32_32x32x32_i8).  No carry chain is needed: with K = 0x80 repeated PX_S times,
// the BYTES of X + K are b_s = d_s + 128 for exactly that digit set (sum_s (b_s - 128) 256^(..) = X + K - K), and b - 128
// reinterpreted as int8 is b ^ 0x80.  So the digits are the bytes of (X + K) ^ K; the top byte stays in [0x40, 0xC0].
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PX_HD __host__ __device__ __forceinline__
#else // plain C++: tests/cpp/digit_word_check.cpp compiles the word functions with g++, without engine.h
#include <cmath>
#define PX_HD inline
#ifndef PX_S_VALUE
#define PX_S_VALUE 5
#endif
namespace ekf {
constexpr int PX_S = PX_S_VALUE;
}
#endif

namespace ekf {

static_assert(PX_S >= 4 && PX_S <= 6, "digit words are written out for 4, 5 or 6 digits");

PX_HD unsigned long long px_digit_word(double v, int sh)
{
    constexpr unsigned long long K = PX_S == 5 ? 0x8080808080ull : (PX_S == 6 ? 0x808080808080ull : 0x80808080ull);
#ifdef __HIP_DEVICE_COMPILE__
    const long long X = __double2ll_rn(ldexp(v, sh));
#else
    const long long X = std::llrint(std::ldexp(v, sh)); // (round to nearest even, the default rounding mode)
#endif
    return ((unsigned long long)X + K) ^ K; // byte (PX_S - 1 - s) = digit s as int8
}

// The integer X of a digit word W = (X + K) ^ K as a double, without 64-bit integer arithmetic: hi = W >> 32 (the top PX_S - 4 digits),
// lo = the low 32 bits.  X = (W ^ K) - K splits into hi's digits as signed bytes times 2^32 plus (lo ^ 0x80808080) - 0x80808080; both
// parts and their sum are integers below 2^(8 PX_S - 1) <= 2^47 in magnitude, so every operation is exact in fp64 and the result has the
// bits of (double)X (k_dx_planes: one conversion per element of B).
PX_HD double px_word_value(unsigned hi, unsigned lo)
{
    const double l = (double)(lo ^ 0x80808080u) - 2155905152.0; // 0x80808080
    if (PX_S == 4) return l;
    // (b ^ 0x80) - 0x80 is the byte b read as int8
    const int h = PX_S == 5 ? (int)(signed char)(hi & 255u) : 256 * (int)(signed char)((hi >> 8) & 255u) + (int)(signed char)(hi & 255u);
    return fma((double)h, 4294967296.0, l);
}

#ifdef __HIPCC__
// ... for the rows of B under an A-PRIORI column scale (|B_kj| <= sqrt(P_jj), chol_bplanes.h): the bound holds for a positive
// semi-definite P; a covariance uploaded with |P_ij| > sqrt(P_ii P_jj) (or a NaN) breaks it, and digits that wrap would downdate P with
// garbage in silence.  An integer that does not fit the PX_S digits raises the sticky code EKF_ERR_NON_FINITE instead -- the kernels
// behind the sweep then leave the filter untouched (engine.h: filter_frozen) and the update reports it.
__device__ __forceinline__ unsigned long long px_digit_word_checked(double v, int sh, int *counts)
{
    constexpr unsigned long long K = PX_S == 5 ? 0x8080808080ull : (PX_S == 6 ? 0x808080808080ull : 0x80808080ull);
    const long long X = __double2ll_rn(ldexp(v, sh));
    const long long lim = 1ll << (8 * PX_S - 1);
    if (counts && !(X > -lim && X < lim)) atomicMax(&counts[CNT_ERR], (int)EKF_ERR_NON_FINITE);
    return ((unsigned long long)X + K) ^ K;
}
#endif

// digit s of the word
PX_HD unsigned px_digit_byte(unsigned long long w, int s) { return (unsigned)(w >> (8 * (PX_S - 1 - s))) & 255u; }

} // namespace ekf
