// update_ref_ld.cpp -- TEST INFRASTRUCTURE ONLY.  The arithmetic of tests/update_ref.py update_core restated in compiled C++, templated
// on the scalar type: `long double` (the reference of updates too large for interpreted np.longdouble) and `double` (the "fp64 loop
// restatement" that C_ARITH_LARGE_MEASURED is measured with).  tests/update_ref_fast.py builds it with g++ -O2 -fopenmp -shared -fPIC
// and binds it with ctypes.
//
// Operation structure and rounding points are update_core's: A = H P (H in the CSR form of visual_rows, a row's entries in stored
// order), S = A H' + R with the upper triangle mirrored, the lower Cholesky factor by columns from dot products, z and B by forward
// substitution (x_i = (a_i - sum_{k<i} L_ik x_k) / L_ii), W = inv(L) by the same substitution of the identity, dx = B'z,
// P6 = mirror_upper(P/2 + P'/2 - B'B).  Every output entry is ONE sum, accumulated in ascending k by one thread: threads divide
// output entries only, so the bits do not depend on their number (tests/test_update_ref_fast_cpu.py asserts it).  Blocking (several
// entries per pass, k in chunks with the accumulator kept) changes which entries share a pass, never an entry's own order.
//
// -DUPDATE_REF_LD_MAIN: a stand-alone program (n = 40, m = 10) for a run under -fsanitize=address,undefined.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

// out_t[c][i], i = 0 .. m - 1: the solution of L x = rhs column c, for the columns [0, nc); rhs_t[c][i] in the same layout (may alias
// out_t); k0[c] (or 0): the first row with a non-zero right-hand side -- the sums start there (the terms before it are products
// with exact zeros).  Four columns per pass over a row of L.
template <typename T>
void forward_columns(const T *L, int m, T *x_t, int nc, const int *k0, int threads)
{
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int cb = 0; cb < nc; cb += 4) {
        const int w = nc - cb < 4 ? nc - cb : 4;
        T *x[4];
        int s[4];
        for (int u = 0; u < 4; ++u) {
            x[u] = x_t + (size_t)(cb + (u < w ? u : 0)) * m;
            s[u] = k0 ? k0[cb + (u < w ? u : 0)] : 0;
        }
        const int first = k0 ? k0[cb] : 0; // (k0 ascending in c: the block's earliest start)
        for (int i = first; i < m; ++i) {
            const T *Li = L + (size_t)i * m;
            if (w == 4 && s[3] == 0) {
                T a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                for (int k = 0; k < i; ++k) {
                    const T l = Li[k];
                    a0 += l * x[0][k];
                    a1 += l * x[1][k];
                    a2 += l * x[2][k];
                    a3 += l * x[3][k];
                }
                x[0][i] = (x[0][i] - a0) / Li[i];
                x[1][i] = (x[1][i] - a1) / Li[i];
                x[2][i] = (x[2][i] - a2) / Li[i];
                x[3][i] = (x[3][i] - a3) / Li[i];
            } else {
                for (int u = 0; u < w; ++u) {
                    if (i < s[u]) continue;
                    T a = 0;
                    for (int k = s[u]; k < i; ++k) a += Li[k] * x[u][k];
                    x[u][i] = (x[u][i] - a) / Li[i];
                }
            }
        }
    }
}

template <typename T>
int update_core_t(int n, int m, const double *P, const int32_t *row_start, const int32_t *col, const double *val, const double *res,
                  const double *R, T *A, T *S, T *L, T *W, T *B, T *z, T *dx, T *P6, int threads)
{
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    // ---- A = H P
#pragma omp parallel for schedule(static) num_threads(threads)
    for (int i = 0; i < m; ++i) {
        T *Ai = A + (size_t)i * n;
        for (int c = 0; c < n; ++c) {
            T a = 0;
            for (int k = row_start[i]; k < row_start[i + 1]; ++k) a += (T)val[k] * (T)P[(size_t)col[k] * n + c];
            Ai[c] = a;
        }
    }
    // ---- S = A H' + R, upper triangle mirrored
#pragma omp parallel for schedule(dynamic, 8) num_threads(threads)
    for (int i = 0; i < m; ++i)
        for (int j = i; j < m; ++j) {
            T a = 0;
            for (int k = row_start[j]; k < row_start[j + 1]; ++k) a += A[(size_t)i * n + col[k]] * (T)val[k];
            S[(size_t)i * m + j] = S[(size_t)j * m + i] = a + (T)R[(size_t)i * m + j];
        }
    // ---- L L' = S by columns
    for (size_t k = 0; k < (size_t)m * m; ++k) L[k] = 0;
    for (int j = 0; j < m; ++j) {
        const T *Lj = L + (size_t)j * m;
        T d = 0;
        for (int k = 0; k < j; ++k) d += Lj[k] * Lj[k];
        d = S[(size_t)j * m + j] - d;
        if (!(d > 0)) return 1 + j;
        const T ljj = std::sqrt(d);
        L[(size_t)j * m + j] = ljj;
#pragma omp parallel for schedule(static) num_threads(threads) if (j >= 64)
        for (int i = j + 1; i < m; ++i) {
            T *Li = L + (size_t)i * m;
            T a = 0;
            for (int k = 0; k < j; ++k) a += Li[k] * Lj[k];
            Li[j] = (S[(size_t)i * m + j] - a) / ljj;
        }
    }
    // ---- z and B: columns of the transposed right-hand side [n + 1][m], the last one the residual
    std::vector<T> Xt((size_t)(n + 1) * m);
#pragma omp parallel for schedule(static) num_threads(threads)
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < m; ++i) Xt[(size_t)c * m + i] = A[(size_t)i * n + c];
    for (int i = 0; i < m; ++i) Xt[(size_t)n * m + i] = (T)res[i];
    forward_columns(L, m, Xt.data(), n + 1, nullptr, threads);
    for (int i = 0; i < m; ++i) z[i] = Xt[(size_t)n * m + i];
#pragma omp parallel for schedule(static) num_threads(threads)
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < n; ++c) B[(size_t)i * n + c] = Xt[(size_t)c * m + i];
    // ---- dx = B' z
#pragma omp parallel for schedule(static) num_threads(threads)
    for (int c = 0; c < n; ++c) {
        T a = 0;
        for (int k = 0; k < m; ++k) a += Xt[(size_t)c * m + k] * z[k];
        dx[c] = a;
    }
    // ---- W = inv(L): L W = I, column c starts at row c
    {
        std::vector<T> Wt((size_t)m * m, (T)0);
        std::vector<int> k0(m);
        for (int c = 0; c < m; ++c) {
            Wt[(size_t)c * m + c] = 1;
            k0[c] = c;
        }
        forward_columns(L, m, Wt.data(), m, k0.data(), threads);
#pragma omp parallel for schedule(static) num_threads(threads)
        for (int i = 0; i < m; ++i)
            for (int c = 0; c < m; ++c) W[(size_t)i * m + c] = Wt[(size_t)c * m + i];
    }
    // ---- P6 = mirror_upper(P / 2 + P' / 2 - B'B): tiles of TI x TI entries of the upper triangle, k in chunks of KC with the
    // accumulators kept between chunks (one ascending sum per entry)
    constexpr int TI = 32, KC = 512;
    const int nt = (n + TI - 1) / TI;
    const long long pairs = (long long)nt * (nt + 1) / 2;
#pragma omp parallel num_threads(threads)
    {
        std::vector<T> acc((size_t)TI * TI);
#pragma omp for schedule(dynamic, 1)
        for (long long t = 0; t < pairs; ++t) {
            int ti = 0;
            long long left = t;
            while (left >= nt - ti) { // row ti of the tile triangle holds nt - ti tiles
                left -= nt - ti;
                ++ti;
            }
            const int tj = ti + (int)left;
            const int i0 = ti * TI, i1 = i0 + TI < n ? i0 + TI : n, j0 = tj * TI, j1 = j0 + TI < n ? j0 + TI : n;
            for (size_t q = 0; q < acc.size(); ++q) acc[q] = 0;
            for (int kc = 0; kc < m; kc += KC) {
                const int ke = kc + KC < m ? kc + KC : m;
                for (int i = i0; i < i1; ++i) {
                    const T *bi = &Xt[(size_t)i * m];
                    int j = j0;
                    for (; j + 4 <= j1; j += 4) {
                        T *a = &acc[(size_t)(i - i0) * TI + (j - j0)];
                        T a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
                        const T *b0 = &Xt[(size_t)j * m], *b1 = b0 + m, *b2 = b1 + m, *b3 = b2 + m;
                        for (int k = kc; k < ke; ++k) {
                            const T v = bi[k];
                            a0 += v * b0[k];
                            a1 += v * b1[k];
                            a2 += v * b2[k];
                            a3 += v * b3[k];
                        }
                        a[0] = a0; a[1] = a1; a[2] = a2; a[3] = a3;
                    }
                    for (; j < j1; ++j) {
                        T a = acc[(size_t)(i - i0) * TI + (j - j0)];
                        const T *b0 = &Xt[(size_t)j * m];
                        for (int k = kc; k < ke; ++k) a += bi[k] * b0[k];
                        acc[(size_t)(i - i0) * TI + (j - j0)] = a;
                    }
                }
            }
            for (int i = i0; i < i1; ++i)
                for (int j = (j0 > i ? j0 : i); j < j1; ++j) {
                    const T v = (T)0.5 * (T)P[(size_t)i * n + j] + (T)0.5 * (T)P[(size_t)j * n + i] - acc[(size_t)(i - i0) * TI + (j - j0)];
                    P6[(size_t)i * n + j] = P6[(size_t)j * n + i] = v;
                }
        }
    }
    return 0;
}

} // namespace

extern "C" {
int urld_mant_dig(void) { return LDBL_MANT_DIG; }
int urld_sizeof_long_double(void) { return (int)sizeof(long double); }
// 1.0L / 3 into the caller's 16 bytes: the wrapper compares them with numpy's own (the same layout, not only the same size)
void urld_third(void *out)
{
    const long double v = 1.0L / 3.0L;
    std::memset(out, 0, sizeof(long double));
    std::memcpy(out, &v, 10);
}
// -> 0, or 1 + j when the pivot of column j is not positive
int urld_update_core_ld(int n, int m, const double *P, const int32_t *row_start, const int32_t *col, const double *val, const double *res,
                        const double *R, long double *A, long double *S, long double *L, long double *W, long double *B, long double *z,
                        long double *dx, long double *P6, int threads)
{
    return update_core_t<long double>(n, m, P, row_start, col, val, res, R, A, S, L, W, B, z, dx, P6, threads);
}
int urld_update_core_f64(int n, int m, const double *P, const int32_t *row_start, const int32_t *col, const double *val, const double *res,
                         const double *R, double *A, double *S, double *L, double *W, double *B, double *z, double *dx, double *P6,
                         int threads)
{
    return update_core_t<double>(n, m, P, row_start, col, val, res, R, A, S, L, W, B, z, dx, P6, threads);
}
}

#ifdef UPDATE_REF_LD_MAIN
// n = 40, m = 10: a diagonally dominant P, rows of 13 + 3 entries as visual_rows lays them out.  Checks L L' = S, L B = A, L W = I and
// the symmetry of P6 to a few units of the type, in both instances, with 1 and 3 threads; meant to be run under ASan + UBSan.
template <typename T>
static int run_one(int threads, const char *name, T eps)
{
    const int n = 40, m = 10, per = 16;
    std::vector<double> P((size_t)n * n), val((size_t)m * per), res(m), R((size_t)m * m, 0.0);
    std::vector<int32_t> rs(m + 1), col((size_t)m * per);
    uint32_t h = 12345u;
    auto rnd = [&]() { h = h * 1664525u + 1013904223u; return (double)(h >> 8) / 16777216.0 - 0.5; };
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) P[(size_t)i * n + j] = P[(size_t)j * n + i] = i == j ? 2.0 + rnd() : 0.02 * rnd();
    for (int i = 0; i < m; ++i) {
        rs[i] = i * per;
        const int f = 13 + 3 * (i / 2 + 2 * (i % 3)); // a feature's three columns, below n
        for (int k = 0; k < per; ++k) {
            col[(size_t)i * per + k] = k < 13 ? k : f + k - 13;
            val[(size_t)i * per + k] = rnd();
        }
        res[i] = rnd();
        R[(size_t)i * m + i] = 0.25;
    }
    rs[m] = m * per;
    std::vector<T> A((size_t)m * n), S((size_t)m * m), L((size_t)m * m), W((size_t)m * m), B((size_t)m * n), z(m), dx(n), P6((size_t)n * n);
    const int rc = update_core_t<T>(n, m, P.data(), rs.data(), col.data(), val.data(), res.data(), R.data(), A.data(), S.data(), L.data(),
                                    W.data(), B.data(), z.data(), dx.data(), P6.data(), threads);
    if (rc != 0) {
        std::printf("%s: pivot %d not positive\n", name, rc - 1);
        return 1;
    }
    T worst = 0;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            T s = 0, w = 0;
            for (int k = 0; k < m; ++k) {
                s += L[(size_t)i * m + k] * L[(size_t)j * m + k];
                w += L[(size_t)i * m + k] * W[(size_t)k * m + j];
            }
            worst = std::fmax(worst, std::fabs(s - S[(size_t)i * m + j]));
            worst = std::fmax(worst, std::fabs(w - (i == j ? (T)1 : (T)0)));
        }
        for (int c = 0; c < n; ++c) {
            T s = 0;
            for (int k = 0; k <= i; ++k) s += L[(size_t)i * m + k] * B[(size_t)k * n + c];
            worst = std::fmax(worst, std::fabs(s - A[(size_t)i * n + c]));
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (P6[(size_t)i * n + j] != P6[(size_t)j * n + i]) worst = 1;
    std::printf("%s, %d thread(s): worst residual %.3Le\n", name, threads, (long double)worst);
    return worst <= 200 * eps ? 0 : 1;
}

int main()
{
    int bad = 0;
    for (int threads : {1, 3}) {
        bad += run_one<long double>(threads, "long double", LDBL_EPSILON);
        bad += run_one<double>(threads, "double", (double)DBL_EPSILON);
    }
    if (bad) return 1;
    std::printf("update_ref_ld_check: ok\n");
    return 0;
}
#endif
