// kernels_fixedmap.hip -- the Schmidt-Kalman ("consider") camera update on a fixed map (ekf_update_fixed_map; gfx950).
//
// The gain rows of the map states are zero: K = [K_c; 0].  The map still enters S = H P H' + R with its full uncertainty and its
// correlations; with the optimal K_c the Joseph form reduces to the camera's strip of the full update,
//     x[0:13]   += B_c' z                          B = inv(L) H P, B_c its first 13 columns, z = inv(L) nu
//     P[0:13,:] <- (0.5 P + 0.5 P')[0:13,:] - B_c' B,   P[:,0:13] its transpose,   P[13:,13:] and the map: not written
// followed by normalizeCovariance on rows / columns 3..6.  S, L, nu and z are those of ekf_update (the launcher of
// kernels_update.hip runs the same gather, assembly and sweep); everything here is fp64 arithmetic, T is the storage type of P (an
// fp32 entry widens exactly, a result is rounded to T after the downdate and after the normalisation, as kernels_external.hip does).
//
// The strip is a skinny product Y' X, Y of m x 13 and X of m x n, 13 FMA per 8-byte load of X (3.25 flop / byte: bound by reading X
// once from HBM):
//   up to B_SWEEP_MAX rows, below 8192 state columns   the sweep formed the fp64 rows of B in d.A:   Y = B[:, 0:13],  X = B
//   otherwise (update_route.h)   inv(L) exists (V = inv(L), W = V'), B does not:   B_c = V G[:, 0:13],  K_c' = W B_c  (k_fm_gain,
//                                2 x 13 m^2 flop instead of the m x m x n product),  Y = K_c',  X = G, the gathered rows of H P
//
//   k_fm_gain   one wavefront per 4 rows of V (or W): the m x 13 tables B_c and K_c'
//   k_fm_strip  partial sums of Y' X: one thread per state column, 13 accumulators, the rows cut into FM_SPLIT slices (grid.y)
//   k_fm_tail   sums the slices in ascending order, downdates the strip, forms dx = B_c' z, applies the camera state with its
//               dead-band, normalises the quaternion and applies normalizeCovariance -- each element and its mirror written once
//
// Nothing is added atomically and no workgroup waits for another: the same inputs give the same bits.  The tail leaves x and P alone
// when the sweep failed (filter_frozen, engine.h).  Unsharded engines only: every row of P is local.
#include "engine.h"

namespace ekf {

constexpr int FM_SPLIT = DX_SPLIT; // row slices of the strip product (d.cam_part holds DX_SPLIT x 13 x ldP partial sums)
constexpr int FM_CH = 32;          // rows of Y staged in LDS (and of X requested) at a time

// ------------------------------------------------------------------------------------------- B_c and K_c'
// grid ceil(m / 16); wavefront w of a workgroup owns rows i0 + 4 w .. + 3, lane l the entries k = k0 + l of a 64-wide chunk of
// them, 4 x 13 accumulators per lane, one butterfly sum per accumulator at the end.  The chunk's 64 x 13 entries of the right-hand
// table are staged in LDS once for the workgroup's 16 rows.
//   PHASE 0: out[i][c] = sum_{k <= i}     Mx[i][k] Yin[k][c]      Mx = V = inv(L),  Yin = G (leading dimension ldin), out = B_c
//   PHASE 1: out[i][c] = sum_{i <= k < m} Mx[i][k] Yin[k][c]      Mx = W = inv(L)', Yin = B_c,                        out = K_c'
// Entries of Mx outside the triangle named are not read (V's other triangle is scratch of the inversion).
template <int PHASE>
__global__ void __launch_bounds__(256)
k_fm_gain(const double *__restrict__ Mx, int ldw, const double *__restrict__ Yin, int ldin, double *__restrict__ out, int m)
{
    __shared__ double sY[64][14];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i0 = blockIdx.x * 16;
    const int klo = PHASE == 0 ? 0 : i0 / 64 * 64, khi = PHASE == 0 ? min(m, i0 + 16) : m;
    double acc[4][13];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 13; ++c) acc[r][c] = 0.0;
    for (int k0 = klo; k0 < khi; k0 += 64) {
        __syncthreads();
        for (int i = tid; i < 64 * 13; i += 256) {
            const int r = i / 13, c = i % 13;
            sY[r][c] = k0 + r < khi ? Yin[(size_t)(k0 + r) * ldin + c] : 0.0;
        }
        __syncthreads();
        const int k = k0 + lane;
        double y[13], v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * wv + r;
            const bool live = i < m && k < khi && (PHASE == 0 ? k <= i : k >= i);
            v[r] = live ? Mx[(size_t)i * ldw + k] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < 13; ++c) y[c] = sY[lane][c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 13; ++c) acc[r][c] += v[r] * y[c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * wv + r;
#pragma unroll
        for (int c = 0; c < 13; ++c) {
            const double s = wave_sum(acc[r][c]);
            if (lane == 0 && i < m) out[(size_t)i * FM_LD + c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------- partial sums of Y' X
// grid (ceil(n / 256), FM_SPLIT).  Thread j of slice ks: part[ks][c][j] = sum_k Y[k][c] X[k][j] over the slice's rows, k ascending,
// c = 0..12 in registers.  The 13 values Y[k][.] of a row are the same for every column: a chunk of FM_CH rows of them is staged in
// LDS once per workgroup and read back as broadcasts; the chunk's FM_CH entries of X are requested together, ahead of the staging
// (one round trip to memory per chunk, as k_dx_partial does it).  X is read once, along the state columns.
// Workgroup (0, 0) also keeps the camera state as it is before the update for the tail (FmCtl).
__global__ void __launch_bounds__(256)
k_fm_strip(const double *__restrict__ Y, int ldy, const double *__restrict__ X, int ldx, int m, int n, double *__restrict__ part,
           int ldp, const double *__restrict__ st, FmCtl *__restrict__ ctl)
{
    __shared__ __align__(16) double sY[FM_CH][14];
    const int tid = threadIdx.x;
    const int j = blockIdx.x * 256 + tid, ks = blockIdx.y;
    if (blockIdx.x == 0 && ks == 0 && tid < 13) ctl->x_save[tid] = st[ST_X + tid];
    const int per = (m + FM_SPLIT - 1) / FM_SPLIT;
    const int kb = ks * per, ke = min(m, kb + per);
    double acc[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) acc[c] = 0.0;
    for (int k0 = kb; k0 < ke; k0 += FM_CH) {
        const int cnt = min(FM_CH, ke - k0);
        // the chunk's entries of X are requested BEFORE the rows of Y are staged: one round trip to memory per chunk, not two
        double xv[FM_CH];
#pragma unroll
        for (int u = 0; u < FM_CH; ++u) xv[u] = j < n ? X[(size_t)(k0 + min(u, cnt - 1)) * ldx + j] : 0.0;
        __syncthreads();
        for (int i = tid; i < FM_CH * 13; i += 256) {
            const int r = i / 13, c = i % 13;
            sY[r][c] = r < cnt ? Y[(size_t)(k0 + r) * ldy + c] : 0.0;
        }
        __syncthreads();
        if (j < n) {
#pragma unroll
            for (int u = 0; u < FM_CH; ++u) {
                if (u < cnt) {
#pragma unroll
                    for (int c = 0; c < 13; ++c) acc[c] += sY[u][c] * xv[u];
                }
            }
        }
    }
    if (j >= n) return;
#pragma unroll
    for (int c = 0; c < 13; ++c) part[((size_t)ks * 13 + c) * ldp + j] = acc[c];
}

// ------------------------------------------------------------------- strip downdate, camera state, normalisation
// grid ceil(n / 256); thread j owns column j of the strip's rows and row j of its columns.
//   dx_c = sum_k Yb[k][c] z[k] (Yb = B_c: the first columns of B, or the table of k_fm_gain): every workgroup forms all 13 sums, in
//     the same order -- each needs J, the Jacobian of the quaternion normalisation at the updated, un-normalised q, and workgroup 0
//     rewrites the live state meanwhile (the state as it was: FmCtl::x_save, written by k_fm_strip)
//   workgroup 0, thread 0: x += dx where |dx| > EKF_DELTA, J, q /= |q|, R(q) (quat_norm_dev's arithmetic) and the count of applied
//     updates -- stores only: what it needs of the state it has from x_save
//   strip: s = sum of the FM_SPLIT slices, ascending; o = T((0.5 P[c][j] + 0.5 P[j][c]) - s) for c <= min(j, 12) -- one value per
//     pair, so the 13 x 13 block is bitwise symmetric although K_c G is not; then D P D' (normalizeCovariance, Update.cpp:64-85) on
//     rows / columns 3..6 from the ROUNDED o, rounded to T again.  Columns j >= 13 are finished by their own thread (P[c][j] and
//     its mirror P[j][c]); the 13 x 13 block is collected in LDS and written by workgroup 0 once.
// Nothing beyond rows / columns 0..12 is written.
template <typename T>
__global__ void __launch_bounds__(256)
k_fm_tail(T *P, int ld, int n, double *st, const double *__restrict__ part, int ldp, const double *__restrict__ Yb, int ldyb,
          const double *__restrict__ z, int m, FmCtl *ctl, const int *counts)
{
    __shared__ double J[16];
    __shared__ double C[13][13];
    __shared__ double wsum[4][13];
    __shared__ double cam[13];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (filter_frozen(counts)) return; // the update's sweep failed: x and P stay as they were (engine.h)
    // everything this thread reads from memory is requested here, before the first barrier: the kernel is a chain of round trips
    // to memory, not of arithmetic (measured at N = 1000: 23 us with the loads where they are used)
    const int j = blockIdx.x * 256 + tid;
    const int cmax = min(j, 12);
    double o[13]; // (0.5 P[c][j] + 0.5 P[j][c]) - sum of the slices, before its rounding
#pragma unroll
    for (int c = 0; c < 13; ++c) {
        o[c] = 0.0;
        if (j < n && c <= cmax) {
            double s = 0.0;
#pragma unroll
            for (int ks = 0; ks < FM_SPLIT; ++ks) s += part[((size_t)ks * 13 + c) * ldp + j];
            const double u = (double)P[(size_t)c * ld + j], v = (double)P[(size_t)j * ld + c];
            o[c] = (0.5 * u + 0.5 * v) - s;
        }
    }
    double xs = 0.0;
    if (tid < 13) xs = ctl->x_save[tid];
    {
        double a[13];
#pragma unroll
        for (int c = 0; c < 13; ++c) a[c] = 0.0;
        for (int k = tid; k < m; k += 256) {
            const double zk = z[k];
#pragma unroll
            for (int c = 0; c < 13; ++c) a[c] += Yb[(size_t)k * ldyb + c] * zk;
        }
#pragma unroll
        for (int c = 0; c < 13; ++c) {
            const double s = wave_sum(a[c]);
            if (lane == 0) wsum[wv][c] = s;
        }
    }
    __syncthreads();
    if (tid < 13) { // the camera state with its dead-band: x as it was (FmCtl::x_save) + dx
        const double d = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
        cam[tid] = fabs(d) > EKF_DELTA ? xs + d : xs;
    }
    __syncthreads();
    if (tid == 0) {
        // J from the un-normalised q, then q /= |q| and R(q): quat_norm_dev's arithmetic (engine.h) on registers -- every workgroup
        // forms the same J; workgroup 0 also stores the state, and loads nothing of it
        const double r = cam[3], x = cam[4], y = cam[5], zz = cam[6];
        const double nrm = sqrt(r * r + x * x + y * y + zz * zz);
        const double a = 1.0 / (nrm * nrm * nrm);
        const double M[16] = {x * x + y * y + zz * zz, -r * x, -r * y, -r * zz,
                              -x * r, r * r + y * y + zz * zz, -x * y, -x * zz,
                              -y * r, -y * x, r * r + x * x + zz * zz, -y * zz,
                              -zz * r, -zz * x, -zz * y, r * r + x * x + y * y};
        for (int i = 0; i < 16; ++i) J[i] = M[i] * a;
        if (blockIdx.x == 0) {
            double xn[13], R[9];
            for (int i = 0; i < 13; ++i) xn[i] = cam[i];
            xn[3] = r / nrm; xn[4] = x / nrm; xn[5] = y / nrm; xn[6] = zz / nrm;
            quat_to_rot(xn + 3, R);
            for (int i = 0; i < 13; ++i) st[ST_X + i] = xn[i];
            for (int i = 0; i < 9; ++i) st[ST_R + i] = R[i];
            for (int i = 0; i < 16; ++i) st[ST_JN + i] = M[i] * a;
            ctl->updates += 1;
        }
    }
    __syncthreads();
    if (j < n) {
#pragma unroll
        for (int c = 0; c < 13; ++c) o[c] = (double)(T)o[c]; // the rounding behind the downdate; the normalisation reads the rounded strip
        if (j < 13) {
#pragma unroll
            for (int c = 0; c < 13; ++c)
                if (c <= cmax) C[c][j] = C[j][c] = o[c];
        } else {
            T *prow = P + (size_t)j * ld;
#pragma unroll
            for (int c = 0; c < 13; ++c) {
                double s = o[c];
                if (c >= 3 && c < 7) {
                    s = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s += J[(c - 3) * 4 + k] * o[3 + k];
                }
                const T val = (T)s;
                P[(size_t)c * ld + j] = val;
                prow[c] = val;
            }
        }
    }
    if (blockIdx.x != 0) return;
    __syncthreads();
    if (tid < 169) {
        const int i = tid / 13, jj = tid % 13;
        const bool ri = i >= 3 && i < 7, rj = jj >= 3 && jj < 7;
        double s;
        if (ri && rj) { // J P[3:7,3:7] J': the upper-triangle value on both sides
            const int a = min(i, jj) - 3, b = max(i, jj) - 3;
            s = 0.0;
            for (int l = 0; l < 4; ++l) {
                double u = 0.0;
                for (int k = 0; k < 4; ++k) u += J[a * 4 + k] * C[3 + k][3 + l];
                s += u * J[b * 4 + l];
            }
        } else if (ri) { // J P[3:7, jj]
            s = 0.0;
            for (int k = 0; k < 4; ++k) s += J[(i - 3) * 4 + k] * C[3 + k][jj];
        } else if (rj) { // P[i, 3:7] J' (C is symmetric: the same products in the same order as its mirror)
            s = 0.0;
            for (int k = 0; k < 4; ++k) s += J[(jj - 3) * 4 + k] * C[i][3 + k];
        } else {
            s = C[i][jj];
        }
        P[(size_t)i * ld + jj] = (T)s;
    }
}

void launch_fixed_map_gain(EkfEngine *e, int m, const double *G)
{
    hipStream_t s = e->stream;
    double *Bc = e->d.fm_gain, *Kc = e->d.fm_gain + (size_t)e->fm_rows * FM_LD;
    k_fm_gain<0><<<(m + 15) / 16, 256, 0, s>>>(e->d.Dinv, e->ldW, G, e->ldP, Bc, m);
    k_fm_gain<1><<<(m + 15) / 16, 256, 0, s>>>(e->d.W, e->ldW, Bc, FM_LD, Kc, m);
}

template <typename T>
static void fixed_map_strip_t(EkfEngine *e, int m, const double *X, bool from_gain)
{
    hipStream_t s = e->stream;
    const int n = e->n, ld = e->ldP, nb = (n + 255) / 256;
    const double *Bc = from_gain ? e->d.fm_gain : (const double *)e->d.A;                 // B[:, 0:13]
    const double *Y = from_gain ? e->d.fm_gain + (size_t)e->fm_rows * FM_LD : Bc;         // K_c' above B_SWEEP_MAX rows
    const int ldy = from_gain ? FM_LD : ld;
    k_fm_strip<<<dim3(nb, FM_SPLIT), 256, 0, s>>>(Y, ldy, X, ld, m, n, e->d.cam_part, ld, e->d.state, e->d.fm_ctl);
    k_fm_tail<T><<<nb, 256, 0, s>>>((T *)e->d.P, ld, n, e->d.state, e->d.cam_part, ld, Bc, ldy, e->d.zvec, m, e->d.fm_ctl, e->d.counts);
}

void launch_fixed_map_strip(EkfEngine *e, int m, const double *X, bool from_gain)
{
    if (e->f32) fixed_map_strip_t<float>(e, m, X, from_gain);
    else fixed_map_strip_t<double>(e, m, X, from_gain);
}

} // namespace ekf
