// kernels_external.hip -- EKF update with an external, linearised measurement (ekf_update_external; gfx950).
//
// H arrives as m <= 16 sparse rows over state indices (ExtCtl, engine.h).  With S = H P H' + R = L L':
//     A = H P,  z = inv(L) residual,  B = inv(L) A,  x += B'z,  P <- 0.5 (P + P') - B'B,  normalizeCovariance
// -- update_algorithmic and the tail of orc_update (oracle/ekf_oracle.c) with a general H.  All arithmetic is fp64; T is the
// storage type of P (an fp32 entry widens exactly, a result is rounded to T once).  Five launches on the engine's stream, ordered
// by launch order alone: no workgroup waits for another and nothing is added atomically.
//
//   k_ext_rows      A = H P, one thread per column, and in one extra workgroup per row the entries A[i, col_e] that S reads
//   k_ext_solve     every workgroup forms and factorises the <= 16 x 16 S in LDS (a few thousand flops: cheaper than a hand-off),
//                   reaches the same verdict, and substitutes its own 256 columns of B and of dx; workgroup 0 leaves the record
//   k_ext_state     x += dx with the reference's dead-band, quaternion normalisation (k_state_apply's arithmetic)
//   k_ext_downdate  P <- 0.5 (P + P') - B'B over upper-triangle tiles, each element and its mirror written once: bandwidth-bound
//   k_ext_normalize normalizeCovariance on rows / columns 3..6 (k_normalize_cov's arithmetic)
//
// A gate that rejects, or an S that is not positive definite, is the solve kernel's verdict in ExtResult: the kernels behind it read
// it and return (the pattern of filter_frozen), so x, P and the map stay as they were, bit for bit.  The engine's sticky error flag
// is not involved.  Not available on a sharded engine: every row of P is local.
#include "engine.h"

namespace ekf {

constexpr int XT = 64; // tile side of the downdate

// ------------------------------------------------------------------------------------------------------- A = H P
// grid (ceil(n / 256) + 1, m).  A[i][j] = sum_k val_k P[col_k][j], k in CSR order: every read runs along j.  The last workgroup
// of a row forms the same sums at the columns H itself names (sel[i][e] = A[i][col_e] for every entry e of every row): S = A H'
// needs nothing else, and the solve can then overwrite A with B while other workgroups still form S.
template <typename T>
__global__ void __launch_bounds__(256)
k_ext_rows(const T *__restrict__ P, int ld, int n, const ExtCtl *__restrict__ ctl, double *__restrict__ A, int lda,
           double *__restrict__ sel)
{
    const int i = blockIdx.y;
    const int k0 = ctl->row_start[i], k1 = ctl->row_start[i + 1];
    if (blockIdx.x + 1 < gridDim.x) {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j >= n) return;
        double s = 0.0;
        for (int k = k0; k < k1; ++k) s += ctl->val[k] * (double)P[(size_t)ctl->col[k] * ld + j];
        A[(size_t)i * lda + j] = s;
        return;
    }
    const int total = ctl->row_start[ctl->m];
    for (int e = threadIdx.x; e < total; e += 256) {
        const int j = ctl->col[e];
        double s = 0.0;
        for (int k = k0; k < k1; ++k) s += ctl->val[k] * (double)P[(size_t)ctl->col[k] * ld + j];
        sel[i * EXT_ENTRIES + e] = s;
    }
}

// ---------------------------------------------------------------------------------------------- S, L, z, B and dx
// grid ceil(n / 256).  S[i][j] = sum_k A[i][col_jk] val_jk + R[i][j] for i <= j, mirrored; lower Cholesky factor by columns in the
// order of update_algorithmic (a pivot that is not > 0: EXT_NOT_PD); z = inv(L) residual, nis = z'z; then every thread substitutes
// its own column of B = inv(L) A in registers, writes it over A and forms dx_j = sum_k B[k][j] z[k], k ascending.
__global__ void __launch_bounds__(256)
k_ext_solve(const ExtCtl *__restrict__ ctl, ExtResult *res, double *A, int lda, const double *__restrict__ sel, double *dx, int n)
{
    __shared__ double L[EXT_ROWS][EXT_ROWS + 1];
    __shared__ double z[EXT_ROWS], dinv[EXT_ROWS];
    __shared__ int verdict;
    const int tid = threadIdx.x, m = ctl->m;
    {
        const int i = tid >> 4, j = tid & 15;
        if (i <= j && j < m) {
            double s = 0.0;
            for (int k = ctl->row_start[j]; k < ctl->row_start[j + 1]; ++k) s += sel[i * EXT_ENTRIES + k] * ctl->val[k];
            s += ctl->R[i * EXT_ROWS + j];
            L[i][j] = s;
            L[j][i] = s;
        }
        if (tid == 0) verdict = EXT_APPLIED;
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) { // (m and the verdict are the same in every thread: the barriers are met by all)
        if (tid == 0) {
            double d = L[j][j];
            for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
            if (!(d > 0.0)) verdict = EXT_NOT_PD;
            else L[j][j] = sqrt(d);
        }
        __syncthreads();
        if (verdict != EXT_APPLIED) break;
        if (tid > j && tid < m) {
            double s = L[tid][j];
            for (int k = 0; k < j; ++k) s -= L[tid][k] * L[j][k];
            L[tid][j] = s / L[j][j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double nis = 0.0;
        for (int i = 0; i < EXT_ROWS; ++i) z[i] = 0.0;
        if (verdict == EXT_APPLIED) {
            for (int i = 0; i < m; ++i) {
                double zi = ctl->residual[i];
                for (int k = 0; k < i; ++k) zi -= L[i][k] * z[k];
                z[i] = zi / L[i][i];
                dinv[i] = 1.0 / L[i][i];
            }
            for (int i = 0; i < m; ++i) nis += z[i] * z[i];
            if (ctl->gate_nis > 0.0 && !(nis <= ctl->gate_nis)) verdict = EXT_GATED;
        }
        if (blockIdx.x == 0) {
            res->out.nis = nis;
            for (int i = 0; i < EXT_ROWS; ++i) res->out.z[i] = z[i];
            res->out.rows = m;
            res->out.applied = verdict == EXT_APPLIED ? 1 : 0;
            res->verdict = verdict;
        }
    }
    __syncthreads();
    if (verdict != EXT_APPLIED) return;
    const int j = blockIdx.x * 256 + tid;
    if (j >= n) return;
    double b[EXT_ROWS], d = 0.0;
#pragma unroll
    for (int i = 0; i < EXT_ROWS; ++i) {
        b[i] = 0.0;
        if (i < m) {
            double s = A[(size_t)i * lda + j];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= L[i][k] * b[k];
            b[i] = s * dinv[i];
            A[(size_t)i * lda + j] = b[i];
        }
    }
#pragma unroll
    for (int k = 0; k < EXT_ROWS; ++k)
        if (k < m) d += b[k] * z[k];
    dx[j] = d;
}

// -------------------------------------------------------------------------------------------------- x += dx
// stateUpdate (Update.cpp:147-204) and the quaternion normalisation behind it, as k_state_apply does them for a covariance
// update: the dead-band on every component, then J, q /= |q| and R(q) (quat_norm_dev).  One thread per feature parameter;
// thread 0 also takes the camera.
__global__ void __launch_bounds__(256)
k_ext_state(double *st, double *feat_pos, const int *feat_type, const int *feat_covpos, int N, const double *__restrict__ dx,
            const ExtResult *res)
{
    if (res->verdict != EXT_APPLIED) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        double *x = st + ST_X;
        for (int i = 0; i < 13; ++i)
            if (fabs(dx[i]) > EKF_DELTA) x[i] += dx[i];
        quat_norm_dev(st);
    }
    if (t >= N * 6 || (t % 6) >= feat_dim(feat_type[t / 6])) return;
    const double s = dx[feat_covpos[t / 6] + t % 6];
    if (fabs(s) > EKF_DELTA) feat_pos[t] += s;
}

// ------------------------------------------------------------------------------------- P <- 0.5 (P + P') - B'B
// One workgroup per upper-triangle tile (I, J), I <= J, of XT x XT elements; wave w takes the rows w, w + 4, ... of the tile and
// lane c its column c, so every global access runs along a row.  The tile's XT columns of B sit in the lanes' registers, its XT
// rows of B in LDS (one row of 16 doubles per tile row, read as a broadcast).  The mirror tile (J, I) is read along its rows into
// LDS, the averaged and downdated element replaces it there, and the tile is written back along its rows: P is read once and
// written once, each pair i <= j computed once and stored in both places.  A diagonal tile computes i <= j and writes back its
// strictly lower part.  Rows of B at or beyond m enter as zeros (m is not a compile-time constant; the sum has 16 terms).
// Elements at or beyond n are neither read nor written.
template <typename T>
__global__ void __launch_bounds__(256)
k_ext_downdate(T *P, int ld, int n, const double *__restrict__ B, int ldb, const ExtCtl *__restrict__ ctl, const ExtResult *res)
{
    if (res->verdict != EXT_APPLIED) return;
    __shared__ __align__(16) double Bi[XT][EXT_ROWS];
    __shared__ T Mt[XT][XT + 1];
    const int m = ctl->m;
    const int bid = blockIdx.x;
    int J = (int)((sqrt(8.0 * (double)bid + 1.0) - 1.0) * 0.5);
    while ((J + 1) * (J + 2) / 2 <= bid) ++J;
    while (J * (J + 1) / 2 > bid) --J;
    const int I = bid - J * (J + 1) / 2;
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = I * XT, j0 = J * XT;
    const bool diag = I == J;
    double bj[EXT_ROWS];
#pragma unroll
    for (int k = 0; k < EXT_ROWS; ++k) bj[k] = (k < m && j0 + c < n) ? B[(size_t)k * ldb + j0 + c] : 0.0;
#pragma unroll
    for (int q = 0; q < EXT_ROWS / 4; ++q) {
        const int k = w + 4 * q;
        Bi[c][k] = (k < m && i0 + c < n) ? B[(size_t)k * ldb + i0 + c] : 0.0;
    }
#pragma unroll 4
    for (int p = 0; p < XT / 4; ++p) {
        const int rr = w + 4 * p;
        Mt[rr][c] = (j0 + rr < n && i0 + c < n) ? P[(size_t)(j0 + rr) * ld + i0 + c] : (T)0;
    }
    __syncthreads();
    const int j = j0 + c;
#pragma unroll 4
    for (int p = 0; p < XT / 4; ++p) {
        const int ii = w + 4 * p, i = i0 + ii;
        if (i < n && j < n && (!diag || ii <= c)) {
            const double u = (double)P[(size_t)i * ld + j], v = (double)Mt[c][ii];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < EXT_ROWS; ++k) s += Bi[ii][k] * bj[k];
            const T o = (T)((0.5 * u + 0.5 * v) - s);
            P[(size_t)i * ld + j] = o;
            Mt[c][ii] = o;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int p = 0; p < XT / 4; ++p) {
        const int rr = w + 4 * p;
        if (j0 + rr < n && i0 + c < n && (!diag || rr > c)) P[(size_t)(j0 + rr) * ld + i0 + c] = Mt[rr][c];
    }
}

// ------------------------------------------------------------------------------------------ normalizeCovariance
// P <- D P D', D = diag(I3, J, I) (Update.cpp:64-85) with k_normalize_cov's arithmetic on an unsharded P: block 0 owns the 7 x 7
// corner pieces, every other thread column j of the row strip 3..6 and row j of the column strip.
template <typename T>
__global__ void __launch_bounds__(256) k_ext_normalize(T *P, int ld, int n, const double *st, const ExtResult *res)
{
    __shared__ double J[16];
    __shared__ double C[7][7];
    const int tid = threadIdx.x;
    if (res->verdict != EXT_APPLIED) return;
    if (tid < 16) J[tid] = st[ST_JN + tid];
    if (blockIdx.x == 0) {
        if (tid < 49) C[tid / 7][tid % 7] = (double)P[(size_t)(tid / 7) * ld + tid % 7];
        __syncthreads();
        if (tid < 12) { // P[0:3,3:7] J'
            const int i = tid / 4, a = tid % 4;
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += C[i][3 + k] * J[a * 4 + k];
            P[(size_t)i * ld + 3 + a] = (T)s;
        } else if (tid < 24) { // J P[3:7,0:3]
            const int t = tid - 12, a = t / 3, j = t % 3;
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += J[a * 4 + k] * C[3 + k][j];
            P[(size_t)(3 + a) * ld + j] = (T)s;
        } else if (tid < 40) { // J P[3:7,3:7] J' : upper triangle, mirrored (keeps P bitwise symmetric)
            const int t = tid - 24, a = t / 4, b = t % 4;
            if (a <= b) {
                double s = 0.0;
                for (int l = 0; l < 4; ++l) {
                    double u = 0.0;
                    for (int k = 0; k < 4; ++k) u += J[a * 4 + k] * C[3 + k][3 + l];
                    s += u * J[b * 4 + l];
                }
                P[(size_t)(3 + a) * ld + 3 + b] = (T)s;
                P[(size_t)(3 + b) * ld + 3 + a] = (T)s;
            }
        }
        return;
    }
    __syncthreads();
    const int j = 7 + (blockIdx.x - 1) * 256 + tid;
    if (j >= n) return;
    T *prow = P + (size_t)j * ld;
    double col[4], row[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        col[k] = (double)P[(size_t)(3 + k) * ld + j];
        row[k] = (double)prow[3 + k];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double s = 0.0, t = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s += J[a * 4 + k] * col[k];
            t += row[k] * J[a * 4 + k];
        }
        P[(size_t)(3 + a) * ld + j] = (T)s;
        prow[3 + a] = (T)t;
    }
}

template <typename T>
static void external_update_t(EkfEngine *e, int m)
{
    hipStream_t s = e->stream;
    const int n = e->n, ld = e->ldP, nb = (n + 255) / 256;
    T *P = (T *)e->d.P;
    double *A = e->d.ext_A, *dx = A + (size_t)EXT_ROWS * ld;
    k_ext_rows<T><<<dim3(nb + 1, m), 256, 0, s>>>(P, ld, n, e->d.ext_ctl, A, ld, e->d.ext_sel);
    k_ext_solve<<<nb, 256, 0, s>>>(e->d.ext_ctl, e->d.ext_res, A, ld, e->d.ext_sel, dx, n);
    const int nt = max(e->N * 6, 1);
    k_ext_state<<<(nt + 255) / 256, 256, 0, s>>>(e->d.state, e->d.feat_pos, e->d.feat_type, e->d.feat_covpos, e->N, dx, e->d.ext_res);
    const int tiles = (n + XT - 1) / XT;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing) { // the downdate's bracket joins the P-update log (ekf_timing_p_update_launches)
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, s);
    }
    k_ext_downdate<T><<<tiles * (tiles + 1) / 2, 256, 0, s>>>(P, ld, n, A, ld, e->d.ext_ctl, e->d.ext_res);
    if (e->timing) {
        (void)hipEventRecord(e1, s);
        e->pu_events.push_back(PuBracket{e0, e1, (double)n * (double)n * (double)m, m});
    }
    k_ext_normalize<T><<<1 + (n > 7 ? (n - 7 + 255) / 256 : 0), 256, 0, s>>>(P, ld, n, e->d.state, e->d.ext_res);
}

void launch_external_update(EkfEngine *e, int m)
{
    if (e->f32) external_update_t<float>(e, m);
    else external_update_t<double>(e, m);
}

} // namespace ekf
