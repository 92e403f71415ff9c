// kernels_mapblob.hip -- the device side of the map blob (ekf_save_map / ekf_load_map): the P section is packed,
// checked and unpacked here, so that one copy moves n (n + 1) / 2 elements of the storage type and the blob's checksum of P never
// needs a pass on the host.  Bandwidth kernels: grids sized from n, 16-byte accesses where the alignment allows.
#include <algorithm>

#include "engine.h"
#include "map_blob.h"

namespace ekf {

using u64 = unsigned long long;

// the share of element d of the section (32-bit words 2 d, 2 d + 1 for a double) in the section's checksum
__device__ __forceinline__ u64 elem_sum(float v, u64 d) { return (u64)__float_as_uint(v) * (2 * d + 1); }
__device__ __forceinline__ u64 elem_sum(double v, u64 d)
{
    const u64 u = (u64)__double_as_longlong(v);
    return (u & 0xffffffffull) * (4 * d + 1) + (u >> 32) * (4 * d + 3);
}

template <typename T>
struct alignas(16) Vec16 {
    T v[16 / sizeof(T)];
};

// first element of row i of the packed upper triangle
__device__ __forceinline__ u64 tri_row(int i, int n) { return (u64)i * (u64)n - (u64)i * (u64)(i > 0 ? i - 1 : 0) / 2; }

// every thread of a 256-thread block hands in its partial sums; thread 0 adds the block's to the control record (integer sums:
// the order of the atomics does not show in the result)
__device__ __forceinline__ void block_add(u64 s, unsigned a, unsigned b, MapBlobCtl *ctl)
{
    __shared__ u64 ws[4];
    __shared__ unsigned wa[4], wb[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        ws[wv] = s;
        wa[wv] = a;
        wb[wv] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 S = ws[0] + ws[1] + ws[2] + ws[3];
        const unsigned A = wa[0] + wa[1] + wa[2] + wa[3], B = wb[0] + wb[1] + wb[2] + wb[3];
        if (S) atomicAdd(&ctl->sum, S);
        if (A) atomicAdd(&ctl->non_finite, A);
        if (B) atomicAdd(&ctl->bad_diag, B);
    }
}

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// Is P bitwise symmetric?  One workgroup per pair of 64 x 64 tiles (ti, tj >= ti): tile (ti, tj) goes to LDS, tile (tj, ti) is read
// along its rows and compared with the transposed LDS tile, so both global reads are coalesced.  Read-only; counts the pairs that
// differ (the bits are compared: a NaN equals itself, -0 differs from +0).
template <typename T>
__global__ void __launch_bounds__(256) k_map_asym(const T *__restrict__ P, int ldP, int n, MapBlobCtl *ctl)
{
    __shared__ T tile[64][65];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < 64; r += 4) {
        const int i = ti * 64 + r, j = tj * 64 + c;
        tile[r][c] = i < n && j < n ? P[(size_t)i * ldP + j] : (T)0;
    }
    __syncthreads();
    unsigned diff = 0;
    for (int r = r0; r < 64; r += 4) {
        const int i = tj * 64 + r, j = ti * 64 + c; // entry (i, j) of the mirror tile against (j, i) = tile[c][r]
        if (i < n && j < n && i > j) diff += same_bits(P[(size_t)i * ldP + j], tile[c][r]) ? 0u : 1u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) diff += __shfl_down(diff, o, 64);
    if ((threadIdx.x & 63) == 0 && diff) atomicAdd(&ctl->asym, diff);
}

// One workgroup per row i of P (leading dimension ldP): columns i..n-1 (triangle) or 0..n-1 (square) go to the flat section `out`
// behind each other, and the section's checksum is accumulated on the way.  The stores are 16 bytes wide from the section's first
// aligned element of the row on; the loads too when the row's source is aligned with them (always in the square layout when n is
// a multiple of the vector).
template <typename T>
__global__ void __launch_bounds__(256) k_map_pack(const T *__restrict__ P, int ldP, int n, int layout, T *__restrict__ out, MapBlobCtl *ctl)
{
    constexpr int V = 16 / sizeof(T);
    const int i = blockIdx.x, t = threadIdx.x;
    const bool tri = layout == mapblob::P_TRIANGLE;
    const int j0 = tri ? i : 0, len = n - j0;
    const u64 o = tri ? tri_row(i, n) : (u64)i * (u64)n;
    const T *src = P + (size_t)i * ldP + j0;
    T *dst = out + o;
    const int head = min(len, (int)((V - (int)(o % V)) % V));
    const int groups = (len - head) / V, tail0 = head + groups * V;
    const bool src_aligned = (j0 + head) % V == 0;
    u64 s = 0;
    if (t < head) {
        const T v = src[t];
        dst[t] = v;
        s += elem_sum(v, o + t);
    }
    for (int g = t; g < groups; g += 256) {
        const int at = head + g * V;
        Vec16<T> x;
        if (src_aligned) x = *reinterpret_cast<const Vec16<T> *>(src + at);
        else {
#pragma unroll
            for (int a = 0; a < V; ++a) x.v[a] = src[at + a];
        }
        *reinterpret_cast<Vec16<T> *>(dst + at) = x;
#pragma unroll
        for (int a = 0; a < V; ++a) s += elem_sum(x.v[a], o + at + a);
    }
    if (tail0 + t < len) { // fewer than V elements
        const T v = src[tail0 + t];
        dst[tail0 + t] = v;
        s += elem_sum(v, o + tail0 + t);
    }
    block_add(s, 0u, 0u, ctl);
}

// Read-only pass over an uploaded P section (count elements, 16-byte aligned): its checksum, the entries that are not finite, and
// the diagonal entries that are not > 0.
template <typename T>
__global__ void __launch_bounds__(256) k_map_check(const T *__restrict__ src, int n, int layout, u64 count, MapBlobCtl *ctl)
{
    constexpr int V = 16 / sizeof(T);
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, nthreads = (u64)gridDim.x * 256;
    const u64 groups = count / V;
    u64 s = 0;
    unsigned bad = 0, diag = 0;
    for (u64 g = tid; g < groups; g += nthreads) {
        const Vec16<T> x = *reinterpret_cast<const Vec16<T> *>(src + g * V);
#pragma unroll
        for (int a = 0; a < V; ++a) {
            s += elem_sum(x.v[a], g * V + a);
            bad += isfinite(x.v[a]) ? 0u : 1u;
        }
    }
    if (tid < count - groups * V) {
        const T v = src[groups * V + tid];
        s += elem_sum(v, groups * V + tid);
        bad += isfinite(v) ? 0u : 1u;
    }
    for (u64 i = tid; i < (u64)n; i += nthreads) {
        const T v = src[layout == mapblob::P_TRIANGLE ? tri_row((int)i, n) : i * (u64)n + i];
        diag += v > (T)0 ? 0u : 1u;
    }
    block_add(s, bad, diag, ctl);
}

// One workgroup per 64 x 64 tile (ti, tj) of the engine's P: the tile is read from the section (packed triangle: tiles with
// tj >= ti only, entries on and above the diagonal; square: every tile), converted to the storage type (fp32 -> fp64 exact,
// fp64 -> fp32 rounded once to nearest) and written in rows of 16-byte stores.  For the triangle the tile also goes through LDS
// and is written transposed to its mirror place, again along rows of P (as k_convert_all_P writes its mirror): the row stride of
// 65 elements keeps both the row-wise writes and the column-wise reads of the LDS tile off each other's banks.
template <typename Ts, typename Td>
__global__ void __launch_bounds__(256) k_map_unpack(const Ts *__restrict__ src, int n, int layout, Td *__restrict__ P, int ldP)
{
    constexpr int V = 16 / sizeof(Td), TPR = 64 / V, RPP = 256 / TPR;
    __shared__ Td tile[64][65];
    const bool tri = layout == mapblob::P_TRIANGLE;
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tri && tj < ti) return;
    const int c = (threadIdx.x % TPR) * V, r0 = threadIdx.x / TPR;
    for (int r = r0; r < 64; r += RPP) {
        const int i = ti * 64 + r, j = tj * 64 + c;
        const bool whole = i < n && j + V <= n && (!tri || j >= i);
        Vec16<Td> x;
        if (whole) {
            const u64 at = tri ? tri_row(i, n) + (u64)(j - i) : (u64)i * (u64)n + (u64)j;
            if (sizeof(Ts) == sizeof(Td) && at % V == 0) {
                const Vec16<Ts> y = *reinterpret_cast<const Vec16<Ts> *>(src + at);
#pragma unroll
                for (int a = 0; a < V; ++a) x.v[a] = (Td)y.v[a];
            } else {
#pragma unroll
                for (int a = 0; a < V; ++a) x.v[a] = (Td)src[at + a];
            }
            *reinterpret_cast<Vec16<Td> *>(P + (size_t)i * ldP + j) = x;
        } else {
#pragma unroll
            for (int a = 0; a < V; ++a) {
                const int jj = j + a;
                const bool valid = i < n && jj < n && (!tri || jj >= i);
                x.v[a] = (Td)0;
                if (valid) {
                    x.v[a] = (Td)src[tri ? tri_row(i, n) + (u64)(jj - i) : (u64)i * (u64)n + (u64)jj];
                    P[(size_t)i * ldP + jj] = x.v[a];
                }
            }
        }
        if (tri) {
#pragma unroll
            for (int a = 0; a < V; ++a) tile[r][c + a] = x.v[a];
        }
    }
    if (!tri) return;
    __syncthreads();
    // the mirror: row (tj, cc) of P takes column cc of the tile
    for (int cc = r0; cc < 64; cc += RPP) {
        const int row = tj * 64 + cc;
        if (row >= n) continue;
        if (tj > ti) { // (ti * 64 + 63 < tj * 64 <= row < n: the whole 16 bytes are inside the matrix)
            Vec16<Td> x;
#pragma unroll
            for (int a = 0; a < V; ++a) x.v[a] = tile[c + a][cc];
            *reinterpret_cast<Vec16<Td> *>(P + (size_t)row * ldP + ti * 64 + c) = x;
        } else { // the diagonal tile: strictly below the diagonal only
#pragma unroll
            for (int a = 0; a < V; ++a)
                if (c + a < cc) P[(size_t)row * ldP + ti * 64 + c + a] = tile[c + a][cc];
        }
    }
}

void launch_map_asym(EkfEngine *e, MapBlobCtl *d_ctl)
{
    (void)hipMemsetAsync(d_ctl, 0, sizeof(MapBlobCtl), e->stream);
    const int nt = (e->n + 63) / 64;
    const dim3 g(nt, nt);
    if (e->f32) k_map_asym<float><<<g, 256, 0, e->stream>>>((const float *)e->d.P, e->ldP, e->n, d_ctl);
    else k_map_asym<double><<<g, 256, 0, e->stream>>>((const double *)e->d.P, e->ldP, e->n, d_ctl);
}

void launch_map_pack(EkfEngine *e, int layout, void *staging, MapBlobCtl *d_ctl)
{
    (void)hipMemsetAsync(d_ctl, 0, sizeof(MapBlobCtl), e->stream);
    if (e->f32) k_map_pack<float><<<e->n, 256, 0, e->stream>>>((const float *)e->d.P, e->ldP, e->n, layout, (float *)staging, d_ctl);
    else k_map_pack<double><<<e->n, 256, 0, e->stream>>>((const double *)e->d.P, e->ldP, e->n, layout, (double *)staging, d_ctl);
}

void launch_map_check(EkfEngine *e, const void *staging, int n, int elem_bytes, int layout, MapBlobCtl *d_ctl)
{
    (void)hipMemsetAsync(d_ctl, 0, sizeof(MapBlobCtl), e->stream);
    const u64 count = mapblob::p_elements(n, layout);
    const u64 groups = count / (16 / elem_bytes) + 1;
    const int nb = (int)std::min<u64>((groups + 255) / 256, 4096);
    if (elem_bytes == 4) k_map_check<float><<<nb, 256, 0, e->stream>>>((const float *)staging, n, layout, count, d_ctl);
    else k_map_check<double><<<nb, 256, 0, e->stream>>>((const double *)staging, n, layout, count, d_ctl);
}

void launch_map_unpack(EkfEngine *e, const void *staging, int n, int elem_bytes, int layout)
{
    const int nt = (n + 63) / 64;
    const dim3 g(nt, nt);
    hipStream_t s = e->stream;
    if (elem_bytes == 4) {
        if (e->f32) k_map_unpack<float, float><<<g, 256, 0, s>>>((const float *)staging, n, layout, (float *)e->d.P, e->ldP);
        else k_map_unpack<float, double><<<g, 256, 0, s>>>((const float *)staging, n, layout, (double *)e->d.P, e->ldP);
    } else {
        if (e->f32) k_map_unpack<double, float><<<g, 256, 0, s>>>((const double *)staging, n, layout, (float *)e->d.P, e->ldP);
        else k_map_unpack<double, double><<<g, 256, 0, s>>>((const double *)staging, n, layout, (double *)e->d.P, e->ldP);
    }
}

} // namespace ekf
