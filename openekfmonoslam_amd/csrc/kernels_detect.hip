// kernels_detect.hip -- candidate pixels for NEW map features, the detector half of detectNewImageFeatures
// (EKF/DetectNewImageFeatures.cpp:337-367) for matcher mode B.  The reference masks the image with the uncertainty
// ellipses of the current predictions (buildImageMask :102-127), runs an OpenCV detector (STAR, third-party, absent
// here) and spreads the picks over image zones (:171-330, done on the host in engine.cpp).  This build's detector is
// its own: a Harris-type corner measure in INTEGER arithmetic on the gray level-0 image,
//     R = 16 (Sxx Syy - Sxy^2) - (Sxx + Syy)^2,   S.. = 5x5 sums of products of 3x3 Sobel gradients,
// reduced to the best unmasked pixel of every 16x16 cell (ties: raster order).  Integer => bit-identical to the CPU
// definition in oracle/ekf_oracle.c.  HBM traffic: one read of the frame; everything else lives in LDS.
#include "brief_pattern.h"
#include "engine.h"
#include "gate.h"

namespace ekf {

constexpr int DC = 16;      // cell edge
constexpr int DBORDER = 16; // no candidates closer than this to the frame edge

// 3x3 Sobel gradients of the gray window whose top-left pixel is g (row pitch ld): centre g[ld + 1]
__device__ __forceinline__ void sobel3x3(const int *g, int ld, short *ix, short *iy)
{
    const int a = g[0], b = g[1], c = g[2];
    const int d = g[ld], f = g[ld + 2];
    const int gg = g[2 * ld], hh = g[2 * ld + 1], k = g[2 * ld + 2];
    *ix = (short)((c + 2 * f + k) - (a + 2 * d + gg));
    *iy = (short)((gg + 2 * hh + k) - (a + 2 * b + c));
}

// the corner measure R = 16 (Sxx Syy - Sxy^2) - (Sxx + Syy)^2 of the 5x5 window of Sobel values whose top-left entry is
// ix / iy (row pitch ld), centred on ix[2 ld + 2]: the one definition both detectors use (and oracle/ekf_oracle.c restates)
__device__ __forceinline__ long long corner_response(const short *ix, const short *iy, int ld)
{
    long long sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            const int gx = ix[dy * ld + dx], gy = iy[dy * ld + dx];
            sxx += gx * gx;
            syy += gy * gy;
            sxy += gx * gy;
        }
    const long long tr = sxx + syy;
    return 16 * (sxx * syy - sxy * sxy) - tr * tr;
}

// gate (foci form) + bounding radius of every prediction of the last full prediction, in prediction order
__global__ void __launch_bounds__(256)
k_gate_snapshot(const int *plist, int n_pred, const double *uv_tab, const double *S_tab, double *gates)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_pred) return;
    const int fi = plist[k];
    float axes[2];
    double angle;
    ellipse_from_cov(S_tab + 4 * fi, axes, &angle);
    const int aw = (int)rintf(axes[0]), ah = (int)rintf(axes[1]);
    Gate g;
    const float cx = (float)uv_tab[2 * fi], cy = (float)uv_tab[2 * fi + 1];
    gate_from_ellipse(cx, cy, aw, ah, angle, &g);
    double *o = gates + 8 * (size_t)k;
    o[0] = g.f1x; o[1] = g.f1y; o[2] = g.f2x; o[3] = g.f2y; o[4] = g.two_major;
    o[5] = (double)cx; o[6] = (double)cy; o[7] = (double)(aw > ah ? aw : ah);
}

__global__ void __launch_bounds__(256)
k_detect_cells(const uint8_t *img, int w, int h, const double *gates, int n_gates, int cells_x, long long *cell_resp,
               int *cell_xy)
{
    __shared__ int sg[DC + 6][DC + 6];      // gray, halo 3
    __shared__ short sIx[DC + 4][DC + 4];   // Sobel, halo 2
    __shared__ short sIy[DC + 4][DC + 4];
    __shared__ double sGate[64][8];
    __shared__ long long s_best[4];
    __shared__ int s_idx[4];
    const int tid = threadIdx.x;
    const int cx0 = (blockIdx.x % cells_x) * DC, cy0 = (blockIdx.x / cells_x) * DC;
    for (int i = tid; i < (DC + 6) * (DC + 6); i += 256) {
        const int ly = i / (DC + 6), lx = i % (DC + 6);
        const int x = min(max(cx0 + lx - 3, 0), w - 1), y = min(max(cy0 + ly - 3, 0), h - 1);
        sg[ly][lx] = img[(size_t)y * w + x];
    }
    __syncthreads();
    for (int i = tid; i < (DC + 4) * (DC + 4); i += 256) {
        const int ly = i / (DC + 4), lx = i % (DC + 4); // centre at sg[ly + 1][lx + 1]
        sobel3x3(&sg[ly][lx], DC + 6, &sIx[ly][lx], &sIy[ly][lx]);
    }
    __syncthreads();
    const int lx = tid % DC, ly = tid / DC;
    const int x = cx0 + lx, y = cy0 + ly;
    long long resp = -1;
    bool ok = x >= DBORDER && y >= DBORDER && x < w - DBORDER && y < h - DBORDER;
    if (ok) resp = corner_response(&sIx[ly][lx], &sIy[ly][lx], DC + 4);
    // mask: inside any prediction's gate ellipse (buildImageMask)
    const double px = (double)(float)x, py = (double)(float)y;
    for (int base = 0; base < n_gates; base += 64) {
        const int cnt = min(64, n_gates - base);
        __syncthreads();
        for (int i = tid; i < cnt * 8; i += 256) sGate[i / 8][i % 8] = gates[(size_t)(base + i / 8) * 8 + i % 8];
        __syncthreads();
        if (ok)
            for (int gk = 0; gk < cnt; ++gk) {
                const double *g = sGate[gk];
                if (fabs(px - g[5]) > g[7] + 1.0 || fabs(py - g[6]) > g[7] + 1.0) continue;
                const double a1x = px - g[0], a1y = py - g[1], a2x = px - g[2], a2y = py - g[3];
                if (sqrt(a1x * a1x + a1y * a1y) + sqrt(a2x * a2x + a2y * a2y) <= g[4]) { ok = false; break; }
            }
    }
    if (!ok) resp = -1;
    // block argmax, ties -> smallest pixel index in the cell (raster order)
    int idx = tid;
    const int lane = tid & 63, wv = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const long long r2 = __shfl_down(resp, o);
        const int i2 = __shfl_down(idx, o);
        if (r2 > resp || (r2 == resp && i2 < idx)) { resp = r2; idx = i2; }
    }
    if (lane == 0) { s_best[wv] = resp; s_idx[wv] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q)
            if (s_best[q] > resp || (s_best[q] == resp && s_idx[q] < idx)) { resp = s_best[q]; idx = s_idx[q]; }
        cell_resp[blockIdx.x] = resp;
        cell_xy[2 * blockIdx.x] = cx0 + idx % DC;
        cell_xy[2 * blockIdx.x + 1] = cy0 + idx / DC;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Keypoints + BRIEF-32 for the descriptor matcher fed from images (ekf_set_image_matcher(EKF_IMAGE_MATCHER_KEYPOINTS)):
// the stage the reference runs through OpenCV in front of matchPredictedFeatures (STAR + BRIEF-32, EKF/Matching.cpp:188-210).
// Both definitions are this build's own, integer throughout, restated in numpy by tests/keypoint_ref.py:
//   keypoint   R (corner_response) >= thr, >= DBORDER px from every edge, 5x5 non-maximum suppression (strictly greater
//              than the neighbours before it in raster order, >= those after it), and -- masked -- inside the gate of at
//              least one prediction of the last full prediction (the predicate k_match applies, on the same floats);
//   descriptor 256 tests S(c + a_i) < S(c + b_i) of brief_pattern.h, S = 9x9 box sum of the gray level, reads clamped to
//              the frame; test i -> bit 7 - i % 8 of byte i / 8.
// k_kp_detect: one workgroup per 64 x 16 tile, the frame read once into LDS with a 5-px halo (Sobel 1 + box 2 + NMS 2);
// one wavefront per 64-pixel row segment, whose keypoints leave as ONE 64-bit ballot word.  k_kp_compact (one workgroup)
// scans the popcounts of those words in raster order and writes the list: the order is fixed by the scan, not by atomics.
constexpr int KTW = 64, KTH = 16; // detector tile (KTW = wavefront width: a tile row is one mask word)
constexpr int BRIEF_R = EKF_BRIEF_RADIUS; // largest test offset
constexpr int BRIEF_S = 2 * BRIEF_R + 1;  // box sums needed per keypoint (per side)
constexpr int BRIEF_W = BRIEF_S + 8;      // gray window per side (9x9 boxes)

__constant__ signed char c_brief[EKF_BRIEF_PAIRS][4] = EKF_BRIEF_PATTERN;

__global__ void __launch_bounds__(256)
k_kp_detect(const uint8_t *img, int w, int h, long long thr, int masked, const double *gates, int n_gates, int tiles_x,
            unsigned long long *rowmask)
{
    __shared__ int sg[KTH + 10][KTW + 10];   // gray, halo 5
    __shared__ short sIx[KTH + 8][KTW + 8];  // Sobel, halo 4
    __shared__ short sIy[KTH + 8][KTW + 8];
    __shared__ long long sR[KTH + 4][KTW + 4]; // response, halo 2 (the NMS ring)
    __shared__ double sGate[256][8];         // the gates that reach this tile, one pass of 256
    __shared__ int s_wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx = blockIdx.x % tiles_x, x0 = tx * KTW, y0 = (blockIdx.x / tiles_x) * KTH;
    for (int i = tid; i < (KTH + 10) * (KTW + 10); i += 256) {
        const int ly = i / (KTW + 10), lx = i % (KTW + 10);
        const int x = min(max(x0 + lx - 5, 0), w - 1), y = min(max(y0 + ly - 5, 0), h - 1);
        sg[ly][lx] = img[(size_t)y * w + x];
    }
    __syncthreads();
    for (int i = tid; i < (KTH + 8) * (KTW + 8); i += 256) {
        const int ly = i / (KTW + 8), lx = i % (KTW + 8);
        sobel3x3(&sg[ly][lx], KTW + 10, &sIx[ly][lx], &sIy[ly][lx]);
    }
    __syncthreads();
    for (int i = tid; i < (KTH + 4) * (KTW + 4); i += 256) {
        const int ly = i / (KTW + 4), lx = i % (KTW + 4);
        sR[ly][lx] = corner_response(&sIx[ly][lx], &sIy[ly][lx], KTW + 8);
    }
    __syncthreads();
    // rows wv, wv + 4, ...: lane = column of the tile
    constexpr int RPW = KTH / 4;
    bool cand[RPW];
    bool any = false;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int ly = wv + 4 * r, x = x0 + lane, y = y0 + ly;
        const long long R = sR[ly + 2][lane + 2];
        bool ok = x >= DBORDER && y >= DBORDER && x < w - DBORDER && y < h - DBORDER && R >= thr;
        if (ok) {
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) {
                    const long long q = sR[ly + dy][lane + dx];
                    const bool before = dy < 2 || (dy == 2 && dx < 2);
                    if (before ? q >= R : q > R) ok = false;
                }
        }
        cand[r] = ok;
        any |= ok;
    }
    if (masked) {
        bool inside[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) inside[r] = false;
        if (__syncthreads_or(any)) { // block-uniform: tiles without a candidate skip the gates
            // the gates, 256 at a time: thread t culls gate base + t against the tile's box, the survivors are packed into LDS
            // (ballot ranks, wave by wave) and only they are tested per candidate.  The cull is conservative: a point of a gate
            // is within its major semi-axis (g[7]) of the centre up to rounding, and the +1 px covers the rounding; it only
            // decides which gates are looked at, the membership itself is gate_contains, k_match's predicate
            const double tx0 = (double)x0, tx1 = (double)(x0 + KTW - 1), ty0 = (double)y0, ty1 = (double)(y0 + KTH - 1);
            for (int base = 0; base < n_gates; base += 256) {
                const int gi = base + tid;
                bool hit = false;
                if (gi < n_gates) {
                    const double *g = gates + (size_t)gi * 8;
                    const double cx = g[5], cy = g[6], rr = g[7] + 1.0;
                    hit = !(tx0 - cx > rr || cx - tx1 > rr || ty0 - cy > rr || cy - ty1 > rr);
                }
                const unsigned long long bal = __ballot(hit);
                __syncthreads(); // the previous pass's list is consumed
                if (lane == 0) s_wcnt[wv] = __popcll(bal);
                __syncthreads();
                int off = 0, cnt = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    off += q < wv ? s_wcnt[q] : 0;
                    cnt += s_wcnt[q];
                }
                if (hit) {
                    const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
                    for (int j = 0; j < 8; ++j) sGate[slot][j] = gates[(size_t)gi * 8 + j];
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    if (!cand[r] || inside[r]) continue;
                    const double px = (double)(float)(x0 + lane), py = (double)(float)(y0 + wv + 4 * r);
                    for (int gk = 0; gk < cnt; ++gk) {
                        const double *g = sGate[gk];
                        if (fabs(px - g[5]) > g[7] + 1.0 || fabs(py - g[6]) > g[7] + 1.0) continue;
                        const Gate gg{g[0], g[1], g[2], g[3], g[4]};
                        if (gate_contains(gg, px, py)) { inside[r] = true; break; }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) cand[r] = cand[r] && inside[r];
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const unsigned long long m = __ballot(cand[r]);
        const int y = y0 + wv + 4 * r;
        if (lane == 0 && y < h) rowmask[(size_t)y * tiles_x + tx] = m;
    }
}

// raster-order list of the keypoints flagged in rowmask (word y * tiles_x + tx holds pixels tx * 64 + bit of row y): the
// first `cap` are written, *found = all of them
__global__ void __launch_bounds__(1024)
k_kp_compact(const unsigned long long *rowmask, int n_words, int tiles_x, int cap, EkfKeypoint *kps, int *found)
{
    __shared__ int wtot[16];
    const int tid = threadIdx.x;
    const int per = (n_words + 1023) / 1024;
    const int w0 = min(tid * per, n_words), w1 = min(w0 + per, n_words);
    int c = 0;
    for (int i = w0; i < w1; ++i) c += __popcll(rowmask[i]);
    int total = 0;
    int pos = block_exclusive_scan_1024(c, wtot, &total);
    for (int i = w0; i < w1 && pos < cap; ++i) {
        unsigned long long m = rowmask[i];
        const int y = i / tiles_x, xb = (i % tiles_x) * KTW;
        while (m && pos < cap) {
            const int b = __ffsll((long long)m) - 1;
            kps[pos++] = EkfKeypoint{(float)(xb + b), (float)y};
            m &= m - 1;
        }
    }
    if (tid == 0) *found = total;
}

// BRIEF-32 of n keypoints (centres: integer pixel pairs, or null: the keypoints' own integer positions), one wavefront per
// keypoint, four per workgroup.  d_n != null: n is an upper bound, the count is min(*d_n, n).  The 47x47 window around the
// centre (clamped reads) -> 9-wide row sums -> 9-tall column sums = the 39x39 box sums the tests can address; each lane
// evaluates four tests and a 64-bit ballot assembles 64 of them.
__global__ void __launch_bounds__(256)
k_brief(const uint8_t *img, int w, int h, const EkfKeypoint *kps, const int *centres, int n, const int *d_n, uint8_t *desc)
{
    __shared__ unsigned short sG[4][BRIEF_W][BRIEF_W];
    __shared__ unsigned short sRow[4][BRIEF_W][BRIEF_S];
    __shared__ unsigned short sBox[4][BRIEF_S][BRIEF_S];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wv;
    const int cnt = d_n ? min(*d_n, n) : n;
    if ((int)blockIdx.x * 4 >= cnt) return; // whole workgroup idle (grid sized by the bound): before any barrier
    const bool active = k < cnt;
    int cx = 0, cy = 0;
    if (active) {
        if (centres) { cx = centres[2 * k]; cy = centres[2 * k + 1]; }
        else { cx = (int)kps[k].x; cy = (int)kps[k].y; }
    }
    const int ox = cx - BRIEF_R - 4, oy = cy - BRIEF_R - 4;
    for (int i = lane; i < BRIEF_W * BRIEF_W; i += 64) {
        const int ly = i / BRIEF_W, lx = i % BRIEF_W;
        const int x = min(max(ox + lx, 0), w - 1), y = min(max(oy + ly, 0), h - 1);
        sG[wv][ly][lx] = active ? img[(size_t)y * w + x] : 0;
    }
    __syncthreads();
    for (int i = lane; i < BRIEF_W * BRIEF_S; i += 64) {
        const int ly = i / BRIEF_S, lx = i % BRIEF_S;
        int s = 0;
#pragma unroll
        for (int d = 0; d < 9; ++d) s += sG[wv][ly][lx + d];
        sRow[wv][ly][lx] = (unsigned short)s;
    }
    __syncthreads();
    for (int i = lane; i < BRIEF_S * BRIEF_S; i += 64) {
        const int ly = i / BRIEF_S, lx = i % BRIEF_S;
        int s = 0;
#pragma unroll
        for (int d = 0; d < 9; ++d) s += sRow[wv][ly + d][lx];
        sBox[wv][ly][lx] = (unsigned short)s; // <= 81 * 255
    }
    __syncthreads();
    unsigned long long bal[EKF_BRIEF_PAIRS / 64];
#pragma unroll
    for (int j = 0; j < EKF_BRIEF_PAIRS / 64; ++j) {
        const signed char *p = c_brief[64 * j + lane];
        bal[j] = __ballot(sBox[wv][p[1] + BRIEF_R][p[0] + BRIEF_R] < sBox[wv][p[3] + BRIEF_R][p[2] + BRIEF_R]);
    }
    if (active && lane < EKF_DESC_BYTES) { // byte b = tests 8b .. 8b + 7, test 8b first in the most significant bit
        const unsigned byte = (unsigned)(bal[lane / 8] >> (8 * (lane % 8))) & 0xffu;
        desc[(size_t)k * EKF_DESC_BYTES + lane] = (uint8_t)(__brev(byte) >> 24);
    }
}

void launch_kp_detect(EkfEngine *e, long long thr, bool masked, unsigned long long *rowmask, EkfKeypoint *out, int cap, int *d_found)
{
    const int w = e->img.w[0], h = e->img.h[0];
    const int tiles_x = (w + KTW - 1) / KTW, tiles_y = (h + KTH - 1) / KTH;
    k_kp_detect<<<tiles_x * tiles_y, 256, 0, e->stream>>>(e->img.px[0], w, h, thr, masked ? 1 : 0, e->d.gates,
                                                          masked ? e->n_gates : 0, tiles_x, rowmask);
    k_kp_compact<<<1, 1024, 0, e->stream>>>(rowmask, h * tiles_x, tiles_x, cap, out, d_found);
}

size_t kp_rowmask_words(int w, int h) { return (size_t)h * ((w + KTW - 1) / KTW); }

void launch_brief(EkfEngine *e, const EkfKeypoint *kps, const int *centres, int n, const int *d_n, uint8_t *desc)
{
    if (n <= 0) return;
    k_brief<<<(n + 3) / 4, 256, 0, e->stream>>>(e->img.px[0], e->img.w[0], e->img.h[0], kps, centres, n, d_n, desc);
}

void launch_gate_snapshot(EkfEngine *e, int n_pred)
{
    if (n_pred > 0)
        k_gate_snapshot<<<(n_pred + 255) / 256, 256, 0, e->stream>>>(e->d.plist, n_pred, e->d.pred_uv, e->d.pred_S, e->d.gates);
}

void launch_detect_cells(EkfEngine *e, int n_gates, int cells_x, int cells_y, long long *d_resp, int *d_xy)
{
    k_detect_cells<<<cells_x * cells_y, 256, 0, e->stream>>>(e->img.px[0], e->img.w[0], e->img.h[0], e->d.gates, n_gates,
                                                             cells_x, d_resp, d_xy);
}

} // namespace ekf
