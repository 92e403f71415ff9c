// kernels_ncc.hip -- matcher mode B: the image-taking form of matchPredictedFeatures (EKF/Matching.h:66 takes the
// cv::Mat frame) done without a detector: an 11x11 template per map feature, zero-mean NCC evaluated at every pixel
// of the predicted uncertainty ellipse (the gate of Matching.cpp:217-241) on the coarsest level of a 3-level 2x
// pyramid, then refined through the 4x4 children at the two finer levels.  All image arithmetic is integer, the
// score is num^2/den in fp64 (one multiply, one divide of identically rounded operands), so the result is
// bit-identical to the CPU definition the tests check against.
//
// The coarse search of the default path is capped at a 33x33 candidate square (NCC_MAXRAD = 16 coarse pixels): "every pixel of
// the ellipse" holds for gates whose major semi-axis is below 64 px; a larger gate is searched within about +-66 px of the
// prediction only.  The wide search (ekf_set_ncc_wide_search) searches such gates whole.
//
// Byte work: a frame is ~1.6 MB of pyramid, a prediction touches a <= 43x43 window of the coarse level.  One
// workgroup per prediction stages the window and the template in LDS; nothing here is GEMM-shaped.
#include "engine.h"
#include "gate.h"

namespace ekf {

constexpr int NCC_R = 5, NCC_T = 11, NCC_TT = 121, NCC_MAXRAD = 16;
constexpr int NCC_WIN = 2 * NCC_MAXRAD + 1 + 2 * NCC_R; // 43

// ---- pyramid -----------------------------------------------------------------------------------------------
// gray = (77 R + 150 G + 29 B + 128) >> 8; 3 channels = B G R (cv::imread order, Img/FileSequenceImageGenerator),
// 4 channels = R G B A (android jni/EKFNative.cpp:163)
__global__ void __launch_bounds__(256)
k_ncc_gray(const uint8_t *raw, int w, int h, int stride, int channels, uint8_t *out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t *p = raw + (size_t)y * stride + (size_t)x * channels;
    int g;
    if (channels == 1) g = p[0];
    else if (channels == 3) g = (77 * p[2] + 150 * p[1] + 29 * p[0] + 128) >> 8;
    else g = (77 * p[0] + 150 * p[1] + 29 * p[2] + 128) >> 8;
    out[(size_t)y * w + x] = (uint8_t)g;
}

__global__ void __launch_bounds__(256) k_ncc_down(const uint8_t *src, int sw, uint8_t *dst, int dw, int dh)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw || y >= dh) return;
    const uint8_t *r0 = src + (size_t)(2 * y) * sw + 2 * x, *r1 = r0 + sw;
    dst[(size_t)y * dw + x] = (uint8_t)((r0[0] + r0[1] + r1[0] + r1[1] + 2) >> 2);
}

struct Pyr {
    const uint8_t *px[3];
    int w[3], h[3];
};

__device__ inline int pyr_at(const Pyr &p, int l, int x, int y)
{
    x = min(max(x, 0), p.w[l] - 1);
    y = min(max(y, 0), p.h[l] - 1);
    return p.px[l][(size_t)y * p.w[l] + x];
}

__device__ inline int to_level(double u, int l) { return (int)floor((u + 0.5) / (double)(1 << l)); }

// templates of the listed features from the current pyramid: block = (item, level), 121 active lanes
__global__ void __launch_bounds__(128)
k_ncc_capture(Pyr pyr, const int *feat_idx, const double *uv, uint8_t *tmpl)
{
    const int i = blockIdx.x, l = blockIdx.y, t = threadIdx.x;
    if (t >= NCC_TT) return;
    const int cx = to_level(uv[2 * i], l), cy = to_level(uv[2 * i + 1], l);
    const int dy = t / NCC_T - NCC_R, dx = t % NCC_T - NCC_R;
    tmpl[((size_t)feat_idx[i] * 3 + l) * NCC_TT + t] = (uint8_t)pyr_at(pyr, l, cx + dx, cy + dy);
}

// ---- template warp -------------------------------------------------------------------------
// A template is the image of a small plane through the feature's world point X that faces the camera which first saw it.
// k_ncc_warp_capture keeps, per feature and level, the 41 x 41 pixels around the capture pixel and the capture pose;
// k_ncc_warp re-renders the 11 x 11 template of every prediction slot from the current pose estimate before the search:
// template pixel -> ray of the current camera -> plane -> pixel of the capture camera -> bilinear sample of the source.
// A level whose samples leave the source (or whose geometry is degenerate) keeps the stored template, whole.
constexpr int WARP_S = 41, WARP_SS = WARP_S * WARP_S, WARP_R = WARP_S / 2;

// block = (item, level): source patch; the level-0 block also writes the pose record (keep = 0: zeros = "no source patch")
__global__ void __launch_bounds__(256)
k_ncc_warp_capture(Pyr pyr, const int *feat_idx, const double *uv, const double *st, uint8_t *wsrc, double *wpose, int keep,
                   PatchNormalRec *wnorm)
{
    const int i = blockIdx.x, l = blockIdx.y, fi = feat_idx[i];
    if (l == 0 && threadIdx.x == 9 && wnorm) wnorm[fi] = PatchNormalRec{}; // patch normals: a capture resets the estimate
    if (l == 0 && threadIdx.x < 9) {
        const int t = threadIdx.x;
        wpose[9 * (size_t)fi + t] = !keep ? 0.0 : (t < 7 ? st[ST_X + t] : uv[2 * i + t - 7]);
    }
    if (!keep) return;
    const int cx = to_level(uv[2 * i], l), cy = to_level(uv[2 * i + 1], l);
    for (int t = threadIdx.x; t < WARP_SS; t += 256)
        wsrc[((size_t)fi * 3 + l) * WARP_SS + t] = (uint8_t)pyr_at(pyr, l, cx + t % WARP_S - WARP_R, cy + t / WARP_S - WARP_R);
}

// unit normal in world axes of the slope (p, q) in the capture camera's axes: R0 (p, q, -1) / |(p, q, -1)|
__device__ __forceinline__ void pn_normal(const double *R0, double p, double q, double *n)
{
    const double nrm = sqrt(p * p + q * q + 1.0);
    for (int i = 0; i < 3; ++i) n[i] = (R0[3 * i] * p + R0[3 * i + 1] * q - R0[3 * i + 2]) / nrm;
}

// One workgroup per prediction slot, 128 lanes per level (121 active): fp64, everything a lane touches after the staging
// is in LDS (5 KB of source bytes, 30 doubles of constants).  Latency-bound like k_ncc_match: ~0.4 KFLOP and one 10-step
// Newton solve per lane.  out already holds a copy of the stored templates; only whole warped levels are written.
__global__ void __launch_bounds__(384)
k_ncc_warp(const int *plist, const int *d_npred, const double *uv_tab, const double *st, CamD c, const double *feat_pos,
           const int *feat_type, const uint8_t *wsrc, const double *wpose, uint8_t *out, int *counts, const PatchNormalRec *wnorm)
{
    __shared__ uint8_t s_src[3 * WARP_SS + 1];
    __shared__ double s_R[9], s_R0[9], s_n[3], s_r[3], s_r0[3], s_nXr, s_uv0[2];
    __shared__ int s_bad[3];

    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= *d_npred) return;
    const int fi = plist[k];
    const double *pose = wpose + 9 * (size_t)fi;
    const bool has_src = pose[3] != 0.0 || pose[4] != 0.0 || pose[5] != 0.0 || pose[6] != 0.0; // uniform over the block
    if (!has_src) {
        if (tid == 0) atomicAdd(counts + CNT_WARP_FB, 3);
        return;
    }
    for (int i = tid; i < 3 * WARP_SS; i += 384) s_src[i] = wsrc[(size_t)fi * 3 * WARP_SS + i];
    if (tid < 3) s_bad[tid] = 0;
    if (tid == 0) {
        const double *x = st + ST_X, *y = feat_pos + 6 * (size_t)fi;
        double X[3] = {y[0], y[1], y[2]};
        if (feat_type[fi] == EKF_FEATURE_INVERSE_DEPTH) {
            double m[3];
            dir_vec(y[3], y[4], m);
            X[0] += m[0] / y[5]; X[1] += m[1] / y[5]; X[2] += m[2] / y[5];
        }
        quat_to_rot(x + 3, s_R);
        quat_to_rot(pose + 3, s_R0);
        const double a[3] = {pose[0] - X[0], pose[1] - X[1], pose[2] - X[2]};
        const double an = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const bool estimated = wnorm && wnorm[fi].updates > 0; // patch normals: n(p, q) instead of the rule
        double pqn[3] = {0.0, 0.0, 1.0};
        if (estimated) pn_normal(s_R0, wnorm[fi].pq[0], wnorm[fi].pq[1], pqn);
        double nXr = 0.0;
        for (int i = 0; i < 3; ++i) {
            s_n[i] = estimated ? pqn[i] : a[i] / an;
            s_r[i] = x[i];
            s_r0[i] = pose[i];
            nXr += s_n[i] * (X[i] - x[i]);
        }
        s_nXr = nXr;
        s_uv0[0] = pose[7];
        s_uv0[1] = pose[8];
    }
    __syncthreads();

    const int l = tid >> 7, t = tid & 127;
    const bool live = t < NCC_TT;
    const double sc = (double)(1 << l);
    bool bad = false;
    int val = 0;
    if (live) {
        const int cxl = to_level(uv_tab[2 * fi], l), cyl = to_level(uv_tab[2 * fi + 1], l);
        const double px = ((double)(cxl + t % NCC_T - NCC_R) + 0.5) * sc - 0.5, py = ((double)(cyl + t / NCC_T - NCC_R) + 0.5) * sc - 0.5;
        // undistortPoint (closed form), then the ray in world axes
        const double pdx = px - c.cx, pdy = py - c.cy;
        const double mx = c.dx * pdx, my = c.dy * pdy;
        const double rd2 = mx * mx + my * my;
        const double f = 1.0 + c.k1 * rd2 + c.k2 * rd2 * rd2;
        const double hc[3] = {pdx * f / c.fx, pdy * f / c.fy, 1.0};
        double d[3];
        mat3_vec(s_R, hc, d);
        const double nd = s_n[0] * d[0] + s_n[1] * d[1] + s_n[2] * d[2];
        bad = !(nd < 0.0); // n points from the plane to the capturing camera: a ray that meets its front has n . d < 0
        if (!bad) {
            const double lam = s_nXr / nd;
            bad = !(lam > 0.0);
            if (!bad) {
                const double w[3] = {s_r[0] + lam * d[0] - s_r0[0], s_r[1] + lam * d[1] - s_r0[1], s_r[2] + lam * d[2] - s_r0[2]};
                const double h0 = s_R0[0] * w[0] + s_R0[3] * w[1] + s_R0[6] * w[2];
                const double h1 = s_R0[1] * w[0] + s_R0[4] * w[1] + s_R0[7] * w[2];
                const double h2 = s_R0[2] * w[0] + s_R0[5] * w[1] + s_R0[8] * w[2];
                bad = !(h2 > 0.0);
                if (!bad) {
                    double s[2];
                    distort(c, c.cx + c.fx * h0 / h2, c.cy + c.fy * h1 / h2, s);
                    const double sx = (s[0] + 0.5) / sc - 0.5 - (double)(to_level(s_uv0[0], l) - WARP_R);
                    const double sy = (s[1] + 0.5) / sc - 0.5 - (double)(to_level(s_uv0[1], l) - WARP_R);
                    bad = !(sx >= 0.0 && sx <= (double)(WARP_S - 1) && sy >= 0.0 && sy <= (double)(WARP_S - 1));
                    if (!bad) {
                        const int x0 = min((int)floor(sx), WARP_S - 2), y0 = min((int)floor(sy), WARP_S - 2);
                        const double ax = sx - (double)x0, ay = sy - (double)y0;
                        const uint8_t *p = s_src + l * WARP_SS + y0 * WARP_S + x0;
                        const double top = (1.0 - ax) * (double)p[0] + ax * (double)p[1];
                        const double bot = (1.0 - ax) * (double)p[WARP_S] + ax * (double)p[WARP_S + 1];
                        const double b = (1.0 - ay) * top + ay * bot;
                        val = min(max((int)floor(b + 0.5), 0), 255);
                    }
                }
            }
        }
        if (bad) s_bad[l] = 1; // any lane of the level: the whole level falls back
    }
    __syncthreads();
    if (live && !s_bad[l]) out[((size_t)fi * 3 + l) * NCC_TT + t] = (uint8_t)val;
    if (tid == 0) {
        const int nfb = s_bad[0] + s_bad[1] + s_bad[2];
        if (nfb) atomicAdd(counts + CNT_WARP_FB, nfb);
        if (nfb < 3) atomicAdd(counts + CNT_WARP_OK, 3 - nfb);
    }
}

// ---- patch normals ---------------------------------------------------------------------------
// One estimator step per listed match: the feature's source patches are aligned to the current frame around the match's pixel
// and the slope (p, q) of its patch plane takes one information-filter step.  tests/patch_normal_ref.py is the definition; every
// operation below is in its order (fp64, no contraction, sums in pixel order, then levels 0, 1, 2).

// steps 2-4 of k_ncc_warp for one ray d (world axes) and one plane: level-0 position in the capture frame; false: not valid
__device__ __forceinline__ bool pn_to_source(const CamD &c, const double *d, const double *n, double nXr, const double *r, const double *r0,
                                             const double *R0, double *s)
{
    const double nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
    if (!(nd < 0.0)) return false;
    const double lam = nXr / nd;
    if (!(lam > 0.0)) return false;
    const double w[3] = {r[0] + lam * d[0] - r0[0], r[1] + lam * d[1] - r0[1], r[2] + lam * d[2] - r0[2]};
    const double h0 = R0[0] * w[0] + R0[3] * w[1] + R0[6] * w[2];
    const double h1 = R0[1] * w[0] + R0[4] * w[1] + R0[7] * w[2];
    const double h2 = R0[2] * w[0] + R0[5] * w[1] + R0[8] * w[2];
    if (!(h2 > 0.0)) return false;
    distort(c, c.cx + c.fx * h0 / h2, c.cy + c.fy * h1 / h2, s);
    return true;
}

// ray of the level-0 position (px, py) in world axes (step 2 of k_ncc_warp)
__device__ __forceinline__ void pn_ray(const CamD &c, const double *R, double px, double py, double *d)
{
    const double pdx = px - c.cx, pdy = py - c.cy;
    const double mx = c.dx * pdx, my = c.dy * pdy;
    const double rd2 = mx * mx + my * my;
    const double f = 1.0 + c.k1 * rd2 + c.k2 * rd2 * rd2;
    const double hc[3] = {pdx * f / c.fx, pdy * f / c.fy, 1.0};
    mat3_vec(R, hc, d);
}

constexpr int PN_VEC = 6; // vectors per level: the prediction at the five slopes, the measurement

// One workgroup per match, 128 lanes per level (121 active, lanes 121..125 of level 0 carry the anchor at the five slopes).
// Latency-bound: five plane intersections and Newton solves per lane, six barriers-separated serial sums of 121 terms by six lanes
// per level (the order of the restatement), 18 KB of vectors and 5 KB of source bytes in LDS.
__global__ void __launch_bounds__(384)
k_ncc_normal(Pyr pyr, const EkfMatch *list, int M, int N, const double *st, CamD c, const double *feat_pos, const int *feat_type,
             const uint8_t *wsrc, const double *wpose, PatchNormalRec *wnorm, int *counts)
{
    __shared__ uint8_t s_src[3 * WARP_SS + 1];
    __shared__ double s_vec[3][PN_VEC][128];
    __shared__ double s_sum[3][PN_VEC];
    __shared__ double s_R[9], s_R0[9], s_n[5][3], s_nXr[5], s_r[3], s_r0[3], s_anc[5][2], s_pq[2];
    __shared__ int s_bad[3], s_anchor[2], s_uv0l[3][2], s_ctr0[2];

    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= M) return;
    const int fi = list[k].featureIndex;
    if (fi < 0 || fi >= N) return; // (the host validates the list)
    const double *pose = wpose + 9 * (size_t)fi;
    const bool has_src = pose[3] != 0.0 || pose[4] != 0.0 || pose[5] != 0.0 || pose[6] != 0.0; // uniform over the block
    if (!has_src) {
        if (tid == 0) atomicAdd(counts + CNT_PN_SKIP, 1);
        return;
    }
    for (int i = tid; i < 3 * WARP_SS; i += 384) s_src[i] = wsrc[(size_t)fi * 3 * WARP_SS + i];
    if (tid < 3) s_bad[tid] = 0;
    if (tid == 0) {
        const double *x = st + ST_X, *y = feat_pos + 6 * (size_t)fi;
        double X[3] = {y[0], y[1], y[2]};
        if (feat_type[fi] == EKF_FEATURE_INVERSE_DEPTH) {
            double m[3];
            dir_vec(y[3], y[4], m);
            X[0] += m[0] / y[5]; X[1] += m[1] / y[5]; X[2] += m[2] / y[5];
        }
        quat_to_rot(x + 3, s_R);
        quat_to_rot(pose + 3, s_R0);
        double p, q;
        if (wnorm[fi].updates > 0) {
            p = wnorm[fi].pq[0];
            q = wnorm[fi].pq[1];
        } else { // first update: the rule of 4.6 as a slope
            const double w[3] = {X[0] - pose[0], X[1] - pose[1], X[2] - pose[2]};
            const double h0 = s_R0[0] * w[0] + s_R0[3] * w[1] + s_R0[6] * w[2];
            const double h1 = s_R0[1] * w[0] + s_R0[4] * w[1] + s_R0[7] * w[2];
            const double h2 = s_R0[2] * w[0] + s_R0[5] * w[1] + s_R0[8] * w[2];
            p = -h0 / h2;
            q = -h1 / h2;
        }
        s_pq[0] = p;
        s_pq[1] = q;
        for (int j = 0; j < 5; ++j) { // the slope, p + h, p - h, q + h, q - h
            const double dp = j == 1 ? PN_FD_STEP : (j == 2 ? -PN_FD_STEP : 0.0), dq = j == 3 ? PN_FD_STEP : (j == 4 ? -PN_FD_STEP : 0.0);
            double n[3];
            pn_normal(s_R0, p + dp, q + dq, n);
            double nXr = 0.0;
            for (int i = 0; i < 3; ++i) {
                s_n[j][i] = n[i];
                nXr += n[i] * (X[i] - x[i]);
            }
            s_nXr[j] = nXr;
        }
        for (int i = 0; i < 3; ++i) {
            s_r[i] = x[i];
            s_r0[i] = pose[i];
        }
        s_anchor[0] = to_level(list[k].imagePos[0], 0);
        s_anchor[1] = to_level(list[k].imagePos[1], 0);
        for (int l = 0; l < 3; ++l) {
            s_uv0l[l][0] = to_level(pose[7], l);
            s_uv0l[l][1] = to_level(pose[8], l);
        }
    }
    __syncthreads();

    const int l = tid >> 7, t = tid & 127;
    const bool live = t < NCC_TT;
    const bool anchor_lane = l == 0 && t >= NCC_TT && t < NCC_TT + 5;
    const double sc = (double)(1 << l);
    const int cxl = to_level((double)s_anchor[0], l), cyl = to_level((double)s_anchor[1], l);
    double s5[5][2];
    bool bad = false;
    if (live) {
        double d[3];
        pn_ray(c, s_R, ((double)(cxl + t % NCC_T - NCC_R) + 0.5) * sc - 0.5, ((double)(cyl + t / NCC_T - NCC_R) + 0.5) * sc - 0.5, d);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (!pn_to_source(c, d, s_n[j], s_nXr[j], s_r, s_r0, s_R0, s5[j])) bad = true;
    } else if (anchor_lane) { // where the anchor itself lands at slope j
        const int j = t - NCC_TT;
        double d[3], s[2] = {0.0, 0.0};
        pn_ray(c, s_R, (double)s_anchor[0], (double)s_anchor[1], d);
        if (!pn_to_source(c, d, s_n[j], s_nXr[j], s_r, s_r0, s_R0, s)) s_bad[0] = s_bad[1] = s_bad[2] = 1;
        s_anc[j][0] = s[0];
        s_anc[j][1] = s[1];
    }
    __syncthreads();
    if (live) {
        const double offx = (double)(s_uv0l[l][0] - WARP_R), offy = (double)(s_uv0l[l][1] - WARP_R);
        // the source's centre pixel (level 0) in this level's source coordinates: the anchor is moved onto it
        const double ctrx = ((double)s_uv0l[0][0] + 0.5) / sc - 0.5 - offx, ctry = ((double)s_uv0l[0][1] + 0.5) / sc - 0.5 - offy;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double b = 0.0;
            if (!bad) {
                const double sx = ((s5[j][0] + 0.5) / sc - 0.5 - offx) - (((s_anc[j][0] + 0.5) / sc - 0.5 - offx) - ctrx);
                const double sy = ((s5[j][1] + 0.5) / sc - 0.5 - offy) - (((s_anc[j][1] + 0.5) / sc - 0.5 - offy) - ctry);
                if (sx >= 0.0 && sx <= (double)(WARP_S - 1) && sy >= 0.0 && sy <= (double)(WARP_S - 1)) {
                    const int x0 = min((int)floor(sx), WARP_S - 2), y0 = min((int)floor(sy), WARP_S - 2);
                    const double ax = sx - (double)x0, ay = sy - (double)y0;
                    const uint8_t *p = s_src + l * WARP_SS + y0 * WARP_S + x0;
                    const double top = (1.0 - ax) * (double)p[0] + ax * (double)p[1];
                    const double bot = (1.0 - ax) * (double)p[WARP_S] + ax * (double)p[WARP_S + 1];
                    b = (1.0 - ay) * top + ay * bot;
                } else {
                    bad = true;
                }
            }
            s_vec[l][j][t] = b;
        }
        s_vec[l][5][t] = (double)pyr_at(pyr, l, cxl + t % NCC_T - NCC_R, cyl + t / NCC_T - NCC_R);
        if (bad) s_bad[l] = 1; // any lane of the level: the level is left out
    }
    __syncthreads();
    // zero mean, unit norm per vector; a level that failed above goes through the same steps on zeros and is dropped at the end
    if (t < PN_VEC) {
        double s = 0.0;
        for (int i = 0; i < NCC_TT; ++i) s += s_vec[l][t][i];
        s_sum[l][t] = s / (double)NCC_TT;
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int v = 0; v < PN_VEC; ++v) s_vec[l][v][t] = s_vec[l][v][t] - s_sum[l][v];
    }
    __syncthreads();
    if (t < PN_VEC) {
        double ss = 0.0;
        for (int i = 0; i < NCC_TT; ++i) ss += s_vec[l][t][i] * s_vec[l][t][i];
        if (!(ss > PN_MIN_SS)) s_bad[l] = 1; // a constant vector
        s_sum[l][t] = sqrt(ss);
    }
    __syncthreads();
    if (live) {
        double hat[PN_VEC];
#pragma unroll
        for (int v = 0; v < PN_VEC; ++v) hat[v] = s_vec[l][v][t] / s_sum[l][v];
        s_vec[l][0][t] = (hat[1] - hat[2]) * (0.5 / PN_FD_STEP); // d prediction / dp
        s_vec[l][1][t] = (hat[3] - hat[4]) * (0.5 / PN_FD_STEP); // d prediction / dq
        s_vec[l][2][t] = hat[5] - hat[0];                        // residual: measurement - prediction
    }
    __syncthreads();
    if (t < PN_VEC) { // Jp Jp, Jp Jq, Jq Jq, Jp r, Jq r, r r
        const double *a = s_vec[l][t == 0 || t == 1 || t == 3 ? 0 : (t == 2 || t == 4 ? 1 : 2)];
        const double *b = s_vec[l][t == 0 ? 0 : (t == 1 || t == 2 ? 1 : 2)];
        double s = 0.0;
        for (int i = 0; i < NCC_TT; ++i) s += a[i] * b[i];
        s_sum[l][t] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double A[PN_VEC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int used = 0;
        for (int lv = 0; lv < 3; ++lv)
            if (!s_bad[lv]) {
                for (int v = 0; v < PN_VEC; ++v) A[v] += s_sum[lv][v];
                ++used;
            }
        bool done = false;
        if (used > 0) {
            const PatchNormalRec old = wnorm[fi];
            const bool first = old.updates <= 0;
            const double i00 = first ? PN_PRIOR_INFO : old.info[0], i01 = first ? 0.0 : old.info[1], i11 = first ? PN_PRIOR_INFO : old.info[2];
            const double m = (double)(NCC_TT * used);
            const double s2 = fmax(A[5] / (m - 2.0), PN_S_MIN * PN_S_MIN);
            const double l00 = i00 + A[0] / s2, l01 = i01 + A[1] / s2, l11 = i11 + A[2] / s2;
            const double b0 = A[3] / s2, b1 = A[4] / s2;
            const double det = l00 * l11 - l01 * l01;
            double d0 = (l11 * b0 - l01 * b1) / det, d1 = (l00 * b1 - l01 * b0) / det;
            const double len = sqrt(d0 * d0 + d1 * d1);
            if (len > PN_STEP_MAX) {
                const double f = PN_STEP_MAX / len;
                d0 = d0 * f;
                d1 = d1 * f;
            }
            PatchNormalRec rec;
            rec.pq[0] = s_pq[0] + d0;
            rec.pq[1] = s_pq[1] + d1;
            rec.info[0] = l00;
            rec.info[1] = l01;
            rec.info[2] = l11;
            rec.updates = first ? 1 : (old.updates < 0x7fffffff ? old.updates + 1 : old.updates);
            rec.pad = 0;
            if (det > 0.0 && isfinite(rec.pq[0]) && isfinite(rec.pq[1]) && isfinite(l00) && isfinite(l01) && isfinite(l11)) {
                wnorm[fi] = rec;
                done = true;
            }
        }
        atomicAdd(counts + (done ? CNT_PN_UPD : CNT_PN_SKIP), 1);
    }
}

// ---- matching ----------------------------------------------------------------------------------------------
// zncc^2 of a candidate whose 11x11 window starts at sw[oy][ox] (LDS window of row pitch `pitch`)
__device__ inline double ncc_key(const uint8_t *win, int pitch, int ox, int oy, const uint8_t *tp, int st, int stt)
{
    int s = 0, ss = 0, sx = 0;
    for (int dy = 0; dy < NCC_T; ++dy) {
        const uint8_t *wr = win + (oy + dy) * pitch + ox;
        const uint8_t *tr = tp + dy * NCC_T;
#pragma unroll
        for (int dx = 0; dx < NCC_T; ++dx) {
            const int wv = wr[dx], tv = tr[dx];
            s += wv;
            ss += wv * wv;
            sx += wv * tv;
        }
    }
    const long long n = NCC_TT;
    const long long num = n * sx - (long long)s * st;
    const long long den = (n * ss - (long long)s * s) * (n * stt - (long long)st * st);
    if (num <= 0 || den <= 0) return -1.0;
    const double dn = (double)num;
    return dn * dn / (double)den;
}

// block argmax of (key, candidate index): larger key wins, equal keys -> smaller index (raster order, the
// CPU loop's strict '>')
__device__ inline void block_argmax(double &key, int &idx, double *s_key, int *s_idx)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_down(key, o);
        const int i2 = __shfl_down(idx, o);
        if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
    if (lane == 0) { s_key[wv] = key; s_idx[wv] = idx; }
    __syncthreads();
    key = s_key[0]; idx = s_idx[0];
    for (int w = 1; w < 4; ++w)
        if (s_key[w] > key || (s_key[w] == key && s_idx[w] < idx)) { key = s_key[w]; idx = s_idx[w]; }
    __syncthreads();
}

// ---- sub-pixel fit --------------------------------------------------------------------------
// Offset of the vertex of the parabola through the keys at -1, 0, +1 pixels, one axis; *fit = 0 and offset 0 where the
// rule leaves the integer: a neighbour outside the frame (key -2, see k_ncc_match) or without a score (-1), a neighbour
// above the centre (the 4x4 child window does not make the best pixel a 3x3 maximum), or no curvature.  Every
// operation is one correctly rounded fp64 add, multiply by a power of two or divide, in the order of the numpy
// restatement (tests/ncc_subpixel_ref.py): the result is the same bits.
__device__ inline double subpix_offset(double km, double k0, double kp, int *fit)
{
#pragma clang fp contract(off)
    *fit = 0;
    if (km < 0.0 || kp < 0.0 || km > k0 || kp > k0) return 0.0;
    const double a = km - kp;
    const double b = (km - 2.0 * k0) + kp;
    if (b >= 0.0) return 0.0;
    *fit = 1;
    const double d = (0.5 * a) / b;
    return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
}

// One level of the search by the whole workgroup (256 lanes): stages the (cw + 10)^2 window whose candidates start at (x0, y0) and the
// level's template tl in LDS, evaluates the candidates inside the frame -- at the coarse level (l == 2) only the predicted pixel
// (gcx, gcy) and those whose centre lies in the gate -- and leaves the best one in (bx, by), its key in bkey: -3 and an unchanged
// position when the level had no candidate (position carried over, as the CPU loop does).  Shared by k_ncc_match and
// k_ncc_wide_finish.
__device__ __forceinline__ void ncc_search_level(const Pyr &pyr, int l, int x0, int y0, int cw, const uint8_t *tl, const Gate &g, int gcx,
                                                 int gcy, uint8_t *s_win, uint8_t *s_t, int *s_tsum, double *s_key, int *s_idx, int &bx,
                                                 int &by, double &bkey)
{
    const int tid = threadIdx.x;
    const int pitch = cw + 2 * NCC_R;
    for (int i = tid; i < pitch * pitch; i += 256)
        s_win[i] = (uint8_t)pyr_at(pyr, l, x0 - NCC_R + i % pitch, y0 - NCC_R + i / pitch);
    if (tid < NCC_TT) s_t[tid] = tl[tid];
    __syncthreads();
    if (tid == 0) {
        int st = 0, stt = 0;
        for (int i = 0; i < NCC_TT; ++i) { st += s_t[i]; stt += s_t[i] * s_t[i]; }
        s_tsum[0] = st; s_tsum[1] = stt;
    }
    __syncthreads();
    const int st = s_tsum[0], stt = s_tsum[1];
    double key = -3.0;
    int idx = 0x7fffffff;
    for (int c = tid; c < cw * cw; c += 256) {
        const int ox = c % cw, oy = c / cw, x = x0 + ox, y = y0 + oy;
        if (x < 0 || y < 0 || x >= pyr.w[l] || y >= pyr.h[l]) continue;
        if (l == 2 && !(x == gcx && y == gcy)) {
            const float fx = (float)((x + 0.5) * 4 - 0.5), fy = (float)((y + 0.5) * 4 - 0.5);
            if (!gate_contains(g, (double)fx, (double)fy)) continue;
        }
        const double kk = ncc_key(s_win, pitch, ox, oy, s_t, st, stt);
        if (kk > key) { key = kk; idx = c; } // c ascending per thread: first maximum kept
    }
    block_argmax(key, idx, s_key, s_idx);
    if (idx != 0x7fffffff) { bx = x0 + idx % cw; by = y0 + idx / cw; }
    bkey = key;
}

// What follows the level-0 search of prediction slot k, by the whole workgroup: the acceptance test and the slot's entries of the
// match tables.  SUBPIX (ekf_set_subpixel_matches): the keys of the best pixel's four level-0 neighbours are evaluated first and
// each axis of the reported position is moved by subpix_offset; counts then receives the fitted / integer axes of the valid
// matches.  SUBPIX = false is the integer matcher as it was.  s_t and s_tsum still hold the level-0 template and its sums.
template <bool SUBPIX>
__device__ __forceinline__ void ncc_finish_slot(const Pyr &pyr, const Gate &g, int k, int bx, int by, double bkey, uint8_t *s_win,
                                                const uint8_t *s_t, const int *s_tsum, double *s_key, int *mt_valid, EkfKeypoint *mt_xy,
                                                float *mt_dist, int *counts)
{
    const int tid = threadIdx.x;
    if constexpr (SUBPIX) {
        // bkey is uniform over the block; every read of s_win and s_key lies before the barrier that ends block_argmax.
        if (bkey >= 0.0) {
            constexpr int SP = 3 + 2 * NCC_R; // 13: the 3x3 candidates around (bx, by) and their 5-pixel border
            if (tid < SP * SP) s_win[tid] = (uint8_t)pyr_at(pyr, 0, bx - 1 - NCC_R + tid % SP, by - 1 - NCC_R + tid / SP);
            __syncthreads();
            if (tid < 4) { // lanes 0..3: the neighbours at x - 1, x + 1, y - 1, y + 1
                const int ox = tid < 2 ? 2 * tid : 1, oy = tid < 2 ? 1 : 2 * (tid - 2);
                const int x = bx - 1 + ox, y = by - 1 + oy;
                const bool inside = x >= 0 && y >= 0 && x < pyr.w[0] && y < pyr.h[0]; // the candidate loop's rule
                s_key[tid] = inside ? ncc_key(s_win, SP, ox, oy, s_t, s_tsum[0], s_tsum[1]) : -2.0;
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        const bool ok = bkey >= 0.64 && gate_contains(g, (double)(float)bx, (double)(float)by);
        mt_valid[k] = ok ? 1 : 0;
        EkfKeypoint p;
        if constexpr (SUBPIX) {
            int fx = 0, fy = 0;
            double dx = 0.0, dy = 0.0;
            if (bkey >= 0.0) {
                dx = subpix_offset(s_key[0], bkey, s_key[1], &fx);
                dy = subpix_offset(s_key[2], bkey, s_key[3], &fy);
            }
            p.x = (float)((double)bx + dx);
            p.y = (float)((double)by + dy);
            if (ok) {
                if (fx + fy > 0) atomicAdd(counts + CNT_SUBPIX_FIT, fx + fy);
                if (fx + fy < 2) atomicAdd(counts + CNT_SUBPIX_INT, 2 - fx - fy);
            }
        } else {
            p.x = (float)bx;
            p.y = (float)by;
        }
        mt_xy[k] = p;
        mt_dist[k] = ok ? (float)(1.0 - sqrt(bkey)) : 0.f;
    }
}

// gate, coarse centre and UNCAPPED coarse radius of a prediction (one lane)
__device__ __forceinline__ void ncc_slot_geometry(double pu, double pv, const double *S, Gate *g, int *cx, int *cy, int *rad)
{
    float axes[2];
    double angle;
    ellipse_from_cov(S, axes, &angle);
    const int aw = (int)rintf(axes[0]), ah = (int)rintf(axes[1]);
    // (always_inline: with several call sites the compiler would stop inlining it, in the integer matcher too)
    [[clang::always_inline]] gate_from_ellipse((float)pu, (float)pv, aw, ah, angle, g);
    const int major = aw > ah ? aw : ah;
    *cx = to_level(pu, 2);
    *cy = to_level(pv, 2);
    *rad = (major >> 2) + 1; // major <= INT_MAX: no overflow
}

// One workgroup per prediction slot.  The coarse level covers the square of radius min(rad, NCC_MAXRAD) around the prediction: a
// gate whose major semi-axis is 64 px or more is searched within +-16 coarse pixels (about +-66 px) only.  skip_wide (wide search,
// DESIGN.md 4.8): such a slot is left to k_ncc_wide_coarse / k_ncc_wide_finish and this workgroup returns without writing anything.
template <bool SUBPIX>
__global__ void __launch_bounds__(256)
k_ncc_match(Pyr pyr, const int *plist, const double *uv_tab, const double *S_tab, const uint8_t *tmpl,
            int *mt_valid, EkfKeypoint *mt_xy, float *mt_dist, int slot0, int *counts, int skip_wide)
{
    __shared__ Gate g;
    __shared__ int s_geom[4]; // c2x, c2y, rad, skipped
    __shared__ uint8_t s_win[NCC_WIN * NCC_WIN + 3];
    __shared__ uint8_t s_t[NCC_TT + 3];
    __shared__ int s_tsum[2];
    __shared__ double s_key[4];
    __shared__ int s_idx[4];

    const int k = slot0 + (int)blockIdx.x, tid = threadIdx.x; // slot0: see launch_match_ncc_slots
    const int fi = plist[k];
    if (tid == 0) {
        int rad;
        ncc_slot_geometry(uv_tab[2 * fi], uv_tab[2 * fi + 1], S_tab + 4 * fi, &g, &s_geom[0], &s_geom[1], &rad);
        s_geom[2] = min(rad, NCC_MAXRAD);
        s_geom[3] = skip_wide && rad > NCC_MAXRAD;
    }
    __syncthreads();
    if (s_geom[3]) return; // uniform

    int bx = s_geom[0], by = s_geom[1];
    double bkey = -3.0;
    for (int l = 2; l >= 0; --l) {
        // candidate window at this level: coarse = the gated square around the prediction, finer = 4x4 children
        int x0, y0, cw;
        if (l == 2) { x0 = s_geom[0] - s_geom[2]; y0 = s_geom[1] - s_geom[2]; cw = 2 * s_geom[2] + 1; }
        else { x0 = 2 * bx - 1; y0 = 2 * by - 1; cw = 4; }
        ncc_search_level(pyr, l, x0, y0, cw, tmpl + ((size_t)fi * 3 + l) * NCC_TT, g, s_geom[0], s_geom[1], s_win, s_t, s_tsum, s_key,
                         s_idx, bx, by, bkey);
    }
    ncc_finish_slot<SUBPIX>(pyr, g, k, bx, by, bkey, s_win, s_t, s_tsum, s_key, mt_valid, mt_xy, mt_dist, counts);
}

// ---- wide search ----------------------------------------------------------------------------
// A slot whose uncapped coarse radius exceeds NCC_MAXRAD has its coarse level searched over the whole gate within the frame: the
// result is what k_ncc_match would give with NCC_MAXRAD unbounded.  Three launches: the wide slots are listed in slot order, every
// 32 x 32 tile of a slot's candidate box is searched by a workgroup of its own, and one workgroup per slot reduces the tiles'
// results and runs the two finer levels and the tail that k_ncc_match runs.
struct WideSlot {
    Gate g;
    int slot, cx, cy;       // prediction slot, coarse pixel of the prediction
    int x0, y0, x1, y1;     // candidate box at the coarse level, clamped to the frame, inclusive (empty: x1 < x0 or y1 < y0)
    int tx, ty;             // tiles of the box
    int pad;
};
struct WidePartial {
    double key;             // best key of the tile (-3: no candidate)
    int idx;                // its pixel as y * w2 + x (0x7fffffff: none): raster order over the whole level
    int ncand;              // candidates evaluated
};
struct WideTotals {         // behind the cap records of d.wide_list
    unsigned long long ncand; // candidates of the slots finished so far
    unsigned done, pad;       // slots finished
};
static_assert(sizeof(WideTotals) == NCC_WIDE_TOTALS_BYTES, "engine.h sizes the tables");
static_assert(sizeof(WideSlot) == NCC_WIDE_SLOT_BYTES && sizeof(WidePartial) == NCC_WIDE_PARTIAL_BYTES, "engine.h sizes the tables");
constexpr int WIDE_WIN = NCC_WIDE_TILE + 2 * NCC_R; // 42

// One lane per prediction slot, one workgroup: the wide slots are compacted in slot order by a block scan, 1024 slots per pass.
__global__ void __launch_bounds__(1024)
k_ncc_wide_classify(const int *plist, const int *d_npred, int n_pred, const double *uv_tab, const double *S_tab, int w2, int h2,
                    WideSlot *list, WideTotals *totals, int *counts)
{
    __shared__ int s_wtot[16];
    const int tid = threadIdx.x, n = min(n_pred, *d_npred);
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += 1024) { // uniform
        const int k = k0 + tid;
        WideSlot ws;
        int wide = 0;
        if (k < n) {
            const int fi = plist[k];
            int rad;
            ncc_slot_geometry(uv_tab[2 * fi], uv_tab[2 * fi + 1], S_tab + 4 * fi, &ws.g, &ws.cx, &ws.cy, &rad);
            wide = rad > NCC_MAXRAD;
            rad = min(rad, max(w2, h2)); // a huge or degenerate S: the box is the frame, and nothing below overflows
            ws.slot = k;
            ws.x0 = (int)max((long long)ws.cx - rad, 0LL);
            ws.y0 = (int)max((long long)ws.cy - rad, 0LL);
            ws.x1 = (int)min((long long)ws.cx + rad, (long long)w2 - 1);
            ws.y1 = (int)min((long long)ws.cy + rad, (long long)h2 - 1);
            const bool empty = ws.x1 < ws.x0 || ws.y1 < ws.y0;
            ws.tx = empty ? 0 : (ws.x1 - ws.x0) / NCC_WIDE_TILE + 1;
            ws.ty = empty ? 0 : (ws.y1 - ws.y0) / NCC_WIDE_TILE + 1;
            ws.pad = 0;
        }
        int total;
        const int pos = block_exclusive_scan_1024(wide, s_wtot, &total);
        if (wide) list[base + pos] = ws;
        base += total;
        __syncthreads(); // s_wtot is written again by the next pass
    }
    if (tid == 0) {
        counts[CNT_WIDE_SLOTS] = base;
        counts[CNT_WIDE_CANDS] = 0;
        totals->ncand = 0;
        totals->done = 0;
    }
}

// grid = (tiles of the coarse level, prediction slots): workgroup (t, j) searches tile t of the j-th wide slot's box and writes one
// partial result.  The sums of ncc_key are integers, so the tile's candidates give the bits k_ncc_match would give.
__global__ void __launch_bounds__(256)
k_ncc_wide_coarse(Pyr pyr, const int *plist, const uint8_t *tmpl, const WideSlot *list, const int *counts, WidePartial *part, int max_tiles)
{
    __shared__ uint8_t s_win[WIDE_WIN * WIDE_WIN];
    __shared__ uint8_t s_t[NCC_TT + 3];
    __shared__ int s_tsum[2];
    __shared__ double s_key[4];
    __shared__ int s_idx[4];
    __shared__ int s_cnt[4];

    const int j = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    if (j >= counts[CNT_WIDE_SLOTS]) return;
    const WideSlot &ws = list[j];
    const int ntx = ws.tx;
    if (tile >= ntx * ws.ty) return;
    const int cx = ws.cx, cy = ws.cy;
    const int tx0 = ws.x0 + (tile % ntx) * NCC_WIDE_TILE, ty0 = ws.y0 + (tile / ntx) * NCC_WIDE_TILE;
    const int cwx = min(NCC_WIDE_TILE, ws.x1 - tx0 + 1), cwy = min(NCC_WIDE_TILE, ws.y1 - ty0 + 1); // inside the frame: the box is
    const Gate g = ws.g;
    const int fi = plist[ws.slot];
    const int wr = cwx + 2 * NCC_R, hr = cwy + 2 * NCC_R;
    for (int i = tid; i < WIDE_WIN * hr; i += 256) {
        const int ix = i % WIDE_WIN, iy = i / WIDE_WIN;
        if (ix < wr) s_win[i] = (uint8_t)pyr_at(pyr, 2, tx0 - NCC_R + ix, ty0 - NCC_R + iy);
    }
    if (tid < NCC_TT) s_t[tid] = tmpl[((size_t)fi * 3 + 2) * NCC_TT + tid];
    __syncthreads();
    if (tid == 0) {
        int st = 0, stt = 0;
        for (int i = 0; i < NCC_TT; ++i) { st += s_t[i]; stt += s_t[i] * s_t[i]; }
        s_tsum[0] = st; s_tsum[1] = stt;
    }
    __syncthreads();
    const int st = s_tsum[0], stt = s_tsum[1], w2 = pyr.w[2];
    double key = -3.0;
    int idx = 0x7fffffff, ncand = 0;
    for (int c = tid; c < NCC_WIDE_TILE * NCC_WIDE_TILE; c += 256) {
        const int ox = c % NCC_WIDE_TILE, oy = c / NCC_WIDE_TILE, x = tx0 + ox, y = ty0 + oy;
        if (ox >= cwx || oy >= cwy) continue;
        if (!(x == cx && y == cy)) {
            const float fx = (float)((x + 0.5) * 4 - 0.5), fy = (float)((y + 0.5) * 4 - 0.5);
            if (!gate_contains(g, (double)fx, (double)fy)) continue;
        }
        const double kk = ncc_key(s_win, WIDE_WIN, ox, oy, s_t, st, stt);
        ++ncand;
        if (kk > key) { key = kk; idx = y * w2 + x; } // (y, x) ascending per thread: first maximum kept
    }
    for (int o = 32; o > 0; o >>= 1) ncand += __shfl_down(ncand, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = ncand;
    block_argmax(key, idx, s_key, s_idx); // (its barriers order s_cnt too)
    if (tid == 0) {
        WidePartial p;
        p.key = key;
        p.idx = idx;
        p.ncand = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        part[(size_t)j * max_tiles + tile] = p;
    }
}

// One workgroup per wide slot: the best of its tiles (larger key, then the smaller (y, x): block_argmax's rule, whatever the order
// of the tiles), then levels 1 and 0 and the tail of k_ncc_match.
template <bool SUBPIX>
__global__ void __launch_bounds__(256)
k_ncc_wide_finish(Pyr pyr, const int *plist, const uint8_t *tmpl, const WideSlot *list, const WidePartial *part, int max_tiles,
                  WideTotals *totals, int *mt_valid, EkfKeypoint *mt_xy, float *mt_dist, int *counts)
{
    __shared__ Gate g;
    __shared__ uint8_t s_win[14 * 14 + 4]; // 4 x 4 children and their border; the 13 x 13 window of the sub-pixel fit
    __shared__ uint8_t s_t[NCC_TT + 3];
    __shared__ int s_tsum[2];
    __shared__ double s_key[4];
    __shared__ int s_idx[4];
    __shared__ int s_cnt[4];

    const int j = blockIdx.x, tid = threadIdx.x;
    if (j >= counts[CNT_WIDE_SLOTS]) return;
    const WideSlot &ws = list[j];
    const int k = ws.slot, fi = plist[k], ntiles = ws.tx * ws.ty;
    if (tid == 0) g = ws.g;
    double key = -3.0;
    int idx = 0x7fffffff, ncand = 0;
    for (int t = tid; t < ntiles; t += 256) {
        const WidePartial p = part[(size_t)j * max_tiles + t];
        ncand += p.ncand;
        if (p.key > key || (p.key == key && p.idx < idx)) { key = p.key; idx = p.idx; }
    }
    for (int o = 32; o > 0; o >>= 1) ncand += __shfl_down(ncand, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = ncand;
    block_argmax(key, idx, s_key, s_idx); // (its barriers order g and s_cnt too)
    if (tid == 0) {
        // the candidates are summed in 64 bits by plain atomic adds (a compare-and-swap loop on one counter by a thousand workgroups
        // took milliseconds); the slot that finishes last writes the saturated sum to the counter block
        atomicAdd(&totals->ncand, (unsigned long long)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]));
        __threadfence();
        if (atomicAdd(&totals->done, 1u) == (unsigned)counts[CNT_WIDE_SLOTS] - 1u) {
            __threadfence();
            const unsigned long long sum = atomicAdd(&totals->ncand, 0ull);
            counts[CNT_WIDE_CANDS] = sum > 0x7fffffffull ? 0x7fffffff : (int)sum;
        }
    }
    int bx = ws.cx, by = ws.cy;
    if (idx != 0x7fffffff) { bx = idx % pyr.w[2]; by = idx / pyr.w[2]; }
    double bkey = key;
    for (int l = 1; l >= 0; --l)
        ncc_search_level(pyr, l, 2 * bx - 1, 2 * by - 1, 4, tmpl + ((size_t)fi * 3 + l) * NCC_TT, g, 0, 0, s_win, s_t, s_tsum, s_key, s_idx,
                         bx, by, bkey);
    ncc_finish_slot<SUBPIX>(pyr, g, k, bx, by, bkey, s_win, s_t, s_tsum, s_key, mt_valid, mt_xy, mt_dist, counts);
}

static Pyr pyr_of(const EkfEngine *e)
{
    Pyr p;
    for (int l = 0; l < 3; ++l) { p.px[l] = e->img.px[l]; p.w[l] = e->img.w[l]; p.h[l] = e->img.h[l]; }
    return p;
}

void launch_ncc_pyramid_on(EkfEngine *e, hipStream_t stream, uint8_t *const px[3], const uint8_t *d_raw, int stride, int channels)
{
    const int w = e->img.w[0], h = e->img.h[0];
    k_ncc_gray<<<dim3((w + 255) / 256, h), 256, 0, stream>>>(d_raw, w, h, stride, channels, px[0]);
    for (int l = 1; l < 3; ++l)
        if (e->img.w[l] > 0 && e->img.h[l] > 0)
            k_ncc_down<<<dim3((e->img.w[l] + 255) / 256, e->img.h[l]), 256, 0, stream>>>(px[l - 1], e->img.w[l - 1], px[l],
                                                                                         e->img.w[l], e->img.h[l]);
}

void launch_ncc_pyramid(EkfEngine *e, const uint8_t *d_raw, int stride, int channels)
{
    launch_ncc_pyramid_on(e, e->stream, e->img.px, d_raw, stride, channels);
}

void launch_ncc_capture(EkfEngine *e, const int *d_idx, const double *d_uv, int count)
{
    if (count > 0) k_ncc_capture<<<dim3(count, 3), 128, 0, e->stream>>>(pyr_of(e), d_idx, d_uv, e->d.tmpl);
}

void launch_ncc_warp_capture(EkfEngine *e, const int *d_idx, const double *d_uv, int count, bool keep)
{
    if (count > 0)
        k_ncc_warp_capture<<<dim3(count, 3), 256, 0, e->stream>>>(pyr_of(e), d_idx, d_uv, e->d.state, e->d.wsrc, e->d.wpose, keep ? 1 : 0,
                                                                  e->d.wnorm);
}

void launch_ncc_normal(EkfEngine *e, int M)
{
    (void)hipMemsetAsync(e->d.counts + CNT_PN_UPD, 0, 2 * sizeof(int), e->stream);
    if (M > 0)
        k_ncc_normal<<<M, 384, 0, e->stream>>>(pyr_of(e), e->d.pn_list, M, e->N, e->d.state, e->cam, e->d.feat_pos, e->d.feat_type, e->d.wsrc,
                                               e->d.wpose, e->d.wnorm, e->d.counts);
}

void launch_match_compact_slots(EkfEngine *e, int n_pred, const EkfKeypoint *d_slot_xy);

// the templates this match compares: the stored ones, or (ekf_set_template_warp) their re-rendering from the predicted pose
static const uint8_t *match_templates(EkfEngine *e, int n_pred)
{
    if (!e->warp_on) return e->d.tmpl;
    (void)hipMemsetAsync(e->d.counts + CNT_WARP_OK, 0, 2 * sizeof(int), e->stream);
    (void)hipMemcpyAsync(e->d.wtmpl, e->d.tmpl, (size_t)e->N * 3 * NCC_TT, hipMemcpyDeviceToDevice, e->stream);
    if (n_pred > 0)
        k_ncc_warp<<<n_pred, 384, 0, e->stream>>>(e->d.plist, e->d.counts + CNT_NPRED, e->d.pred_uv, e->d.state, e->cam, e->d.feat_pos,
                                                  e->d.feat_type, e->d.wsrc, e->d.wpose, e->d.wtmpl, e->d.counts,
                                                  e->pn_on ? e->d.wnorm : nullptr);
    return e->d.wtmpl;
}

// the NCC search of the prediction slots [s_lo, s_hi); subpix: with the parabola fit, whose axis counters it zeroes first
static void match_ncc_slots(EkfEngine *e, const uint8_t *tmpl, int s_lo, int s_hi, bool subpix, bool skip_wide = false)
{
    if (subpix) {
        (void)hipMemsetAsync(e->d.counts + CNT_SUBPIX_FIT, 0, sizeof(int), e->stream);
        (void)hipMemsetAsync(e->d.counts + CNT_SUBPIX_INT, 0, sizeof(int), e->stream);
    }
    if (s_hi <= s_lo) return;
    auto kern = subpix ? k_ncc_match<true> : k_ncc_match<false>;
    kern<<<s_hi - s_lo, 256, 0, e->stream>>>(pyr_of(e), e->d.plist, e->d.pred_uv, e->d.pred_S, tmpl, e->d.mt_valid, e->d.mt_xy,
                                             e->d.mt_dist, s_lo, e->d.counts, skip_wide ? 1 : 0);
}

void launch_match_ncc(EkfEngine *e, int n_pred, bool subpix, bool wide)
{
    const uint8_t *tmpl = match_templates(e, n_pred);
    WideSlot *list = (WideSlot *)e->d.wide_list;
    WideTotals *totals = (WideTotals *)((uint8_t *)e->d.wide_list + (size_t)e->cap * NCC_WIDE_SLOT_BYTES);
    if (wide && n_pred > 0) // before k_ncc_match: it zeroes CNT_WIDE_CANDS, and nothing of the wide path depends on the narrow one
        k_ncc_wide_classify<<<1, 1024, 0, e->stream>>>(e->d.plist, e->d.counts + CNT_NPRED, n_pred, e->d.pred_uv, e->d.pred_S, e->img.w[2],
                                                       e->img.h[2], list, totals, e->d.counts);
    match_ncc_slots(e, tmpl, 0, n_pred, subpix, wide);
    if (n_pred <= 0) {
        (void)hipMemsetAsync(e->d.counts + CNT_NMATCH, 0, sizeof(int), e->stream);
        if (wide) (void)hipMemsetAsync(e->d.counts + CNT_WIDE_SLOTS, 0, 2 * sizeof(int), e->stream);
        return;
    }
    if (wide) { // k_ncc_match has skipped the wide slots (and left their sub-pixel counts to k_ncc_wide_finish)
        const int tiles = ncc_wide_tiles(e->img.w[2], e->img.h[2]);
        WidePartial *part = (WidePartial *)e->d.wide_part;
        k_ncc_wide_coarse<<<dim3(tiles, n_pred), 256, 0, e->stream>>>(pyr_of(e), e->d.plist, tmpl, list, e->d.counts, part, e->wide_tiles);
        auto fin = subpix ? k_ncc_wide_finish<true> : k_ncc_wide_finish<false>;
        fin<<<n_pred, 256, 0, e->stream>>>(pyr_of(e), e->d.plist, tmpl, list, part, e->wide_tiles, totals, e->d.mt_valid, e->d.mt_xy, e->d.mt_dist,
                                            e->d.counts);
    }
    launch_match_compact_slots(e, n_pred, e->d.mt_xy);
}

// sharded filter: the NCC search of the prediction slots [s_lo, s_hi) only (see launch_match_slots, kernels_match.hip); the per-slot
// tables are completed by an all-gather and compacted by launch_match_compact_slots on every rank
// (subpix: a sharded engine refuses ekf_set_subpixel_matches, so its callers pass false; the axis counters of a rank would
// cover its own slots only)
void launch_match_ncc_slots(EkfEngine *e, int s_lo, int s_hi, bool subpix)
{
    match_ncc_slots(e, e->d.tmpl, s_lo, s_hi, subpix);
}

} // namespace ekf
