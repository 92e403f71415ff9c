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

constexpr int NCC_R = 5, NCC_T = 11, NCC_MAXRAD = 16; // (NCC_TT = NCC_T * NCC_T: engine.h)
constexpr int NCC_BLOCK = 256;   // lanes of the matching kernels' workgroups (k_ncc_match, k_ncc_wide_coarse, k_ncc_wide_finish)
constexpr int PATCH_BLOCK = 384; // ... and of k_ncc_warp / k_ncc_normal: 128 per pyramid level
static_assert(NCC_TT == NCC_T * NCC_T, "engine.h sizes the template tables");
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

// ---- patch-plane geometry --------------------------------------------------------------
// A template is the image of a small plane through the feature's world point X.  k_ncc_warp_capture keeps, per feature and
// level, the 41 x 41 pixels around the capture pixel and the capture pose; k_ncc_warp and k_ncc_normal re-render template
// pixels from them through one chain, the functions of this block: position of the template pixel at level 0 (tmpl_pos) ->
// ray of the current camera (patch_ray) -> plane -> level-0 position in the capture camera (patch_to_source) -> the level's
// source coordinates (src_coord) -> bilinear sample of the staged source (patch_sample).  The numpy restatements
// (tests/template_warp_ref.py, tests/patch_normal_ref.py) define every result to the bit: fp64, no contraction, this order.
constexpr int WARP_R = WARP_S / 2;

// block = (item, level): source patch; the level-0 block also writes the pose record (keep = 0: zeros = "no source patch")
__global__ void __launch_bounds__(256)
k_ncc_warp_capture(Pyr pyr, const int *feat_idx, const double *uv, const double *st, uint8_t *wsrc, double *wpose, int keep,
                   PatchNormalRec *wnorm)
{
    const int i = blockIdx.x, l = blockIdx.y, fi = feat_idx[i];
    if (l == 0 && threadIdx.x == WPOSE_DOUBLES && wnorm) wnorm[fi] = PatchNormalRec{}; // patch normals: a capture resets the estimate
    if (l == 0 && threadIdx.x < WPOSE_DOUBLES) {
        const int t = threadIdx.x;
        wpose[WPOSE_DOUBLES * (size_t)fi + t] = !keep ? 0.0 : (t < 7 ? st[ST_X + t] : uv[2 * i + t - 7]);
    }
    if (!keep) return;
    const int cx = to_level(uv[2 * i], l), cy = to_level(uv[2 * i + 1], l);
    for (int t = threadIdx.x; t < WARP_SS; t += 256)
        wsrc[((size_t)fi * 3 + l) * WARP_SS + t] = (uint8_t)pyr_at(pyr, l, cx + t % WARP_S - WARP_R, cy + t / WARP_S - WARP_R);
}

// what the chain needs of one feature, in LDS: world point, rotation and position of the current camera (R, r) and of the
// capture camera (R0, r0), capture pixel per level
struct PatchView {
    double X[3], R[9], R0[9], r[3], r0[3];
    int uv0[3][2];
};
// a plane through X: unit normal in world axes, pointing to the side the capture camera saw, and n . (X - r)
struct PatchPlane {
    double n[3], nXr;
};

// one lane: the view of feature fi from the filter state st, the map tables and the feature's capture pose record
__device__ __forceinline__ void patch_view_fill(PatchView &v, const double *st, const double *feat_pos, const int *feat_type, int fi,
                                                const double *pose)
{
    const double *x = st + ST_X;
    patch_world_point(feat_pos + 6 * (size_t)fi, feat_type[fi], v.X);
    quat_to_rot(x + 3, v.R);
    quat_to_rot(pose + 3, v.R0);
    for (int i = 0; i < 3; ++i) {
        v.r[i] = x[i];
        v.r0[i] = pose[i];
    }
    for (int l = 0; l < 3; ++l) {
        v.uv0[l][0] = to_level(pose[7], l);
        v.uv0[l][1] = to_level(pose[8], l);
    }
}

__device__ __forceinline__ void patch_plane_set(PatchPlane &pl, const PatchView &v, const double *n)
{
    double nXr = 0.0;
    for (int i = 0; i < 3; ++i) {
        pl.n[i] = n[i];
        nXr += n[i] * (v.X[i] - v.r[i]);
    }
    pl.nXr = nXr;
}

// the three source levels of feature fi into LDS, by the whole workgroup (the caller's barrier follows)
__device__ __forceinline__ void patch_stage_source(uint8_t *s_src, const uint8_t *wsrc, int fi)
{
    for (int i = threadIdx.x; i < 3 * WARP_SS; i += PATCH_BLOCK) s_src[i] = wsrc[(size_t)fi * 3 * WARP_SS + i];
}

// level-0 position of the centre of template pixel o (0..10 along one axis) of the template centred on pixel cl of the level of scale sc
__device__ __forceinline__ double tmpl_pos(int cl, int o, double sc) { return ((double)(cl + o - NCC_R) + 0.5) * sc - 0.5; }

// ray of the level-0 position (px, py) in world axes: undistortPoint (closed form), then R
__device__ __forceinline__ void patch_ray(const CamD &c, const double *R, double px, double py, double *d)
{
    const double pdx = px - c.cx, pdy = py - c.cy;
    const double mx = c.dx * pdx, my = c.dy * pdy;
    const double rd2 = mx * mx + my * my;
    const double f = 1.0 + c.k1 * rd2 + c.k2 * rd2 * rd2;
    const double hc[3] = {pdx * f / c.fx, pdy * f / c.fy, 1.0};
    mat3_vec(R, hc, d);
}

// where the ray d from r meets the plane, projected into the capture camera and distorted: level-0 position s; false: the ray
// does not meet the plane's front (n . d < 0 does), or meets it behind one of the two cameras
__device__ __forceinline__ bool patch_to_source(const CamD &c, const PatchView &v, const PatchPlane &pl, const double *d, double *s)
{
    const double nd = pl.n[0] * d[0] + pl.n[1] * d[1] + pl.n[2] * d[2];
    if (!(nd < 0.0)) return false;
    const double lam = pl.nXr / nd;
    if (!(lam > 0.0)) return false;
    const double w[3] = {v.r[0] + lam * d[0] - v.r0[0], v.r[1] + lam * d[1] - v.r0[1], v.r[2] + lam * d[2] - v.r0[2]};
    const double h0 = v.R0[0] * w[0] + v.R0[3] * w[1] + v.R0[6] * w[2];
    const double h1 = v.R0[1] * w[0] + v.R0[4] * w[1] + v.R0[7] * w[2];
    const double h2 = v.R0[2] * w[0] + v.R0[5] * w[1] + v.R0[8] * w[2];
    if (!(h2 > 0.0)) return false;
    distort(c, c.cx + c.fx * h0 / h2, c.cy + c.fy * h1 / h2, s);
    return true;
}

// one axis of the level-0 position s in the coordinates of the source patch of the level of scale sc, whose centre is pixel uv0l
__device__ __forceinline__ double src_coord(double s, double sc, int uv0l) { return (s + 0.5) / sc - 0.5 - (double)(uv0l - WARP_R); }

// bilinear sample of the staged source of level l at (sx, sy); false outside [0, WARP_S - 1]^2
__device__ __forceinline__ bool patch_sample(const uint8_t *s_src, int l, double sx, double sy, double *b)
{
    if (!(sx >= 0.0 && sx <= (double)(WARP_S - 1) && sy >= 0.0 && sy <= (double)(WARP_S - 1))) return false;
    const int x0 = min((int)floor(sx), WARP_S - 2), y0 = min((int)floor(sy), WARP_S - 2);
    const double ax = sx - (double)x0, ay = sy - (double)y0;
    const uint8_t *p = s_src + l * WARP_SS + y0 * WARP_S + x0;
    const double top = (1.0 - ax) * (double)p[0] + ax * (double)p[1];
    const double bot = (1.0 - ax) * (double)p[WARP_S] + ax * (double)p[WARP_S + 1];
    *b = (1.0 - ay) * top + ay * bot;
    return true;
}

// ---- template warp -------------------------------------------------------------------------
// k_ncc_warp re-renders the 11 x 11 template of every prediction slot from the current pose estimate before the search.  The
// plane faces the camera which first saw the feature (n = a / |a|, a = r0 - X) or, with patch normals on, has the estimated
// slope.  A level whose samples leave the source (or whose geometry is degenerate) keeps the stored template, whole.
// One workgroup per prediction slot, 128 lanes per level (121 active): fp64, everything a lane touches after the staging
// is in LDS (5 KB of source bytes, 34 doubles of constants).  Latency-bound like k_ncc_match: ~0.4 KFLOP and one 10-step
// Newton solve per lane.  out already holds a copy of the stored templates; only whole warped levels are written.
__global__ void __launch_bounds__(PATCH_BLOCK)
k_ncc_warp(const int *plist, const int *d_npred, const double *uv_tab, const double *st, CamD c, const double *feat_pos,
           const int *feat_type, const uint8_t *wsrc, const double *wpose, uint8_t *out, int *counts, const PatchNormalRec *wnorm)
{
    __shared__ uint8_t s_src[3 * WARP_SS + 1];
    __shared__ PatchView s_v;
    __shared__ PatchPlane s_pl;
    __shared__ int s_bad[3];

    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= *d_npred) return;
    const int fi = plist[k];
    const double *pose = wpose + WPOSE_DOUBLES * (size_t)fi;
    if (!patch_has_source(pose)) { // uniform over the block
        if (tid == 0) atomicAdd(counts + CNT_WARP_FB, 3);
        return;
    }
    patch_stage_source(s_src, wsrc, fi);
    if (tid < 3) s_bad[tid] = 0;
    if (tid == 0) {
        patch_view_fill(s_v, st, feat_pos, feat_type, fi, pose);
        double n[3];
        if (wnorm && wnorm[fi].updates > 0) { // patch normals: n(p, q) instead of the rule
            pn_normal(s_v.R0, wnorm[fi].pq[0], wnorm[fi].pq[1], n);
        } else {
            const double a[3] = {s_v.r0[0] - s_v.X[0], s_v.r0[1] - s_v.X[1], s_v.r0[2] - s_v.X[2]};
            const double an = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            for (int i = 0; i < 3; ++i) n[i] = a[i] / an;
        }
        patch_plane_set(s_pl, s_v, n);
    }
    __syncthreads();

    const int l = tid >> 7, t = tid & 127;
    const bool live = t < NCC_TT;
    const double sc = (double)(1 << l);
    int val = 0;
    if (live) {
        const int cxl = to_level(uv_tab[2 * fi], l), cyl = to_level(uv_tab[2 * fi + 1], l);
        double d[3], s[2], b;
        patch_ray(c, s_v.R, tmpl_pos(cxl, t % NCC_T, sc), tmpl_pos(cyl, t / NCC_T, sc), d);
        if (patch_to_source(c, s_v, s_pl, d, s) &&
            patch_sample(s_src, l, src_coord(s[0], sc, s_v.uv0[l][0]), src_coord(s[1], sc, s_v.uv0[l][1]), &b))
            val = min(max((int)floor(b + 0.5), 0), 255);
        else
            s_bad[l] = 1; // any lane of the level: the whole level falls back
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
constexpr int PN_VEC = 6; // vectors per level: the prediction at the five slopes, the measurement

// One workgroup per match, 128 lanes per level (121 active, lanes 121..125 of level 0 carry the anchor at the five slopes).
// Latency-bound: five plane intersections and Newton solves per lane, six barriers-separated serial sums of 121 terms by six lanes
// per level (the order of the restatement), 18 KB of vectors and 5 KB of source bytes in LDS.
__global__ void __launch_bounds__(PATCH_BLOCK)
k_ncc_normal(Pyr pyr, const EkfMatch *list, int M, int N, const double *st, CamD c, const double *feat_pos, const int *feat_type,
             const uint8_t *wsrc, const double *wpose, PatchNormalRec *wnorm, int *counts)
{
    __shared__ uint8_t s_src[3 * WARP_SS + 1];
    __shared__ double s_vec[3][PN_VEC][128];
    __shared__ double s_sum[3][PN_VEC];
    __shared__ PatchView s_v;
    __shared__ PatchPlane s_pl[5]; // the slope, p + h, p - h, q + h, q - h
    __shared__ double s_anc[5][2], s_pq[2];
    __shared__ int s_bad[3], s_anchor[2];

    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= M) return;
    const int fi = list[k].featureIndex;
    if (fi < 0 || fi >= N) return; // (the host validates the list)
    const double *pose = wpose + WPOSE_DOUBLES * (size_t)fi;
    if (!patch_has_source(pose)) { // uniform over the block
        if (tid == 0) atomicAdd(counts + CNT_PN_SKIP, 1);
        return;
    }
    patch_stage_source(s_src, wsrc, fi);
    if (tid < 3) s_bad[tid] = 0;
    if (tid == 0) {
        patch_view_fill(s_v, st, feat_pos, feat_type, fi, pose);
        double pq[2] = {wnorm[fi].pq[0], wnorm[fi].pq[1]};
        if (wnorm[fi].updates <= 0) pn_rule_slope(s_v.R0, s_v.X, s_v.r0, pq); // first update: the rule of 4.6 as a slope
        s_pq[0] = pq[0];
        s_pq[1] = pq[1];
        for (int j = 0; j < 5; ++j) {
            const double dp = j == 1 ? PN_FD_STEP : (j == 2 ? -PN_FD_STEP : 0.0), dq = j == 3 ? PN_FD_STEP : (j == 4 ? -PN_FD_STEP : 0.0);
            double n[3];
            pn_normal(s_v.R0, pq[0] + dp, pq[1] + dq, n);
            patch_plane_set(s_pl[j], s_v, n);
        }
        s_anchor[0] = to_level(list[k].imagePos[0], 0);
        s_anchor[1] = to_level(list[k].imagePos[1], 0);
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
        patch_ray(c, s_v.R, tmpl_pos(cxl, t % NCC_T, sc), tmpl_pos(cyl, t / NCC_T, sc), d);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (!patch_to_source(c, s_v, s_pl[j], d, s5[j])) bad = true;
    } else if (anchor_lane) { // where the anchor itself lands at slope j
        const int j = t - NCC_TT;
        double d[3], s[2] = {0.0, 0.0};
        patch_ray(c, s_v.R, (double)s_anchor[0], (double)s_anchor[1], d);
        if (!patch_to_source(c, s_v, s_pl[j], d, s)) s_bad[0] = s_bad[1] = s_bad[2] = 1;
        s_anc[j][0] = s[0];
        s_anc[j][1] = s[1];
    }
    __syncthreads();
    if (live) {
        const int ux = s_v.uv0[l][0], uy = s_v.uv0[l][1];
        // the source's centre pixel (level 0) in this level's source coordinates: the anchor is moved onto it
        const double ctrx = src_coord((double)s_v.uv0[0][0], sc, ux), ctry = src_coord((double)s_v.uv0[0][1], sc, uy);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double b = 0.0;
            if (!bad) {
                const double sx = src_coord(s5[j][0], sc, ux) - (src_coord(s_anc[j][0], sc, ux) - ctrx);
                const double sy = src_coord(s5[j][1], sc, uy) - (src_coord(s_anc[j][1], sc, uy) - ctry);
                if (!patch_sample(s_src, l, sx, sy, &b)) bad = true;
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

// sum of v over the workgroup in two halves around a barrier the caller has anyway (block_argmax's): every wavefront posts its
// sum to s_cnt (NCC_BLOCK / 64 ints), and after the barrier block_sum_get adds them
__device__ __forceinline__ void block_sum_post(int v, int *s_cnt)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ int block_sum_get(const int *s_cnt)
{
    int v = 0;
    for (int w = 0; w < NCC_BLOCK / 64; ++w) v += s_cnt[w];
    return v;
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

// The candidate scan, shared by every level of k_ncc_match / k_ncc_wide_finish (ncc_search_level) and by the tiles of
// k_ncc_wide_coarse.  The candidate rule, written once: a candidate is a pixel of the scanned box that lies inside the frame and,
// at the coarse level (l == 2), is the predicted pixel (gcx, gcy) or has its centre in the gate; the best one is the first
// maximum of the key in raster order.  block_argmax orders equal keys by idx, the candidate's raster position: in the frame
// (comparable between the tiles of the wide search) or in the box (what the levels of one slot need; undone by a division by a
// constant at the fine levels).

// the level's template tl and its sums (s_tsum = sum, sum of squares) into LDS, by the whole workgroup
__device__ __forceinline__ void ncc_stage_template(const uint8_t *tl, uint8_t *s_t, int *s_tsum)
{
    const int tid = threadIdx.x;
    if (tid < NCC_TT) s_t[tid] = tl[tid];
    __syncthreads();
    if (tid == 0) {
        int st = 0, stt = 0;
        for (int i = 0; i < NCC_TT; ++i) { st += s_t[i]; stt += s_t[i] * s_t[i]; }
        s_tsum[0] = st; s_tsum[1] = stt;
    }
    __syncthreads();
}

// Stages the (cwx + 10) x (cwy + 10) window of the box of cwx x cwy candidates that starts at (x0, y0) and the template, and scans
// the box: the lane's best key (-3: none) and its idx (0x7fffffff: none).  The two callers differ at compile time only:
//   TILE = false (ncc_search_level): a square box, cwx == cwy, rows of cwx candidates, idx = the position in the box;
//   TILE = true (k_ncc_wide_coarse): a box of up to 32 x 32 in rows of NCC_WIDE_TILE (no division), idx = y * w[l] + x, and the
//   candidates the lane evaluated are counted in ncand.
// EXCL (the rival pass of the distinctiveness test): the candidates within NCC_RIVAL_EXCL pixels (Chebyshev) of
// (ex, ey) are left out; SCAN_EXCL_STAGED: and the window and the template are those an earlier scan of the same box staged.
enum { SCAN_ALL = 0, SCAN_EXCL = 1, SCAN_EXCL_STAGED = 2 };
constexpr int NCC_RIVAL_EXCL = 2; // the best peak's own lobe: 5 x 5 coarse pixels
template <bool TILE, int EXCL = SCAN_ALL>
__device__ __forceinline__ void ncc_scan(const Pyr &pyr, int l, int x0, int y0, int cwx, int cwy, const uint8_t *tl, const Gate &g, int gcx,
                                         int gcy, uint8_t *s_win, uint8_t *s_t, int *s_tsum, double &key, int &idx, int &ncand, int ex = 0,
                                         int ey = 0)
{
    const int tid = threadIdx.x, row = TILE ? NCC_WIDE_TILE : cwx, pitch = row + 2 * NCC_R;
    if constexpr (EXCL != SCAN_EXCL_STAGED) {
        for (int i = tid; i < pitch * (cwy + 2 * NCC_R); i += NCC_BLOCK) {
            const int ix = i % pitch, iy = i / pitch;
            if (!TILE || ix < cwx + 2 * NCC_R) s_win[i] = (uint8_t)pyr_at(pyr, l, x0 - NCC_R + ix, y0 - NCC_R + iy);
        }
        ncc_stage_template(tl, s_t, s_tsum);
    }
    const int st = s_tsum[0], stt = s_tsum[1];
    key = -3.0;
    idx = 0x7fffffff;
    ncand = 0;
    for (int c = tid; c < row * cwy; c += NCC_BLOCK) {
        const int ox = c % row, oy = c / row, x = x0 + ox, y = y0 + oy;
        if (TILE && ox >= cwx) continue;
        if (x < 0 || y < 0 || x >= pyr.w[l] || y >= pyr.h[l]) continue;
        if constexpr (EXCL != SCAN_ALL)
            if (abs(x - ex) <= NCC_RIVAL_EXCL && abs(y - ey) <= NCC_RIVAL_EXCL) continue;
        if (l == 2 && !(x == gcx && y == gcy)) {
            const float fx = (float)((x + 0.5) * 4 - 0.5), fy = (float)((y + 0.5) * 4 - 0.5);
            if (!gate_contains(g, (double)fx, (double)fy)) continue;
        }
        const double kk = ncc_key(s_win, pitch, ox, oy, s_t, st, stt);
        if (TILE) ++ncand;
        if (kk > key) { key = kk; idx = TILE ? y * pyr.w[l] + x : c; } // (y, x) ascending per lane: first maximum kept
    }
}

// One level of the search by the whole workgroup (256 lanes): scans the cw x cw candidates that start at (x0, y0) and leaves the
// best one in (bx, by), its key in bkey: -3 and an unchanged position when the level had no candidate (position carried over, as
// the CPU loop does).  s_t and s_tsum keep the level's template and its sums.
__device__ __forceinline__ void ncc_search_level(const Pyr &pyr, int l, int x0, int y0, int cw, const uint8_t *tl, const Gate &g, int gcx,
                                                 int gcy, uint8_t *s_win, uint8_t *s_t, int *s_tsum, double *s_key, int *s_idx, int &bx,
                                                 int &by, double &bkey)
{
    double key;
    int idx, ncand;
    ncc_scan<false>(pyr, l, x0, y0, cw, cw, tl, g, gcx, gcy, s_win, s_t, s_tsum, key, idx, ncand);
    block_argmax(key, idx, s_key, s_idx);
    if (idx != 0x7fffffff) { bx = x0 + idx % cw; by = y0 + idx / cw; }
    bkey = key;
}

// Levels 1 and 0 from the coarse pixel (bx, by): the 4 x 4 children of the best parent, twice.  t3 = the feature's three templates.
__device__ __forceinline__ void ncc_refine(const Pyr &pyr, const uint8_t *t3, const Gate &g, uint8_t *s_win, uint8_t *s_t, int *s_tsum,
                                           double *s_key, int *s_idx, int &bx, int &by, double &bkey)
{
    for (int l = 1; l >= 0; --l)
        ncc_search_level(pyr, l, 2 * bx - 1, 2 * by - 1, 4, t3 + l * NCC_TT, g, 0, 0, s_win, s_t, s_tsum, s_key, s_idx, bx, by, bkey);
}

// Distinctiveness test (ekf_set_ncc_distinct; tests/ncc_distinct_ref.py is the definition): the slot's table and
// the coefficient, and what the rival pass of one slot found (uniform over the workgroup)
struct NccRivalOut {
    NccRivalRec *tab;
    double coef;
};
struct NccRival {
    int x, y;   // coarse pixel, then the refined level-0 pixel
    double key; // < 0: no rival
};

// What follows the level-0 search of prediction slot k, by the whole workgroup: the acceptance test and the slot's entries of the
// match tables.  SUBPIX (ekf_set_subpixel_matches): the keys of the best pixel's four level-0 neighbours are evaluated first and
// each axis of the reported position is moved by subpix_offset; counts then receives the fitted / integer axes of the valid
// matches.  SUBPIX = false is the integer matcher as it was.  s_t and s_tsum still hold the level-0 template and its sums.
// RIVAL: an accepted match whose refined rival rv lies in the gate is kept only if d1 < d2 * coef; the slot's record goes to out.tab.
template <bool SUBPIX, bool RIVAL>
__device__ __forceinline__ void ncc_finish_slot(const Pyr &pyr, const Gate &g, int k, int bx, int by, double bkey, uint8_t *s_win,
                                                const uint8_t *s_t, const int *s_tsum, double *s_key, int *mt_valid, EkfKeypoint *mt_xy,
                                                float *mt_dist, int *counts, const NccRival &rv, const NccRivalOut &out)
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
        bool ok = bkey >= 0.64 && gate_contains(g, (double)(float)bx, (double)(float)by);
        if constexpr (RIVAL) {
            NccRivalRec rec = {ok ? 1 : 0, 0, 0, ok ? (float)(1.0 - sqrt(bkey)) : 0.f, 0.f};
            if (ok && rv.key >= 0.0 && gate_contains(g, (double)(float)rv.x, (double)(float)rv.y)) { // a place that could have been accepted
                rec.rx = rv.x;
                rec.ry = rv.y;
                rec.d2 = (float)(1.0 - sqrt(rv.key));
                ok = (double)rec.d1 < (double)rec.d2 * out.coef; // strict: two perfect repetitions are ambiguous
                rec.state = ok ? 2 : 3;
                atomicAdd(counts + CNT_RIVAL_WITH, 1);
                if (!ok) atomicAdd(counts + CNT_RIVAL_REJ, 1);
            }
            out.tab[k] = rec;
        }
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
// RIVAL: the coarse window staged in LDS is scanned a second time without the 5 x 5 block around the coarse best,
// and the best of that pass is refined like the best itself.
template <bool SUBPIX, bool RIVAL>
__global__ void __launch_bounds__(256)
k_ncc_match(Pyr pyr, const int *plist, const double *uv_tab, const double *S_tab, const uint8_t *tmpl,
            int *mt_valid, EkfKeypoint *mt_xy, float *mt_dist, int slot0, int *counts, int skip_wide, NccRivalOut rout)
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
    const uint8_t *t3 = tmpl + (size_t)fi * 3 * NCC_TT;
    // coarse level: the gated square around the prediction; then the 4x4 children, twice
    const int x0 = s_geom[0] - s_geom[2], y0 = s_geom[1] - s_geom[2], cw = 2 * s_geom[2] + 1;
    ncc_search_level(pyr, 2, x0, y0, cw, t3 + 2 * NCC_TT, g, s_geom[0], s_geom[1], s_win, s_t, s_tsum, s_key, s_idx, bx, by, bkey);
    NccRival rv = {0, 0, -3.0};
    if constexpr (RIVAL) { // the keys outside the block are evaluated again: fewer registers than keeping them
        int idx, ncand;
        ncc_scan<false, SCAN_EXCL_STAGED>(pyr, 2, x0, y0, cw, cw, nullptr, g, s_geom[0], s_geom[1], s_win, s_t, s_tsum, rv.key, idx, ncand, bx, by);
        block_argmax(rv.key, idx, s_key, s_idx);
        if (rv.key >= 0.0) { // uniform
            rv.x = x0 + idx % cw;
            rv.y = y0 + idx / cw;
            ncc_refine(pyr, t3, g, s_win, s_t, s_tsum, s_key, s_idx, rv.x, rv.y, rv.key);
        }
    }
    ncc_refine(pyr, t3, g, s_win, s_t, s_tsum, s_key, s_idx, bx, by, bkey); // (last: s_t ends as the level-0 template either way)
    ncc_finish_slot<SUBPIX, RIVAL>(pyr, g, k, bx, by, bkey, s_win, s_t, s_tsum, s_key, mt_valid, mt_xy, mt_dist, counts, rv, rout);
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
// RIVAL: a second launch behind the first.  Every workgroup reduces the slot's partials of the first launch (first)
// to the coarse best, as k_ncc_wide_finish does -- a handful of records, and no order of the tiles can change the result --, and
// scans its tile without the block around it.
template <bool RIVAL>
__global__ void __launch_bounds__(256)
k_ncc_wide_coarse(Pyr pyr, const int *plist, const uint8_t *tmpl, const WideSlot *list, const int *counts, WidePartial *part, int max_tiles,
                  const WidePartial *first)
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
    const int tx0 = ws.x0 + (tile % ntx) * NCC_WIDE_TILE, ty0 = ws.y0 + (tile / ntx) * NCC_WIDE_TILE;
    const int cwx = min(NCC_WIDE_TILE, ws.x1 - tx0 + 1), cwy = min(NCC_WIDE_TILE, ws.y1 - ty0 + 1); // inside the frame: the box is
    const Gate g = ws.g;
    const int fi = plist[ws.slot];
    double key;
    int idx, ncand, ex = 0, ey = 0;
    if constexpr (RIVAL) {
        key = -3.0;
        idx = 0x7fffffff;
        for (int t = tid; t < ntx * ws.ty; t += NCC_BLOCK) {
            const WidePartial p = first[(size_t)j * max_tiles + t];
            if (p.key > key || (p.key == key && p.idx < idx)) { key = p.key; idx = p.idx; }
        }
        block_argmax(key, idx, s_key, s_idx);
        if (idx == 0x7fffffff) { // uniform: the slot has no candidate at all
            if (tid == 0) part[(size_t)j * max_tiles + tile] = WidePartial{-3.0, 0x7fffffff, 0};
            return;
        }
        ex = idx % pyr.w[2];
        ey = idx / pyr.w[2];
    }
    ncc_scan<true, RIVAL ? SCAN_EXCL : SCAN_ALL>(pyr, 2, tx0, ty0, cwx, cwy, tmpl + ((size_t)fi * 3 + 2) * NCC_TT, g, ws.cx, ws.cy, s_win, s_t,
                                                 s_tsum, key, idx, ncand, ex, ey);
    block_sum_post(ncand, s_cnt);
    block_argmax(key, idx, s_key, s_idx); // (its barriers order s_cnt too)
    if (tid == 0) {
        WidePartial p;
        p.key = key;
        p.idx = idx;
        p.ncand = block_sum_get(s_cnt);
        part[(size_t)j * max_tiles + tile] = p;
    }
}

// One workgroup per wide slot: the best of its tiles (larger key, then the smaller (y, x): block_argmax's rule, whatever the order
// of the tiles), then levels 1 and 0 and the tail of k_ncc_match.  RIVAL: the rival pass's table part2 is reduced the same way.
template <bool SUBPIX, bool RIVAL>
__global__ void __launch_bounds__(256)
k_ncc_wide_finish(Pyr pyr, const int *plist, const uint8_t *tmpl, const WideSlot *list, const WidePartial *part, int max_tiles,
                  WideTotals *totals, int *mt_valid, EkfKeypoint *mt_xy, float *mt_dist, int *counts, const WidePartial *part2,
                  NccRivalOut rout)
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
    block_sum_post(ncand, s_cnt);
    block_argmax(key, idx, s_key, s_idx); // (its barriers order g and s_cnt too)
    if (tid == 0) {
        // the candidates are summed in 64 bits by plain atomic adds (a compare-and-swap loop on one counter by a thousand workgroups
        // took milliseconds); the slot that finishes last writes the saturated sum to the counter block
        atomicAdd(&totals->ncand, (unsigned long long)block_sum_get(s_cnt));
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
    const uint8_t *t3 = tmpl + (size_t)fi * 3 * NCC_TT;
    NccRival rv = {0, 0, -3.0};
    if constexpr (RIVAL) {
        int ridx = 0x7fffffff;
        for (int t = tid; t < ntiles; t += NCC_BLOCK) {
            const WidePartial p = part2[(size_t)j * max_tiles + t];
            if (p.key > rv.key || (p.key == rv.key && p.idx < ridx)) { rv.key = p.key; ridx = p.idx; }
        }
        block_argmax(rv.key, ridx, s_key, s_idx);
        if (rv.key >= 0.0) { // uniform
            rv.x = ridx % pyr.w[2];
            rv.y = ridx / pyr.w[2];
            ncc_refine(pyr, t3, g, s_win, s_t, s_tsum, s_key, s_idx, rv.x, rv.y, rv.key);
        }
    }
    ncc_refine(pyr, t3, g, s_win, s_t, s_tsum, s_key, s_idx, bx, by, bkey);
    ncc_finish_slot<SUBPIX, RIVAL>(pyr, g, k, bx, by, bkey, s_win, s_t, s_tsum, s_key, mt_valid, mt_xy, mt_dist, counts, rv, rout);
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
        k_ncc_normal<<<M, PATCH_BLOCK, 0, e->stream>>>(pyr_of(e), e->d.pn_list, M, e->N, e->d.state, e->cam, e->d.feat_pos, e->d.feat_type, e->d.wsrc,
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
        k_ncc_warp<<<n_pred, PATCH_BLOCK, 0, e->stream>>>(e->d.plist, e->d.counts + CNT_NPRED, e->d.pred_uv, e->d.state, e->cam, e->d.feat_pos,
                                                  e->d.feat_type, e->d.wsrc, e->d.wpose, e->d.wtmpl, e->d.counts,
                                                  e->pn_on ? e->d.wnorm : nullptr);
    return e->d.wtmpl;
}

// the NCC search of the prediction slots [s_lo, s_hi); subpix: with the parabola fit, whose axis counters it zeroes first
// coef > 0: with the distinctiveness test (its counters are zeroed by launch_match_ncc)
static void match_ncc_slots(EkfEngine *e, const uint8_t *tmpl, int s_lo, int s_hi, bool subpix, bool skip_wide = false, double coef = 0.0)
{
    if (subpix) {
        (void)hipMemsetAsync(e->d.counts + CNT_SUBPIX_FIT, 0, sizeof(int), e->stream);
        (void)hipMemsetAsync(e->d.counts + CNT_SUBPIX_INT, 0, sizeof(int), e->stream);
    }
    if (s_hi <= s_lo) return;
    const bool rival = coef > 0.0;
    auto kern = rival ? (subpix ? k_ncc_match<true, true> : k_ncc_match<false, true>) : (subpix ? k_ncc_match<true, false> : k_ncc_match<false, false>);
    kern<<<s_hi - s_lo, 256, 0, e->stream>>>(pyr_of(e), e->d.plist, e->d.pred_uv, e->d.pred_S, tmpl, e->d.mt_valid, e->d.mt_xy,
                                             e->d.mt_dist, s_lo, e->d.counts, skip_wide ? 1 : 0, NccRivalOut{rival ? e->d.mt_rival : nullptr, coef});
}

void launch_match_ncc(EkfEngine *e, int n_pred, bool subpix, bool wide, double coef)
{
    const uint8_t *tmpl = match_templates(e, n_pred);
    const bool rival = coef > 0.0;
    if (rival) (void)hipMemsetAsync(e->d.counts + CNT_RIVAL_WITH, 0, 2 * sizeof(int), e->stream);
    WideSlot *list = (WideSlot *)e->d.wide_list;
    WideTotals *totals = (WideTotals *)((uint8_t *)e->d.wide_list + (size_t)e->cap * NCC_WIDE_SLOT_BYTES);
    if (wide && n_pred > 0) // before k_ncc_match: it zeroes CNT_WIDE_CANDS, and nothing of the wide path depends on the narrow one
        k_ncc_wide_classify<<<1, 1024, 0, e->stream>>>(e->d.plist, e->d.counts + CNT_NPRED, n_pred, e->d.pred_uv, e->d.pred_S, e->img.w[2],
                                                       e->img.h[2], list, totals, e->d.counts);
    match_ncc_slots(e, tmpl, 0, n_pred, subpix, wide, coef);
    if (n_pred <= 0) {
        (void)hipMemsetAsync(e->d.counts + CNT_NMATCH, 0, sizeof(int), e->stream);
        if (wide) (void)hipMemsetAsync(e->d.counts + CNT_WIDE_SLOTS, 0, 2 * sizeof(int), e->stream);
        return;
    }
    if (wide) { // k_ncc_match has skipped the wide slots (and left their sub-pixel counts to k_ncc_wide_finish)
        const int tiles = ncc_wide_tiles(e->img.w[2], e->img.h[2]);
        WidePartial *part = (WidePartial *)e->d.wide_part, *part2 = rival ? part + (size_t)e->cap * e->wide_tiles : nullptr;
        k_ncc_wide_coarse<false><<<dim3(tiles, n_pred), 256, 0, e->stream>>>(pyr_of(e), e->d.plist, tmpl, list, e->d.counts, part, e->wide_tiles,
                                                                             nullptr);
        if (rival) // the rival pass: the same tiles without the block around the slot's coarse best, into the second table
            k_ncc_wide_coarse<true><<<dim3(tiles, n_pred), 256, 0, e->stream>>>(pyr_of(e), e->d.plist, tmpl, list, e->d.counts, part2,
                                                                                e->wide_tiles, part);
        auto fin = rival ? (subpix ? k_ncc_wide_finish<true, true> : k_ncc_wide_finish<false, true>)
                         : (subpix ? k_ncc_wide_finish<true, false> : k_ncc_wide_finish<false, false>);
        fin<<<n_pred, 256, 0, e->stream>>>(pyr_of(e), e->d.plist, tmpl, list, part, e->wide_tiles, totals, e->d.mt_valid, e->d.mt_xy, e->d.mt_dist,
                                            e->d.counts, part2, NccRivalOut{rival ? e->d.mt_rival : nullptr, coef});
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
