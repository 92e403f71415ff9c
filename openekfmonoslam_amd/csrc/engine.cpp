// engine.cpp -- C ABI of the MI355X EKF engine (see include/ekf_engine.h).  Host orchestration only: every
// number is produced by the HIP kernels in kernels_*.hip; there is no CPU compute path.
#include "engine_host.h"
#include "../../include/ekf_test_hooks.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include <dlfcn.h>
#include <rccl/rccl.h> // types only: the library is loaded at run time (rccl_api)

using namespace ekf;

// RCCL entry points used by the sharded engine, resolved from librccl.so.1 on first use (the same library
// torch.distributed's "nccl" backend has loaded, when the host is PyTorch)
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};

static RcclApi &rccl_api()
{
    static RcclApi api;
    static std::once_flag once; // engines may be created from several threads: the table is filled exactly once
    std::call_once(once, [] {
        // a copy that is already mapped (torch.distributed's "nccl" backend) first: two RCCL copies in one process would
        // each keep their own device state
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        // EKF_RCCL_LIBRARY: this library and no other (a site's own RCCL build; the test suite's in-process stand-in,
        // tests/cpp/mock_rccl.cpp, which lets a one-GPU box drive the in-stream exchange with several ranks)
        if (const char *own = std::getenv("EKF_RCCL_LIBRARY")) {
            if (*own) {
                api.lib = dlopen(own, RTLD_NOW | RTLD_LOCAL);
                if (!api.lib) return;
            }
        }
        for (const char *name : names)
            if (api.lib || (api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD))) break;
        for (int i = 0; !api.lib && i < 3; ++i) api.lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
        if (!api.lib) return;
#define RCCL_SYM(field, sym) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.lib, sym))
        RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
        RCCL_SYM(CommInitRank, "ncclCommInitRank");
        RCCL_SYM(CommDestroy, "ncclCommDestroy");
        RCCL_SYM(GroupStart, "ncclGroupStart");
        RCCL_SYM(GroupEnd, "ncclGroupEnd");
        RCCL_SYM(Send, "ncclSend");
        RCCL_SYM(Recv, "ncclRecv");
        RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.GroupStart && api.GroupEnd && api.Send && api.Recv;
    });
    return api;
}

int ekf::alloc_failed(EkfEngine *e, hipError_t st, const char *what)
{
    e->err = std::string(what) + ": " + hipGetErrorString(st);
    return EKF_ERR_HIP;
}

int ekf_abi_version(void) { return 1; }

int ekf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ekf_shard_rows(int n_features, int world, int rank, int *row_begin, int *row_end)
{
    if (world <= 0 || rank < 0 || rank >= world || n_features < 0 || !row_begin || !row_end) return EKF_ERR_INVALID_ARG;
    const int per = n_features / world, extra = n_features % world;
    const int f0 = rank * per + (rank < extra ? rank : extra);
    const int f1 = f0 + per + (rank < extra ? 1 : 0);
    *row_begin = (rank == 0) ? 0 : 13 + 6 * f0;
    *row_end = 13 + 6 * f1;
    return EKF_OK;
}

const char *ekf_last_error(const EkfEngine *e) { return e ? e->err.c_str() : "null engine"; }

void ekf_engine_destroy(EkfEngine *e)
{
    if (!e) return;
    sweep_registry_detach(e->ps_reg, e);
    e->ps_reg.reset();
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    e->bufs.release_all();
    for (auto &ev : e->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &pr : e->px_events) (void)hipEventDestroy(pr.first);
    if (e->px_mid) (void)hipEventDestroy(e->px_mid);
    for (auto &pr : e->pu_events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (auto &pr : e->sw_events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (e->comm && rccl_api().ok) (void)rccl_api().CommDestroy((ncclComm_t)e->comm);
    if (e->h_mirror) (void)hipHostFree(e->h_mirror);
    if (e->stream2) { (void)hipStreamSynchronize(e->stream2); (void)hipStreamDestroy(e->stream2); }
    if (e->ev_main) (void)hipEventDestroy(e->ev_main);
    if (e->ev_prefetch) (void)hipEventDestroy(e->ev_prefetch);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

static int create_impl(const EkfEngineConfig *cfg, int rank, int world, EkfEngine **out)
{
    if (!cfg || !out || cfg->max_features <= 0 || world < 1 || rank < 0 || rank >= world) return EKF_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return EKF_ERR_NO_DEVICE;
    EkfEngine *e = new (std::nothrow) EkfEngine();
    if (!e) return EKF_ERR_CAPACITY;
    e->cfg = *cfg;
    if (e->cfg.ransac_batch <= 0) e->cfg.ransac_batch = 32;
    if (cfg->device >= 0) e->device = cfg->device;
    else if (hipGetDevice(&e->device) != hipSuccess) e->device = 0;
    const EkfCamera &c = cfg->cam;
    e->cam = CamD{c.fx, c.fy, c.k1, c.k2, c.cx, c.cy, c.dx, c.dy, c.pixelErrorX, c.pixelErrorY, c.angularVisionX,
                  c.angularVisionY, c.pixelsX, c.pixelsY};
    const EkfParams &p = cfg->par;
    e->par = ParD{p.linearAccelSD, p.angularAccelSD, p.matchingCompCoefSecondBestVSFirst,
                  p.ransacThresholdPredictDistance, p.ransacAllInliersProbability, p.ransacChi2Threshold};
    if (cfg->precision < EKF_PRECISION_F64 || cfg->precision > EKF_PRECISION_AUTO) {
        delete e;
        return EKF_ERR_INVALID_ARG;
    }
    // EKF_PRECISION_AUTO: the fastest configuration that holds EVERY feature parameter within 1e-5 of the fp64 reference on the
    // maps it was measured on: the exact int8 update on an fp32-stored covariance up to
    // EKF_AUTO_F32_MAX_FEATURES features; on an fp64-stored one up to EKF_AUTO_EXACT_MAX_FEATURES (fp32 storage alone leaves 1e-5
    // on fresh maps of >= 1400 features); all-fp64 above (at N = 5000 the 38-bit digits of the exact update themselves leave
    // 2.5e-5 ... 3.4e-5 on one far feature in the third frame of a fresh map)
    if (cfg->precision == EKF_PRECISION_AUTO)
        e->cfg.precision = cfg->max_features <= EKF_AUTO_F32_MAX_FEATURES ? EKF_PRECISION_F32_EXACT
                           : (cfg->max_features <= EKF_AUTO_EXACT_MAX_FEATURES ? EKF_PRECISION_F64_EXACT : EKF_PRECISION_F64);
    e->exact = e->cfg.precision == EKF_PRECISION_F32_EXACT || e->cfg.precision == EKF_PRECISION_F64_EXACT;
    e->f32 = e->cfg.precision == EKF_PRECISION_F32 || e->cfg.precision == EKF_PRECISION_F32_EXACT;
    if ((cfg->flags & 0xff) == 1) { // EKF_DESCRIPTOR_F32_L2(cols)
        const int cols = (cfg->flags >> 8) & 0xffff;
        if (cols < 1 || cols > 1024) { delete e; return EKF_ERR_INVALID_ARG; }
        e->desc_f32 = true;
        e->desc_bytes = 4 * cols;
    } else if ((cfg->flags & 0xff) != 0) { delete e; return EKF_ERR_INVALID_ARG; }
    e->shard_rank = rank;
    e->shard_world = world;
    e->cap = cfg->max_features;
    e->ncap = 13 + 6 * e->cap;
    e->mcap = round_up(2 * e->cap, NB);
    // the exact downdate accumulates digit products in int32: five products of |d d'| <= 2^14 per level and row of k, so the sums
    // are exact only while 5 * 2^14 * m < 2^31 (kernels_pexact.hip); refuse maps whose updates could exceed that
    if (e->exact && e->mcap > PX_MAX_ROWS) {
        delete e;
        return EKF_ERR_INVALID_ARG;
    }
    e->kcap = cfg->max_keypoints > 0 ? cfg->max_keypoints : 4 * e->cap;
    e->ldP = round_up(e->ncap, LD_ALIGN);
    e->ldS = round_up(e->mcap, 128) + 128;
    auto fail = [&](hipError_t st, const char *what) {
        e->err = std::string(what) + ": " + hipGetErrorString(st);
        std::fprintf(stderr, "ekf_engine_create: %s\n", e->err.c_str());
        ekf_engine_destroy(e);
        return EKF_ERR_HIP;
    };
    hipError_t st;
    if ((st = hipSetDevice(e->device)) != hipSuccess) return fail(st, "hipSetDevice");
    (void)hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, e->device);
    if (e->n_cus <= 0) e->n_cus = 256;
#ifdef EKF_SWEEP_TRACE // debug builds only (scripts/build_trace_variant.sh), for scripts/contention_probe.py: "first,count" of the CU mask of the main stream
    if (const char *cm = std::getenv("EKF_PROBE_CU_MASK")) {
        int first = 0, count = 0;
        if (std::sscanf(cm, "%d,%d", &first, &count) == 2 && count > 0) {
            std::vector<uint32_t> mask((e->n_cus + 31) / 32, 0u);
            for (int c = first; c < first + count && c < e->n_cus; ++c) mask[c / 32] |= 1u << (c % 32);
            if ((st = hipExtStreamCreateWithCUMask(&e->stream, (uint32_t)mask.size(), mask.data())) != hipSuccess) return fail(st, "hipExtStreamCreateWithCUMask");
        }
    }
#endif
    if (!e->stream && (st = hipStreamCreate(&e->stream)) != hipSuccess) return fail(st, "hipStreamCreate");
    if ((st = hipStreamCreate(&e->stream2)) != hipSuccess) return fail(st, "hipStreamCreate");
    if ((st = hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming)) != hipSuccess) return fail(st, "hipEventCreate");
    if ((st = hipEventCreateWithFlags(&e->ev_prefetch, hipEventDisableTiming)) != hipSuccess) return fail(st, "hipEventCreate");
    DeviceArrays &d = e->d;
    const size_t w = e->f32 ? 4 : 8;
    const size_t cap = e->cap, mcap = e->mcap;
#define ALLOC_AS(name, call) \
    if ((st = e->bufs.call) != hipSuccess) return fail(st, "hipMalloc " name)
#define ALLOC(ptr, count) ALLOC_AS(#ptr, alloc(&(ptr), (count)))
    ALLOC(d.state, ST_COUNT);
    ALLOC(d.cam_ahead, 13 + 169);
    ALLOC(d.feat_pos, 6 * cap);
    ALLOC(d.feat_type, cap);
    ALLOC(d.feat_covpos, cap);
    ALLOC(d.feat_desc, (size_t)e->desc_bytes * cap);
    ALLOC(d.feat_times_predicted, cap);
    ALLOC(d.feat_times_matched, cap);
    {
        // rows of P kept here: all of them, or (sharded) camera block + the largest share of the features
        e->p_rows_cap = world == 1 ? round_up(e->ncap, LD_ALIGN)
                                   : SHARD_BASE + round_up(6 * ((e->cap + world - 1) / world), LD_ALIGN) + LD_ALIGN;
        ALLOC_AS("P", alloc_bytes(&d.P, (size_t)e->p_rows_cap * e->ldP * w));
        const size_t wb = e->exact ? 8 : w; // element size of H P, its gathered rows and B = inv(L) G
        ALLOC_AS("HP", alloc_bytes(&d.HP, (size_t)mcap * e->ldP * wb));
        // + one row: the row operand of a sharded downdate tile may read up to 127 columns past n
        ALLOC_AS("A", alloc_bytes(&d.A, (size_t)(mcap + 1) * e->ldP * wb));
        if (e->exact) { // digit planes of B and their column scales (kernels_pexact.hip)
            e->bq_rows = round_up((int)mcap, 64) + 64;
            ALLOC_AS("Bq", alloc(&d.Bq, (size_t)PX_S * e->bq_rows * e->ldP));
            ALLOC_AS("Bexp", alloc(&d.Bexp, (size_t)e->ldP));
            e->px_scale_shift = 0; // engine.h: measured, and left at 0 -- one bit already costs the 1e-5 component-wise gate in one of five N = 1000 scenes
            if (const char *ev = std::getenv("EKF_PX_SCALE_SHIFT")) e->px_scale_shift = std::max(0, std::min(6, std::atoi(ev)));
            e->bz_stride = e->bq_rows / 16;
            ALLOC_AS("Bz", alloc(&d.Bz, (size_t)(e->ldP / 32 + 8) * e->bz_stride));
            {   // rows of B from digit planes (chol_bplanes.h): planes of L for the sweeps that form B
                e->lq_nbk = (std::min((int)mcap, B_SWEEP_MAX) + NB - 1) / NB + 2;
                ALLOC_AS("Lq", alloc(&d.Lq, (size_t)PX_S * e->lq_nbk * e->lq_nbk * 1024));
                ALLOC_AS("Lexp", alloc(&d.Lexp, (size_t)mcap + 256));
                ALLOC_AS("Grow", alloc(&d.Grow, (size_t)mcap + 256));
            }
            if ((int)mcap > B_SWEEP_MAX) { // B = inv(L) G on the int8 MFMA for updates above B_SWEEP_MAX rows: planes of inv(L)' and of G
                ALLOC_AS("Wq", alloc(&d.Wq, (size_t)PX_S * e->bq_rows * (round_up((int)mcap, 128) + 128)));
                ALLOC_AS("Gq", alloc(&d.Gq, (size_t)PX_S * e->bq_rows * e->ldP));
                ALLOC_AS("Wexp", alloc(&d.Wexp, (size_t)round_up((int)mcap, 128) + 128));
                ALLOC_AS("Gexp", alloc(&d.Gexp, (size_t)e->ldP));
                // their tables of non-zero pieces of plane 0 (k_slice_B writes them, k_b_gemm_i8p reads them)
                ALLOC_AS("Wz", alloc(&d.Wz, (size_t)((round_up((int)mcap, 128) + 128) / 32 + 8) * e->bz_stride));
                ALLOC_AS("Gz", alloc(&d.Gz, (size_t)(e->ldP / 32 + 8) * e->bz_stride));
            }
            if (world > 1) { // sharded: the diagonal table and the exchange image of the planes (rows of B up to B_SWEEP_MAX)
                ALLOC_AS("Pdiag", alloc(&d.Pdiag, (size_t)e->ldP));
                e->bstage_rows = e->bq_rows; // any update's rows of B
                ALLOC_AS("Bstage", alloc(&d.Bstage, (size_t)PX_S * e->bstage_rows * e->ldP));
            }
        }
        ALLOC_AS("G", alloc_bytes(&d.G, (size_t)(mcap + 1) * e->ldP * wb));
    }
    ALLOC(d.mm_scratch, (size_t)60 * cap + 4 * (size_t)e->ldP + 64);
    ALLOC(d.mm_index, (size_t)e->ncap + 8);
    ALLOC(d.pred_vis, cap);
    ALLOC(d.pred_vis_full, cap);
    ALLOC(d.step_preds, cap);
    ALLOC(d.pred_uv, 2 * cap);
    ALLOC(d.pred_vis2, cap);
    ALLOC(d.pred_uv2, 2 * cap);
    ALLOC(d.pred_S, 4 * cap);
    if (world == 1) ALLOC(d.match_gates, 5 * cap);
    ALLOC(d.Hs, 14 * cap);
    ALLOC(d.Hf, 12 * cap);
    ALLOC(d.work_idx, cap);
    ALLOC(d.work_flag, cap);
    ALLOC(d.plist, cap);
    ALLOC(d.plist_sub, cap);
    ALLOC(d.counts, CNT_COUNT);
    ALLOC(d.shard_feat, MAX_SHARD_WORLD + 1);
    ALLOC(d.kps, (size_t)e->kcap);
    ALLOC(d.kdesc, (size_t)e->kcap * e->desc_bytes);
    ALLOC(d.mt_valid, cap);
    ALLOC(d.mt_kp, cap);
    ALLOC(d.mt_dist, cap);
    ALLOC(d.mt_xy, cap);
    ALLOC(d.tmpl, (size_t)mapblob::TEMPLATE_BYTES * cap);
    ALLOC(d.gates, (size_t)8 * cap);
    ALLOC(d.matches, cap);
    ALLOC(d.msel, cap);
    ALLOC(d.mout, cap);
    ALLOC(d.match_of_feat, cap);
    ALLOC(d.ransac_rec, mcap);
    // (a frame's first batch is ransac_batch hypotheses; the batches behind it -- a fresh map needs hundreds of hypotheses -- are
    // RANSAC_WIDE_FACTOR times wider: one workgroup per hypothesis, and 32 workgroups leave seven eighths of the chip idle)
    ALLOC(d.hyp_count, (size_t)e->cfg.ransac_batch * RANSAC_WIDE_FACTOR);
    ALLOC(d.hyp_flags, (size_t)e->cfg.ransac_batch * RANSAC_WIDE_FACTOR * mcap);
    ALLOC(d.best_flags, mcap);
    // tiles of the GEMM-shaped kernels read whole 128-wide slabs: leading dimensions and row counts carry slack
    e->ldW = round_up((int)mcap, 128) + 128;
    const size_t mw = (size_t)round_up((int)mcap, 128) + 128;
    ALLOC(d.S, mw * e->ldS);
    ALLOC(d.LL, mw * e->ldS);
    if (e->f32 && !e->exact) ALLOC(d.LLf, mw * e->ldS);
    ALLOC(d.nu, mcap);
    ALLOC(d.Dinv, mw * e->ldW);
    ALLOC(d.W, mw * e->ldW);
    ALLOC(d.Tbuf, mw * e->ldW);
    {   // flags of the persistent sweep (chol_persist.h): done / lrdy tables of (B_SWEEP_MAX / 32 + 2)^2 words each, zeroed here once
        ALLOC_AS("sweep_ctl", alloc_bytes(&d.sweep_ctl, (size_t)256 + sizeof(unsigned) * 2 * (B_SWEEP_MAX / NB + 2) * (B_SWEEP_MAX / NB + 2)));
    }
    if (e->f32 && !e->exact) ALLOC(d.Wf, mw * e->ldW);
    ALLOC(d.mHs, 14 * cap);
    ALLOC(d.mHf, 12 * cap);
    ALLOC(d.mpos, cap);
    ALLOC(d.mdim, cap);
    ALLOC(d.dx_part, (size_t)DX_SPLIT * e->ldP + 8); // + the quaternion before the update (k_apply_normalize)
    ALLOC(d.sq_part, (size_t)DX_SPLIT * e->ldP);
    ALLOC(d.diag_save, (size_t)e->ldP);
    ALLOC(d.cam_part, (size_t)DX_SPLIT * 13 * e->ldP);
    ALLOC(d.cam_save, (size_t)13 * e->ldP);
    ALLOC(d.HPc, (size_t)mcap * 16);
    ALLOC(d.Gc, mw * 16);
    ALLOC(d.Bc, mw * 16);
    ALLOC(d.zvec, mw);
    ALLOC(d.yvec, mw);
    ALLOC(d.mask, mcap);
    ALLOC(d.preds_out, cap);
#undef ALLOC
#undef ALLOC_AS
    for (auto &ev : e->ev)
        if ((st = hipEventCreate(&ev)) != hipSuccess) return fail(st, "hipEventCreate");
    e->h_counts.assign(CNT_COUNT, 0);
    {   // host mirror of the counter block (optional: without it read_counts (step.cpp) falls back to memcpy + synchronise)
        void *hp = nullptr;
        if (hipHostMalloc(&hp, 64 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            std::memset(hp, 0, 64 * sizeof(int));
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                e->h_mirror = (int *)hp;
                e->d_mirror = (int *)dp;
            } else {
                (void)hipHostFree(hp);
            }
        }
    }
    e->shard_feat_begin.assign(world + 1, 0);
    e->exchange_hook = exchange_rows;
    e->ps_reg = sweep_registry_attach(e->device); // persistent sweeps of the engines on one device are ordered (engine.h)
    *out = e;
    return EKF_OK;
}

int ekf_engine_create(const EkfEngineConfig *cfg, EkfEngine **out) { return create_impl(cfg, 0, 1, out); }

int ekf_engine_create_sharded(const EkfEngineConfig *cfg, int rank, int world, EkfEngine **out)
{
    if (world > MAX_SHARD_WORLD) return EKF_ERR_INVALID_ARG;
    return create_impl(cfg, rank, world, out);
}

int ekf_set_exchange(EkfEngine *e, EkfExchangeFn fn, void *user)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->xchg = fn;
    e->xchg_user = user;
    return EKF_OK;
}

int ekf_comm_unique_id(uint8_t id[EKF_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == EKF_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    if (!id) return EKF_ERR_INVALID_ARG;
    RcclApi &api = rccl_api();
    if (!api.ok) return EKF_ERR_COMM;
    ncclUniqueId u;
    if (api.GetUniqueId(&u) != ncclSuccess) return EKF_ERR_COMM;
    std::memcpy(id, &u, EKF_COMM_ID_BYTES);
    return EKF_OK;
}

int ekf_comm_init(EkfEngine *e, const uint8_t id[EKF_COMM_ID_BYTES])
{
    if (!e || !id) return EKF_ERR_INVALID_ARG;
    RcclApi &api = rccl_api();
    if (!api.ok) {
        e->err = "librccl.so.1 could not be loaded";
        return EKF_ERR_COMM;
    }
    HIPCHK(hipSetDevice(e->device));
    if (e->comm) {
        (void)api.CommDestroy((ncclComm_t)e->comm);
        e->comm = nullptr;
    }
    ncclUniqueId u;
    std::memcpy(&u, id, EKF_COMM_ID_BYTES);
    ncclComm_t c = nullptr;
    const ncclResult_t r = api.CommInitRank(&c, e->shard_world, u, e->shard_rank);
    if (r != ncclSuccess) {
        e->err = std::string("ncclCommInitRank: ") + (api.GetErrorString ? api.GetErrorString(r) : "error");
        return EKF_ERR_COMM;
    }
    e->comm = c;
    return EKF_OK;
}

// Completes a replicated per-feature table: rank r owns rows [rb[r], rb[r+1]) of row_bytes each and has just written
// them (on the engine's stream).  In-engine transport: every pair of ranks exchanges its blocks directly, enqueued on the
// same stream; otherwise the host's callback (which needs the stream idle).
int ekf::exchange_rows(EkfEngine *e, int what, void *base, size_t row_bytes, const std::vector<int32_t> &rb, const char *name)
{
    const int world = e->shard_world, me = e->shard_rank;
    if (what == EKF_XCHG_BPLANES) e->xchg_bytes_planes += (long long)((size_t)(rb[world] - rb[0] - (rb[me + 1] - rb[me])) * row_bytes);
    if (e->comm && !e->xchg) { // a callback installed after ekf_comm_init takes over (ranks that fell back by consensus)
        RcclApi &api = rccl_api();
        ncclComm_t c = (ncclComm_t)e->comm;
        uint8_t *b = (uint8_t *)base;
        const size_t my_lo = (size_t)rb[me] * row_bytes, my_n = (size_t)(rb[me + 1] - rb[me]) * row_bytes;
        ncclResult_t r = api.GroupStart();
        for (int p = 0; p < world && r == ncclSuccess; ++p) {
            if (p == me) continue;
            const size_t lo = (size_t)rb[p] * row_bytes, cnt = (size_t)(rb[p + 1] - rb[p]) * row_bytes;
            if (my_n > 0) r = api.Send(b + my_lo, my_n, ncclChar, p, c, e->stream);
            if (r == ncclSuccess && cnt > 0) r = api.Recv(b + lo, cnt, ncclChar, p, c, e->stream);
        }
        const ncclResult_t r2 = api.GroupEnd();
        if (r != ncclSuccess || r2 != ncclSuccess) {
            e->err = std::string("RCCL exchange of ") + name + " failed";
            return EKF_ERR_COMM;
        }
        return EKF_OK;
    }
    if (!e->xchg) {
        e->err = "sharded engine without a transport (ekf_comm_init or ekf_set_exchange)";
        return EKF_ERR_COMM;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->xchg(e->xchg_user, what, base, row_bytes, rb.data(), world, me)) {
        e->err = std::string("exchange of ") + name + " failed";
        return EKF_ERR_COMM;
    }
    return EKF_OK;
}

int ekf_shard_info(const EkfEngine *e, int *rank, int *world, int *row_begin, int *row_end)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (rank) *rank = e->shard_rank;
    if (world) *world = e->shard_world;
    if (row_begin) *row_begin = e->shard_rank == 0 ? 0 : e->rm.r0;
    if (row_end) *row_end = e->rm.r1;
    return EKF_OK;
}

int ekf_shard_counters(EkfEngine *e, int64_t *plane_bytes_received, int32_t *own_columns_begin, int32_t *own_columns_end)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (plane_bytes_received) *plane_bytes_received = e->xchg_bytes_planes;
    const int n_pad = round_up(e->n, LD_ALIGN), W = e->shard_world, r = e->shard_rank;
    // the shares the last update actually used (they end at the ownership boundaries on the by-symmetry route, at multiples of
    // 32 on the inverse + GEMM route); before the first update: the rounded convention
    auto col = [&](int k) {
        if ((int)e->last_col_rb.size() == W + 1) return (int)e->last_col_rb[k];
        return k <= 0 ? 0 : (k >= W ? n_pad : std::min(n_pad, round_up(e->shard_row_begin.size() > (size_t)k ? e->shard_row_begin[k] : e->n, NB)));
    };
    if (own_columns_begin) *own_columns_begin = col(r);
    if (own_columns_end) *own_columns_end = col(r + 1);
    return EKF_OK;
}

int ekf_device_copy(EkfEngine *e, void *dst, const void *src, size_t bytes)
{
    if (!e || (bytes > 0 && (!dst || !src))) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    if (bytes > 0) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    return EKF_OK;
}

int ekf_state_dim(const EkfEngine *e) { return e ? e->n : 0; }
int ekf_descriptor_bytes(const EkfEngine *e) { return e ? e->desc_bytes : 0; }
int ekf_get_precision(const EkfEngine *e) { return e ? e->cfg.precision : -1; }
int ekf_num_features(const EkfEngine *e) { return e ? e->N : 0; }

int ekf_synchronize(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    return take_pending_error(e);
}

int ekf_keep_step_predictions(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->keep_step_preds = on != 0;
    if (!on) e->n_step_preds = 0;
    return EKF_OK;
}

int ekf_get_step_predictions(EkfEngine *e, EkfPrediction *preds, int *n_preds)
{
    if (!e || !n_preds) return EKF_ERR_INVALID_ARG;
    *n_preds = e->n_step_preds;
    if (!preds || e->n_step_preds == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(preds, e->d.step_preds, (size_t)e->n_step_preds * sizeof(EkfPrediction), hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf::check_async(EkfEngine *e)
{
    HIPCHK(hipGetLastError());
    return EKF_OK;
}

// ---------------------------------------------------------------------------------------------------- stages
int ekf_predict(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    launch_predict(e, e->frame_interval);
    return check_async(e);
}

// ---- frame intervals: an interval is finite and greater than 0, or the call does nothing
static bool valid_interval(double dt) { return std::isfinite(dt) && dt > 0.0; }

static int bad_interval(const EkfEngine *e, const char *who, const char *what, double dt)
{
    const_cast<EkfEngine *>(e)->err = std::string(who) + ": " + what + " = " + std::to_string(dt) + " is not a finite interval greater than 0";
    return EKF_ERR_INVALID_ARG;
}

// the interval of staged frame i: its entry of ekf_set_staged_intervals' table, the set interval beyond the table
static double staged_interval(const EkfEngine *e, int frame)
{
    return frame >= 0 && (size_t)frame < e->staged_dt.size() ? e->staged_dt[frame] : e->frame_interval;
}

int ekf_set_frame_interval(EkfEngine *e, double dt)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (!valid_interval(dt)) return bad_interval(e, "ekf_set_frame_interval", "dt", dt);
    e->frame_interval = dt;
    return EKF_OK;
}

int ekf_get_frame_interval(const EkfEngine *e, double *dt)
{
    if (!e || !dt) return EKF_ERR_INVALID_ARG;
    *dt = e->frame_interval;
    return EKF_OK;
}

int ekf_predict_dt(EkfEngine *e, double dt)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (!valid_interval(dt)) return bad_interval(e, "ekf_predict_dt", "dt", dt);
    HIPCHK(hipSetDevice(e->device));
    launch_predict(e, dt);
    return check_async(e);
}

int ekf_set_staged_intervals(EkfEngine *e, int n, const double *dt)
{
    if (!e || n < 0 || (n > 0 && !dt)) return EKF_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (!valid_interval(dt[i])) return bad_interval(e, "ekf_set_staged_intervals", ("dt[" + std::to_string(i) + "]").c_str(), dt[i]);
    e->staged_dt.assign(dt, dt + n);
    return EKF_OK;
}

int ekf_predict_camera_ahead(const EkfEngine *ce, double tau, double x13[13], double P13[169])
{
    if (!ce) return EKF_ERR_INVALID_ARG;
    EkfEngine *e = const_cast<EkfEngine *>(ce); // (the message of a failure is the only thing of the engine written here)
    if (!valid_interval(tau)) return bad_interval(e, "ekf_predict_camera_ahead", "tau", tau);
    HIPCHK(hipSetDevice(e->device));
    launch_camera_ahead(e, tau, e->d.cam_ahead);
    HIPCHK(hipGetLastError());
    double h[13 + 169];
    HIPCHK(hipMemcpyAsync(h, e->d.cam_ahead, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (x13) std::memcpy(x13, h, 13 * sizeof(double));
    if (P13) std::memcpy(P13, h + 13, 169 * sizeof(double));
    return EKF_OK;
}

int ekf_predict_measurement_state(EkfEngine *e, EkfPrediction *preds, int *n_preds)
{
    if (!e || !preds || !n_preds) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    launch_state_only_predict(e, e->d.preds_out);
    int rc = read_counts(e);
    if (rc) return rc;
    const int np = e->h_counts[CNT_NPRED_SUB];
    if (np > 0) HIPCHK(hipMemcpy(preds, e->d.preds_out, (size_t)np * sizeof(EkfPrediction), hipMemcpyDeviceToHost));
    *n_preds = np;
    return EKF_OK;
}

// ------------------------------------------------------------------------------ fixed map
// why the fixed-map update is not available on this engine, or null
static const char *fixed_map_refusal(const EkfEngine *e)
{
    if (e->shard_world > 1) return "not available on a sharded engine";
    if (e->f32 && !e->exact) return "not available in EKF_PRECISION_F32";
    return nullptr;
}

// the mode's scratch, on its first use: the control block and the two m x 13 gain tables of updates above B_SWEEP_MAX rows (the
// partial sums of the strip share d.cam_part with the fast fp32 configuration's repair, which the mode refuses)
int ekf::fixed_map_scratch(EkfEngine *e)
{
    if (e->d.fm_ctl) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    e->fm_rows = round_up(e->mcap, 128) + 128;
    auto g = e->bufs.group();
    g.alloc(&e->d.fm_ctl, 1);
    g.alloc(&e->d.fm_gain, (size_t)2 * e->fm_rows * FM_LD);
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "fixed-map update scratch");
    return EKF_OK;
}

int ekf_update_fixed_map(EkfEngine *e, const EkfMatch *matches, int M)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (const char *why = fixed_map_refusal(e)) {
        e->err = std::string("ekf_update_fixed_map: ") + why;
        return EKF_ERR_INVALID_ARG;
    }
    return update_stage(e, matches, M, UPDATE_FIXED_MAP);
}

int ekf_set_fixed_map(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (on) {
        if (const char *why = fixed_map_refusal(e)) {
            e->err = std::string("ekf_set_fixed_map: ") + why;
            return EKF_ERR_INVALID_ARG;
        }
        if (e->update_iterations > 1) { // the fixed-map update has no state-only form
            e->err = "ekf_set_fixed_map: not available while ekf_set_update_iterations asks for more than one pass";
            return EKF_ERR_INVALID_ARG;
        }
        int rc = fixed_map_scratch(e);
        if (rc) return rc;
    }
    e->fixed_map = on != 0;
    return EKF_OK;
}

int ekf_get_fixed_map(const EkfEngine *e, int *on, int64_t *updates)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (on) *on = e->fixed_map ? 1 : 0;
    if (updates) {
        *updates = 0;
        if (e->d.fm_ctl) { // (never allocated: no fixed-map update ran)
            long long v = 0;
            if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(&v, &e->d.fm_ctl->updates, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
                return EKF_ERR_HIP;
            *updates = (int64_t)v;
        }
    }
    return EKF_OK;
}

// ------------------------------------------------------------------------- external measurements
int ekf_update_external(EkfEngine *e, int m, const int32_t *row_start, const int32_t *col, const double *val, const double *residual,
                        const double *R, double gate_nis, EkfExternalUpdate *out)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    auto invalid = [&](const std::string &why) {
        e->err = "ekf_update_external: " + why;
        return EKF_ERR_INVALID_ARG;
    };
    if (e->shard_world > 1) return invalid("not available on a sharded engine");
    if (m < 1 || m > EXT_ROWS) return invalid("m = " + std::to_string(m) + " is outside 1.." + std::to_string(EXT_ROWS));
    if (!row_start || !col || !val || !residual || !R) return invalid("a null argument");
    if (!(gate_nis >= 0.0)) return invalid("gate_nis is negative or not a number");
    ExtCtl ctl;
    std::memset(&ctl, 0, sizeof(ctl));
    ctl.m = m;
    ctl.gate_nis = gate_nis;
    const int base = row_start[0];
    if (base < 0) return invalid("row_start[0] < 0");
    for (int i = 0; i < m; ++i) {
        const int k0 = row_start[i], k1 = row_start[i + 1];
        if (k1 <= k0 || k1 - k0 > EXT_NNZ)
            return invalid("row " + std::to_string(i) + " has " + std::to_string((long long)k1 - k0) + " entries (1.." + std::to_string(EXT_NNZ) + ")");
        for (int k = k0; k < k1; ++k) {
            if (col[k] < 0 || col[k] >= e->n || (k > k0 && col[k] <= col[k - 1]))
                return invalid("row " + std::to_string(i) + ": columns must ascend strictly inside [0, " + std::to_string(e->n) + ")");
            if (!std::isfinite(val[k])) return invalid("a value of H is not finite");
            ctl.col[k - base] = col[k];
            ctl.val[k - base] = val[k];
        }
        ctl.row_start[i] = k0 - base;
        ctl.row_start[i + 1] = k1 - base;
        if (!std::isfinite(residual[i])) return invalid("a residual is not finite");
        ctl.residual[i] = residual[i];
        for (int j = i; j < m; ++j) {
            if (!std::isfinite(R[(size_t)i * m + j])) return invalid("an entry of R is not finite");
            ctl.R[i * EXT_ROWS + j] = R[(size_t)i * m + j];
        }
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = take_pending_error(e); // as ekf_get_state; the failed update it reports is not this call's
    if (rc) return rc;
    if (!e->d.ext_A) {
        auto g = e->bufs.group();
        g.alloc(&e->d.ext_A, (size_t)(EXT_ROWS + 1) * e->ldP);
        g.alloc(&e->d.ext_sel, (size_t)EXT_ROWS * EXT_ENTRIES);
        g.alloc(&e->d.ext_ctl, 1);
        g.alloc(&e->d.ext_res, 1);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "external update scratch");
    }
    HIPCHK(hipMemcpyAsync(e->d.ext_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, e->stream));
    launch_external_update(e, m);
    HIPCHK(hipGetLastError());
    ExtResult res;
    HIPCHK(hipMemcpyAsync(&res, e->d.ext_res, sizeof(res), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (out) *out = res.out;
    if (res.verdict == EXT_NOT_PD) {
        e->err = "ekf_update_external: S = H P H' + R is not positive definite";
        return EKF_ERR_NOT_POSITIVE_DEFINITE;
    }
    if (res.verdict == EXT_APPLIED) e->p_exact_sym = true; // every pair was averaged and written to both places
    return EKF_OK;
}

int ekf_fuse_camera_position(EkfEngine *e, const double r[3], const double R[9], double gate_nis, EkfExternalUpdate *out)
{
    if (!e || !r || !R) return EKF_ERR_INVALID_ARG;
    NOT_WHEN_SHARDED(e)
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    double x[3];
    HIPCHK(hipMemcpy(x, e->d.state + ST_X, sizeof(x), hipMemcpyDeviceToHost));
    const int32_t row_start[4] = {0, 1, 2, 3}, col[3] = {0, 1, 2};
    const double val[3] = {1.0, 1.0, 1.0}, residual[3] = {r[0] - x[0], r[1] - x[1], r[2] - x[2]};
    return ekf_update_external(e, 3, row_start, col, val, residual, R, gate_nis, out);
}

// world point X of a feature and Jw = dX/dy (3 x 6 row-major, the identity block for a depth feature), as k_map_points forms them
static void feature_world_point(const double *y, int type, double *X, double *Jw)
{
    for (int i = 0; i < 18; ++i) Jw[i] = 0.0;
    Jw[0] = Jw[7] = Jw[14] = 1.0;
    for (int i = 0; i < 3; ++i) X[i] = y[i];
    if (type != EKF_FEATURE_INVERSE_DEPTH) return;
    const double theta = y[3], phi = y[4], rho = y[5];
    double mi[3];
    dir_vec(theta, phi, mi);
    Jw[0 * 6 + 3] = std::cos(phi) * std::cos(theta) / rho;  Jw[2 * 6 + 3] = -std::cos(phi) * std::sin(theta) / rho;
    Jw[0 * 6 + 4] = -std::sin(phi) * std::sin(theta) / rho; Jw[1 * 6 + 4] = -std::cos(phi) / rho;
    Jw[2 * 6 + 4] = -std::sin(phi) * std::cos(theta) / rho;
    for (int i = 0; i < 3; ++i) {
        Jw[i * 6 + 5] = -mi[i] / (rho * rho);
        X[i] += mi[i] / rho;
    }
}

int ekf_fuse_feature_distance(EkfEngine *e, int feat_i, int feat_j, double distance, double sigma, double gate_nis,
                              EkfExternalUpdate *out)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    NOT_WHEN_SHARDED(e)
    auto invalid = [&](const char *why) {
        e->err = std::string("ekf_fuse_feature_distance: ") + why;
        return EKF_ERR_INVALID_ARG;
    };
    if (feat_i < 0 || feat_i >= e->N || feat_j < 0 || feat_j >= e->N || feat_i == feat_j) return invalid("two different map features are needed");
    if (!(sigma > 0.0) || !(distance > 0.0) || !std::isfinite(sigma) || !std::isfinite(distance)) return invalid("distance and sigma must be positive");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int f[2] = {feat_i, feat_j};
    double y[2][6], X[2][3], Jw[2][18];
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipMemcpy(y[s], e->d.feat_pos + 6 * (size_t)f[s], sizeof(y[s]), hipMemcpyDeviceToHost));
        feature_world_point(y[s], e->h_type[f[s]], X[s], Jw[s]);
    }
    const double dX[3] = {X[0][0] - X[1][0], X[0][1] - X[1][1], X[0][2] - X[1][2]};
    const double h = std::sqrt(dX[0] * dX[0] + dX[1] * dX[1] + dX[2] * dX[2]);
    if (!(h > 0.0) || !std::isfinite(h)) return invalid("the two features coincide");
    const double u[3] = {dX[0] / h, dX[1] / h, dX[2] / h};
    int32_t col[12];
    double val[12];
    int nnz = 0;
    const int first = e->h_covpos[feat_i] < e->h_covpos[feat_j] ? 0 : 1; // columns ascend: the feature stored first comes first
    for (int t = 0; t < 2; ++t) {
        const int s = t == 0 ? first : 1 - first;
        const int d = feature_dims(e->h_type[f[s]]), pos = e->h_covpos[f[s]];
        const double sign = s == 0 ? 1.0 : -1.0;
        for (int k = 0; k < d; ++k) {
            col[nnz] = pos + k;
            val[nnz++] = sign * (u[0] * Jw[s][k] + u[1] * Jw[s][6 + k] + u[2] * Jw[s][12 + k]);
        }
    }
    const int32_t row_start[2] = {0, nnz};
    const double residual = distance - h, R = sigma * sigma;
    return ekf_update_external(e, 1, row_start, col, val, &residual, &R, gate_nis, out);
}

int ekf_rescue(EkfEngine *e, const EkfMatch *outliers, int M, uint8_t *rescued_mask)
{
    if (!e || !rescued_mask) return EKF_ERR_INVALID_ARG;
    int rc = validate_matches(e, outliers, M);
    if (rc) return rc;
    if (M == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->d.mout, outliers, (size_t)M * sizeof(EkfMatch), hipMemcpyHostToDevice, e->stream));
    launch_rescue(e, e->d.mout, M);
    HIPCHK(hipMemcpyAsync(rescued_mask, e->d.mask, (size_t)M, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_async(e);
}

int ekf_set_async_errors(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->async_errors = on != 0;
    return EKF_OK;
}

int ekf_set_update_path(EkfEngine *e, int path)
{
    if (!e || path < EKF_UPDATE_PATH_AUTO || path > EKF_UPDATE_PATH_GEMM) return EKF_ERR_INVALID_ARG;
    e->b_path = path;
    return EKF_OK;
}

int ekf_set_sweep_mode(EkfEngine *e, int mode)
{
    if (!e || mode < EKF_SWEEP_PAIRS || mode > EKF_SWEEP_LAUNCHES) return EKF_ERR_INVALID_ARG;
    e->sweep_mode = mode;
    return EKF_OK;
}

int ekf_frames_upload(EkfEngine *e, int n_frames, const int32_t *kp_counts, const EkfKeypoint *kps_concat,
                      const uint8_t *desc_concat)
{
    if (!e || n_frames < 0 || (n_frames > 0 && (!kp_counts || !kps_concat || !desc_concat))) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->bufs.release(&e->frames.kps);
    e->bufs.release(&e->frames.desc);
    e->frames = Frames(); // what every failure below leaves: no frames
    Frames f;
    size_t total = 0;
    for (int i = 0; i < n_frames; ++i) {
        if (kp_counts[i] < 0) return EKF_ERR_INVALID_ARG;
        f.offset.push_back((int)total);
        f.count.push_back(kp_counts[i]);
        total += (size_t)kp_counts[i];
    }
    f.n = n_frames;
    if (total > 0) {
        auto g = e->bufs.group();
        g.alloc(&f.kps, total, false);
        g.alloc(&f.desc, total * e->desc_bytes, false);
        if (g.status() != hipSuccess) return alloc_failed(e, g.status(), "hipMalloc frames");
        HIPCHK(hipMemcpy(f.kps, kps_concat, total * sizeof(EkfKeypoint), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.desc, desc_concat, total * e->desc_bytes, hipMemcpyHostToDevice));
        (void)g.commit();
    }
    e->frames = f;
    return EKF_OK;
}

int ekf_step_frame(EkfEngine *e, int frame, EkfStepInfo *info)
{
    if (!e || frame < 0 || frame >= e->frames.n) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    const size_t off = (size_t)e->frames.offset[frame];
    e->step_dt = staged_interval(e, frame);
    StepInput in;
    in.d_kps = e->frames.kps + off; in.d_desc = e->frames.desc + off * e->desc_bytes; in.n_kp = e->frames.count[frame];
    return run_step(e, in, info);
}

// ------------------------------------------------------------------------------------- NCC matcher (mode B)
static int ensure_pyramid(EkfEngine *e, int w, int h)
{
    if (e->img.w[0] == w && e->img.h[0] == h && e->img.px[0]) return EKF_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->stream2) HIPCHK(hipStreamSynchronize(e->stream2));
    e->img.prefetched = -1;
    e->img.valid = false; // until all six levels exist there is no pyramid: no size, no image
    for (int l = 0; l < 3; ++l) {
        e->bufs.release(&e->img.px[l]);
        e->bufs.release(&e->img.px2[l]);
        e->img.w[l] = e->img.h[l] = 0;
    }
    auto g = e->bufs.group();
    for (int l = 0; l < 3; ++l) {
        const size_t bytes = (size_t)std::max(w >> l, 1) * std::max(h >> l, 1);
        g.alloc(&e->img.px[l], bytes, false);
        g.alloc(&e->img.px2[l], bytes, false);
    }
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "hipMalloc image pyramid");
    for (int l = 0; l < 3; ++l) {
        e->img.w[l] = w >> l;
        e->img.h[l] = h >> l;
    }
    return EKF_OK;
}

static int valid_image_args(const uint8_t *image, int w, int h, int stride, int channels)
{
    return image && w >= 4 && h >= 4 && (channels == 1 || channels == 3 || channels == 4) && stride >= w * channels;
}

int ekf_image_upload(EkfEngine *e, const uint8_t *image, int width, int height, int stride, int channels)
{
    if (!e || !valid_image_args(image, width, height, stride, channels)) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int rc = ensure_pyramid(e, width, height);
    if (rc) return rc;
    const size_t bytes = (size_t)stride * height;
    if (e->img.raw_cap < bytes) {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->bufs.release(&e->img.raw);
        e->img.raw_cap = 0;
        const hipError_t st = e->bufs.alloc(&e->img.raw, bytes, false);
        if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc image staging");
        e->img.raw_cap = bytes;
    }
    HIPCHK(hipMemcpyAsync(e->img.raw, image, bytes, hipMemcpyHostToDevice, e->stream));
    launch_ncc_pyramid(e, e->img.raw, stride, channels);
    e->img.valid = true;
    return check_async(e);
}

int ekf_get_image_level(EkfEngine *e, int level, uint8_t *out, int *width, int *height)
{
    if (!e || level < 0 || level > 2 || !e->img.valid) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (width) *width = e->img.w[level];
    if (height) *height = e->img.h[level];
    if (out) HIPCHK(hipMemcpy(out, e->img.px[level], (size_t)e->img.w[level] * e->img.h[level], hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_capture_templates(EkfEngine *e, const int32_t *feat_idx, const double *uv, int count)
{
    if (!e || count < 0 || (count > 0 && (!feat_idx || !uv)) || !e->img.valid) return EKF_ERR_INVALID_ARG;
    if (count > e->cap) return EKF_ERR_CAPACITY;
    for (int i = 0; i < count; ++i)
        if (feat_idx[i] < 0 || feat_idx[i] >= e->N) return EKF_ERR_INVALID_ARG;
    if (count == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    // work_idx / pred_uv2 are free between stages
    HIPCHK(hipMemcpyAsync(e->d.work_idx, feat_idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.pred_uv2, uv, (size_t)count * 2 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    launch_ncc_capture(e, e->d.work_idx, e->d.pred_uv2, count);
    // template warp: source patches and the capture pose with the mode on; a capture with it off leaves "no source patch"
    if (e->d.wpose) launch_ncc_warp_capture(e, e->d.work_idx, e->d.pred_uv2, count, e->warp_on);
    HIPCHK(hipStreamSynchronize(e->stream)); // the host arrays may be reused by the caller
    return check_async(e);
}

// the detector threshold on the integer corner measure, from the double of the ABI (not NaN: the callers refuse it)
static long long response_threshold(double min_response)
{
    return min_response >= 9.2e18 ? 0x7fffffffffffffffLL : (min_response <= 0 ? 0 : (long long)min_response);
}

// detectNewImageFeatures (EKF/DetectNewImageFeatures.cpp:337-367) on the current image: device = masked corner
// candidates (kernels_detect.hip), host = the zone heuristic of searchFeaturesByZone (:171-330), with the two
// nondeterministic choices of the reference made deterministic: zones of equal population keep their id order (qsort
// is unstable) and the pick inside a zone is its strongest remaining candidate (the reference draws rand()).
int ekf_detect_new_features(EkfEngine *e, int max_new, int divide_times, double mask_ellipse_size, double min_response,
                            double *uv_out, int *count)
{
    if (!e || !count || max_new < 0 || divide_times < 0 || divide_times > 6 || (max_new > 0 && !uv_out) || std::isnan(min_response))
        return EKF_ERR_INVALID_ARG;
    *count = 0;
    if (!e->img.valid) {
        e->err = "new-feature detection: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    if (max_new == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    const int w = e->img.w[0], h = e->img.h[0];
    const int cells_x = w / 16, cells_y = h / 16, ncell = cells_x * cells_y;
    if (ncell <= 0) return EKF_OK;
    if (e->cells_cap < ncell) {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->bufs.release(&e->d.cell_resp);
        e->bufs.release(&e->d.cell_xy);
        e->cells_cap = 0;
        auto g = e->bufs.group();
        g.alloc(&e->d.cell_resp, (size_t)ncell, false);
        g.alloc(&e->d.cell_xy, (size_t)ncell * 2, false);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "hipMalloc detector cells");
        e->cells_cap = ncell;
    }
    launch_detect_cells(e, e->n_gates, cells_x, cells_y, e->d.cell_resp, e->d.cell_xy);
    std::vector<long long> resp(ncell);
    std::vector<int> xy(2 * (size_t)ncell);
    std::vector<double> gates(8 * (size_t)std::max(e->n_gates, 1));
    HIPCHK(hipMemcpyAsync(resp.data(), e->d.cell_resp, resp.size() * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(xy.data(), e->d.cell_xy, xy.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if (e->n_gates > 0)
        HIPCHK(hipMemcpyAsync(gates.data(), e->d.gates, (size_t)e->n_gates * 8 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc = check_async(e);
    if (rc) return rc;

    struct Cand { int x, y; long long r; };
    std::vector<Cand> cands;
    const long long thr = response_threshold(min_response);
    for (int c = 0; c < ncell; ++c)
        if (resp[c] >= 0 && resp[c] >= thr) cands.push_back(Cand{xy[2 * c], xy[2 * c + 1], resp[c]});
    if ((int)cands.size() <= max_new) { // :357-370: fewer than asked for -> all of them
        for (size_t i = 0; i < cands.size(); ++i) {
            uv_out[2 * i] = cands[i].x;
            uv_out[2 * i + 1] = cands[i].y;
        }
        *count = (int)cands.size();
        return EKF_OK;
    }
    const int zones_row = 1 << divide_times;
    const int zw = std::max(w / zones_row, 1), zh = std::max(h / zones_row, 1);
    const int nzone = zones_row * zones_row;
    auto zone_of = [&](double x, double y) { // getPointZone :87-92
        const int id = ((int)y / zh) * (w / zw) + (int)x / zw;
        return std::min(std::max(id, 0), nzone - 1);
    };
    struct Zone { int id, count; std::vector<int> cand; };
    std::vector<Zone> zones(nzone);
    for (int z = 0; z < nzone; ++z) zones[z] = Zone{z, 0, {}};
    for (size_t i = 0; i < cands.size(); ++i) zones[zone_of(cands[i].x, cands[i].y)].cand.push_back((int)i);
    for (int k = 0; k < e->n_gates; ++k) zones[zone_of(gates[8 * (size_t)k + 5], gates[8 * (size_t)k + 6])].count++;
    std::vector<int> order(nzone);
    for (int z = 0; z < nzone; ++z) order[z] = z;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return zones[a].count < zones[b].count; });
    // mask of the features added in this call: the "ellipse" of diag(size, size), a disc of integer radius
    const int radius = (int)std::nearbyint((float)(2.0 * std::sqrt(mask_ellipse_size * EKF_CHISQ_95_2)));
    std::vector<std::pair<int, int>> added;
    int left = max_new, n_out = 0;
    size_t head = 0; // order[head..] is the list; zones without candidates are popped from the front
    while (head < order.size() && left > 0) {
        Zone &z = zones[order[head]];
        if (z.cand.empty()) {
            ++head;
            continue;
        }
        size_t best = 0;
        for (size_t i = 1; i < z.cand.size(); ++i) { // strongest, ties -> first in cell order
            const Cand &a = cands[z.cand[i]], &bb = cands[z.cand[best]];
            if (a.r > bb.r || (a.r == bb.r && z.cand[i] < z.cand[best])) best = i;
        }
        const Cand c = cands[z.cand[best]];
        bool free_px = true;
        for (const auto &a : added) {
            const double dx = (double)(float)c.x - (double)(float)a.first, dy = (double)(float)c.y - (double)(float)a.second;
            if (2.0 * std::sqrt(dx * dx + dy * dy) <= 2.0 * radius) { free_px = false; break; }
        }
        if (free_px) {
            uv_out[2 * n_out] = c.x;
            uv_out[2 * n_out + 1] = c.y;
            ++n_out;
            z.count++;
            for (size_t p = head; p + 1 < order.size(); ++p) { // :272-296: keep the list ordered by population
                if (zones[order[p]].count >= zones[order[p + 1]].count) std::swap(order[p], order[p + 1]);
                else break;
            }
            added.emplace_back(c.x, c.y);
            --left;
        }
        // the candidate is consumed either way (:314-318); z may have moved, so erase through the zone object
        Zone &zz = zones[zone_of(c.x, c.y)];
        for (size_t i = 0; i < zz.cand.size(); ++i)
            if (cands[zz.cand[i]].x == c.x && cands[zz.cand[i]].y == c.y) {
                zz.cand[i] = zz.cand.back();
                zz.cand.pop_back();
                break;
            }
    }
    *count = n_out;
    return EKF_OK;
}

// ------------------------------------------------------------------------ keypoints + BRIEF-32 (image in, descriptor matcher)
// scratch of the detector (one bit per pixel of the current frame) and the staging of the stage calls (det_cap entries)
static int ensure_kp_scratch(EkfEngine *e, int det_cap)
{
    const size_t words = kp_rowmask_words(e->img.w[0], e->img.h[0]);
    if (e->rowmask_cap < words) {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->bufs.release(&e->d.kp_rowmask);
        e->rowmask_cap = 0;
        const hipError_t st = e->bufs.alloc(&e->d.kp_rowmask, words, false);
        if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc keypoint row mask");
        e->rowmask_cap = words;
    }
    if (e->det_cap < det_cap) {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->bufs.release(&e->d.det_kps);
        e->bufs.release(&e->d.det_desc);
        e->bufs.release(&e->d.det_centres);
        e->det_cap = 0;
        auto g = e->bufs.group();
        g.alloc(&e->d.det_kps, (size_t)det_cap, false);
        g.alloc(&e->d.det_desc, (size_t)det_cap * EKF_DESC_BYTES, false);
        g.alloc(&e->d.det_centres, (size_t)det_cap * 2, false);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "hipMalloc keypoint staging");
        e->det_cap = det_cap;
    }
    return EKF_OK;
}

// the step's keypoints: masked detection into d.kps (the first kcap in raster order), their descriptors into d.kdesc; the
// count stays on the device (counts[CNT_KP_FOUND]) for k_match and k_brief -- no read-back
int ekf::detect_step_keypoints(EkfEngine *e) { return detect_frame_keypoints(e, e->kp_min_response, true); }

// the same two launches with the threshold and the mask as arguments (the step: its own threshold, masked; ekf_relocalise_image:
// the caller's, unmasked)
int ekf::detect_frame_keypoints(EkfEngine *e, double min_response, bool masked)
{
    if (!e->img.valid) {
        e->err = "keypoint matcher: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    int rc = ensure_kp_scratch(e, 0);
    if (rc) return rc;
    launch_kp_detect(e, response_threshold(min_response), masked, e->d.kp_rowmask, e->d.kps, e->kcap, e->d.counts + CNT_KP_FOUND);
    launch_brief(e, e->d.kps, nullptr, e->kcap, e->d.counts + CNT_KP_FOUND, e->d.kdesc);
    return check_async(e);
}

static int step_image_dev(EkfEngine *e, EkfStepInfo *info)
{
    StepInput in;
    in.source = STEP_NCC;
    if (e->image_matcher == EKF_IMAGE_MATCHER_KEYPOINTS) {
        in.source = STEP_DETECT_KEYPOINTS;
        in.d_kps = e->d.kps; in.d_desc = e->d.kdesc; in.n_kp = e->kcap;
    }
    return run_step(e, in, info);
}

int ekf_set_image_matcher(EkfEngine *e, int matcher, double min_response)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if ((matcher != EKF_IMAGE_MATCHER_NCC && matcher != EKF_IMAGE_MATCHER_KEYPOINTS) || std::isnan(min_response)) {
        e->err = "ekf_set_image_matcher: unknown matcher or NaN threshold";
        return EKF_ERR_INVALID_ARG;
    }
    if (matcher == EKF_IMAGE_MATCHER_KEYPOINTS && e->desc_f32) {
        e->err = "keypoint matcher: BRIEF-32 needs an EKF_DESCRIPTOR_U8_HAMMING engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (matcher == EKF_IMAGE_MATCHER_KEYPOINTS && e->shard_world > 1) {
        e->err = "keypoint matcher: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    e->image_matcher = matcher;
    e->kp_min_response = min_response;
    return EKF_OK;
}

int ekf_detect_keypoints(EkfEngine *e, double min_response, int masked, EkfKeypoint *kps, uint8_t *desc32, int capacity,
                         int *n_found)
{
    if (!e || !n_found || capacity < 0 || std::isnan(min_response)) return EKF_ERR_INVALID_ARG;
    *n_found = 0;
    if (!e->img.valid) {
        e->err = "keypoint detection: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    if (desc32 && e->desc_f32) {
        e->err = "keypoint detection: BRIEF-32 descriptors need an EKF_DESCRIPTOR_U8_HAMMING engine";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    int rc = ensure_kp_scratch(e, std::max(capacity, 1));
    if (rc) return rc;
    launch_kp_detect(e, response_threshold(min_response), masked != 0, e->d.kp_rowmask, e->d.det_kps, capacity,
                     e->d.counts + CNT_KP_FOUND);
    if ((rc = read_counts(e))) return rc;
    const int found = e->h_counts[CNT_KP_FOUND], n = std::min(found, capacity);
    if (desc32 && n > 0) launch_brief(e, e->d.det_kps, nullptr, n, nullptr, e->d.det_desc);
    if (kps && n > 0) HIPCHK(hipMemcpyAsync(kps, e->d.det_kps, (size_t)n * sizeof(EkfKeypoint), hipMemcpyDeviceToHost, e->stream));
    if (desc32 && n > 0) HIPCHK(hipMemcpyAsync(desc32, e->d.det_desc, (size_t)n * EKF_DESC_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *n_found = found;
    return check_async(e);
}

int ekf_describe(EkfEngine *e, const double *uv, int count, uint8_t *desc32)
{
    if (!e || count < 0 || (count > 0 && (!uv || !desc32))) return EKF_ERR_INVALID_ARG;
    if (!e->img.valid) {
        e->err = "ekf_describe: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    if (e->desc_f32) {
        e->err = "ekf_describe: BRIEF-32 descriptors need an EKF_DESCRIPTOR_U8_HAMMING engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (count == 0) return EKF_OK;
    std::vector<int> c(2 * (size_t)count);
    for (size_t i = 0; i < c.size(); ++i) {
        if (!(std::fabs(uv[i]) <= 1.0e7)) { // also NaN
            e->err = "ekf_describe: pixel position not finite or out of range";
            return EKF_ERR_INVALID_ARG;
        }
        c[i] = (int)std::floor(uv[i] + 0.5);
    }
    HIPCHK(hipSetDevice(e->device));
    int rc = ensure_kp_scratch(e, count);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(e->d.det_centres, c.data(), c.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    launch_brief(e, nullptr, e->d.det_centres, count, nullptr, e->d.det_desc);
    HIPCHK(hipMemcpyAsync(desc32, e->d.det_desc, (size_t)count * EKF_DESC_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_async(e);
}

int ekf_get_step_keypoints(const EkfEngine *e, int *detected, int *kept)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (detected) *detected = e->step_kp_detected;
    if (kept) *kept = e->step_kp_kept;
    return EKF_OK;
}

// wide search: the list of wide slots (cap records) and their per-tile partial results (cap x tiles of the coarse level), allocated
// by the first match that needs them and again when a larger frame brings more tiles
// (parts = 2: a second partial table behind the first, for the rival pass of the distinctiveness test)
static int ensure_wide_tables(EkfEngine *e, int parts)
{
    const int tiles = ncc_wide_tiles(e->img.w[2], e->img.h[2]);
    if (e->d.wide_list && tiles <= e->wide_tiles && parts <= e->wide_parts) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->bufs.release(&e->d.wide_list);
    e->bufs.release(&e->d.wide_part);
    e->wide_tiles = e->wide_parts = 0;
    auto g = e->bufs.group();
    g.alloc_bytes(&e->d.wide_list, (size_t)e->cap * NCC_WIDE_SLOT_BYTES + NCC_WIDE_TOTALS_BYTES);
    g.alloc_bytes(&e->d.wide_part, (size_t)parts * e->cap * (size_t)std::max(tiles, 1) * NCC_WIDE_PARTIAL_BYTES);
    if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "wide search tables");
    e->wide_tiles = tiles;
    e->wide_parts = parts;
    return EKF_OK;
}

int ekf::match_ncc_dev(EkfEngine *e, int *n_matches)
{
    if (!e->img.valid) {
        e->err = "NCC matcher: no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    e->last_match_warped = e->warp_on;
    const bool subpix = e->subpix_on, wide = e->wide_on;
    const double coef = e->distinct_coef;
    int rc = wide ? ensure_wide_tables(e, coef > 0.0 ? 2 : 1) : EKF_OK;
    if (rc) return rc;
    launch_match_ncc(e, e->n_pred, subpix, wide, coef);
    rc = read_counts(e);
    if (rc) return rc;
    *n_matches = e->h_counts[CNT_NMATCH];
    e->warp_counts[0] = e->last_match_warped ? e->h_counts[CNT_WARP_OK] : 0;
    e->warp_counts[1] = e->last_match_warped ? e->h_counts[CNT_WARP_FB] : 0;
    e->subpix_counts[0] = subpix ? e->h_counts[CNT_SUBPIX_FIT] : 0;
    e->subpix_counts[1] = subpix ? e->h_counts[CNT_SUBPIX_INT] : 0;
    e->wide_counts[0] = wide ? e->h_counts[CNT_WIDE_SLOTS] : 0;
    e->wide_counts[1] = wide ? e->h_counts[CNT_WIDE_CANDS] : 0;
    e->distinct_counts[0] = coef > 0.0 ? e->h_counts[CNT_RIVAL_WITH] : 0;
    e->distinct_counts[1] = coef > 0.0 ? e->h_counts[CNT_RIVAL_REJ] : 0;
    e->rival_slots = coef > 0.0 ? std::max(e->n_pred, 0) : 0;
    return check_async(e);
}

int ekf_set_template_warp(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) {
        e->err = "template warp: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (on && !e->d.wpose) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (const int rc = ensure_warp_tables(e)) return rc;
    }
    e->warp_on = on != 0;
    if (!e->warp_on) e->pn_on = false; // the patch normals live in the warp
    return EKF_OK;
}

int ekf_set_patch_normals(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) {
        e->err = "patch normals: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (!e->warp_on) {
        e->err = "patch normals: the template warp is off (ekf_set_template_warp)";
        return EKF_ERR_INVALID_ARG;
    }
    if (on && !e->d.wnorm) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (const int rc = ensure_patch_normal_tables(e)) return rc;
    }
    e->pn_on = on != 0;
    return EKF_OK;
}

int ekf_refine_patch_normals(EkfEngine *e, const EkfMatch *matches, int M)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (!e->pn_on || !e->img.valid) {
        e->err = "ekf_refine_patch_normals: the mode is off, or no image uploaded";
        return EKF_ERR_INVALID_ARG;
    }
    int rc = validate_matches(e, matches, M);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    if (M > 0) HIPCHK(hipMemcpyAsync(e->d.pn_list, matches, (size_t)M * sizeof(EkfMatch), hipMemcpyHostToDevice, e->stream));
    launch_ncc_normal(e, M);
    if ((rc = read_counts(e))) return rc; // (synchronises: the caller's list has been read)
    harvest_pn_counts(e);
    return check_async(e);
}

int ekf_get_patch_normals(EkfEngine *e, const int32_t *feat_idx, int count, EkfPatchNormal *out)
{
    if (!e || count < 0 || (count > 0 && (!feat_idx || !out))) return EKF_ERR_INVALID_ARG;
    for (int i = 0; i < count; ++i)
        if (feat_idx[i] < 0 || feat_idx[i] >= e->N) return EKF_ERR_INVALID_ARG;
    if (!e->d.wnorm) {
        e->err = "ekf_get_patch_normals: the mode has never been on";
        return EKF_ERR_INVALID_ARG;
    }
    if (count == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t N = (size_t)e->N;
    std::vector<PatchNormalRec> rec(N);
    std::vector<double> pose(WPOSE_DOUBLES * N), pos(6 * N);
    std::vector<int> type(N);
    HIPCHK(hipMemcpy(rec.data(), e->d.wnorm, N * sizeof(PatchNormalRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pose.data(), e->d.wpose, WPOSE_DOUBLES * N * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos.data(), e->d.feat_pos, 6 * N * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(type.data(), e->d.feat_type, N * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) {
        const size_t f = (size_t)feat_idx[i];
        const double *ps = &pose[WPOSE_DOUBLES * f];
        EkfPatchNormal o;
        std::memset(&o, 0, sizeof(o));
        if (patch_has_source(ps)) {
            double R0[9];
            quat_to_rot(ps + 3, R0);
            if (rec[f].updates > 0) {
                o.pq[0] = rec[f].pq[0];
                o.pq[1] = rec[f].pq[1];
                for (int k = 0; k < 3; ++k) o.info[k] = rec[f].info[k];
                o.updates = rec[f].updates;
            } else { // the rule of DESIGN.md 4.6 as a slope, and the first update's prior
                double X[3];
                patch_world_point(&pos[6 * f], type[f], X);
                pn_rule_slope(R0, X, ps, o.pq);
                o.info[0] = o.info[2] = PN_PRIOR_INFO;
            }
            pn_normal(R0, o.pq[0], o.pq[1], o.normal);
        }
        out[i] = o;
    }
    return EKF_OK;
}

int ekf_set_patch_normal(EkfEngine *e, int feat, const double pq[2], const double info[3])
{
    if (!e || !pq || !info || feat < 0 || feat >= e->N || !e->d.wnorm) return EKF_ERR_INVALID_ARG;
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(pq[k])) return EKF_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(info[k])) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    PatchNormalRec rec;
    HIPCHK(hipMemcpy(&rec, e->d.wnorm + feat, sizeof(rec), hipMemcpyDeviceToHost));
    rec.pq[0] = pq[0];
    rec.pq[1] = pq[1];
    for (int k = 0; k < 3; ++k) rec.info[k] = info[k];
    rec.updates = std::max(rec.updates, 1);
    rec.pad = 0;
    HIPCHK(hipMemcpy(e->d.wnorm + feat, &rec, sizeof(rec), hipMemcpyHostToDevice));
    return EKF_OK;
}

int ekf_get_patch_normal_counts(const EkfEngine *e, int *updated, int *skipped)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (updated) *updated = e->pn_counts[0];
    if (skipped) *skipped = e->pn_counts[1];
    return EKF_OK;
}

int ekf_get_template_warp_counts(const EkfEngine *e, int *warped_levels, int *fallback_levels)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (warped_levels) *warped_levels = e->warp_counts[0];
    if (fallback_levels) *fallback_levels = e->warp_counts[1];
    return EKF_OK;
}

int ekf_set_subpixel_matches(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) {
        e->err = "sub-pixel matches: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    e->subpix_on = on != 0;
    return EKF_OK;
}

int ekf_get_subpixel_counts(const EkfEngine *e, int *refined_axes, int *integer_axes)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (refined_axes) *refined_axes = e->subpix_counts[0];
    if (integer_axes) *integer_axes = e->subpix_counts[1];
    return EKF_OK;
}

int ekf_set_ncc_wide_search(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) {
        e->err = "wide search: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    e->wide_on = on != 0;
    return EKF_OK;
}

int ekf_get_ncc_wide_counts(const EkfEngine *e, int *wide_slots, int *wide_candidates)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (wide_slots) *wide_slots = e->wide_counts[0];
    if (wide_candidates) *wide_candidates = e->wide_counts[1];
    return EKF_OK;
}

int ekf_set_ncc_distinct(EkfEngine *e, double coef)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (!(coef >= 0.0 && coef <= 1.0)) { // (NaN fails both)
        e->err = "NCC distinctiveness test: the coefficient lies outside [0, 1]";
        return EKF_ERR_INVALID_ARG;
    }
    if (coef > 0.0 && e->shard_world > 1) {
        e->err = "NCC distinctiveness test: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (coef > 0.0 && !e->d.mt_rival) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamSynchronize(e->stream));
        const hipError_t st = e->bufs.alloc(&e->d.mt_rival, (size_t)e->cap);
        if (st != hipSuccess) return alloc_failed(e, st, "NCC distinctiveness table");
    }
    e->distinct_coef = coef;
    if (coef == 0.0) e->rival_slots = 0; // off: ekf_get_ncc_rivals has nothing to return
    return EKF_OK;
}

int ekf_get_ncc_distinct_counts(const EkfEngine *e, int *with_rival, int *rejected)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (with_rival) *with_rival = e->distinct_counts[0];
    if (rejected) *rejected = e->distinct_counts[1];
    return EKF_OK;
}

int ekf_get_ncc_rivals(EkfEngine *e, EkfNccRival *out, int capacity, int *count)
{
    if (!e || !count || capacity < 0 || (capacity > 0 && !out)) return EKF_ERR_INVALID_ARG;
    const int n = e->distinct_coef > 0.0 ? e->rival_slots : 0;
    *count = n;
    if (n == 0) return EKF_OK;
    if (capacity < n) {
        e->err = "ekf_get_ncc_rivals: the buffer holds fewer records than the last match had prediction slots";
        return EKF_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<NccRivalRec> rec((size_t)n);
    std::vector<int> feat((size_t)n);
    HIPCHK(hipMemcpy(rec.data(), e->d.mt_rival, (size_t)n * sizeof(NccRivalRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(feat.data(), e->d.plist, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) {
        EkfNccRival o;
        o.featureIndex = feat[k];
        o.state = rec[k].state;
        o.rivalPos[0] = (float)rec[k].rx;
        o.rivalPos[1] = (float)rec[k].ry;
        o.distance = rec[k].d1;
        o.rivalDistance = rec[k].d2;
        out[k] = o;
    }
    return EKF_OK;
}

// ---------------------------------------------------------------------------------- filter consistency
int ekf_set_consistency(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) {
        e->err = "filter consistency: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (on && !e->d.cons_ctl) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamSynchronize(e->stream));
        auto g = e->bufs.group();
        g.alloc(&e->d.cons_recs, (size_t)CONS_SLOTS * e->cap);
        g.alloc(&e->d.cons_ctl, 1);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "filter consistency tables");
    }
    if (on && !e->consistency) ++e->cons_epoch; // records of an earlier period with the mode on are not this one's
    e->consistency = on != 0;
    return EKF_OK;
}

// synchronises, reports a pending asynchronous error (whose retry may record) and reads the control block; *n = records of the
// current epoch
static int read_consistency(EkfEngine *e, ConsCtl *ctl, int *n, int *pending)
{
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    *pending = take_pending_error(e);
    std::memset(ctl, 0, sizeof(*ctl));
    if (e->d.cons_ctl) HIPCHK(hipMemcpy(ctl, e->d.cons_ctl, sizeof(*ctl), hipMemcpyDeviceToHost));
    *n = (e->consistency && ctl->epoch == e->cons_epoch) ? std::min(std::max(ctl->count, 0), CONS_SLOTS) : 0;
    return EKF_OK;
}

int ekf_get_consistency(EkfEngine *e, EkfUpdateConsistency *out, int capacity, int *count)
{
    if (!e || !count || (out && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    ConsCtl ctl;
    int n = 0, pending = EKF_OK, rc;
    if ((rc = read_consistency(e, &ctl, &n, &pending))) return rc;
    *count = n;
    if (n == 0 || !out) return pending;
    if (capacity < n) {
        e->err = "ekf_get_consistency: capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " records";
        return EKF_ERR_CAPACITY;
    }
    for (int k = 0; k < n; ++k) out[k] = ctl.rec[k];
    return pending;
}

int ekf_get_innovations(EkfEngine *e, int which, EkfInnovation *out, int capacity, int *count)
{
    if (!e || !count || (out && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    ConsCtl ctl;
    int n = 0, pending = EKF_OK, rc;
    if ((rc = read_consistency(e, &ctl, &n, &pending))) return rc;
    if (which < 0 || which >= n) {
        e->err = "ekf_get_innovations: record " + std::to_string(which) + " of " + std::to_string(n);
        return EKF_ERR_INVALID_ARG;
    }
    const int M = std::min(std::max(ctl.rec[which].matches, 0), e->cap);
    *count = M;
    if (M == 0 || !out) return pending;
    if (capacity < M) {
        e->err = "ekf_get_innovations: capacity " + std::to_string(capacity) + " < " + std::to_string(M) + " matches";
        return EKF_ERR_CAPACITY;
    }
    HIPCHK(hipMemcpy(out, e->d.cons_recs + (size_t)which * e->cap, (size_t)M * sizeof(EkfInnovation), hipMemcpyDeviceToHost));
    return pending;
}

int ekf_get_consistency_totals(EkfEngine *e, double *nis_sum, int64_t *rows_sum, int64_t *updates)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    ConsCtl ctl;
    int n = 0, pending = EKF_OK, rc;
    if ((rc = read_consistency(e, &ctl, &n, &pending))) return rc;
    if (nis_sum) *nis_sum = ctl.nis_sum;
    if (rows_sum) *rows_sum = ctl.rows_sum;
    if (updates) *updates = ctl.updates;
    return pending;
}

int ekf_reset_consistency_totals(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (!e->d.cons_ctl) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    static_assert(offsetof(ConsCtl, nis_sum) == 8 && offsetof(ConsCtl, rec) == 32, "layout of the totals");
    HIPCHK(hipMemsetAsync((char *)e->d.cons_ctl + offsetof(ConsCtl, nis_sum), 0, offsetof(ConsCtl, rec) - offsetof(ConsCtl, nis_sum), e->stream));
    return EKF_OK;
}

// ---------------------------------------------------------------------------------- measurement budget
int ekf_set_measurement_budget(EkfEngine *e, int K)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (K < 0) {
        e->err = "measurement budget: K < 0";
        return EKF_ERR_INVALID_ARG;
    }
    if (K > 0 && e->shard_world > 1) {
        e->err = "measurement budget: not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    if (K > 0 && !e->d.bud_recs) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamSynchronize(e->stream));
        auto g = e->bufs.group();
        g.alloc(&e->d.bud_key, e->cap);
        g.alloc(&e->d.bud_all, e->cap);
        g.alloc(&e->d.bud_flag, e->cap);
        g.alloc(&e->d.bud_recs, e->cap);
        if (g.commit() != hipSuccess) return alloc_failed(e, g.status(), "measurement budget tables");
    }
    if (K == 0) e->bud_recs_n = 0;
    e->budget_K = K;
    return EKF_OK;
}

int ekf_get_measurement_ranks(EkfEngine *e, EkfMeasurementRank *out, int capacity, int *count)
{
    if (!e || !count || (out && capacity < 0)) return EKF_ERR_INVALID_ARG;
    *count = 0;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int pending = take_pending_error(e);
    const int n = e->d.bud_recs ? std::min(std::max(e->bud_recs_n, 0), e->cap) : 0;
    *count = n;
    if (n == 0 || !out) return pending;
    if (capacity < n) {
        e->err = "ekf_get_measurement_ranks: capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " records";
        return EKF_ERR_CAPACITY;
    }
    HIPCHK(hipMemcpy(out, e->d.bud_recs, (size_t)n * sizeof(EkfMeasurementRank), hipMemcpyDeviceToHost));
    return pending;
}

int ekf_get_measurement_budget_counts(const EkfEngine *e, int *predicted, int *selected)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (predicted) *predicted = e->bud_predicted;
    if (selected) *selected = e->bud_selected;
    return EKF_OK;
}

int ekf_get_match_templates(EkfEngine *e, const int32_t *feat_idx, int count, uint8_t *out)
{
    if (!e || count < 0 || (count > 0 && (!feat_idx || !out))) return EKF_ERR_INVALID_ARG;
    for (int i = 0; i < count; ++i)
        if (feat_idx[i] < 0 || feat_idx[i] >= e->N) return EKF_ERR_INVALID_ARG;
    if (count == 0) return EKF_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const uint8_t *src = e->last_match_warped ? e->d.wtmpl : e->d.tmpl;
    constexpr size_t TMPL = mapblob::TEMPLATE_BYTES;
    std::vector<uint8_t> all((size_t)e->N * TMPL);
    HIPCHK(hipMemcpy(all.data(), src, all.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) std::memcpy(out + i * TMPL, &all[feat_idx[i] * TMPL], TMPL);
    return EKF_OK;
}

int ekf_match_ncc(EkfEngine *e, EkfMatch *matches, int *n_matches)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int M = 0;
    int rc = match_ncc_dev(e, &M);
    if (rc) return rc;
    if (n_matches) *n_matches = M;
    if (matches && M > 0) HIPCHK(hipMemcpy(matches, e->d.matches, (size_t)M * sizeof(EkfMatch), hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_step_image(EkfEngine *e, const uint8_t *image, int width, int height, int stride, int channels, EkfStepInfo *info)
{
    int rc = ekf_image_upload(e, image, width, height, stride, channels);
    if (rc) return rc;
    e->step_dt = e->frame_interval;
    return step_image_dev(e, info);
}

int ekf_images_upload(EkfEngine *e, int n_frames, const uint8_t *images, int width, int height, int stride, int channels)
{
    if (!e || n_frames < 0 || (n_frames > 0 && !valid_image_args(images, width, height, stride, channels))) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->stream2) HIPCHK(hipStreamSynchronize(e->stream2));
    e->img.prefetched = -1;
    e->bufs.release(&e->img.seq);
    e->img.seq_n = 0;
    if (n_frames == 0) return EKF_OK;
    const size_t bytes = (size_t)stride * height * n_frames;
    const hipError_t st = e->bufs.alloc(&e->img.seq, bytes, false);
    if (st != hipSuccess) return alloc_failed(e, st, "hipMalloc image sequence");
    HIPCHK(hipMemcpy(e->img.seq, images, bytes, hipMemcpyHostToDevice));
    e->img.seq_n = n_frames;
    e->img.seq_w = width;
    e->img.seq_h = height;
    e->img.seq_stride = stride;
    e->img.seq_channels = channels;
    return EKF_OK;
}

static int staged_pyramid(EkfEngine *e, int frame)
{
    if (frame < 0 || frame >= e->img.seq_n) return EKF_ERR_INVALID_ARG;
    int rc = ensure_pyramid(e, e->img.seq_w, e->img.seq_h);
    if (rc) return rc;
    const size_t frame_bytes = (size_t)e->img.seq_stride * e->img.seq_h;
    if (frame == e->img.prefetched) { // reduced on stream2 while the previous frame was being filtered
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_prefetch, 0));
        for (int l = 0; l < 3; ++l) std::swap(e->img.px[l], e->img.px2[l]);
    } else {
        launch_ncc_pyramid(e, e->img.seq + (size_t)frame * frame_bytes, e->img.seq_stride, e->img.seq_channels);
    }
    e->img.prefetched = -1;
    e->img.valid = true;
    // image-only work of the NEXT staged frame goes to the second stream, behind everything already queued on the main
    // stream (the last readers of the buffer it overwrites), and runs concurrently with this frame's filter step
    if (frame + 1 < e->img.seq_n && e->stream2) {
        HIPCHK(hipEventRecord(e->ev_main, e->stream));
        HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_main, 0));
        launch_ncc_pyramid_on(e, e->stream2, e->img.px2, e->img.seq + (size_t)(frame + 1) * frame_bytes, e->img.seq_stride,
                              e->img.seq_channels);
        HIPCHK(hipEventRecord(e->ev_prefetch, e->stream2));
        e->img.prefetched = frame + 1;
    }
    return EKF_OK;
}

int ekf_select_staged_image(EkfEngine *e, int frame)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int rc = staged_pyramid(e, frame);
    return rc ? rc : check_async(e);
}

int ekf_step_staged_image(EkfEngine *e, int frame, EkfStepInfo *info)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    int rc = staged_pyramid(e, frame);
    if (rc) return rc;
    e->step_dt = staged_interval(e, frame);
    return step_image_dev(e, info);
}

// -------------------------------------------------------------------------------------------------- timing
int ekf_timing_enable(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->timing = on != 0;
    return EKF_OK;
}

int ekf_timing_reset(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(e->stream);
    harvest_pu_events(e);
    e->pu_log.clear();
    std::memset(&e->times, 0, sizeof(e->times));
    e->sweep_ms = e->sweep_flops_f64 = e->sweep_flops_b = 0.0;
    e->sweep_panels = e->sweep_updates = e->sweep_launches = 0;
    e->slice_ms = 0.0;
    return EKF_OK;
}

int ekf_timing_get(EkfEngine *e, EkfStageTimes *out)
{
    if (!e || !out) return EKF_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(e->stream);
    harvest_pu_events(e);
    *out = e->times;
    return EKF_OK;
}

int ekf_timing_sweep(EkfEngine *e, double *kernel_ms, int64_t *panels, int64_t *updates, double *flops_fp64, double *flops_b)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(e->stream);
    harvest_pu_events(e);
    if (kernel_ms) *kernel_ms = e->sweep_ms;
    if (panels) *panels = e->sweep_panels;
    if (updates) *updates = e->sweep_updates;
    if (flops_fp64) *flops_fp64 = e->sweep_flops_f64;
    if (flops_b) *flops_b = e->sweep_flops_b;
    return EKF_OK;
}

int ekf_get_sweep_retries(const EkfEngine *e) { return e ? e->sweep_retries : 0; }

int ekf_debug_stall_next_sweep(EkfEngine *e) // include/ekf_test_hooks.h
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->ps_fault = 1;
    return EKF_OK;
}

int ekf_debug_dense_products(EkfEngine *e, int on)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    e->px_dense = on != 0;
    return EKF_OK;
}

int ekf_debug_plane0_pieces(EkfEngine *e, int *nonzero, int *total)
{
    if (!e || !nonzero || !total || !e->d.Bz) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int cbs = (e->n + 31) / 32, groups = (2 * e->last_update.call.M + 15) / 16;
    std::vector<uint8_t> row((size_t)e->bz_stride);
    int nz = 0;
    for (int c = 0; c < cbs; ++c) {
        HIPCHK(hipMemcpy(row.data(), e->d.Bz + (size_t)c * e->bz_stride, (size_t)groups, hipMemcpyDeviceToHost));
        for (int k = 0; k < groups; ++k) nz += row[k] ? 1 : 0;
    }
    *nonzero = nz;
    *total = cbs * groups;
    return EKF_OK;
}

int ekf_debug_get_hp_rows(EkfEngine *e, const int32_t *feat_idx, int count, double *HP, double *HPc)
{
    if (!e || count < 0 || (count > 0 && (!feat_idx || !HP))) return EKF_ERR_INVALID_ARG;
    if (e->shard_world > 1) { // a rank holds only the rows of the features it owns
        e->err = "ekf_debug_get_hp_rows is not available on a sharded engine";
        return EKF_ERR_INVALID_ARG;
    }
    for (int k = 0; k < count; ++k)
        if (feat_idx[k] < 0 || feat_idx[k] >= e->N) return EKF_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int n = e->n;
    const size_t w = hp_elem_bytes(e);
    std::vector<float> tmp(w == 4 ? (size_t)2 * n : 0);
    for (int k = 0; k < count; ++k) {
        // rows 2 fi and 2 fi + 1 are adjacent: one strided copy of 2 x n elements
        const uint8_t *src = (const uint8_t *)e->d.HP + (size_t)2 * feat_idx[k] * e->ldP * w;
        double *dst = HP + (size_t)2 * n * k;
        if (w == 4) {
            HIPCHK(hipMemcpy2D(tmp.data(), (size_t)n * 4, src, (size_t)e->ldP * 4, (size_t)n * 4, 2, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < (size_t)2 * n; ++i) dst[i] = (double)tmp[i];
        } else {
            HIPCHK(hipMemcpy2D(dst, (size_t)n * 8, src, (size_t)e->ldP * 8, (size_t)n * 8, 2, hipMemcpyDeviceToHost));
        }
        if (HPc && e->d.HPc)
            HIPCHK(hipMemcpy2D(HPc + (size_t)26 * k, 13 * 8, e->d.HPc + (size_t)2 * feat_idx[k] * 16, 16 * 8, 13 * 8, 2, hipMemcpyDeviceToHost));
    }
    return EKF_OK;
}

int ekf_debug_stall_sweep_after(EkfEngine *e, int skip)
{
    if (!e || skip < 0) return EKF_ERR_INVALID_ARG;
    e->ps_fault = skip + 1; // counted down by the persistent launches; the one that reaches zero runs without its chain workgroup
    return EKF_OK;
}

int ekf_round_covariance_to_f32(EkfEngine *e)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    if (e->f32) return EKF_ERR_INVALID_ARG; // an fp64 engine only: the fp32 configurations store fp32 already
    HIPCHK(hipSetDevice(e->device));
    launch_round_P_f32(e);
    return EKF_OK;
}

int ekf_timing_sweep_launches(EkfEngine *e, int64_t *launches, double *slice_ms)
{
    if (!e) return EKF_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(e->stream);
    harvest_pu_events(e);
    if (launches) *launches = e->sweep_launches;
    if (slice_ms) *slice_ms = e->slice_ms;
    return EKF_OK;
}

int ekf_timing_p_update_launches(EkfEngine *e, int capacity, int32_t *m_rows, float *ms, int *count)
{
    if (!e || !count) return EKF_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(e->stream);
    harvest_pu_events(e);
    *count = (int)e->pu_log.size();
    for (int i = 0; i < *count && i < capacity; ++i) {
        if (m_rows) m_rows[i] = e->pu_log[i].first;
        if (ms) ms[i] = e->pu_log[i].second;
    }
    return EKF_OK;
}

