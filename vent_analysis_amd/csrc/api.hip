// api.hip -- the extern "C" boundary of libventhip.so (include/vent_hip.h).
// Contexts own a HIP stream on one device; batches own the device buffers of nb studies.
// No exception crosses the ABI: every entry point maps failures to a status code and keeps the
// message for vh_last_error().
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <memory>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "vh_internal.h"
#include "register_maps_host.h"
#include "resample_host.h"
#include "zones_host.h"

// ---------------------------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------------------------
static void kst_reset(vh_batch *b) {
    HIP_TRY(hipMemsetAsync(b->d_kst, 0xFF, sizeof(unsigned long long) * VH_KST_CAP, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_kst + VH_KST_CAP, 0, sizeof(unsigned long long) * VH_KST_CAP, b->stream));
    b->kst_n = 0;
}

ScopedKTimer::ScopedKTimer(vh_batch *bb, const char *name, double bytes, bool stamped, hipStream_t on)
    : b(bb), t(nullptr), s(on ? on : bb->stream) {
    if (!b->profile) return;
    t = &b->timers[name];
    if (bytes > 0) t->bytes_per_launch = bytes;
    if (stamped) {
        if (b->d_kst.reserve(2 * VH_KST_CAP)) kst_reset(b);
        if (b->kst_n < VH_KST_CAP) {
            const int s = b->kst_n++;
            t->slots.push_back(s);
            ks = b->d_kst + s;
            return;
        }   // (every slot taken until the next resolve: events)
    }
    hipEvent_t e0;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, s));
    t->ev.push_back(e0);
}
ScopedKTimer::~ScopedKTimer() {
    if (!t || ks) return;
    (void)hipEventRecord(e1, s);
    t->ev.push_back(e1);
}

static void clear_timers(vh_batch *b) {
    for (auto &kv : b->timers)
        for (auto e : kv.second.ev) (void)hipEventDestroy(e);
    b->timers.clear();
    if (b->d_kst && b->kst_n) kst_reset(b);
}

static void resolve_timers(vh_batch *b) {
    std::vector<unsigned long long> ks;
    double ticks_per_ms = 0.0;
    if (b->d_kst && b->kst_n) {   // the stamped launches' spans (wall clock ticks; the rate in kHz)
        HIP_TRY(hipStreamSynchronize(b->stream));
        ks.resize(2 * VH_KST_CAP);
        HIP_TRY(hipMemcpy(ks.data(), b->d_kst, sizeof(unsigned long long) * 2 * VH_KST_CAP,
                          hipMemcpyDeviceToHost));
        int khz = 0;
        HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, b->ctx->device));
        ticks_per_ms = (double)khz;
    }
    for (auto &kv : b->timers) {
        KTimer &t = kv.second;
        for (size_t i = 0; i + 1 < t.ev.size(); i += 2) {
            float ms = 0.f;
            HIP_TRY(hipEventSynchronize(t.ev[i + 1]));
            HIP_TRY(hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
            t.total_ms += ms;
            t.launches += 1;
            (void)hipEventDestroy(t.ev[i]);
            (void)hipEventDestroy(t.ev[i + 1]);
        }
        t.ev.clear();
        for (int s : t.slots) {
            const unsigned long long s0 = ks[s], s1 = ks[VH_KST_CAP + s];
            if (s1 >= s0 && ticks_per_ms > 0.0) t.total_ms += (double)(s1 - s0) / ticks_per_ms;
            t.launches += 1;
        }
        t.slots.clear();
    }
    if (!ks.empty()) kst_reset(b);
}

// the resolved totals of one kernel class of b (a null b, or a class that never ran: zeros)
static void timer_totals(vh_batch *b, const char *name, double *total_ms, int64_t *launches, double *bytes) {
    KTimer t;
    if (b) {
        resolve_timers(b);
        auto it = b->timers.find(name);
        if (it != b->timers.end()) t = it->second;
    }
    *total_ms = t.total_ms;
    *launches = t.launches;
    if (bytes) *bytes = t.bytes_per_launch;
}

// ---------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------
int vh_fail(vh_ctx *c, int code, const std::string &msg) {
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);
        c->last_error = msg;
    }
    return code;
}

// Buf's allocator (devbuf.h): the library's only device and pinned-host allocations, but for
// vh_host_alloc / vh_host_free, whose memory the caller owns
void *vh_mem_alloc(int kind, size_t bytes) {
    void *p = nullptr;
    if (kind == 0)
        HIP_TRY(hipMalloc(&p, bytes));
    else
        HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    return p;
}
void vh_mem_free(int kind, void *p) {
    if (kind == 0)
        (void)hipFree(p);
    else
        (void)hipHostFree(p);
}

static void check_dims(int64_t R, int64_t C, int64_t Z, int64_t batch) {
    if (R < 2 || C < 2 || Z < 1 || batch < 1)
        throw VhError{VH_ERR_ARG, "dims must be R>=2, C>=2, Z>=1, batch>=1"};
    if (R * C * Z >= (int64_t)1 << 31)
        throw VhError{VH_ERR_ARG, "a volume must have < 2^31 voxels"};
    if (R > 65535 || C * Z > ((int64_t)1 << 31))
        throw VhError{VH_ERR_ARG, "volume dims out of range"};
}

void vh_free_batch(vh_batch *b) {
    if (!b) return;
    b->kst_n = 0;   // no stamp reset: nothing is enqueued on the drained stream
    clear_timers(b);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    if (b->st_n4) (void)hipStreamDestroy(b->st_n4);
    if (b->ev_n4_pre) (void)hipEventDestroy(b->ev_n4_pre);
    if (b->ev_n4_post) (void)hipEventDestroy(b->ev_n4_post);
    if (b->ev_cpre) (void)hipEventDestroy(b->ev_cpre);
    if (b->ev_cpost) (void)hipEventDestroy(b->ev_cpost);
    delete b;   // the buffers (every caller has drained the batch's stream)
}

vh_batch *vh_new_batch(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t nb) {
    check_dims(R, C, Z, nb);
    HIP_TRY(hipSetDevice(ctx->device));
    vh_batch *b = new vh_batch;
    b->ctx = ctx;
    // Study-kernel stream (A/B options, off by default).  VH_PRIO=1: the batch's stream at the
    // highest priority and its study kernel on a second stream at the lowest.  VH_ST_RESERVE=k
    // (1-4): the study kernel on a second stream whose CU mask leaves k CUs per XCD to the batch's
    // other kernels (mask bits 33 j + 8 m, j < 8, m < k: one per XCD whether the bits map to XCDs
    // in blocks of 32 or interleaved), so another batch's short kernels never wait for a CU that
    // studies hold.
    const char *pe = getenv("VH_PRIO"), *re = getenv("VH_ST_RESERVE");
    const bool prio = pe && atoi(pe) != 0;
    const int reserve = re ? std::max(0, std::min(4, atoi(re))) : 0;
    int lo = 0, hi = 0;
    if (prio) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    hipError_t se = prio ? hipStreamCreateWithPriority(&b->stream, hipStreamNonBlocking, hi)
                         : hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (se == hipSuccess && reserve > 0) {
        int ncu = 0;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device);
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0xffffffffu);
        for (int j = 0; j < 8; ++j)
            for (int m = 0; m < reserve; ++m) {
                const int i = 33 * j + 8 * m;
                if (i < ncu) mask[i / 32] &= ~(1u << (i % 32));
            }
        se = hipExtStreamCreateWithCUMask(&b->st_n4, (uint32_t)mask.size(), mask.data());
    } else if (se == hipSuccess && prio) {
        se = hipStreamCreateWithPriority(&b->st_n4, hipStreamNonBlocking, lo);
    }
    if (se == hipSuccess && b->st_n4)
        se = hipEventCreateWithFlags(&b->ev_n4_pre, hipEventDisableTiming);
    if (se == hipSuccess && b->st_n4)
        se = hipEventCreateWithFlags(&b->ev_n4_post, hipEventDisableTiming);
    if (se != hipSuccess) {
        if (b->ev_n4_pre) (void)hipEventDestroy(b->ev_n4_pre);
        if (b->stream) (void)hipStreamDestroy(b->stream);
        if (b->st_n4) (void)hipStreamDestroy(b->st_n4);
        delete b;
        throw VhError{VH_ERR_HIP, "batch stream creation failed"};
    }
    b->R = R; b->C = C; b->Z = Z; b->nb = nb;
    b->V = R * C * Z;
    b->CZ = C * Z;
    b->max_tiles = (b->V + VH_SORT_TILE - 1) / VH_SORT_TILE;
    const size_t NV = (size_t)nb * b->V;
    try {
        b->d_hp.reserve(NV);
        b->d_mask.reserve(NV);
        b->d_n4.reserve(NV);
        b->d_defect.reserve(NV);
        b->d_border.reserve(NV);
        b->d_lb.reserve(NV);
        b->d_colrange.reserve((size_t)nb * b->CZ * 2);
        b->d_colcount.reserve((size_t)nb * b->CZ);
        b->d_colbits.reserve((size_t)nb * ((R + 31) / 32) * b->CZ);
        b->d_colbnz.reserve((size_t)nb * ((R + 31) / 32) * b->CZ);
        b->d_colstart.reserve((size_t)nb * b->CZ);
        b->d_rowany.reserve((size_t)nb * R);
        b->d_colany.reserve((size_t)nb * C);
        b->d_sliceany.reserve((size_t)nb * Z);
        b->d_sc.reserve((size_t)nb);
        b->part_blocks = (b->CZ + VH_TPB - 1) / VH_TPB;
        b->slab_blocks = b->part_blocks * ((R + VH_SLAB - 1) / VH_SLAB);
        b->d_snrpart.reserve((size_t)nb * b->slab_blocks * 4);
        const int64_t max_chunks = (b->V + 8191) / 8192;
        const int64_t eval_slots = ((b->CZ + 63) / 64) * ((R + 15) / 16);   // n4 eval partial slots
        b->d_part.reserve((size_t)nb * std::max<int64_t>(std::max<int64_t>(b->part_blocks * 4, max_chunks),
                                                         eval_slots * 2));
        b->d_keys0.reserve(NV);
        b->d_keys1.reserve(NV);
        b->d_tilecnt.reserve((size_t)nb * 256 * b->max_tiles);
        if (b->d_cohort.reserve((size_t)VH_COHORT_BINS))
            HIP_TRY(hipMemset(b->d_cohort, 0, sizeof(uint64_t) * VH_COHORT_BINS));
    } catch (...) {
        vh_free_batch(b);
        throw;
    }
    return b;
}

static void batch_upload(vh_batch *b, const float *hp, const uint8_t *mask) {
    hipStream_t st = b->stream;
    const size_t NV = (size_t)b->nb * b->V;
    if (hp) HIP_TRY(hipMemcpyAsync(b->d_hp, hp, sizeof(float) * NV, hipMemcpyHostToDevice, st));
    if (mask) HIP_TRY(hipMemcpyAsync(b->d_mask, mask, NV, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
}

static void check_n4_params(const vh_batch *b, const vh_n4_params &p) {
    if (p.n_levels < 1 || p.n_levels > VH_MAX_LEVELS || p.spline_order != 3 || p.n_bins < 2 ||
        p.n_bins > VH_MAX_BINS || p.ncp[0] < 4 || p.ncp[1] < 4 || p.ncp[2] < 4 || b->Z < 2 ||
        p.conv_mode < 0 || p.conv_mode > 1)
        throw VhError{VH_ERR_ARG, "unsupported N4 parameters (spline order 3, bins <= 256, ncp >= 4, "
                                  "Z >= 2, conv_mode 0 or 1)"};
    int tot = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        if (p.max_iters[l] < 1) throw VhError{VH_ERR_ARG, "max_iters must be >= 1"};
        tot += p.max_iters[l];
    }
    if (tot > 8 * 1024 - 1) throw VhError{VH_ERR_ARG, "too many N4 iterations"};
}

// n4_src: 0 = run N4 from d_hp, 1 = identity (d_hp), 2 = caller-uploaded d_n4
void vh_run_batch(vh_batch *b, const vh_run_opts &o, int n4_src) {
    HIP_TRY(hipSetDevice(b->ctx->device));
    b->profile = o.profile != 0;
    b->opts = o;
    b->n4_subbatch = o.n4_subbatch;
    b->n4_mode = o.n4_mode;
    if (o.do_n4) check_n4_params(b, o.n4);
    vh_launch_mask_stats(b);
    if (o.do_n4) vh_launch_n4(b, o.n4);
    const bool from_n4 = o.do_n4 || n4_src == 2;
    vh_launch_vdp_chain(b, from_n4 ? b->d_n4.get() : b->d_hp.get(), o);
    // (the run replaced the defect maps and the mask statistics: whatever was derived from them is gone)
    b->state.ran(from_n4 ? N4Source::n4 : N4Source::hp, o.do_kmeans != 0);
}

// the study kernel's spin-wait watchdog (n4_study.hip st_spin) leaves N4State.active = -2
static void check_n4_watchdog(const N4State *st, int64_t nb) {
    for (int64_t i = 0; i < nb; ++i)
        if (st[i].active == -2) throw VhError{VH_ERR_HIP, "N4 study kernel: a synchronisation wait timed out"};
}

// small device -> host copy ordered on the batch's own stream: a synchronous hipMemcpy goes through
// the null stream, whose hardware queue is shared with one of the pipe slots' streams once there are
// more streams than queues (GPU_MAX_HW_QUEUES), so it waited for that slot's queued work
static void d2h_on_stream(vh_batch *b, void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
}

// host copies of every study's scalars / N4 state; each waits for the batch's stream
static std::vector<VolScalars> read_scalars(vh_batch *b) {
    std::vector<VolScalars> sc(b->nb);
    d2h_on_stream(b, sc.data(), b->d_sc, sizeof(VolScalars) * b->nb);
    return sc;
}
static std::vector<N4State> read_n4_states(vh_batch *b) {
    std::vector<N4State> st(b->nb);
    d2h_on_stream(b, st.data(), b->d_st, sizeof(N4State) * b->nb);
    return st;
}

// the host-buffer calls' last check, after their outputs are written; with_snr: calculate_SNR's too
static void throw_if_empty_mask(const std::vector<VolScalars> &sc, bool with_snr = false) {
    for (const VolScalars &s : sc) {
        if (s.n_mask <= 0) throw VhError{VH_ERR_EMPTY, "empty mask"};
        if (with_snr && !s.snr_ok) throw VhError{VH_ERR_ARG, "calculate_SNR: no masked column > 0"};
    }
}

// per-study results from host copies of the scalars (and N4 states when the batch ran N4)
void vh_fill_results(const vh_batch *b, const VolScalars *sc, const N4State *st, vh_vdp_result *res) {
    if (b->opts.do_n4) check_n4_watchdog(st, b->nb);
    const double *vox = b->opts.vox;
    // np.prod(np.divide(vox, 10)): sequential multiply (Vent_Analysis.py:166, 252)
    const double pv = ((vox[0] / 10.0) * (vox[1] / 10.0)) * (vox[2] / 10.0);
    for (int64_t i = 0; i < b->nb; ++i) {
        vh_vdp_result &r = res[i];
        memset(&r, 0, sizeof r);
        const VolScalars &s = sc[i];
        const double nm = (double)s.n_mask;
        r.n_mask = s.n_mask;
        r.n_defect = s.n_defect;
        r.n_lb12 = s.n_lb12;
        r.n_km0 = s.n_km0;
        r.vdp = (100.0 * (double)s.n_defect) / nm;
        r.vdp_lb = (100.0 * (double)s.n_lb12) / nm;
        r.vdp_km = b->opts.do_kmeans ? (100.0 * (double)s.n_km0) / nm : 0.0;
        r.defect_volume = (double)s.n_defect * pv / 1000.0;
        r.lung_volume = (double)s.n_mask1 * pv / 1000.0;
        for (int j = 0; j < 4; ++j) r.km_centres[j] = s.km_c[j];
        r.snr = b->opts.do_snr ? s.snr : 0.0;
        r.mean_anchor = s.mean_anchor;
        r.p99 = s.p99;
        if (b->opts.do_n4)
            for (int l = 0; l < b->opts.n4.n_levels; ++l) {
                r.n4_iters[l] = st[i].iters_level[l];
                r.n4_conv[l] = st[i].conv_level[l];
            }
    }
}

// returns the scalars it read for res (none when res is null)
static std::vector<VolScalars> batch_download(vh_batch *b, float *n4, uint8_t *defect, uint8_t *border,
                                              uint8_t *lb, vh_vdp_result *res) {
    hipStream_t st = b->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const size_t NV = (size_t)b->nb * b->V;
    if (n4) HIP_TRY(hipMemcpy(n4, b->opts.do_n4 ? b->d_n4 : b->d_hp, sizeof(float) * NV, hipMemcpyDeviceToHost));
    if (defect) HIP_TRY(hipMemcpy(defect, b->d_defect, NV, hipMemcpyDeviceToHost));
    if (border) HIP_TRY(hipMemcpy(border, b->d_border, NV, hipMemcpyDeviceToHost));
    if (lb) HIP_TRY(hipMemcpy(lb, b->d_lb, NV, hipMemcpyDeviceToHost));
    if (!res) return {};
    const std::vector<VolScalars> sc = read_scalars(b);
    const std::vector<N4State> n4st = b->opts.do_n4 ? read_n4_states(b) : std::vector<N4State>();
    vh_fill_results(b, sc.data(), n4st.data(), res);
    return sc;
}

// The context's cached scratch batch for the host-buffer entry points (caller holds ctx->mu), with
// the context's device current for what the caller enqueues on it.
static vh_batch *scratch_batch(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t nb) {
    HIP_TRY(hipSetDevice(ctx->device));
    vh_batch *&s = ctx->scratch;
    if (s && s->R == R && s->C == C && s->Z == Z && s->nb == nb) return s;
    if (s) {
        (void)hipStreamSynchronize(s->stream);
        vh_free_batch(s);
    }
    s = nullptr;
    s = vh_new_batch(ctx, R, C, Z, nb);
    return s;
}

// the default options with N4 off: the host-buffer calls that bring their own N4 volume
static vh_run_opts chain_only_opts(float thresh, bool do_snr, bool do_kmeans, int profile) {
    vh_run_opts o;
    vh_default_run_opts(&o);
    o.do_n4 = 0;
    o.do_snr = do_snr;
    o.do_kmeans = do_kmeans;
    o.thresh = thresh;
    o.profile = profile;
    return o;
}

// Host arrays in, the chain run on the scratch batch (caller holds ctx->mu): n4 goes to d_n4, which the
// chain reads; hp is nullable.  The caller enqueues its feature and downloads.
static vh_batch *run_host_arrays(vh_ctx *ctx, const float *hp, const float *n4, const uint8_t *mask, int64_t R,
                                 int64_t C, int64_t Z, int64_t batch, const vh_run_opts &o) {
    vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
    HIP_TRY(hipMemcpyAsync(b->d_n4, n4, sizeof(float) * (size_t)batch * b->V, hipMemcpyHostToDevice, b->stream));
    batch_upload(b, hp, mask);
    vh_run_batch(b, o, 2);
    return b;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int vh_abi_version(void) { return VH_ABI_VERSION; }

const char *vh_status_string(int s) {
    switch (s) {
        case VH_OK: return "ok";
        case VH_ERR_ARG: return "invalid argument";
        case VH_ERR_HIP: return "HIP runtime error";
        case VH_ERR_NOMEM: return "out of device memory";
        case VH_ERR_MAXRADIUS: return "cluster index: maximum radius reached";
        case VH_ERR_EMPTY: return "empty mask or defect list";
        case VH_ERR_RCCL: return "RCCL error";
        case VH_ERR_NODEV: return "no GPU device";
        case VH_ERR_INDEX: return "index out of range";
        default: return "unknown status";
    }
}

int vh_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = e == hipSuccess ? c : 0;
    return VH_OK;
}

void vh_n4_default_params(vh_n4_params *p) {
    memset(p, 0, sizeof *p);
    p->n_levels = 4;
    for (int i = 0; i < 4; ++i) p->max_iters[i] = 50;
    p->conv_threshold = 0.001f;
    p->ncp[0] = p->ncp[1] = p->ncp[2] = 4;
    p->spline_order = 3;
    p->n_bins = 200;
    p->wiener_noise = 0.01f;
    p->fwhm = 0.15f;
    p->conv_mode = 0;
}

void vh_default_run_opts(vh_run_opts *o) {
    memset(o, 0, sizeof *o);
    o->do_n4 = 1;
    vh_n4_default_params(&o->n4);
    o->thresh = 0.6f;
    o->do_snr = 1;
    o->do_kmeans = 1;
    o->do_cohort = 0;
    o->profile = 0;
    o->vox[0] = o->vox[1] = o->vox[2] = 1.0;
}

int vh_create(int device, vh_ctx **out) {
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return VH_ERR_NODEV;
    if (device < 0 || device >= n) return VH_ERR_ARG;
    vh_ctx *c = new vh_ctx;
    c->device = device;
    API_TRY(c, {
        HIP_TRY(hipSetDevice(device));
        *out = c;
    })
}

int vh_destroy(vh_ctx *ctx) {
    if (!ctx) return VH_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->scratch) {
        (void)hipStreamSynchronize(ctx->scratch->stream);
        vh_free_batch(ctx->scratch);
        ctx->scratch = nullptr;
    }
    if (ctx->comm) ncclCommDestroy((ncclComm_t)ctx->comm);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->comm_st) (void)hipStreamDestroy(ctx->comm_st);
    delete ctx;   // recon_buf, h_ci_sc
    return VH_OK;
}

const char *vh_last_error(const vh_ctx *ctx) {
    static thread_local std::string copy;   // stable until this thread's next call
    if (!ctx) return "";
    std::lock_guard<std::mutex> g(ctx->err_mu);
    copy = ctx->last_error;
    return copy.c_str();
}

int vh_synchronize(vh_ctx *ctx) {
    API_TRY(ctx, {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipDeviceSynchronize());
    })
}

int vh_n4(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
          int64_t batch, const vh_n4_params *prm, float *out, int32_t *iters, float *conv) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!hp || !mask || !out || !prm) throw VhError{VH_ERR_ARG, "null buffer"};
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        check_n4_params(b, *prm);
        batch_upload(b, hp, mask);
        vh_run_opts o;
        vh_default_run_opts(&o);
        o.n4 = *prm;
        o.do_n4 = 1;
        clear_timers(b);
        b->profile = false;
        b->opts = o;
        HIP_TRY(hipSetDevice(ctx->device));
        vh_launch_mask_stats(b);
        vh_launch_n4(b, o.n4);
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipMemcpy(out, b->d_n4, sizeof(float) * batch * b->V, hipMemcpyDeviceToHost));
        const std::vector<N4State> st = read_n4_states(b);
        check_n4_watchdog(st.data(), batch);
        for (int64_t i = 0; i < batch; ++i)
            for (int l = 0; l < prm->n_levels; ++l) {
                if (iters) iters[i * prm->n_levels + l] = st[i].iters_level[l];
                if (conv) conv[i * prm->n_levels + l] = st[i].conv_level[l];
            }
        for (const VolScalars &s : read_scalars(b))
            if (s.n_mask1 < 2) throw VhError{VH_ERR_EMPTY, "N4 needs at least 2 voxels with mask == 1"};
    })
}

int vh_border(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch,
              uint8_t *border) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!a || !border) throw VhError{VH_ERR_ARG, "null buffer"};
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = false;
        const size_t NV = (size_t)batch * b->V;
        HIP_TRY(hipMemcpyAsync(b->d_defect, a, NV, hipMemcpyHostToDevice, b->stream));
        vh_launch_border(b, b->d_defect, b->d_border);
        HIP_TRY(hipMemcpyAsync(border, b->d_border, NV, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    })
}

int vh_snr(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
           int64_t batch, double *snr) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!hp || !mask || !snr) throw VhError{VH_ERR_ARG, "null buffer"};
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        batch_upload(b, hp, mask);
        b->profile = false;
        vh_launch_mask_stats(b);
        vh_launch_snr(b);
        const std::vector<VolScalars> sc = read_scalars(b);
        for (int64_t i = 0; i < batch; ++i) {
            if (!sc[i].snr_ok) throw VhError{VH_ERR_ARG, "calculate_SNR: no masked column > 0 (numpy min of an empty array)"};
            snr[i] = sc[i].snr;
        }
    })
}

int vh_vdp(vh_ctx *ctx, const float *hp, const float *n4, const uint8_t *mask, int64_t R,
           int64_t C, int64_t Z, int64_t batch, float thresh, const double vox[3],
           uint8_t *defect, uint8_t *defect_border, uint8_t *lb, vh_vdp_result *res) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!n4 || !mask || !res || !vox) throw VhError{VH_ERR_ARG, "null buffer"};
        vh_run_opts o = chain_only_opts(thresh, hp != nullptr, true, 0);
        for (int i = 0; i < 3; ++i) o.vox[i] = vox[i];
        vh_batch *b = run_host_arrays(ctx, hp, n4, mask, R, C, Z, batch, o);
        throw_if_empty_mask(batch_download(b, nullptr, defect, defect_border, lb, res), hp != nullptr);
    })
}

// page-locked host buffers handed out by vh_host_alloc, by base address: a CI map destined for one
// is written there by the scatter kernel directly (device-mapped), with no staging copy
static std::mutex g_host_mu;
static std::map<uintptr_t, std::pair<size_t, void *>> g_host;   // base -> (bytes, device pointer)

static void *host_mapped(const void *p, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_host_mu);
    const uintptr_t a = (uintptr_t)p;
    auto it = g_host.upper_bound(a);
    if (it == g_host.begin()) return nullptr;
    --it;
    if (a + bytes > it->first + it->second.first) return nullptr;
    return (char *)it->second.second + (a - it->first);
}

// CI on host buffers through a device-resident table; shared by vh_ci and vh_ci_tab
static void ci_host(vh_ctx *ctx, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
                    const vh_ci_table *t, double minvox, double *ci_array, double *ci_scalar, int32_t *shell) {
    if (!defect || !t) throw VhError{VH_ERR_ARG, "null defect map / table"};
    if (t->ctx != ctx) throw VhError{VH_ERR_ARG, "sphere table of another context"};
    vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
    b->profile = ctx->profile != 0;
    const size_t NV = (size_t)batch * b->V;
    HIP_TRY(hipMemcpyAsync(b->d_defect, defect, NV, hipMemcpyHostToDevice, b->stream));
    // the map straight into the caller's buffer when it is one of vh_host_alloc's (the scatter's
    // stores cross the link; no device map, no copy), else a device map and one D2H
    double *d_map = ci_array ? (double *)host_mapped(ci_array, sizeof(double) * NV) : nullptr;
    if (ci_array && !d_map) {
        b->d_ci_map.reserve(NV);
        d_map = b->d_ci_map;
    }
    // the scalars likewise, into the context's device-mapped page-locked array (a small D2H runs as
    // a blit kernel, r4al: 4.7 us plus its gap)
    ctx->h_ci_sc.reserve((size_t)batch);
    VolScalars *d_hsc = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void **)&d_hsc, ctx->h_ci_sc, 0));
    vh_ci_run(b, t, minvox, d_map, d_hsc);
    if (ci_array && d_map == b->d_ci_map)
        HIP_TRY(hipMemcpyAsync(ci_array, b->d_ci_map, sizeof(double) * NV, hipMemcpyDeviceToHost, b->stream));
    if (shell) HIP_TRY(hipMemcpyAsync(shell, b->d_ci_shell, sizeof(int32_t) * NV, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    vh_ci_debug_check();
    const VolScalars *sc = ctx->h_ci_sc;
    for (int64_t i = 0; i < batch; ++i) {
        if (ci_scalar) ci_scalar[i] = sc[i].ci_scalar;
        if (sc[i].ci_status == VH_ERR_MAXRADIUS)
            throw VhError{VH_ERR_MAXRADIUS, "--MAX RADIUS REACHED-- (CI.py:101-103)"};
        if (sc[i].ci_status == VH_ERR_EMPTY)
            throw VhError{VH_ERR_EMPTY, "no defect voxels (Vent_Analysis.py:270 IndexError)"};
    }
}

int vh_ci(vh_ctx *ctx, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
          const int16_t *offs, const uint8_t *dup, int64_t rows, const int32_t *bounds,
          const double *radii, int64_t nb, double minvox, double *ci_array, double *ci_scalar,
          int32_t *shell) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        std::unique_ptr<vh_ci_table, void (*)(vh_ci_table *)> t(
            vh_ci_table_build(ctx, R, C, offs, dup, rows, bounds, radii, nb), vh_ci_table_free);
        ci_host(ctx, defect, R, C, Z, batch, t.get(), minvox, ci_array, ci_scalar, shell);
    })
}

int vh_ci_table_create(vh_ctx *ctx, int64_t R, int64_t C, const int16_t *offs, const uint8_t *dup,
                       int64_t rows, const int32_t *bounds, const double *radii, int64_t nb,
                       vh_ci_table **out) {
    if (out) *out = nullptr;
    API_TRY(ctx, {
        if (!out) throw VhError{VH_ERR_ARG, "null out"};
        std::lock_guard<std::mutex> lock(ctx->mu);
        *out = vh_ci_table_build(ctx, R, C, offs, dup, rows, bounds, radii, nb);
    })
}

// Tables have two kinds of user.  ci_host (vh_ci, vh_ci_tab) runs on the context's scratch stream
// under ctx->mu and synchronises before it returns: taking the lock waits for such a call of another
// thread, and the scratch stream is drained before the hipFrees (the destroy ran with
// neither).  vh_batch_ci only enqueues, on the batch's own stream, and returns: it records, still
// under ctx->mu, an event on that stream after its last launch that reads the table (one event per
// batch, vh_ci_table::users), and the destroy waits on every such event.  So no kernel can read a
// freed table, and a table may be destroyed right after vh_batch_ci returns.
int vh_ci_table_destroy(vh_ci_table *t) {
    if (!t) return VH_OK;
    vh_ctx *ctx = t->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (ctx->scratch) (void)hipStreamSynchronize(ctx->scratch->stream);
    for (auto &kv : t->users) {
        (void)hipEventSynchronize(kv.second);
        (void)hipEventDestroy(kv.second);
    }
    t->users.clear();
    vh_ci_table_free(t);
    return VH_OK;
}

int vh_ci_tab(vh_ctx *ctx, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
              const vh_ci_table *t, double minvox, double *ci_array, double *ci_scalar, int32_t *shell) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        ci_host(ctx, defect, R, C, Z, batch, t, minvox, ci_array, ci_scalar, shell);
    })
}

int vh_batch_create(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t batch, vh_batch **out) {
    *out = nullptr;
    API_TRY(ctx, { *out = vh_new_batch(ctx, R, C, Z, batch); })
}

int vh_batch_destroy(vh_batch *b) {
    if (b) {
        (void)hipSetDevice(b->ctx->device);
        (void)hipStreamSynchronize(b->stream);
        vh_free_batch(b);
    }
    return VH_OK;
}

int vh_batch_upload(vh_batch *b, const float *hp, const uint8_t *mask) {
    BATCH_TRY(b, { batch_upload(b, hp, mask); })
}

int vh_batch_run(vh_batch *b, const vh_run_opts *opts) {
    BATCH_TRY(b, {
        if (!opts) throw VhError{VH_ERR_ARG, "null options"};
        vh_run_batch(b, *opts, opts->do_n4 ? 0 : 1);
    })
}

int vh_batch_sync(vh_batch *b) {
    BATCH_TRY(b, { HIP_TRY(hipStreamSynchronize(b->stream)); })
}

int vh_batch_download(vh_batch *b, float *n4, uint8_t *defect, uint8_t *defect_border, uint8_t *lb,
                      vh_vdp_result *res) {
    BATCH_TRY(b, {
        b->state.need_run();
        batch_download(b, n4, defect, defect_border, lb, res);
    })
}

// The CI of the resident defect maps (the last run's, or vh_batch_set_defect's): enqueue only.  The
// table's radii are copied into the batch, so vh_batch_download_ci needs the table no more.
int vh_batch_ci(vh_batch *b, const vh_ci_table *t, double minvox) {
    if (!t) return VH_ERR_ARG;
    BATCH_TRY(b, {
        if (t->ctx != b->ctx) throw VhError{VH_ERR_ARG, "sphere table of another context"};
        b->state.need_defect();
        std::lock_guard<std::mutex> lock(b->ctx->mu);   // against vh_ci_table_destroy of another thread
        hipEvent_t &ev = t->users[b];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        try {
            vh_ci_run(b, t, minvox, nullptr, nullptr, vh_ci_batch_form(b));
            b->d_ci_radii.reserve((size_t)t->nbs);
            HIP_TRY(hipMemcpyAsync(b->d_ci_radii, t->d_radii, sizeof(double) * t->nbs, hipMemcpyDeviceToDevice,
                                   b->stream));
        } catch (...) {   // whatever was launched before the failure still reads the table
            (void)hipEventRecord(ev, b->stream);
            throw;
        }
        HIP_TRY(hipEventRecord(ev, b->stream));
        b->state.ci_enqueued(t->nbs, minvox);
    })
}

int vh_batch_set_defect(vh_batch *b, const uint8_t *defect) {
    BATCH_TRY(b, {
        if (!defect) throw VhError{VH_ERR_ARG, "null defect maps"};
        HIP_TRY(hipMemcpyAsync(b->d_defect, defect, (size_t)b->nb * b->V, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->state.defect_replaced();
    })
}

// the argument checks of the selection calls (host only: nothing is enqueued before they pass)
static void check_select_args(int source, int medfilt) {
    if (source < VH_DEFECT_MEAN || source > VH_DEFECT_KM)
        throw VhError{VH_ERR_ARG, "source must be VH_DEFECT_MEAN, _LB or _KM"};
    if (medfilt < 0 || medfilt > 2) throw VhError{VH_ERR_ARG, "medfilt must be 0, 1 or 2"};
}
static void check_select(const vh_batch *b, int source, int medfilt) {
    check_select_args(source, medfilt);
    b->state.need_run();
    if (source == VH_DEFECT_KM) b->state.need_kmeans();
}

static void batch_select(vh_batch *b, int source, int medfilt) {
    // the label map rides along once a caller has asked for it (d_km exists) and the run has cuts
    uint8_t *km = b->opts.do_kmeans ? b->d_km : nullptr;
    if (!vh_launch_defect_select(b, b->n4_last(), b->opts.thresh, source, medfilt, km))
        throw VhError{VH_ERR_ARG, "vh_batch_select_defect: this shape has no plane-sweep geometry"};
    b->state.selected(km != nullptr);
}

// returns the scalars it read for count
static std::vector<VolScalars> batch_download_defect(vh_batch *b, uint8_t *defect, uint8_t *border, uint8_t *km,
                                                     int64_t *count) {
    const size_t NV = (size_t)b->nb * b->V;
    hipStream_t st = b->stream;
    if (km && !b->state.labels_valid()) {
        b->d_km.reserve(NV);
        vh_launch_km_labels(b, b->n4_last(), b->d_km);
        b->state.labels_built();
    }
    if (defect) HIP_TRY(hipMemcpyAsync(defect, b->d_defect, NV, hipMemcpyDeviceToHost, st));
    if (border) HIP_TRY(hipMemcpyAsync(border, b->d_border, NV, hipMemcpyDeviceToHost, st));
    if (km) HIP_TRY(hipMemcpyAsync(km, b->d_km, NV, hipMemcpyDeviceToHost, st));
    std::vector<VolScalars> sc = read_scalars(b);   // synchronises the stream
    if (count)
        for (int64_t i = 0; i < b->nb; ++i) count[i] = b->state.selection_on() ? sc[i].n_sel : sc[i].n_defect;
    return sc;
}

int vh_batch_select_defect(vh_batch *b, int source, int medfilt) {
    BATCH_TRY(b, {
        check_select(b, source, medfilt);
        batch_select(b, source, medfilt);
    })
}

int vh_batch_download_defect(vh_batch *b, uint8_t *defect, uint8_t *border, uint8_t *km, int64_t *count) {
    BATCH_TRY(b, {
        b->state.need_run();
        if (km) b->state.need_kmeans();
        batch_download_defect(b, defect, border, km, count);
    })
}

int vh_batch_km_cuts(vh_batch *b, float *cuts) {
    BATCH_TRY(b, {
        if (!cuts) throw VhError{VH_ERR_ARG, "null cuts"};
        b->state.need_kmeans();
        const std::vector<VolScalars> sc = read_scalars(b);
        for (int64_t i = 0; i < b->nb; ++i)
            for (int j = 0; j < 3; ++j) {
                // (an empty study has no cuts: km_valid is 0 from the run's initialisation)
                const uint32_t k = sc[i].km_cut[j];
                const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;   // key2f on the host
                float f = std::numeric_limits<float>::infinity();
                if (sc[i].n_mask > 0 && ((sc[i].km_valid >> j) & 1)) memcpy(&f, &u, sizeof f);
                cuts[i * 3 + j] = f;
            }
    })
}

int vh_defect_map(vh_ctx *ctx, const float *n4, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                  int64_t batch, float thresh, int source, int medfilt, uint8_t *defect, uint8_t *border,
                  uint8_t *km, int64_t *count) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!n4 || !mask) throw VhError{VH_ERR_ARG, "null buffer"};
        check_select_args(source, medfilt);
        const vh_run_opts o = chain_only_opts(thresh, false, source == VH_DEFECT_KM || km != nullptr, ctx->profile);
        vh_batch *b = run_host_arrays(ctx, nullptr, n4, mask, R, C, Z, batch, o);
        batch_select(b, source, medfilt);
        throw_if_empty_mask(batch_download_defect(b, defect, border, km, count));
    })
}

int vh_batch_download_ci(vh_batch *b, double *ci_array, int16_t *shell, double *ci_scalar, int32_t *status) {
    BATCH_TRY(b, {
        b->state.need_ci();
        const size_t NV = (size_t)b->nb * b->V;
        if (ci_array) {
            b->d_ci_map.reserve(NV);
            vh_ci_expand(b, b->d_ci_map);
            HIP_TRY(hipMemcpyAsync(ci_array, b->d_ci_map, sizeof(double) * NV, hipMemcpyDeviceToHost, b->stream));
        }
        if (shell)
            HIP_TRY(hipMemcpyAsync(shell, b->d_ci_shell16, sizeof(int16_t) * NV, hipMemcpyDeviceToHost, b->stream));
        const std::vector<VolScalars> sc = read_scalars(b);   // synchronises the stream
        vh_ci_debug_check();
        for (int64_t i = 0; i < b->nb; ++i) {
            if (ci_scalar) ci_scalar[i] = sc[i].ci_scalar;
            if (status) status[i] = sc[i].ci_status;
        }
    })
}

int vh_batch_cohort_hist(vh_batch *b, uint64_t *hist) {
    BATCH_TRY(b, {
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipMemcpy(hist, b->d_cohort, sizeof(uint64_t) * VH_COHORT_BINS, hipMemcpyDeviceToHost));
    })
}

const char *vh_batch_kernel_names(void) {
    return "mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
           "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;ci_walk_b;defect_sel";
}

int vh_batch_reset_timers(vh_batch *b) {
    BATCH_TRY(b, {
        HIP_TRY(hipStreamSynchronize(b->stream));
        clear_timers(b);
    })
}

int vh_batch_kernel_time(vh_batch *b, const char *name, double *total_ms, int64_t *launches,
                         double *bytes_per_launch) {
    BATCH_TRY(b, { timer_totals(b, name, total_ms, launches, bytes_per_launch); })
}

int vh_ctx_profile(vh_ctx *ctx, int on) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        ctx->profile = on ? 1 : 0;
        if (ctx->scratch) {
            HIP_TRY(hipStreamSynchronize(ctx->scratch->stream));
            clear_timers(ctx->scratch);
        }
    })
}

int vh_ctx_kernel_time(vh_ctx *ctx, const char *name, double *total_ms, int64_t *launches) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!name || !total_ms || !launches) throw VhError{VH_ERR_ARG, "null argument"};
        timer_totals(ctx->scratch, name, total_ms, launches, nullptr);
    })
}

int vh_batch_study_times(vh_batch *b, double *us) {
    BATCH_TRY(b, {
        if (!us) throw VhError{VH_ERR_ARG, "null buffer"};
        HIP_TRY(hipStreamSynchronize(b->stream));
        for (int64_t i = 0; i < b->nb; ++i) us[i] = 0.0;
        if (!b->state.has_run() || !b->opts.do_n4 || !b->n4_used_study) return VH_OK;
        const std::vector<N4State> st = read_n4_states(b);
        int rate_khz = 0;
        HIP_TRY(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, b->ctx->device));
        if (rate_khz <= 0) throw VhError{VH_ERR_HIP, "no device wall clock rate"};
        for (int64_t i = 0; i < b->nb; ++i)
            us[i] = (double)(st[i].t_end - st[i].t_start) * 1000.0 / (double)rate_khz;
        if (const char *path = getenv("VH_STUDY_TRACE")) {   // per study: start, end, placement
            if (FILE *f = fopen(path, "a")) {
                for (int64_t i = 0; i < b->nb; ++i)
                    fprintf(f, "%p,%lld,%llu,%llu,%u,%u,%d,%d,%d,%d\n", (void *)b, (long long)i,
                            (unsigned long long)st[i].t_start, (unsigned long long)st[i].t_end,
                            st[i].hw_id, st[i].xcc_id, rate_khz, st[i].pc_rounds,
                            st[i].pc_fallbacks, st[i].iters_level[0] + st[i].iters_level[1] +
                                st[i].iters_level[2] + st[i].iters_level[3]);
                fclose(f);
            }
        }
    })
}

// ---- rendering (export.hip) ------------------------------------------------------------------
int vh_overlay(vh_ctx *ctx, const float *n4, const uint8_t *defect, int64_t R, int64_t C, int64_t Z,
               int64_t batch, uint8_t *rgb) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!n4 || !defect || !rgb) throw VhError{VH_ERR_ARG, "overlay: null buffer"};
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        const size_t NV = (size_t)batch * R * C * Z;
        HIP_TRY(hipMemcpyAsync(b->d_n4, n4, sizeof(float) * NV, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->d_defect, defect, NV, hipMemcpyHostToDevice, b->stream));
        // rgb (3 B/voxel) in the sort-key buffer (4 B/voxel), the |x| min/max in the partials
        uint8_t *d_rgb = reinterpret_cast<uint8_t *>(b->d_keys0.get());
        uint32_t *d_mm = reinterpret_cast<uint32_t *>(b->d_part.get());
        vh_overlay_launch(b->stream, b->d_n4, b->d_defect, R, C, Z, batch, d_mm, d_rgb);
        HIP_TRY(hipMemcpyAsync(rgb, d_rgb, 3 * NV, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    })
}

int vh_montage(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, const void *proton, int proton_is64,
               const void *hp, int hp_is64, const float *n4, const uint8_t *mask_border,
               const uint8_t *defect, const double *ci, const double *parula, int64_t prow,
               const int64_t crop[6], uint8_t *image) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!proton || !hp || !n4 || !mask_border || !defect || !parula || !crop || !image)
            throw VhError{VH_ERR_ARG, "montage: null buffer"};
        check_dims(R, C, Z, 1);
        vh_batch *b = scratch_batch(ctx, R, C, Z, 1);
        vh_montage_run(b->stream, R, C, Z, proton, proton_is64, hp, hp_is64, n4, mask_border, defect,
                       ci, parula, prow, crop, image);
    })
}

// ---- the renderings of a device-resident batch --------------------------------------------------
// exportDICOM's frames of every study from the resident N4 (the volume the last run's chain read)
// and defect maps: vh_overlay's kernels on the batch's own buffers.  The frames go to a buffer of
// their own, allocated on first demand like d_km: a rendering writes nothing
// another call on the batch reads.
int vh_batch_overlay(vh_batch *b) {
    BATCH_TRY(b, {
        b->state.need_run();
        if (b->nb > 65535 || b->R > 65535) throw VhError{VH_ERR_ARG, "overlay: batch or rows out of range"};
        const size_t NV = (size_t)b->nb * b->V;
        b->d_ov_rgb.reserve(3 * NV);
        b->d_ov_mm.reserve(2 * (size_t)b->nb);
        // N4 twice (min/max, then the frames), the defect map, 3 bytes out
        ScopedKTimer tm(b, "overlay_b", 12.0 * (double)NV);
        vh_overlay_launch(b->stream, b->n4_last(), b->d_defect, b->R, b->C, b->Z, b->nb, b->d_ov_mm, b->d_ov_rgb);
        b->state.overlay_enqueued();
    })
}

int vh_batch_download_overlay(vh_batch *b, uint8_t *rgb) {
    BATCH_TRY(b, {
        if (!rgb) throw VhError{VH_ERR_ARG, "null buffer"};
        b->state.need_overlay();
        d2h_on_stream(b, rgb, b->d_ov_rgb, 3 * (size_t)b->nb * b->V);
    })
}

// cropToData of every resident mask and the compact buffer's layout; cached until the next run.
// One small kernel, a copy of nb x 32 bytes back, the prefix on the host, nb + 1 records up.
static void batch_montage_layout(vh_batch *b) {
    b->state.need_run();
    if (b->state.layout_is_cached()) return;
    const int64_t nb = b->nb;
    b->d_mt_crop.reserve((size_t)nb * 8);
    b->d_mt_st.reserve((size_t)nb + 1);
    vh_crop_layout_launch(b);
    std::vector<int32_t> h((size_t)nb * 8);
    d2h_on_stream(b, h.data(), b->d_mt_crop, sizeof(int32_t) * h.size());
    b->mt_st.assign((size_t)nb + 1, MtStudy{});
    b->mt_status.assign((size_t)nb, VH_OK);
    int64_t off = 0, wg = 0;
    for (int64_t i = 0; i < nb; ++i) {
        MtStudy &s = b->mt_st[i];
        const int32_t *c = &h[(size_t)i * 8];
        s.r0 = c[0]; s.nr = c[1]; s.c0 = c[2]; s.nc = c[3]; s.s0 = c[4]; s.ns = c[5];
        b->mt_status[i] = c[6];
        s.ncc = (s.nc + VH_MT_COLS - 1) / VH_MT_COLS;
        s.nzc = (s.ns + VH_MT_ZC - 1) / VH_MT_ZC;
        s.off = off;
        s.wg0 = wg;
        const int64_t bytes = (int64_t)21 * s.nr * s.nc * s.ns;
        off += (bytes + VH_MT_ALIGN - 1) / VH_MT_ALIGN * VH_MT_ALIGN;
        wg += (int64_t)s.nr * s.ncc * s.nzc;
    }
    if (wg > 0x7fffffff) throw VhError{VH_ERR_ARG, "montage: too many crop rows for one launch"};
    b->mt_st[nb].off = off;
    b->mt_st[nb].wg0 = wg;
    HIP_TRY(hipMemcpyAsync(b->d_mt_st, b->mt_st.data(), sizeof(MtStudy) * (nb + 1), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->state.layout_cached();
}

int vh_batch_montage_layout(vh_batch *b, int64_t *crop, int64_t *offset, int32_t *status) {
    BATCH_TRY(b, {
        batch_montage_layout(b);
        for (int64_t i = 0; i < b->nb; ++i) {
            const MtStudy &s = b->mt_st[i];
            const int64_t c[6] = {s.r0, s.nr, s.c0, s.nc, s.s0, s.ns};
            if (crop) memcpy(crop + 6 * i, c, sizeof c);
            if (offset) offset[i] = s.off;
            if (status) status[i] = b->mt_status[i];
        }
        if (offset) offset[b->nb] = b->mt_st[b->nb].off;
    })
}

// screenShot's montage of every study, rendered from the resident buffers (export.hip k_montage_b).
// Enqueue only once the layout is cached (vh_batch_montage_layout; otherwise it is computed here,
// which waits for the stream once).  The CI panel is drawn when vh_batch_ci was enqueued after the
// last change of the resident defect maps.
int vh_batch_montage(vh_batch *b, const float *proton, const double *parula, int64_t prow) {
    BATCH_TRY(b, {
        b->state.need_run();
        if (!parula || prow < 1) throw VhError{VH_ERR_ARG, "montage: empty colour table"};
        batch_montage_layout(b);
        const size_t NV = (size_t)b->nb * b->V;
        const int64_t total = b->mt_st[b->nb].off;
        b->d_mt_keys.reserve(6 * (size_t)b->nb);
        b->d_mt_flag.reserve((size_t)b->nb);
        b->d_mt_parula.reserve(3 * (size_t)prow);
        if ((size_t)total > b->d_mt_img.size()) {
            HIP_TRY(hipStreamSynchronize(b->stream));   // an earlier montage may still be writing
            b->d_mt_img.reserve((size_t)total);
        }
        if (proton) b->d_proton.reserve(NV);
        HIP_TRY(hipMemcpyAsync(b->d_mt_parula, parula, sizeof(double) * 3 * prow, hipMemcpyHostToDevice, b->stream));
        if (proton) HIP_TRY(hipMemcpyAsync(b->d_proton, proton, sizeof(float) * NV, hipMemcpyHostToDevice, b->stream));
        if (proton) b->state.proton_uploaded();   // (the one buffer: it is the resident proton from here on)
        vh_montage_b_launch(b, proton != nullptr, prow, b->state.ci_is_fresh());
        b->state.montage_enqueued();
    })
}

int vh_batch_download_montage(vh_batch *b, uint8_t *image, int32_t *status) {
    BATCH_TRY(b, {
        b->state.need_montage();
        const int64_t total = b->mt_st[b->nb].off;
        if (total > 0 && !image) throw VhError{VH_ERR_ARG, "null buffer"};
        if (total > 0) HIP_TRY(hipMemcpyAsync(image, b->d_mt_img, (size_t)total, hipMemcpyDeviceToHost, b->stream));
        std::vector<int32_t> flag((size_t)b->nb);
        d2h_on_stream(b, flag.data(), b->d_mt_flag, sizeof(int32_t) * flag.size());   // synchronises the stream
        if (status)
            for (int64_t i = 0; i < b->nb; ++i)
                status[i] = b->mt_status[i] != VH_OK ? b->mt_status[i] : flag[i] ? VH_ERR_INDEX : VH_OK;
    })
}

// ---- the ventilation distribution of a device-resident batch (dist.hip) -------------------------
// the argument checks (host only: nothing is enqueued before they pass)
static void check_distribution(const vh_batch *b, int norm, int32_t n_bins, float hi) {
    if (norm != VH_NORM_MEAN && norm != VH_NORM_P99)
        throw VhError{VH_ERR_ARG, "norm must be VH_NORM_MEAN or VH_NORM_P99"};
    if (n_bins < 1 || n_bins > VH_COHORT_BINS) throw VhError{VH_ERR_ARG, "n_bins must be 1..1024"};
    if (!std::isfinite(hi) || !(hi > 0.0f)) throw VhError{VH_ERR_ARG, "hi must be finite and > 0"};
    if (b) b->state.need_run();
    if (b && !vh_dist_takes(b)) throw VhError{VH_ERR_ARG, "distribution: more than 1900 slices"};
}

// Enqueue the sweep over what the last run left resident: the N4 volume its chain read, the mask,
// the LB classes and the defect map as it stands.  It writes its own three buffers only, so nothing
// another call on the batch reads changes (the CI stays fresh).
static void batch_distribution(vh_batch *b, int norm, int32_t n_bins, float hi) {
    b->d_dist_hist.reserve((size_t)b->nb * VH_COHORT_BINS);   // the largest n_bins: no regrowth
    b->d_dist_out.reserve((size_t)b->nb * 2);
    b->d_dist_sl.reserve((size_t)b->nb * b->Z * VH_DIST_COLS);
    const float scale = (float)n_bins / hi;   // once, in float32: the kernel multiplies by it
    vh_dist_launch(b, norm, n_bins, hi, scale);
    b->state.distribution_enqueued(n_bins);
}

static void batch_download_distribution(vh_batch *b, uint32_t *hist, int64_t *outside, int64_t *slice_counts) {
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (hist)
        HIP_TRY(hipMemcpyAsync(hist, b->d_dist_hist, sizeof(uint32_t) * nb * b->state.dist_bins(), hipMemcpyDeviceToHost, st));
    if (outside)
        HIP_TRY(hipMemcpyAsync(outside, b->d_dist_out, sizeof(int64_t) * nb * 2, hipMemcpyDeviceToHost, st));
    if (slice_counts)
        HIP_TRY(hipMemcpyAsync(slice_counts, b->d_dist_sl, sizeof(int64_t) * nb * b->Z * VH_DIST_COLS,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_distribution(vh_batch *b, int norm, int32_t n_bins, float hi) {
    BATCH_TRY(b, {
        check_distribution(b, norm, n_bins, hi);
        batch_distribution(b, norm, n_bins, hi);
    })
}

int vh_batch_download_distribution(vh_batch *b, uint32_t *hist, int64_t *outside, int64_t *slice_counts) {
    BATCH_TRY(b, {
        b->state.need_distribution();
        batch_download_distribution(b, hist, outside, slice_counts);
    })
}

int vh_distribution(vh_ctx *ctx, const float *n4, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                    int64_t batch, float thresh, int norm, int32_t n_bins, float hi, uint32_t *hist,
                    int64_t *outside, int64_t *slice_counts) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!n4 || !mask) throw VhError{VH_ERR_ARG, "null buffer"};
        check_distribution(nullptr, norm, n_bins, hi);
        check_dims(R, C, Z, batch);   // (before the slice count, as the scratch batch checks them)
        if (Z > VH_DIST_MAX_Z) throw VhError{VH_ERR_ARG, "distribution: more than 1900 slices"};
        const vh_run_opts o = chain_only_opts(thresh, false, false, ctx->profile);
        vh_batch *b = run_host_arrays(ctx, nullptr, n4, mask, R, C, Z, batch, o);
        batch_distribution(b, norm, n_bins, hi);
        batch_download_distribution(b, hist, outside, slice_counts);
        throw_if_empty_mask(read_scalars(b));
    })
}

// ---- the local ventilation heterogeneity of a device-resident batch (heterogeneity.hip) -----------
// the argument checks (host only: nothing is enqueued before they pass)
static void check_heterogeneity(int radius, int32_t min_count, int32_t n_bins, float hi) {
    if (radius < 1 || radius > 5) throw VhError{VH_ERR_ARG, "radius must be 1..5"};
    const int32_t win = (2 * radius + 1) * (2 * radius + 1);
    if (min_count < 2 || min_count > win) throw VhError{VH_ERR_ARG, "min_count must be 2..(2 radius + 1)^2"};
    if (n_bins < 1 || n_bins > VH_COHORT_BINS) throw VhError{VH_ERR_ARG, "n_bins must be 1..1024"};
    if (!std::isfinite(hi) || !(hi > 0.0f) || !(hi <= 16.0f))
        throw VhError{VH_ERR_ARG, "hi must be finite, > 0 and <= 16"};
}

// Enqueue the sweep over src (a volume of the batch) and the resident mask, without the voxels of
// defect (nullable).  It writes its own three buffers only, so nothing another call on the batch reads
// changes (the CI stays fresh).
static void batch_heterogeneity(vh_batch *b, const float *src, const uint8_t *defect, int radius, int32_t min_count,
                                int32_t n_bins, float hi) {
    if (!vh_het_takes(b)) throw VhError{VH_ERR_ARG, "heterogeneity: batch or tile count out of range"};
    b->d_het.reserve((size_t)b->nb * b->V);
    b->d_het_hist.reserve((size_t)b->nb * VH_COHORT_BINS);   // the largest n_bins: no regrowth
    b->d_het_stats.reserve((size_t)b->nb * 4);
    const float scale = (float)n_bins / hi;   // once, in float32: the kernel multiplies by it
    vh_het_launch(b, src, defect, b->d_het, b->d_het_hist, b->d_het_stats, radius, min_count, n_bins, hi, scale);
    b->state.heterogeneity_enqueued(n_bins);
}

static void batch_download_heterogeneity(vh_batch *b, float *map, uint32_t *hist, int64_t *stats) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (map) HIP_TRY(hipMemcpyAsync(map, b->d_het, sizeof(float) * nb * b->V, hipMemcpyDeviceToHost, st));
    if (hist)
        HIP_TRY(hipMemcpyAsync(hist, b->d_het_hist, sizeof(uint32_t) * nb * b->state.het_bins(), hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, b->d_het_stats, sizeof(int64_t) * nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_heterogeneity(vh_batch *b, int radius, int32_t min_count, int32_t n_bins, float hi, int exclude_defect) {
    BATCH_TRY(b, {
        check_heterogeneity(radius, min_count, n_bins, hi);
        if (exclude_defect != 0 && exclude_defect != 1) throw VhError{VH_ERR_ARG, "exclude_defect must be 0 or 1"};
        b->state.need_run();
        batch_heterogeneity(b, b->n4_last(), exclude_defect ? b->d_defect.get() : nullptr, radius, min_count, n_bins, hi);
    })
}

int vh_batch_download_heterogeneity(vh_batch *b, float *map, uint32_t *hist, int64_t *stats) {
    BATCH_TRY(b, {
        b->state.need_heterogeneity();
        batch_download_heterogeneity(b, map, hist, stats);
    })
}

int vh_heterogeneity(vh_ctx *ctx, const float *x, const uint8_t *mask, int64_t R, int64_t C, int64_t Z, int64_t batch,
                     int radius, int32_t min_count, int32_t n_bins, float hi, float *map, uint32_t *hist,
                     int64_t *stats) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!x || !mask) throw VhError{VH_ERR_ARG, "null buffer"};
        check_heterogeneity(radius, min_count, n_bins, hi);
        check_dims(R, C, Z, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, x, mask);
        b->state.forgot_run();   // (the scratch batch's volumes are no run's)
        batch_heterogeneity(b, b->d_hp, nullptr, radius, min_count, n_bins, hi);
        batch_download_heterogeneity(b, map, hist, stats);
    })
}

// ---- the core-rind analysis of a device-resident batch (depth.hip) ---------------------------------
// the argument checks (host only: nothing is enqueued before they pass)
static void check_core_rind(const uint16_t *thr, int32_t n_thr) {
    if (n_thr < 0 || n_thr > 31) throw VhError{VH_ERR_ARG, "n_thr must be 0..31"};
    if (n_thr > 0 && !thr) throw VhError{VH_ERR_ARG, "null thresholds"};
    for (int32_t i = 0; i < n_thr; ++i)
        if (thr[i] == 0 || (i > 0 && thr[i] <= thr[i - 1]))
            throw VhError{VH_ERR_ARG, "thresholds must be strictly increasing and >= 1"};
}

// Enqueue the sweep over the resident mask, with the defect column from defect (nullable).  It writes
// its own buffers only, so nothing another call on the batch reads changes (the CI stays fresh).
static void batch_core_rind(vh_batch *b, const uint8_t *defect, const uint16_t *thr, int32_t n_thr) {
    if (!vh_depth_takes(b)) throw VhError{VH_ERR_ARG, "core_rind: more than 65535 studies"};
    b->d_cr_map.reserve((size_t)b->nb * b->V);
    b->d_cr_g.reserve((size_t)b->nb * b->V);
    b->d_cr_counts.reserve((size_t)b->nb * 64);   // the largest n_thr: no regrowth
    b->d_cr_stats.reserve((size_t)b->nb * 2);
    vh_depth_launch(b, defect, thr, n_thr, b->d_cr_g, b->d_cr_map, b->d_cr_counts, b->d_cr_stats);
    b->state.core_rind_enqueued(n_thr + 1);
}

static void batch_download_core_rind(vh_batch *b, uint16_t *map, int64_t *counts, int64_t *stats) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (map) HIP_TRY(hipMemcpyAsync(map, b->d_cr_map, sizeof(uint16_t) * nb * b->V, hipMemcpyDeviceToHost, st));
    if (counts)
        HIP_TRY(hipMemcpyAsync(counts, b->d_cr_counts, sizeof(int64_t) * nb * 2 * b->state.cr_bands(),
                               hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, b->d_cr_stats, sizeof(int64_t) * nb * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_core_rind(vh_batch *b, const uint16_t *thr, int32_t n_thr, int with_defect) {
    BATCH_TRY(b, {
        check_core_rind(thr, n_thr);
        if (with_defect != 0 && with_defect != 1) throw VhError{VH_ERR_ARG, "with_defect must be 0 or 1"};
        if (with_defect) b->state.need_defect();
        batch_core_rind(b, with_defect ? b->d_defect.get() : nullptr, thr, n_thr);
    })
}

int vh_batch_download_core_rind(vh_batch *b, uint16_t *map, int64_t *counts, int64_t *stats) {
    BATCH_TRY(b, {
        b->state.need_core_rind();
        batch_download_core_rind(b, map, counts, stats);
    })
}

int vh_core_rind_form(int64_t R, int64_t C, int64_t Z) {
    if (R < 1 || C < 1 || Z < 1) return -1;
    return vh_depth_form(R, C, Z);
}

int vh_core_rind(vh_ctx *ctx, const uint8_t *mask, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
                 const uint16_t *thr, int32_t n_thr, uint16_t *map, int64_t *counts, int64_t *stats) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!mask) throw VhError{VH_ERR_ARG, "null buffer"};
        check_core_rind(thr, n_thr);
        check_dims(R, C, Z, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, nullptr, mask);
        if (defect)   // (pageable source, and batch_download_core_rind waits before the call returns)
            HIP_TRY(hipMemcpyAsync(b->d_defect, defect, (size_t)batch * b->V, hipMemcpyHostToDevice, b->stream));
        b->state.forgot_run();   // (the scratch batch's volumes are no run's)
        batch_core_rind(b, defect ? b->d_defect.get() : nullptr, thr, n_thr);
        batch_download_core_rind(b, map, counts, stats);
    })
}

// ---- the connected components of a device-resident batch (components.hip) --------------------------
// the argument checks (host only: nothing is enqueued before they pass)
static void check_cc(int source, int conn) {
    if (source != VH_CC_DEFECT && source != VH_CC_MASK) throw VhError{VH_ERR_ARG, "source must be VH_CC_DEFECT or VH_CC_MASK"};
    if (conn != 4 && conn != 8 && conn != 6 && conn != 26) throw VhError{VH_ERR_ARG, "conn must be 4, 8, 6 or 26"};
}

static void check_cc_edges(const uint32_t *edges, int32_t n_edges) {
    if (n_edges < 0 || n_edges > 31) throw VhError{VH_ERR_ARG, "n_edges must be 0..31"};
    if (n_edges > 0 && !edges) throw VhError{VH_ERR_ARG, "null edges"};
    for (int32_t i = 0; i < n_edges; ++i)
        if (edges[i] < 2 || (i > 0 && edges[i] <= edges[i - 1]))
            throw VhError{VH_ERR_ARG, "edges must be strictly increasing and >= 2"};
}

static void check_cc_filter(const uint32_t *min_size, const int32_t *keep_largest, int64_t nb) {
    if (!min_size) throw VhError{VH_ERR_ARG, "null min_size"};
    for (int64_t i = 0; i < nb; ++i) {
        if (min_size[i] < 1) throw VhError{VH_ERR_ARG, "every min_size must be >= 1 (study " + std::to_string(i) + ")"};
        if (keep_largest && (keep_largest[i] < 0 || keep_largest[i] > 8))
            throw VhError{VH_ERR_ARG, "every keep_largest must be 0..8 (study " + std::to_string(i) + ")"};
    }
}

// the state's check of the source and the volume it names
static uint8_t *cc_source(vh_batch *b, int source) {
    if (source == VH_CC_DEFECT) b->state.need_defect();
    if (!vh_cc_takes(b)) throw VhError{VH_ERR_ARG, "components: more than 65535 studies or a volume of 2^31 voxels"};
    return source == VH_CC_DEFECT ? b->d_defect.get() : b->d_mask.get();
}

// Enqueue the labelling of src.  It writes its own buffers only, so nothing another call on the batch
// reads changes (the CI stays fresh).
static void batch_cc_label(vh_batch *b, const uint8_t *src, int conn, const uint32_t *edges, int32_t n_edges) {
    b->d_cc_root.reserve((size_t)b->nb * b->V);
    b->d_cc_size.reserve((size_t)b->nb * b->V);
    b->d_cc_counts.reserve((size_t)b->nb * 64);   // the largest n_edges: no regrowth
    b->d_cc_stats.reserve((size_t)b->nb * 4);
    vh_cc_launch(b, src, conn, edges, n_edges, b->d_cc_root, b->d_cc_size, b->d_cc_counts, b->d_cc_stats);
}

static void batch_components(vh_batch *b, int source, int conn, const uint32_t *edges, int32_t n_edges) {
    batch_cc_label(b, cc_source(b, source), conn, edges, n_edges);
    b->state.components_enqueued(n_edges + 1);
}

// stats leaves the device as n_set, n_comp, the largest key, 0: the key becomes the size and the root here
static void batch_download_components(vh_batch *b, int32_t *root, uint32_t *size, int64_t *counts, int64_t *stats) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (root) HIP_TRY(hipMemcpyAsync(root, b->d_cc_root, sizeof(int32_t) * nb * b->V, hipMemcpyDeviceToHost, st));
    if (size) HIP_TRY(hipMemcpyAsync(size, b->d_cc_size, sizeof(uint32_t) * nb * b->V, hipMemcpyDeviceToHost, st));
    if (counts)
        HIP_TRY(hipMemcpyAsync(counts, b->d_cc_counts, sizeof(int64_t) * nb * 2 * b->state.cc_classes(),
                               hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, b->d_cc_stats, sizeof(int64_t) * nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stats)
        for (size_t q = 0; q < nb; ++q) {
            const uint64_t key = (uint64_t)stats[4 * q + 2];
            stats[4 * q + 2] = (int64_t)(key >> 32);
            stats[4 * q + 3] = key ? (int64_t)(int32_t)~(uint32_t)(key & 0xffffffffu) : -1;
        }
}

// Enqueue the filter: the labelling of the source as it stands, the picks, the pass that clears; then
// what a change of that source entails.  kept (nullable) waits.
static void batch_filter_components(vh_batch *b, int source, int conn, const uint32_t *min_size,
                                    const int32_t *keep_largest, int64_t *kept) {
    uint8_t *src = cc_source(b, source);
    const size_t nb = (size_t)b->nb;
    const std::vector<int32_t> none(keep_largest ? 0 : nb, 0);
    const int32_t *keep = keep_largest ? keep_largest : none.data();
    const int kmax = *std::max_element(keep, keep + nb);
    b->d_cc_min.reserve(nb);
    b->d_cc_keep.reserve(nb);
    b->d_cc_picks.reserve(nb * 8);
    b->d_cc_kept.reserve(nb * 2);
    b->state.components_filtered();   // (the buffers are relabelled, whatever follows)
    // (pageable sources: the copies have left min_size and keep when the calls return)
    HIP_TRY(hipMemcpyAsync(b->d_cc_min, min_size, sizeof(uint32_t) * nb, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->d_cc_keep, keep, sizeof(int32_t) * nb, hipMemcpyHostToDevice, b->stream));
    batch_cc_label(b, src, conn, nullptr, 0);
    if (source == VH_CC_DEFECT)
        b->state.defect_replaced();
    else
        b->state.forgot_run();
    vh_cc_filter_launch(b, src, b->d_cc_root, b->d_cc_size, b->d_cc_min, b->d_cc_keep, kmax, b->d_cc_picks, b->d_cc_kept);
    if (source == VH_CC_DEFECT) vh_launch_border(b, b->d_defect, b->d_border);
    if (kept) d2h_on_stream(b, kept, b->d_cc_kept, sizeof(int64_t) * nb * 2);
}

int vh_batch_components(vh_batch *b, int source, int conn, const uint32_t *edges, int32_t n_edges) {
    BATCH_TRY(b, {
        check_cc(source, conn);
        check_cc_edges(edges, n_edges);
        batch_components(b, source, conn, edges, n_edges);
    })
}

int vh_batch_download_components(vh_batch *b, int32_t *root, uint32_t *size, int64_t *counts, int64_t *stats) {
    BATCH_TRY(b, {
        b->state.need_components();
        batch_download_components(b, root, size, counts, stats);
    })
}

int vh_batch_filter_components(vh_batch *b, int source, int conn, const uint32_t *min_size,
                               const int32_t *keep_largest, int64_t *kept) {
    BATCH_TRY(b, {
        check_cc(source, conn);
        check_cc_filter(min_size, keep_largest, b->nb);
        batch_filter_components(b, source, conn, min_size, keep_largest, kept);
    })
}

int vh_components(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch, int conn,
                  const uint32_t *edges, int32_t n_edges, int32_t *root, uint32_t *size, int64_t *counts,
                  int64_t *stats) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!a) throw VhError{VH_ERR_ARG, "null buffer"};
        check_cc(VH_CC_MASK, conn);
        check_cc_edges(edges, n_edges);
        check_dims(R, C, Z, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, nullptr, a);   // (the volume rides in the scratch batch's mask)
        b->state.forgot_run();         // (the scratch batch's volumes are no run's)
        batch_components(b, VH_CC_MASK, conn, edges, n_edges);
        batch_download_components(b, root, size, counts, stats);
    })
}

int vh_filter_components(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch, int conn,
                         const uint32_t *min_size, const int32_t *keep_largest, uint8_t *out, int64_t *kept) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!a) throw VhError{VH_ERR_ARG, "null buffer"};
        check_cc(VH_CC_MASK, conn);
        check_dims(R, C, Z, batch);
        check_cc_filter(min_size, keep_largest, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, nullptr, a);
        batch_filter_components(b, VH_CC_MASK, conn, min_size, keep_largest, nullptr);
        if (kept) HIP_TRY(hipMemcpyAsync(kept, b->d_cc_kept, sizeof(int64_t) * (size_t)batch * 2, hipMemcpyDeviceToHost, b->stream));
        if (out) HIP_TRY(hipMemcpyAsync(out, b->d_mask, (size_t)batch * b->V, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    })
}

// ---- the defect table of a device-resident batch (defect_table.hip) ----------------------------------
// Enqueue the table of the resident labelling.  It reads the root and size maps (and the run's N4) and
// writes the table's buffers only, so nothing another call on the batch reads changes.
static void batch_defect_table(vh_batch *b, const uint32_t *min_size, int32_t max_rows, int norm) {
    if (!min_size) throw VhError{VH_ERR_ARG, "null min_size"};
    if (max_rows < 1 || max_rows > VH_DT_MAX_ROWS) throw VhError{VH_ERR_ARG, "max_rows must be 1..1024"};
    if (norm != VH_DT_NO_SIGNAL && norm != VH_NORM_MEAN && norm != VH_NORM_P99)
        throw VhError{VH_ERR_ARG, "norm must be VH_NORM_MEAN, VH_NORM_P99 or VH_DT_NO_SIGNAL"};
    for (int64_t i = 0; i < b->nb; ++i)
        if (min_size[i] < 1) throw VhError{VH_ERR_ARG, "every min_size must be >= 1 (study " + std::to_string(i) + ")"};
    if (norm != VH_DT_NO_SIGNAL) b->state.need_run();
    b->state.need_components();
    if (!vh_dt_takes(b)) throw VhError{VH_ERR_ARG, "defect table: more than 65535 studies or a volume of 2^31 voxels"};
    const size_t nb = (size_t)b->nb;
    b->d_dt_rows.reserve(nb * VH_DT_MAX_ROWS * VH_DT_COLS);   // the largest max_rows: no regrowth
    b->d_dt_stats.reserve(nb * 4);
    b->d_dt_keys.reserve(nb * VH_DT_MAX_ROWS);
    b->d_dt_sel.reserve(nb * 2);
    b->d_dt_cut.reserve(nb);
    b->d_dt_hist.reserve(nb * 2048);
    b->d_dt_cnt.reserve(nb);
    b->d_dt_min.reserve(nb);
    // (a pageable source: the copy has left min_size when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_dt_min, min_size, sizeof(uint32_t) * nb, hipMemcpyHostToDevice, b->stream));
    vh_dt_launch(b, max_rows, norm);
    b->state.defect_table_enqueued(max_rows, norm != VH_DT_NO_SIGNAL);
}

static void batch_download_defect_table(vh_batch *b, int64_t *rows, int64_t *stats) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the rows are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (rows)
        HIP_TRY(hipMemcpyAsync(rows, b->d_dt_rows, sizeof(int64_t) * nb * b->state.dt_rows() * VH_DT_COLS,
                               hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, b->d_dt_stats, sizeof(int64_t) * nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_defect_table(vh_batch *b, const uint32_t *min_size, int32_t max_rows, int norm) {
    BATCH_TRY(b, { batch_defect_table(b, min_size, max_rows, norm); })
}

int vh_batch_download_defect_table(vh_batch *b, int64_t *rows, int64_t *stats) {
    BATCH_TRY(b, {
        b->state.need_defect_table();
        batch_download_defect_table(b, rows, stats);
    })
}

// ---- the regional analysis of a device-resident batch (zones.hip) ------------------------------------
// the argument checks (host only: nothing is enqueued before they pass); returns K
static int32_t check_zones(const uint8_t *labels, int32_t n_zones, const int32_t *parts, int lateral, int by, int norm,
                           int32_t n_bins, float hi) {
    if (norm != VH_NORM_MEAN && norm != VH_NORM_P99)
        throw VhError{VH_ERR_ARG, "norm must be VH_NORM_MEAN or VH_NORM_P99"};
    if (n_bins < 1 || n_bins > 256) throw VhError{VH_ERR_ARG, "n_bins must be 1..256"};
    if (!std::isfinite(hi) || !(hi > 0.0f) || !(hi <= 64.0f))
        throw VhError{VH_ERR_ARG, "hi must be finite, > 0 and <= 64"};
    if (labels) {
        if (n_zones < 1 || n_zones > ZN_MAX_PARTS) throw VhError{VH_ERR_ARG, "n_zones must be 1..32"};
        return n_zones;
    }
    if (by != VH_ZONE_EXTENT && by != VH_ZONE_COUNT) throw VhError{VH_ERR_ARG, "by must be VH_ZONE_EXTENT or VH_ZONE_COUNT"};
    if (!parts) throw VhError{VH_ERR_ARG, "null parts"};
    if (lateral != 0 && lateral != 1) throw VhError{VH_ERR_ARG, "lateral must be 0 or 1"};
    int64_t K = 1;
    for (int a = 0; a < 3; ++a) {
        if (parts[a] < 1) throw VhError{VH_ERR_ARG, "every part count must be >= 1"};
        if (parts[a] > ZN_MAX_PARTS) throw VhError{VH_ERR_ARG, "more than 32 zones"};
        K *= parts[a];
    }
    if (lateral && parts[1] != 1) throw VhError{VH_ERR_ARG, "lateral needs parts[1] = 1"};
    if (lateral) K *= 2;
    if (K > ZN_MAX_PARTS) throw VhError{VH_ERR_ARG, "more than 32 zones"};
    return (int32_t)K;
}

// Enqueue the four kernels over what the last run left resident.  They write the zone buffers only, so
// nothing another call on the batch reads changes (the CI stays fresh).
static void batch_zones(vh_batch *b, const uint8_t *labels, int32_t K, const int32_t *parts, int lateral, int by,
                        int norm, int32_t n_bins, float hi) {
    b->state.need_run();
    if (!vh_zones_takes(b)) throw VhError{VH_ERR_ARG, "zones: more than 65535 studies"};
    const size_t nb = (size_t)b->nb, L = (size_t)(b->R + b->C + b->Z), K1 = ZN_MAX_PARTS + 1;   // the largest K: no regrowth
    b->d_zn_prof.reserve(nb * L);
    b->d_zn_tab.reserve(nb * L);
    b->d_zn_geom.reserve(nb * 8);
    b->d_zn_map.reserve(nb * b->V);
    b->d_zn_counts.reserve(nb * K1 * VH_ZONE_COLS);
    b->d_zn_hist.reserve(nb * K1 * 256);
    b->d_zn_stats.reserve(nb * K1 * 4);
    static const int32_t one[3] = {1, 1, 1};
    if (labels) {   // the caller's buffer is free once the call returns: wait for the copy, and for it alone
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipMemcpyAsync(b->d_zn_map, labels, nb * b->V, hipMemcpyHostToDevice, b->stream);
        if (e == hipSuccess) e = hipEventRecord(ev, b->stream);
        if (e == hipSuccess) e = hipEventSynchronize(ev);
        (void)hipEventDestroy(ev);
        HIP_TRY(e);
    }
    const float scale = (float)n_bins / hi;   // once, in float32: the kernel multiplies by it
    vh_zones_launch(b, labels != nullptr, K, labels ? one : parts, labels ? 0 : lateral, labels ? VH_ZONE_EXTENT : by,
                    norm, n_bins, hi, scale);
    b->state.zones_enqueued(K, n_bins);
}

static void batch_download_zones(vh_batch *b, uint8_t *map, int64_t *counts, uint32_t *hist, int64_t *stats,
                                 int32_t *geom) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb, K1 = (size_t)b->state.zone_k() + 1;
    if (map) HIP_TRY(hipMemcpyAsync(map, b->d_zn_map, nb * b->V, hipMemcpyDeviceToHost, st));
    if (counts)
        HIP_TRY(hipMemcpyAsync(counts, b->d_zn_counts, sizeof(int64_t) * nb * K1 * VH_ZONE_COLS, hipMemcpyDeviceToHost, st));
    if (hist)
        HIP_TRY(hipMemcpyAsync(hist, b->d_zn_hist, sizeof(uint32_t) * nb * K1 * b->state.zone_bins(), hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, b->d_zn_stats, sizeof(int64_t) * nb * K1 * 4, hipMemcpyDeviceToHost, st));
    if (geom) HIP_TRY(hipMemcpyAsync(geom, b->d_zn_geom, sizeof(int32_t) * nb * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_zones(vh_batch *b, const uint8_t *labels, int32_t n_zones, const int32_t parts[3], int lateral, int by,
                   int norm, int32_t n_bins, float hi) {
    BATCH_TRY(b, {
        const int32_t K = check_zones(labels, n_zones, parts, lateral, by, norm, n_bins, hi);
        batch_zones(b, labels, K, parts, lateral, by, norm, n_bins, hi);
    })
}

int vh_batch_download_zones(vh_batch *b, uint8_t *map, int64_t *counts, uint32_t *hist, int64_t *stats, int32_t *geom) {
    BATCH_TRY(b, {
        b->state.need_zones();
        batch_download_zones(b, map, counts, hist, stats, geom);
    })
}

int vh_zones(vh_ctx *ctx, const float *n4, const uint8_t *mask, const uint8_t *defect, int64_t R, int64_t C, int64_t Z,
             int64_t batch, float thresh, const uint8_t *labels, int32_t n_zones, const int32_t parts[3], int lateral,
             int by, int norm, int32_t n_bins, float hi, uint8_t *map, int64_t *counts, uint32_t *hist, int64_t *stats,
             int32_t *geom) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!n4 || !mask) throw VhError{VH_ERR_ARG, "null buffer"};
        const int32_t K = check_zones(labels, n_zones, parts, lateral, by, norm, n_bins, hi);
        check_dims(R, C, Z, batch);
        const vh_run_opts o = chain_only_opts(thresh, false, false, ctx->profile);
        vh_batch *b = run_host_arrays(ctx, nullptr, n4, mask, R, C, Z, batch, o);
        if (defect) {   // (pageable source, and batch_download_zones waits before the call returns)
            HIP_TRY(hipMemcpyAsync(b->d_defect, defect, (size_t)batch * b->V, hipMemcpyHostToDevice, b->stream));
            b->state.defect_replaced();
        }
        batch_zones(b, labels, K, parts, lateral, by, norm, n_bins, hi);
        batch_download_zones(b, map, counts, hist, stats, geom);
        throw_if_empty_mask(read_scalars(b));
    })
}

// the rule on the host (zones_host.h): no device, no context
static bool zone_profile_ok(const int64_t *profile, int64_t n) {
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (profile[i] < 0 || profile[i] > ((int64_t)1 << 57) - total) return false;
        total += profile[i];
    }
    return true;
}

int vh_zone_parts(const int64_t *profile, int64_t n, int32_t p, int by, uint8_t *part, int32_t bounds[2]) {
    if (!profile || !part || !bounds || n < 1 || n > INT32_MAX || p < 1 || p > ZN_MAX_PARTS ||
        (by != VH_ZONE_EXTENT && by != VH_ZONE_COUNT) || !zone_profile_ok(profile, n))
        return VH_ERR_ARG;
    int32_t lo, hi;
    int64_t total;
    zn_bounds(profile, n, lo, hi, total);
    zn_axis_parts(profile, n, p, by, lo, hi, total, part);
    bounds[0] = lo;
    bounds[1] = hi;
    return VH_OK;
}

int vh_zone_split(const int64_t *profile, int64_t n, int32_t *s) {
    if (!profile || !s || n < 1 || n > INT32_MAX || !zone_profile_ok(profile, n)) return VH_ERR_ARG;
    int32_t lo, hi;
    int64_t total;
    zn_bounds(profile, n, lo, hi, total);
    *s = zn_split(profile, lo, hi);
    return VH_OK;
}

// ---- the denoise option of a device-resident batch (denoise.hip) --------------------------------
// The resident HPvent, or the mask statistics and scalars, are no longer the last run's: the calls that
// read a run's results refuse until the next one; an uploaded defect map and an enqueued CI stay.
// (Not a fresh batch's state, and nothing to do with vh_batch_upload, which invalidates nothing.)
static void batch_forget_run(vh_batch *b) { b->state.forgot_run(); }

// the mask statistics and the SNR sweep of the resident HPvent, then the Rayleigh estimate of every
// study from the sweep's noise partials; waits
static void batch_noise_sigma(vh_batch *b, float *sigma) {
    b->d_dn_sigma.reserve((size_t)b->nb);
    vh_launch_mask_stats(b);   // (rewrites the scalars: a run's results are gone)
    batch_forget_run(b);
    vh_launch_snr(b);
    vh_noise_sigma_launch(b, b->d_dn_sigma);
    d2h_on_stream(b, sigma, b->d_dn_sigma, sizeof(float) * (size_t)b->nb);
}

// the argument checks (host only: nothing is enqueued before they pass)
static void check_denoise(const float *sigma, int64_t nb, float strength, int search_r, int patch_r) {
    if (!sigma) throw VhError{VH_ERR_ARG, "null sigma"};
    if (search_r < 1 || search_r > 5) throw VhError{VH_ERR_ARG, "search_r must be 1..5"};
    if (patch_r < 0 || patch_r > 2) throw VhError{VH_ERR_ARG, "patch_r must be 0..2"};
    if (!std::isfinite(strength) || !(strength > 0.0f))
        throw VhError{VH_ERR_ARG, "strength must be finite and > 0"};
    for (int64_t i = 0; i < nb; ++i)
        if (!std::isfinite(sigma[i]) || !(sigma[i] > 0.0f))
            throw VhError{VH_ERR_ARG, "every sigma must be finite and > 0 (study " + std::to_string(i) + ")"};
}

// Enqueue the filter from d_hp into d_n4 (free until the next run writes it) and exchange the two
// buffers: the denoised volumes are the resident HPvent from here on.  Every launch takes the
// buffers' addresses when it is enqueued, on this one stream, so the exchange is safe behind work
// still in flight.
static void batch_denoise(vh_batch *b, const float *sigma, float strength, int search_r, int patch_r, int rician) {
    if (!vh_denoise_takes(b)) throw VhError{VH_ERR_ARG, "denoise: batch or tile count out of range"};
    const double n = (double)((2 * patch_r + 1) * (2 * patch_r + 1));
    std::vector<float> prm(2 * (size_t)b->nb);
    for (int64_t i = 0; i < b->nb; ++i) {   // in double, rounded to float32 once
        const double ks = (double)strength * (double)sigma[i];
        prm[2 * i] = (float)(1.0 / (2.0 * n * (ks * ks)));
        prm[2 * i + 1] = (float)(2.0 * ((double)sigma[i] * (double)sigma[i]));
    }
    b->d_dn_prm.reserve(prm.size());
    // (pageable source: the copy has left prm when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_dn_prm, prm.data(), sizeof(float) * prm.size(), hipMemcpyHostToDevice, b->stream));
    vh_denoise_launch(b, b->d_hp, b->d_n4, b->d_dn_prm, search_r, patch_r, rician);
    std::swap(b->d_hp, b->d_n4);
    batch_forget_run(b);
}

int vh_batch_noise_sigma(vh_batch *b, float *sigma) {
    BATCH_TRY(b, {
        if (!sigma) throw VhError{VH_ERR_ARG, "null buffer"};
        batch_noise_sigma(b, sigma);
    })
}

int vh_batch_denoise(vh_batch *b, const float *sigma, float strength, int search_r, int patch_r, int rician) {
    BATCH_TRY(b, {
        check_denoise(sigma, b->nb, strength, search_r, patch_r);
        batch_denoise(b, sigma, strength, search_r, patch_r, rician);
    })
}

int vh_batch_download_hp(vh_batch *b, float *hp) {
    BATCH_TRY(b, {
        if (!hp) throw VhError{VH_ERR_ARG, "null buffer"};
        d2h_on_stream(b, hp, b->d_hp, sizeof(float) * (size_t)b->nb * b->V);
    })
}

int vh_noise_sigma(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                   int64_t batch, float *sigma) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!hp || !mask || !sigma) throw VhError{VH_ERR_ARG, "null buffer"};
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, hp, mask);
        batch_noise_sigma(b, sigma);
    })
}

int vh_denoise(vh_ctx *ctx, const float *hp, int64_t R, int64_t C, int64_t Z, int64_t batch,
               const float *sigma, float strength, int search_r, int patch_r, int rician, float *out) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!hp || !out) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_denoise(sigma, batch, strength, search_r, patch_r);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, hp, nullptr);
        batch_denoise(b, sigma, strength, search_r, patch_r, rician);
        d2h_on_stream(b, out, b->d_hp, sizeof(float) * (size_t)batch * b->V);
    })
}

// ---- editing the masks of a device-resident batch (mask_edit.hip) -------------------------------
// the argument checks (host only: nothing is enqueued before they pass)
static void check_mask_edit(int op, const int32_t *radius, int64_t nb) {
    if (op < VH_MASK_ERODE || op > VH_MASK_CLOSE)
        throw VhError{VH_ERR_ARG, "op must be VH_MASK_ERODE, _DILATE, _OPEN or _CLOSE"};
    if (!radius) throw VhError{VH_ERR_ARG, "null radius"};
    for (int64_t i = 0; i < nb; ++i)
        if (radius[i] < 0 || radius[i] > 5)
            throw VhError{VH_ERR_ARG, "every radius must be 0..5 (study " + std::to_string(i) + ")"};
}

// Enqueue the morphology.  One step goes from d_mask into d_border (free until the next run writes
// it) and the two buffers are exchanged, as batch_denoise exchanges its volumes; open and close go
// there and back, so the intermediate is a mask volume of its own and the second step pads it like
// any other.  d_hp, d_n4 and d_defect are not touched.
static void batch_edit_mask(vh_batch *b, int op, const int32_t *radius) {
    if (!vh_mask_edit_takes(b)) throw VhError{VH_ERR_ARG, "edit_mask: batch or tile count out of range"};
    b->d_me_radius.reserve((size_t)b->nb);
    // (pageable source: the copy has left radius when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_me_radius, radius, sizeof(int32_t) * (size_t)b->nb, hipMemcpyHostToDevice,
                           b->stream));
    const int first = (op == VH_MASK_ERODE || op == VH_MASK_OPEN) ? 1 : 0;
    vh_mask_morph_launch(b, b->d_mask, b->d_border, b->d_me_radius, first);
    if (op == VH_MASK_OPEN || op == VH_MASK_CLOSE)
        vh_mask_morph_launch(b, b->d_border, b->d_mask, b->d_me_radius, 1 - first);
    else
        std::swap(b->d_mask, b->d_border);
    batch_forget_run(b);
}

// The strokes go into d_lb (free until the next run writes it); the call waits until they have left
// the caller's buffer -- an event behind the copy, not the stream -- and enqueues the kernel.
static void batch_paint_mask(vh_batch *b, const uint8_t *strokes, int how) {
    if (!vh_mask_edit_takes(b)) throw VhError{VH_ERR_ARG, "paint_mask: batch or tile count out of range"};
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipMemcpyAsync(b->d_lb, strokes, (size_t)b->nb * b->V, hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = hipEventRecord(ev, b->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
    batch_forget_run(b);   // (d_lb is no longer the run's, whatever follows)
    HIP_TRY(e);
    vh_mask_paint_launch(b, b->d_mask, b->d_lb, how);
}

static void batch_download_mask(vh_batch *b, uint8_t *mask, int64_t *count) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    if (count) {
        b->d_me_count.reserve(nb);
        HIP_TRY(hipMemsetAsync(b->d_me_count, 0, sizeof(unsigned long long) * nb, st));
        vh_mask_count_launch(b, b->d_mask, b->d_me_count);
        HIP_TRY(hipMemcpyAsync(count, b->d_me_count, sizeof(int64_t) * nb, hipMemcpyDeviceToHost, st));
    }
    if (mask) HIP_TRY(hipMemcpyAsync(mask, b->d_mask, nb * b->V, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
}

int vh_batch_edit_mask(vh_batch *b, int op, const int32_t *radius) {
    BATCH_TRY(b, {
        check_mask_edit(op, radius, b->nb);
        batch_edit_mask(b, op, radius);
    })
}

int vh_batch_paint_mask(vh_batch *b, const uint8_t *strokes, int how) {
    BATCH_TRY(b, {
        if (!strokes) throw VhError{VH_ERR_ARG, "null strokes"};
        if (how < VH_PAINT_OR || how > VH_PAINT_XOR)
            throw VhError{VH_ERR_ARG, "how must be VH_PAINT_OR, _ANDNOT, _AND or _XOR"};
        batch_paint_mask(b, strokes, how);
    })
}

int vh_batch_download_mask(vh_batch *b, uint8_t *mask, int64_t *count) {
    BATCH_TRY(b, { batch_download_mask(b, mask, count); })
}

int vh_edit_mask(vh_ctx *ctx, const uint8_t *mask, int64_t R, int64_t C, int64_t Z, int64_t batch, int op,
                 const int32_t *radius, uint8_t *out, int64_t *count) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!mask) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_mask_edit(op, radius, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, nullptr, mask);
        batch_edit_mask(b, op, radius);
        batch_download_mask(b, out, count);
    })
}

// ---- the lungs from the proton image of a device-resident batch (segment.hip) -------------------
// The Otsu cut of a histogram, on the host alone: the lowest k that maximises d * d / (n0 * (N - n0)),
// d = S * n0 - N * s0, in double and in this operation order.
int vh_otsu(const uint32_t *hist, int32_t n_bins, int32_t *cut) {
#pragma clang fp contract(off)
    if (!hist || !cut || n_bins < 2) return VH_ERR_ARG;
    uint64_t Ni = 0, Si = 0;
    int occupied = 0;
    for (int32_t i = 0; i < n_bins; ++i) {
        Ni += hist[i];
        Si += (uint64_t)i * hist[i];
        occupied += hist[i] != 0;
    }
    if (occupied < 2) return VH_ERR_EMPTY;
    const double N = (double)Ni, S = (double)Si;
    uint64_t n0i = 0, s0i = 0;
    double best = -1.0;
    int32_t at = -1;
    for (int32_t k = 0; k + 1 < n_bins; ++k) {
        n0i += hist[k];
        s0i += (uint64_t)k * hist[k];
        if (n0i == 0 || n0i == Ni) continue;
        const double n0 = (double)n0i, s0 = (double)s0i;
        const double d = S * n0 - N * s0;
        const double v = d * d / (n0 * (N - n0));
        if (v > best) { best = v; at = k; }
    }
    if (at < 0) return VH_ERR_EMPTY;
    *cut = at;
    return VH_OK;
}

// the argument checks of a segmentation (host only: nothing is enqueued before they pass)
static void check_segment(const float *thresh, const int32_t *open_radius, int64_t nb) {
    for (int64_t i = 0; thresh && i < nb; ++i)
        if (!std::isfinite(thresh[i]) || !(thresh[i] > 0.0f))
            throw VhError{VH_ERR_ARG, "every thresh must be finite and > 0 (study " + std::to_string(i) + ")"};
    for (int64_t i = 0; open_radius && i < nb; ++i)
        if (open_radius[i] < 0 || open_radius[i] > 5)
            throw VhError{VH_ERR_ARG, "every open_radius must be 0..5 (study " + std::to_string(i) + ")"};
}

static void batch_upload_proton(vh_batch *b, const float *proton) {
    const size_t NV = (size_t)b->nb * b->V;
    b->d_proton.reserve(NV);
    HIP_TRY(hipMemcpyAsync(b->d_proton, proton, sizeof(float) * NV, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->state.proton_uploaded();
}

// the statistics sweep, then on the host the Otsu cut and the threshold of every study; waits.  It
// writes its own two buffers only.
static void batch_proton_threshold(vh_batch *b, float *thresh, float *pmax, uint32_t *hist) {
#pragma clang fp contract(off)
    const size_t nb = (size_t)b->nb;
    b->d_sg_pmax.reserve(nb);
    b->d_sg_hist.reserve(nb * 256);
    vh_proton_stats_launch(b, b->d_proton, b->d_sg_pmax, b->d_sg_hist);
    std::vector<uint32_t> bits(nb), h(nb * 256);
    HIP_TRY(hipMemcpyAsync(bits.data(), b->d_sg_pmax, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, b->stream));
    d2h_on_stream(b, h.data(), b->d_sg_hist, sizeof(uint32_t) * h.size());
    for (size_t i = 0; i < nb; ++i) {
        float pm;
        memcpy(&pm, &bits[i], sizeof(float));
        int32_t k = 0;
        float t = std::numeric_limits<float>::quiet_NaN();
        if (pm > 0.0f && vh_otsu(h.data() + 256 * i, 256, &k) == VH_OK) {
            const float width = pm / 256.0f;
            t = (float)(k + 1) * width;
        }
        thresh[i] = t;
        if (pmax) pmax[i] = pm;
    }
    if (hist) memcpy(hist, h.data(), sizeof(uint32_t) * h.size());
}

// Enqueue the fill from d_proton into d_border (free until the next run writes it) and exchange it
// with d_mask, as batch_edit_mask does; the opening then goes there and back (a study of radius 0 is
// copied both times).  d_hp, d_n4 and d_defect are not touched.
static void batch_segment(vh_batch *b, const float *thresh, const int32_t *open_radius) {
    b->state.need_proton();
    if (!vh_segment_takes(b)) throw VhError{VH_ERR_ARG, "segment: a plane of at most 512 x 512, at most 65535 studies"};
    bool open = false;
    for (int64_t i = 0; open_radius && i < b->nb; ++i) open = open || open_radius[i] > 0;
    if (open && !vh_mask_edit_takes(b)) throw VhError{VH_ERR_ARG, "segment: batch or tile count out of range"};
    b->d_sg_thresh.reserve((size_t)b->nb);
    // (pageable sources: the copies have left thresh and open_radius when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_sg_thresh, thresh, sizeof(float) * (size_t)b->nb, hipMemcpyHostToDevice, b->stream));
    if (open) {
        b->d_me_radius.reserve((size_t)b->nb);
        HIP_TRY(hipMemcpyAsync(b->d_me_radius, open_radius, sizeof(int32_t) * (size_t)b->nb, hipMemcpyHostToDevice,
                               b->stream));
    }
    vh_segment_launch(b, b->d_proton, b->d_border, b->d_sg_thresh);
    std::swap(b->d_mask, b->d_border);
    if (open) {
        vh_mask_morph_launch(b, b->d_mask, b->d_border, b->d_me_radius, 1);
        vh_mask_morph_launch(b, b->d_border, b->d_mask, b->d_me_radius, 0);
    }
    batch_forget_run(b);
}

// The other mask goes into d_lb (free until the next run writes it), as the strokes of a paint do.
static void batch_mask_overlap(vh_batch *b, const uint8_t *other, int64_t *counts) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
    const size_t nb = (size_t)b->nb;
    b->d_sg_count.reserve(3 * nb);
    batch_forget_run(b);   // (d_lb is no longer the run's, whatever follows)
    HIP_TRY(hipMemcpyAsync(b->d_lb, other, nb * b->V, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_sg_count, 0, sizeof(unsigned long long) * 3 * nb, b->stream));
    vh_mask_overlap_launch(b, b->d_mask, b->d_lb, b->d_sg_count);
    d2h_on_stream(b, counts, b->d_sg_count, sizeof(int64_t) * 3 * nb);
}

int vh_batch_upload_proton(vh_batch *b, const float *proton) {
    BATCH_TRY(b, {
        if (!proton) throw VhError{VH_ERR_ARG, "null buffer"};
        batch_upload_proton(b, proton);
    })
}

int vh_batch_proton_threshold(vh_batch *b, float *thresh, float *pmax, uint32_t *hist) {
    BATCH_TRY(b, {
        if (!thresh) throw VhError{VH_ERR_ARG, "null buffer"};
        b->state.need_proton();
        batch_proton_threshold(b, thresh, pmax, hist);
    })
}

int vh_batch_segment(vh_batch *b, const float *thresh, const int32_t *open_radius) {
    BATCH_TRY(b, {
        if (!thresh) throw VhError{VH_ERR_ARG, "null thresh"};
        check_segment(thresh, open_radius, b->nb);
        batch_segment(b, thresh, open_radius);
    })
}

int vh_batch_mask_overlap(vh_batch *b, const uint8_t *other, int64_t *counts) {
    BATCH_TRY(b, {
        if (!other || !counts) throw VhError{VH_ERR_ARG, "null buffer"};
        batch_mask_overlap(b, other, counts);
    })
}

int vh_segment(vh_ctx *ctx, const float *proton, int64_t R, int64_t C, int64_t Z, int64_t batch, const float *thresh,
               const int32_t *open_radius, uint8_t *mask_out, float *thresh_out, int64_t *count) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!proton) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_segment(thresh, open_radius, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        if (!vh_segment_takes(b)) throw VhError{VH_ERR_ARG, "segment: a plane of at most 512 x 512, at most 65535 studies"};
        batch_upload_proton(b, proton);
        std::vector<float> th((size_t)batch);
        if (thresh)
            std::copy(thresh, thresh + batch, th.begin());
        else
            batch_proton_threshold(b, th.data(), nullptr, nullptr);
        if (thresh_out) std::copy(th.begin(), th.end(), thresh_out);
        for (int64_t i = 0; i < batch; ++i)
            if (std::isnan(th[i]))
                throw VhError{VH_ERR_EMPTY, "segment: no Otsu threshold for study " + std::to_string(i) +
                                                " (fewer than two occupied bins)"};
        batch_segment(b, th.data(), open_radius);
        batch_download_mask(b, mask_out, count);
    })
}

// ---- the proton registered to the xenon image of a device-resident batch (register.hip) -----------
// The mutual information of a joint histogram [levels][levels], on the host alone, as k_reg_score
// evaluates it: sums as exact integers, each term (double)J * log(((double)J * n) / (Ja * Jb)).
int vh_mi(const uint32_t *joint, int32_t levels, double *mi) {
#pragma clang fp contract(off)
    if (!joint || !mi || levels < 1 || levels > 256) return VH_ERR_ARG;
    const size_t L = (size_t)levels;
    std::vector<uint64_t> ja(L, 0), jb(L, 0);
    uint64_t n = 0;
    for (size_t a = 0; a < L; ++a)
        for (size_t c = 0; c < L; ++c) {
            const uint64_t j = joint[a * L + c];
            ja[a] += j;
            jb[c] += j;
            n += j;
        }
    double acc = 0.0;
    for (size_t a = 0; a < L; ++a)
        for (size_t c = 0; c < L; ++c) {
            const uint32_t j = joint[a * L + c];
            if (!j) continue;
            const double num = (double)j * (double)n;
            const double den = (double)ja[a] * (double)jb[c];
            acc += (double)j * std::log(num / den);
        }
    *mi = n ? acc / (double)n : 0.0;
    return VH_OK;
}

// the limits of a search window that do not depend on the volume
static bool search_in_limits(const int32_t *search) {
    return search && search[0] >= 0 && search[0] <= 8 && search[1] >= 0 && search[1] <= 8 && search[2] >= 0 &&
           search[2] <= 2;
}

// The best shift of one study's scores [ns]: the largest score; among equal scores the smallest
// |dr| + |dc| + |dz|, then the lowest index.  A NaN never wins: with nothing but NaN the shift is (0, 0, 0).
int vh_register_pick(const double *score, const int32_t search[3], int32_t best[3]) {
    if (!score || !best || !search_in_limits(search)) return VH_ERR_ARG;
    const int Sr = search[0], Sc = search[1], Sz = search[2];
    int32_t at[3] = {0, 0, 0};
    int l1 = -1;
    double top = 0.0;
    size_t i = 0;
    for (int dz = -Sz; dz <= Sz; ++dz)
        for (int dr = -Sr; dr <= Sr; ++dr)
            for (int dc = -Sc; dc <= Sc; ++dc, ++i) {
                const double v = score[i];
                if (std::isnan(v)) continue;
                const int d = std::abs(dr) + std::abs(dc) + std::abs(dz);
                if (l1 < 0 || v > top || (v == top && d < l1)) {
                    top = v; l1 = d;
                    at[0] = dr; at[1] = dc; at[2] = dz;
                }
            }
    best[0] = at[0]; best[1] = at[1]; best[2] = at[2];
    return VH_OK;
}

// the argument checks of a registration (host only: nothing is enqueued before they pass)
static void check_register(const int32_t *search, int64_t R, int64_t C, int64_t Z) {
    if (!search) throw VhError{VH_ERR_ARG, "null search"};
    if (!search_in_limits(search) || search[0] >= R || search[1] >= C || search[2] >= Z)
        throw VhError{VH_ERR_ARG, "search must be 0..8, 0..8, 0..2 and below the volume's dimensions"};
}

static int64_t search_shifts(const int32_t *search) {
    return (int64_t)(2 * search[0] + 1) * (2 * search[1] + 1) * (2 * search[2] + 1);
}

// The codes, the joint histogram of every shift and the scores of d_proton against d_hp, then on the
// host the pick of every study; waits.  It writes its own buffers only.
static void batch_register(vh_batch *b, const int32_t *search, double *score, int32_t *best, double *best_score,
                           int32_t *status) {
    b->state.need_proton();
    if (!vh_register_takes(b)) throw VhError{VH_ERR_ARG, "register: batch or tile count out of range"};
    const size_t nb = (size_t)b->nb, NV = nb * (size_t)b->V;
    const size_t ns = (size_t)search_shifts(search);
    b->d_rg_max.reserve(2 * nb);
    b->d_rg_cp.reserve(NV);
    b->d_rg_cx.reserve(NV);
    b->d_rg_score.reserve(nb * ns);
    b->rg_ns = 0;   // (a failed growth leaves no histograms to download)
    b->d_rg_hist.reserve(nb * ns * 1024);
    vh_register_launch(b, b->d_proton, b->d_hp, search, b->d_rg_max, b->d_rg_cp, b->d_rg_cx, b->d_rg_hist,
                       b->d_rg_score);
    b->rg_ns = (int64_t)ns;
    std::vector<uint32_t> bits(2 * nb);
    HIP_TRY(hipMemcpyAsync(bits.data(), b->d_rg_max, sizeof(uint32_t) * 2 * nb, hipMemcpyDeviceToHost, b->stream));
    d2h_on_stream(b, score, b->d_rg_score, sizeof(double) * nb * ns);
    for (size_t i = 0; i < nb; ++i) {
        float pm, xm;
        memcpy(&pm, &bits[i], sizeof(float));
        memcpy(&xm, &bits[nb + i], sizeof(float));
        const bool ok = pm > 0.0f && xm > 0.0f;
        int32_t *at = best + 3 * i;
        (void)vh_register_pick(score + ns * i, search, at);
        if (status) status[i] = ok ? 0 : 1;
        if (best_score) {
            const size_t k = ((size_t)(at[2] + search[2]) * (size_t)(2 * search[0] + 1) + (size_t)(at[0] + search[0])) *
                                 (size_t)(2 * search[1] + 1) + (size_t)(at[1] + search[1]);
            best_score[i] = score[ns * i + k];
        }
    }
}

static void check_shift(const vh_batch *b, int what, const int32_t *shift) {
    if (what != VH_SHIFT_PROTON && what != VH_SHIFT_MASK)
        throw VhError{VH_ERR_ARG, "what must be VH_SHIFT_PROTON or VH_SHIFT_MASK"};
    if (!shift) throw VhError{VH_ERR_ARG, "null shift"};
    const int64_t dim[3] = {b->R, b->C, b->Z};
    for (int64_t i = 0; i < b->nb; ++i)
        for (int k = 0; k < 3; ++k)
            if (shift[3 * i + k] > dim[k] || shift[3 * i + k] < -dim[k])
                throw VhError{VH_ERR_ARG, "every shift must be within the volume's dimensions (study " +
                                              std::to_string(i) + ")"};
}

// Enqueue the shift.  The proton goes from d_proton into a volume of its own and the two are exchanged;
// the mask goes from d_mask into d_border (free until the next run writes it) and is exchanged with it,
// as batch_edit_mask does.  d_hp, d_n4 and d_defect are not touched.
static void batch_shift(vh_batch *b, int what, const int32_t *shift) {
    if (what == VH_SHIFT_PROTON) b->state.need_proton();
    const size_t nb = (size_t)b->nb;
    if (what == VH_SHIFT_PROTON) b->d_rg_ptmp.reserve(nb * (size_t)b->V);
    b->d_rg_shift.reserve(3 * nb);
    // (pageable source: the copy has left shift when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_rg_shift, shift, sizeof(int32_t) * 3 * nb, hipMemcpyHostToDevice, b->stream));
    if (what == VH_SHIFT_PROTON) {
        vh_shift_launch_f32(b, b->d_proton, b->d_rg_ptmp, b->d_rg_shift);
        std::swap(b->d_proton, b->d_rg_ptmp);
    } else {
        vh_shift_launch_u8(b, b->d_mask, b->d_border, b->d_rg_shift);
        std::swap(b->d_mask, b->d_border);
        batch_forget_run(b);
    }
}

int vh_batch_register(vh_batch *b, const int32_t search[3], double *score, int32_t *best, double *best_score,
                      int32_t *status) {
    BATCH_TRY(b, {
        if (!score || !best) throw VhError{VH_ERR_ARG, "null buffer"};
        check_register(search, b->R, b->C, b->Z);
        batch_register(b, search, score, best, best_score, status);
    })
}

int vh_batch_download_register_hist(vh_batch *b, uint32_t *hist) {
    BATCH_TRY(b, {
        if (!hist) throw VhError{VH_ERR_ARG, "null buffer"};
        if (b->rg_ns <= 0) throw VhError{VH_ERR_ARG, "vh_batch_register has not been called"};
        d2h_on_stream(b, hist, b->d_rg_hist, sizeof(uint32_t) * (size_t)b->nb * (size_t)b->rg_ns * 1024);
    })
}

int vh_batch_shift(vh_batch *b, int what, const int32_t *shift) {
    BATCH_TRY(b, {
        check_shift(b, what, shift);
        batch_shift(b, what, shift);
    })
}

int vh_batch_download_proton(vh_batch *b, float *proton) {
    BATCH_TRY(b, {
        if (!proton) throw VhError{VH_ERR_ARG, "null buffer"};
        b->state.need_proton();
        d2h_on_stream(b, proton, b->d_proton, sizeof(float) * (size_t)b->nb * b->V);
    })
}

int vh_register(vh_ctx *ctx, const float *proton, const float *hp, int64_t R, int64_t C, int64_t Z, int64_t batch,
                const int32_t search[3], double *score, int32_t *best, int32_t *status, float *shifted_out) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!proton || !hp || !score || !best) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_register(search, R, C, Z);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, hp, nullptr);
        batch_upload_proton(b, proton);
        batch_register(b, search, score, best, nullptr, status);
        if (shifted_out) {
            batch_shift(b, VH_SHIFT_PROTON, best);
            d2h_on_stream(b, shifted_out, b->d_proton, sizeof(float) * (size_t)batch * b->V);
        }
    })
}

// ---- the proton resampled from its own grid onto the batch's (resample.hip) -----------------------
// The tap table of one axis, on the host alone (resample_host.h).
int vh_resample_taps(int64_t n_src, int64_t n_dst, double scale, double offset, int32_t *first, int32_t *count,
                     float *weight) {
    return rs_axis_taps(n_src, n_dst, scale, offset, first, count, weight) ? VH_OK : VH_ERR_ARG;
}

// the argument checks of a resampling (host only: nothing is enqueued before they pass)
static void check_resample_shape(const int64_t *shape) {
    if (!shape) throw VhError{VH_ERR_ARG, "null shape"};
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || shape[k] > RS_MAX_SRC)
            throw VhError{VH_ERR_ARG, "every source dimension must be 1..1024"};
}
static void check_resample_map(const double *map, int64_t nb) {
    if (!map) throw VhError{VH_ERR_ARG, "null map"};
    for (int64_t i = 0; i < nb; ++i)
        for (int a = 0; a < 3; ++a)
            if (!rs_map_in_limits(map[6 * i + 2 * a], map[6 * i + 2 * a + 1]))
                throw VhError{VH_ERR_ARG, "every scale must be in [0.25, 4] and every |offset| <= 2^20, both finite (study " +
                                              std::to_string(i) + ")"};
}

static void batch_upload_proton_src(vh_batch *b, const float *src, const int64_t *shape) {
    const size_t n = (size_t)b->nb * (size_t)(shape[0] * shape[1] * shape[2]);
    // no source resident until the new one has arrived whole: a failed growth or copy leaves none
    b->rs_shape[0] = b->rs_shape[1] = b->rs_shape[2] = 0;
    b->d_proton_src.reserve(n);
    HIP_TRY(hipMemcpyAsync(b->d_proton_src, src, sizeof(float) * n, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::copy(shape, shape + 3, b->rs_shape);
    b->state.proton_src_uploaded();
}

static void need_proton_src(const vh_batch *b) {
    b->state.need_proton_src();
    if (b->rs_shape[0] < 1) throw VhError{VH_ERR_ARG, "no proton source resident: its last upload failed"};
}

// The nb x 3 tables on the host, their upload, and the resampling of d_proton_src into d_proton.
static void batch_resample_proton(vh_batch *b, const double *map) {
    need_proton_src(b);
    const int64_t dim[3] = {b->R, b->C, b->Z};
    const int64_t stride = 10 * (b->R + b->C + b->Z);
    std::vector<int32_t> tab((size_t)(b->nb * stride));
    for (int64_t q = 0; q < b->nb; ++q) {
        int32_t *t = tab.data() + q * stride;
        for (int a = 0; a < 3; ++a) {
            const int64_t n = dim[a];
            if (!rs_axis_taps(b->rs_shape[a], n, map[6 * q + 2 * a], map[6 * q + 2 * a + 1], t, t + n,
                              reinterpret_cast<float *>(t + 2 * n)))
                throw VhError{VH_ERR_ARG, "resample: a dimension of the batch is above 2^20"};
            t += 10 * n;
        }
    }
    RsPlan plan;
    if (!vh_resample_plan(b, b->rs_shape, tab.data(), plan))
        throw VhError{VH_ERR_ARG, "resample: more than 65535 studies"};
    b->d_rs_tab.reserve(tab.size());
    b->d_proton.reserve((size_t)b->nb * b->V);
    // (pageable source: the copy has left tab when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_rs_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, b->stream));
    vh_resample_launch(b, plan, b->d_proton_src, b->d_proton, b->d_rs_tab);
    b->state.proton_uploaded();
}

int vh_batch_upload_proton_src(vh_batch *b, const float *src, const int64_t shape[3]) {
    BATCH_TRY(b, {
        if (!src) throw VhError{VH_ERR_ARG, "null buffer"};
        check_resample_shape(shape);
        batch_upload_proton_src(b, src, shape);
    })
}

int vh_batch_resample_proton(vh_batch *b, const double *map) {
    BATCH_TRY(b, {
        check_resample_map(map, b->nb);
        batch_resample_proton(b, map);
    })
}

int vh_batch_download_proton_src(vh_batch *b, float *src) {
    BATCH_TRY(b, {
        if (!src) throw VhError{VH_ERR_ARG, "null buffer"};
        need_proton_src(b);
        d2h_on_stream(b, src, b->d_proton_src,
                      sizeof(float) * (size_t)b->nb * (size_t)(b->rs_shape[0] * b->rs_shape[1] * b->rs_shape[2]));
    })
}

int vh_resample(vh_ctx *ctx, const float *src, const int64_t src_shape[3], int64_t R, int64_t C, int64_t Z,
                int64_t batch, const double *map, float *out) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!src || !out) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_resample_shape(src_shape);
        check_resample_map(map, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload_proton_src(b, src, src_shape);
        batch_resample_proton(b, map);
        d2h_on_stream(b, out, b->d_proton, sizeof(float) * (size_t)batch * b->V);
    })
}

// ---- the fine registration of a device-resident batch (register_maps.hip) -------------------------
// The candidate list of one axis and the pick, on the host alone (register_maps_host.h).
int vh_axis_candidates(double scale0, double offset0, int64_t n_dst, const double *factors, int32_t nf,
                       const double *shifts, int32_t ns, double *out) {
    return rm_axis_candidates(scale0, offset0, n_dst, factors, nf, shifts, ns, out) ? VH_OK : VH_ERR_ARG;
}

int vh_register_maps_pick(const double *score, const int32_t count[3], const int32_t home[3], int32_t best[3]) {
    return rm_pick(score, count, home, best) ? VH_OK : VH_ERR_ARG;
}

// the argument checks of a fine registration (host only: nothing is enqueued before they pass)
static void check_register_maps(const int32_t *count, const double *axis_maps, const int32_t *home, int64_t nb) {
    if (!rm_count_in_limits(count)) throw VhError{VH_ERR_ARG, "count must be 1..17, 1..17, 1..5"};
    if (!axis_maps) throw VhError{VH_ERR_ARG, "null axis_maps"};
    if (!rm_home_in_lists(count, home)) throw VhError{VH_ERR_ARG, "home must lie inside its lists"};
    const int64_t n = (int64_t)count[0] + count[1] + count[2];
    for (int64_t i = 0; i < nb; ++i)
        for (int64_t k = 0; k < n; ++k)
            if (!rs_map_in_limits(axis_maps[2 * (i * n + k)], axis_maps[2 * (i * n + k) + 1]))
                throw VhError{VH_ERR_ARG, "every scale must be in [0.25, 4] and every |offset| <= 2^20, both finite (study " +
                                              std::to_string(i) + ")"};
}

// The tables of every list entry on the host, their upload, the maxima, the xenon codes, the joint
// histogram of every candidate and the scores of d_proton_src against d_hp, then on the host the pick of
// every study; waits.  It writes its own buffers only.
static void batch_register_maps(vh_batch *b, const int32_t *count, const double *axis_maps, const int32_t *home,
                                double *score, int32_t *best, double *best_map, double *best_score,
                                int32_t *status) {
    need_proton_src(b);
    const int64_t dim[3] = {b->R, b->C, b->Z};
    const int64_t nl = (int64_t)count[0] + count[1] + count[2];
    const int64_t stride = 10 * (count[0] * b->R + count[1] * b->C + count[2] * b->Z);
    std::vector<int32_t> tab((size_t)(b->nb * stride));
    for (int64_t q = 0; q < b->nb; ++q) {
        int32_t *t = tab.data() + q * stride;
        const double *m = axis_maps + 2 * q * nl;
        for (int a = 0; a < 3; ++a) {
            const int64_t n = dim[a];
            for (int k = 0; k < count[a]; ++k, m += 2, t += 10 * n)
                if (!rs_axis_taps(b->rs_shape[a], n, m[0], m[1], t, t + n, reinterpret_cast<float *>(t + 2 * n)))
                    throw VhError{VH_ERR_ARG, "register_maps: a dimension of the batch is above 2^20"};
        }
    }
    RmPlan plan;
    if (!vh_register_maps_plan(b, b->rs_shape, count, tab.data(), plan))
        throw VhError{VH_ERR_ARG, "register_maps: batch or tile count out of range"};
    const size_t nb = (size_t)b->nb, nc = (size_t)count[0] * count[1] * count[2];
    b->d_rm_max.reserve(2 * nb);
    b->d_rm_cx.reserve(nb * (size_t)b->V);
    b->d_rm_tab.reserve(tab.size());
    b->d_rm_score.reserve(nb * nc);
    b->rm_nc = 0;   // (a failed growth leaves no histograms to download)
    b->d_rm_hist.reserve(nb * nc * 1024);
    // (pageable source: the copy has left tab when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_rm_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, b->stream));
    vh_register_maps_launch(b, plan, b->d_proton_src, b->d_hp, b->d_rm_tab, b->d_rm_max, b->d_rm_cx, b->d_rm_hist,
                            b->d_rm_score);
    b->rm_nc = (int64_t)nc;
    std::vector<uint32_t> bits(2 * nb);
    HIP_TRY(hipMemcpyAsync(bits.data(), b->d_rm_max, sizeof(uint32_t) * 2 * nb, hipMemcpyDeviceToHost, b->stream));
    d2h_on_stream(b, score, b->d_rm_score, sizeof(double) * nb * nc);
    for (size_t i = 0; i < nb; ++i) {
        float sm, xm;
        memcpy(&sm, &bits[i], sizeof(float));
        memcpy(&xm, &bits[nb + i], sizeof(float));
        int32_t *at = best + 3 * i;
        (void)rm_pick(score + nc * i, count, home, at);
        if (status) status[i] = (sm > 0.0f && xm > 0.0f) ? 0 : 1;
        if (best_map) {
            const double *m = axis_maps + 2 * (int64_t)i * nl;
            const int64_t off[3] = {at[0], count[0] + at[1], count[0] + count[1] + at[2]};
            for (int a = 0; a < 3; ++a) {
                best_map[6 * i + 2 * a] = m[2 * off[a]];
                best_map[6 * i + 2 * a + 1] = m[2 * off[a] + 1];
            }
        }
        if (best_score)
            best_score[i] = score[nc * i + ((size_t)at[2] * count[0] + (size_t)at[0]) * count[1] + (size_t)at[1]];
    }
}

int vh_batch_register_maps(vh_batch *b, const int32_t count[3], const double *axis_maps, const int32_t *home,
                           double *score, int32_t *best, double *best_map, double *best_score, int32_t *status) {
    BATCH_TRY(b, {
        if (!score || !best) throw VhError{VH_ERR_ARG, "null buffer"};
        check_register_maps(count, axis_maps, home, b->nb);
        batch_register_maps(b, count, axis_maps, home, score, best, best_map, best_score, status);
    })
}

int vh_batch_download_register_maps_hist(vh_batch *b, uint32_t *hist) {
    BATCH_TRY(b, {
        if (!hist) throw VhError{VH_ERR_ARG, "null buffer"};
        if (b->rm_nc <= 0) throw VhError{VH_ERR_ARG, "vh_batch_register_maps has not been called"};
        d2h_on_stream(b, hist, b->d_rm_hist, sizeof(uint32_t) * (size_t)b->nb * (size_t)b->rm_nc * 1024);
    })
}

int vh_register_maps(vh_ctx *ctx, const float *src, const int64_t src_shape[3], const float *hp, int64_t R, int64_t C,
                     int64_t Z, int64_t batch, const int32_t count[3], const double *axis_maps, const int32_t *home,
                     double *score, int32_t *best, double *best_map, int32_t *status) {
    if (!ctx) return VH_ERR_ARG;
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!src || !hp || !score || !best) throw VhError{VH_ERR_ARG, "null buffer"};
        check_dims(R, C, Z, batch);
        check_resample_shape(src_shape);
        check_register_maps(count, axis_maps, home, batch);
        vh_batch *b = scratch_batch(ctx, R, C, Z, batch);
        b->profile = ctx->profile != 0;
        batch_upload(b, hp, nullptr);
        batch_upload_proton_src(b, src, src_shape);
        batch_register_maps(b, count, axis_maps, home, score, best, best_map, nullptr, status);
    })
}

// ---- TWIX recon (recon.hip) -------------------------------------------------------------------
int vh_recon(vh_ctx *ctx, const double *k, int64_t n0, int64_t n1, int64_t nz, double *out) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!k || !out) throw VhError{VH_ERR_ARG, "recon: null buffer"};
        if (n0 < 1 || n1 < 1 || nz < 1 || n0 > 5120 || n1 > 5120 || n0 * n1 * nz >= ((int64_t)1 << 31))
            throw VhError{VH_ERR_ARG, "recon: dims must be 1 <= n0, n1 <= 5120, n0 n1 nz < 2^31"};
        HIP_TRY(hipSetDevice(ctx->device));
        if (!ctx->aux) HIP_TRY(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
        const size_t NV = (size_t)(n0 * n1 * nz), bytes = sizeof(double2) * (3 * NV + n0 + n1);
        ctx->recon_buf.reserve(bytes);
        double2 *d_in = (double2 *)ctx->recon_buf.get(), *d_tmp = d_in + NV, *d_out = d_tmp + NV,
                *d_tw0 = d_out + NV, *d_tw1 = d_tw0 + n0;
        hipStream_t st = ctx->aux;
        HIP_TRY(hipMemcpyAsync(d_in, k, sizeof(double2) * NV, hipMemcpyHostToDevice, st));
        vh_recon_run(st, d_in, d_tmp, d_out, d_tw0, d_tw1, n0, n1, nz);
        HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double2) * NV, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    })
}

int vh_link_probe(vh_ctx *ctx, int64_t bytes, double out_gbps[3]) {
    API_TRY(ctx, {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!out_gbps || bytes <= 0) throw VhError{VH_ERR_ARG, "link probe: bad arguments"};
        HIP_TRY(hipSetDevice(ctx->device));
        Buf<char, 1> h_in, h_out;   // (freed after release(), as the scope ends)
        Buf<char> d_in, d_out;
        hipStream_t s[2] = {nullptr, nullptr};
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        auto release = [&]() {
            for (auto e : ev) if (e) (void)hipEventDestroy(e);
            for (auto x : s) if (x) (void)hipStreamDestroy(x);
        };
        try {
            h_in.reserve((size_t)bytes);
            h_out.reserve((size_t)bytes);
            d_in.reserve((size_t)bytes);
            d_out.reserve((size_t)bytes);
            std::memset(h_in, 1, (size_t)bytes);
            std::memset(h_out, 2, (size_t)bytes);
            for (auto &x : s) HIP_TRY(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
            for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
            auto h2d = [&]() { HIP_TRY(hipMemcpyAsync(d_in, h_in, (size_t)bytes, hipMemcpyHostToDevice, s[0])); };
            auto d2h = [&]() { HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)bytes, hipMemcpyDeviceToHost, s[1])); };
            auto best = [&](int mode) {   // 0 H2D, 1 D2H, 2 both: wall time of the copies, best of 3
                double b = 1e30;
                for (int r = 0; r < 4; ++r) {   // the first pass warms up
                    HIP_TRY(hipDeviceSynchronize());
                    const auto t0 = std::chrono::steady_clock::now();
                    if (mode != 1) h2d();
                    if (mode != 0) d2h();
                    HIP_TRY(hipStreamSynchronize(s[0]));
                    HIP_TRY(hipStreamSynchronize(s[1]));
                    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    if (r > 0) b = std::min(b, dt);
                }
                return b;
            };
            const double t1 = best(0), t2 = best(1), t3 = best(2);
            out_gbps[0] = (double)bytes / t1 / 1e9;
            out_gbps[1] = (double)bytes / t2 / 1e9;
            out_gbps[2] = 2.0 * (double)bytes / t3 / 1e9;
        } catch (...) {
            release();
            throw;
        }
        release();
    })
}

int vh_host_alloc(vh_ctx *ctx, int64_t bytes, void **out) {
    if (out) *out = nullptr;
    API_TRY(ctx, {
        if (!out || bytes <= 0) throw VhError{VH_ERR_ARG, "host alloc: bad arguments"};
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, *out, 0) != hipSuccess || !dp) {
            (void)hipGetLastError();
            dp = nullptr;
        }
        if (dp) {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host[(uintptr_t)*out] = {(size_t)bytes, dp};
        }
    })
}

int vh_host_free(void *p) {
    if (p) {
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host.erase((uintptr_t)p);
        }
        (void)hipHostFree(p);
    }
    return VH_OK;
}

int vh_comm_unique_id(uint8_t id[VH_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) <= VH_COMM_ID_BYTES, "nccl id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return VH_ERR_RCCL;
    memcpy(id, &u, sizeof u);
    return VH_OK;
}

int vh_comm_init(vh_ctx *ctx, int nranks, int rank, const uint8_t id[VH_COMM_ID_BYTES]) {
    API_TRY(ctx, {
        HIP_TRY(hipSetDevice(ctx->device));
        ncclUniqueId u;
        memcpy(&u, id, sizeof u);
        ncclComm_t comm;
        ncclResult_t r = ncclCommInitRank(&comm, nranks, u, rank);
        if (r != ncclSuccess) throw VhError{VH_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)};
        ctx->comm = comm;
        ctx->nranks = nranks;
        ctx->rank = rank;
    })
}

int vh_batch_cohort_allreduce(vh_batch *b) {
    BATCH_TRY(b, {
        vh_ctx *c = b->ctx;
        if (!c->comm) throw VhError{VH_ERR_ARG, "vh_comm_init has not been called"};
        if (!c->comm_st) HIP_TRY(hipStreamCreateWithFlags(&c->comm_st, hipStreamNonBlocking));
        if (!b->ev_cpre) HIP_TRY(hipEventCreateWithFlags(&b->ev_cpre, hipEventDisableTiming));
        if (!b->ev_cpost) HIP_TRY(hipEventCreateWithFlags(&b->ev_cpost, hipEventDisableTiming));
        // after this batch's work, on the communicator's stream (program order across batches),
        // and the batch's later work after it
        HIP_TRY(hipEventRecord(b->ev_cpre, b->stream));
        HIP_TRY(hipStreamWaitEvent(c->comm_st, b->ev_cpre, 0));
        ncclResult_t r = ncclAllReduce(b->d_cohort, b->d_cohort, VH_COHORT_BINS, ncclUint64, ncclSum,
                                       (ncclComm_t)c->comm, c->comm_st);
        if (r != ncclSuccess) throw VhError{VH_ERR_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(r)};
        HIP_TRY(hipEventRecord(b->ev_cpost, c->comm_st));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_cpost, 0));
    })
}

int vh_comm_info(vh_ctx *ctx, int *nranks, int *rank) {
    API_TRY(ctx, {
        if (!nranks || !rank) throw VhError{VH_ERR_ARG, "null out"};
        if (!ctx->comm) throw VhError{VH_ERR_ARG, "vh_comm_init has not been called"};
        int n = 0, r = -1;
        ncclResult_t e = ncclCommCount((ncclComm_t)ctx->comm, &n);
        if (e != ncclSuccess) throw VhError{VH_ERR_RCCL, std::string("ncclCommCount: ") + ncclGetErrorString(e)};
        e = ncclCommUserRank((ncclComm_t)ctx->comm, &r);
        if (e != ncclSuccess) throw VhError{VH_ERR_RCCL, std::string("ncclCommUserRank: ") + ncclGetErrorString(e)};
        *nranks = n;
        *rank = r;
    })
}

int vh_comm_destroy(vh_ctx *ctx) {
    if (ctx && ctx->comm) {
        ncclCommDestroy((ncclComm_t)ctx->comm);
        ctx->comm = nullptr;
    }
    return VH_OK;
}

}  // extern "C"
