// pipe.hip -- the host-to-host pipeline (vh_pipe_*): n host studies streamed through `slots` batches
// of `sub` studies.  One host thread per slot; slot s owns batch b[s] (its own stream) and pinned
// staging, and takes sub-batches s, s + slots, ...  Within a slot the steps are serial (stage in ->
// H2D -> pipeline -> D2H -> stage out); across slots they overlap, so the copy engines, the host
// memcpys and the compute of different sub-batches run at the same time.  The host threads' own
// logic (split copies, page arithmetic, pin budget, chunk ticket) is pipe_host.h.
#include <chrono>
#include <memory>

#include "vh_internal.h"
#include "pipe_host.h"

// The three u8 maps of a pipe chunk leave the GPU as one byte per voxel, defect | border << 1 |
// LB class << 2 (0/1, 0/1, 0..6): PCIe carries H2D and D2H together at ~53 GB/s on the box
// (scripts/dev/h2h_probe.py, both directions at once), so the host-to-host rate is link-bound
// near the device rate; this takes 12 -> 10 bytes per voxel.  The slot's host threads unpack.
__global__ void k_pack_maps(const uint8_t *__restrict__ d, const uint8_t *__restrict__ b,
                            const uint8_t *__restrict__ l, uint8_t *__restrict__ out, int64_t n,
                            const uint32_t *__restrict__ sc, int64_t sc_words,
                            const uint32_t *__restrict__ st, int64_t st_words, uint32_t *__restrict__ scal) {
    // the chunk's scalars and N4 states ahead of the maps (the D2H block's head)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sc_words + st_words;
         i += (int64_t)gridDim.x * blockDim.x)
        scal[i] = i < sc_words ? sc[i] : st[i - sc_words];
    const int64_t n16 = n / 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 vd = reinterpret_cast<const uint4 *>(d)[i], vb = reinterpret_cast<const uint4 *>(b)[i],
                    vl = reinterpret_cast<const uint4 *>(l)[i];
        uint4 o;   // bytes pack lane-wise: no carries (defect, border <= 1, class <= 6)
        o.x = vd.x | (vb.x << 1) | (vl.x << 2);
        o.y = vd.y | (vb.y << 1) | (vl.y << 2);
        o.z = vd.z | (vb.z << 1) | (vl.z << 2);
        o.w = vd.w | (vb.w << 1) | (vl.w << 2);
        reinterpret_cast<uint4 *>(out)[i] = o;
    }
    for (int64_t i = n16 * 16 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)(d[i] | (b[i] << 1) | (l[i] << 2));
}

// studies cnt .. sub - 1 of a ragged pipe chunk := study cnt - 1 (image and mask)
__global__ void k_repeat_last(float *hp, uint8_t *mask, int64_t V, int64_t cnt, int64_t sub) {
    const int64_t n = (sub - cnt) * V;
    const float *sh = hp + (cnt - 1) * V;
    const uint8_t *sm = mask + (cnt - 1) * V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = i % V;
        hp[cnt * V + i] = sh[v];
        mask[cnt * V + i] = sm[v];
    }
}

// par_pack_mask's bits (pipe_host.h) back to the mask bytes on the device
__global__ void k_unpack_mask(const uint8_t *__restrict__ bits, uint8_t *__restrict__ mask, int64_t n) {
    const int64_t nb = (n + 7) / 8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t v = bits[i];
        if (i * 8 + 8 <= n) {
            uint64_t w = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) w |= (uint64_t)((v >> k) & 1u) << (8 * k);
            memcpy(mask + i * 8, &w, 8);
        } else {
            for (int64_t k = 0; i * 8 + k < n; ++k) mask[i * 8 + k] = (uint8_t)((v >> k) & 1u);
        }
    }
}

struct vh_pipe {
    struct Slot {
        vh_batch *b = nullptr;
        Buf<float, 1> hp, n4;                 // pinned staging [sub][V]
        Buf<uint8_t, 1> u8;                   // pinned: mask in [sub][V], then the D2H block (scal + [sub][V])
        hipEvent_t done = nullptr;            // recorded after the slot's current chunk's pipeline
        hipEvent_t h2d = nullptr;             // recorded after the slot's current chunk's H2D
        hipEvent_t packed = nullptr;          // recorded after the chunk's output packing (its D2H may start)
        Buf<uint8_t> d_pack;                  // device: the chunk's D2H block: scalars (scal bytes), packed maps
        size_t scal = 0;                      // bytes of the per-study scalars + N4 states block (4 KiB multiple)
        Buf<uint8_t, 1> mb;                   // pinned: mask bits, two chunks' worth (double buffer)
        size_t mb_half = 0;
        VolScalars *sc = nullptr;             // the chunk's per-study scalars / N4 states: views into u8
        N4State *st = nullptr;
        std::vector<vh_vdp_result> res;
    };
    vh_ctx *ctx = nullptr;
    int64_t R = 0, C = 0, Z = 0, sub = 0;
    std::vector<Slot> slot;
    // caller pages pinned in place during a run (released at its end), capped at pins.cap bytes
    // (VH_PIPE_PIN_CAP, default 32 GiB / LOCAL_WORLD_SIZE): past the cap a range goes through the
    // pinned staging and is counted in staged_spans (vh_pipe_stats)
    PinBudget pins;
    std::atomic<int64_t> staged_spans{0};
};

static void pipe_free(vh_pipe *p) {
    if (!p) return;
    for (auto &q : p->slot) {
        if (q.b) {
            (void)hipStreamSynchronize(q.b->stream);
            vh_free_batch(q.b);
        }
        if (q.done) (void)hipEventDestroy(q.done);
        if (q.h2d) (void)hipEventDestroy(q.h2d);
        if (q.packed) (void)hipEventDestroy(q.packed);
    }
    delete p;   // the slots' staging buffers
}

static bool pipe_stage_all() { return getenv("VH_PIPE_STAGE") != nullptr; }   // no caller page is pinned

// Host buffers the copy engines may read / write in place: hipHostRegister pins the caller's pages
// (the page tables only; measured ~0.4-0.5 TB/s on the box, scripts/dev/h2h_probe.py) and the DMA
// then runs at the link rate with no staging memcpy on a host thread.  A buffer that cannot be
// registered (e.g. pages already registered, past the budget, or VH_PIPE_STAGE=1) goes through the
// pinned staging.
struct HostPin {
    void *p = nullptr;
    size_t n = 0;
    PinBudget *owner = nullptr;   // the budget this registration counts against
    HostPin() = default;
    HostPin(const HostPin &) = delete;
    HostPin &operator=(const HostPin &) = delete;
    bool pin(void *ptr, size_t bytes, bool touch, PinBudget &pins) {
        if (pipe_stage_all() || !pins.take((int64_t)bytes)) return false;
        if (touch) par_touch(ptr, bytes);
        if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            pins.give((int64_t)bytes);
            return false;
        }
        p = ptr;
        n = bytes;
        owner = &pins;
        return true;
    }
    ~HostPin() {
        if (p) {
            (void)hipHostUnregister(p);
            owner->give((int64_t)n);
        }
    }
};

// One caller range of a pipe chunk: h bytes through the slot's pinned staging (at the same offsets),
// then whole pages pinned and DMA'd in place, then t bytes through the staging.  Only whole pages are
// pinned: a page the range shares with the neighbouring chunk or another buffer must never be
// registered twice or unregistered under another range's copy, so a pinned range's head and tail
// fragments (< 1 page each, page_plan) are staged.  A range that cannot be pinned is all head.
struct PipeSpan {
    char *p = nullptr;
    size_t n = 0, h = 0, t = 0;
    HostPin pin;
    void plan(const void *ptr, size_t bytes, bool touch, vh_pipe *pp) {
        p = (char *)ptr;
        n = h = ptr ? bytes : 0;
        const PagePlan pl = page_plan((uintptr_t)p, n);
        if (!pl.eligible) return;   // small: staged
        if (!pin.pin((void *)pl.body, pl.body_bytes, touch, pp->pins)) {
            pp->staged_spans.fetch_add(1);
            return;
        }
        h = pl.head;
        t = pl.tail;
    }
    void h2d(char *dst, char *stage, hipStream_t st) {
        if (h) {
            par_memcpy(stage, p, h);
            HIP_TRY(hipMemcpyAsync(dst, stage, h, hipMemcpyHostToDevice, st));
        }
        if (n - h - t) HIP_TRY(hipMemcpyAsync(dst + h, p + h, n - h - t, hipMemcpyHostToDevice, st));
        if (t) {
            memcpy(stage + n - t, p + n - t, t);
            HIP_TRY(hipMemcpyAsync(dst + n - t, stage + n - t, t, hipMemcpyHostToDevice, st));
        }
    }
    void d2h(const char *src, char *stage, hipStream_t st) {
        if (h) HIP_TRY(hipMemcpyAsync(stage, src, h, hipMemcpyDeviceToHost, st));
        if (n - h - t) HIP_TRY(hipMemcpyAsync(p + h, src + h, n - h - t, hipMemcpyDeviceToHost, st));
        if (t) HIP_TRY(hipMemcpyAsync(stage + n - t, src + n - t, t, hipMemcpyDeviceToHost, st));
    }
    void d2h_finish(const char *stage) {   // after the stream sync
        if (h) par_memcpy(p, stage, h);
        if (t) memcpy(p + n - t, stage + n - t, t);
    }
};

struct PipeArgs {   // vh_pipe_run's arguments: host arrays of n studies (every output may be null)
    const float *hp;
    const uint8_t *mask;
    int64_t n;
    const vh_run_opts *opts;
    float *n4;
    uint8_t *defect, *border, *lb;
    vh_vdp_result *res;
};

// One vh_pipe_run.  Per slot, chunk by chunk: prep (host: pin the input pages, pack the mask bits)
// -> front (enqueue H2D, the pipeline behind its ticket and lag event, the map packing) -> back_pin
// (first-touch + pin the n4 output pages) -> back (enqueue the D2Hs) -> sync -> finish (results,
// fragments, map unpacking).  The next chunk's prep runs before this chunk's sync and its front
// right after it, so the host work of finish overlaps the next chunk's H2D and compute (its D2H is
// enqueued after finish: the staging it writes is free by then).
struct PipeRun : PipeArgs {
    // VH_PIPE_TRACE=1: per chunk, host times (ms from the start) of the input pin + H2D enqueue, the
    // pipeline enqueue, the output pin, the sync, and device times of H2D / compute / D2H ends (stderr)
    struct Mark {
        int64_t k;
        double h[5];
        hipEvent_t e[3];
    };
    struct Chunk {
        int64_t k = -1, v0 = 0, cnt = 0;
        size_t CV = 0;
        PipeSpan *sp = nullptr;   // image in, mask bytes in, n4 out
        bool mbits = false;
        uint8_t *mb = nullptr;
        Mark mk{};
    };
    vh_pipe *const p;
    const int64_t V, sub, nchunk;
    const int slots;
    const bool maps, trace;
    int lag = 0;
    ChunkTicket ticket;   // the chunk whose pipeline is enqueued next
    std::vector<VhError> err;
    std::vector<int> failed;
    // the spans' pins are released only after the whole run (hipHostUnregister waits for the
    // device: released per chunk, it lined every slot up behind the others)
    std::vector<std::vector<std::unique_ptr<PipeSpan[]>>> keep;
    std::vector<std::vector<Mark>> marks;
    hipEvent_t ev0 = nullptr;
    const std::chrono::steady_clock::time_point c0 = std::chrono::steady_clock::now();

    PipeRun(vh_pipe *p_, const PipeArgs &a)
        : PipeArgs(a), p(p_), V(p_->R * p_->C * p_->Z), sub(p_->sub), nchunk((a.n + p_->sub - 1) / p_->sub),
          slots((int)p_->slot.size()), maps(a.defect || a.border || a.lb), trace(getenv("VH_PIPE_TRACE") != nullptr),
          err(slots), failed(slots, 0), keep(slots), marks(slots) {
        // Chunk k's pipeline waits on the device for chunk k - lag's (lag = the chunks that fill the
        // CUs, VH_PIPE_LAG overrides; 0 = no ordering).  Without it the slots ran in lockstep: all
        // computing together, then all copying out / in together with the GPU idle (~60% of the
        // device rate, VH_PIPE_TRACE); with it the computes are staggered and each chunk's copies
        // overlap the next chunks' compute.  Enqueues happen in chunk order (host-side ticket).
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->ctx->device);
        lag = (int)std::max<int64_t>(1, (cus + sub - 1) / sub);
        if (const char *e = getenv("VH_PIPE_LAG")) lag = atoi(e);
        lag = std::min(lag, slots);
    }

    double now_ms() const {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    }
    void mark_ev(Mark &m, int i, hipStream_t st) const {
        if (trace && hipEventCreate(&m.e[i]) == hipSuccess) (void)hipEventRecord(m.e[i], st);
    }

    void prep(int s, Chunk &c, int64_t k) {
        vh_pipe::Slot &q = p->slot[s];
        c.k = k;
        c.v0 = k * sub;
        c.cnt = std::min(sub, n - c.v0);
        c.CV = (size_t)c.cnt * V;
        c.mk = Mark{k, {now_ms(), 0, 0, 0, 0}, {nullptr, nullptr, nullptr}};
        keep[s].emplace_back(new PipeSpan[3]);
        c.sp = keep[s].back().get();
        c.sp[0].plan(hp + c.v0 * V, sizeof(float) * c.CV, false, p);
        c.mb = q.mb + ((k / slots) & 1) * q.mb_half;   // bits double-buffered across chunks
        c.mbits = !pipe_stage_all() && par_pack_mask(mask + c.v0 * V, c.mb, c.CV);
        if (!c.mbits) c.sp[1].plan(mask + c.v0 * V, c.CV, false, p);
    }

    // No copy is enqueued before what it depends on has finished (host-side waits): a copy enqueued
    // behind unfinished work waits on the DMA engine's queue and holds back every later copy of that
    // engine -- an H2D stuck behind another chunk's D2H that waits for a kernel which waits for a CU
    // (r4b trace: 30 ms stalls).  So the H2Ds run in chunk order, each after the one before has
    // finished: at the start the first chunks' inputs get the whole link instead of every slot's
    // sharing it.
    void front(int s, Chunk &c) {
        vh_pipe::Slot &q = p->slot[s];
        vh_batch *b = q.b;
        ticket.wait(c.k);   // enqueues in chunk order
        try {
            if (c.k > 0) HIP_TRY(hipEventSynchronize(p->slot[(c.k - 1) % slots].h2d));
            // the copies first (the event marks their end), then the kernels that consume them
            c.sp[0].h2d((char *)b->d_hp.get(), (char *)q.hp.get(), b->stream);
            if (c.mbits) HIP_TRY(hipMemcpyAsync(q.d_pack, c.mb, (c.CV + 7) / 8, hipMemcpyHostToDevice, b->stream));
            else c.sp[1].h2d((char *)b->d_mask.get(), (char *)q.u8.get(), b->stream);   // (the byte fallback)
            HIP_TRY(hipEventRecord(q.h2d, b->stream));
            if (c.mbits) {
                k_unpack_mask<<<(unsigned)std::min<int64_t>(4096, ((int64_t)(c.CV + 7) / 8 + 255) / 256), 256, 0,
                                b->stream>>>(q.d_pack, b->d_mask, (int64_t)c.CV);
                HIP_TRY(hipGetLastError());
            }
            if (c.cnt < sub) {   // ragged tail: repeat the last study (a kernel, not DMA copies)
                k_repeat_last<<<(unsigned)std::min<int64_t>(4096, (sub - c.cnt) * (V / 4 + 255) / 256 + 1), 256, 0,
                                b->stream>>>(b->d_hp, b->d_mask, V, c.cnt, sub);
                HIP_TRY(hipGetLastError());
            }
            mark_ev(c.mk, 0, b->stream);
            c.mk.h[1] = now_ms();
            if (lag > 0 && c.k >= lag) HIP_TRY(hipStreamWaitEvent(b->stream, p->slot[(c.k - lag) % slots].done, 0));
            vh_run_batch(b, *opts, opts->do_n4 ? 0 : 1);
            HIP_TRY(hipEventRecord(q.done, b->stream));
        } catch (...) {   // the chunks behind this one are not left waiting for its turn to end
            ticket.pass(c.k);
            throw;
        }
        ticket.pass(c.k);
        mark_ev(c.mk, 1, b->stream);
        c.mk.h[2] = now_ms();
        if (maps || res) {   // scalars + the three maps packed into one byte per voxel
            const int64_t cvm = maps ? (int64_t)c.CV : 0;
            const int64_t scw = (int64_t)(sizeof(VolScalars) * sub / 4);
            const int64_t stw = opts->do_n4 ? (int64_t)(sizeof(N4State) * sub / 4) : 0;
            k_pack_maps<<<(unsigned)std::min<int64_t>(4096, (cvm / 16 + 255) / 256 + 1), 256, 0, b->stream>>>(
                b->d_defect, b->d_border, b->d_lb, q.d_pack + q.scal, cvm,
                reinterpret_cast<const uint32_t *>(b->d_sc.get()), scw,
                reinterpret_cast<const uint32_t *>(b->d_st.get()), stw, reinterpret_cast<uint32_t *>(q.d_pack.get()));
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(q.packed, b->stream));
    }

    void back_pin(Chunk &c) {   // while the chunk computes: first touch + pin of its output pages
        c.sp[2].plan(n4 ? n4 + c.v0 * V : nullptr, sizeof(float) * c.CV, true, p);
    }

    // The D2Hs, enqueued only once the chunk's packing kernel has finished (the host waits; not just
    // the pipeline: the packing may itself wait for a free CU), by the rule stated at front:
    // a D2H enqueued earlier would sit on its DMA engine's queue in front of other chunks' copies.
    void back(int s, Chunk &c) {
        vh_pipe::Slot &q = p->slot[s];
        vh_batch *b = q.b;
        HIP_TRY(hipEventSynchronize(q.packed));
        const float *dn4 = opts->do_n4 ? b->d_n4 : b->d_hp;
        c.sp[2].d2h((const char *)dn4, (char *)q.n4.get(), b->stream);
        if (maps || res)   // one D2H: the scalars / states block, then the packed maps
            HIP_TRY(hipMemcpyAsync(q.u8 + sub * V, q.d_pack, q.scal + (maps ? c.CV : 0), hipMemcpyDeviceToHost,
                                   b->stream));
        mark_ev(c.mk, 2, b->stream);
        c.mk.h[3] = now_ms();
    }

    void finish(int s, Chunk &c) {
        vh_pipe::Slot &q = p->slot[s];
        if (res) {
            vh_fill_results(q.b, q.sc, q.st, q.res.data());
            memcpy(res + c.v0, q.res.data(), sizeof(vh_vdp_result) * c.cnt);
        }
        c.sp[2].d2h_finish((const char *)q.n4.get());
        if (maps)   // the D2H block in u8: the mask bytes, the scalars / states, then the packed maps
            par_unpack_maps(q.u8 + sub * V + q.scal, defect ? defect + c.v0 * V : nullptr,
                            border ? border + c.v0 * V : nullptr, lb ? lb + c.v0 * V : nullptr, c.CV);
        if (trace) marks[s].push_back(c.mk);
    }

    void slot_loop(int s) {
        hipStream_t st = p->slot[s].b->stream;
        try {
            HIP_TRY(hipSetDevice(p->ctx->device));
            Chunk cur, nxt;
            if (s < nchunk) try {
                prep(s, cur, s);
                front(s, cur);
                for (;;) {
                    const int64_t kn = cur.k + slots;
                    if (kn < nchunk) prep(s, nxt, kn);   // host work while the GPU has cur
                    back_pin(cur);
                    back(s, cur);
                    HIP_TRY(hipStreamSynchronize(st));
                    cur.mk.h[4] = now_ms();
                    if (kn < nchunk) front(s, nxt);      // the next chunk's H2D + compute first
                    finish(s, cur);                      // then this chunk's host side
                    if (kn >= nchunk) break;
                    cur = nxt;
                }
            } catch (...) {   // no copy may still touch a pinned range when it is released
                (void)hipStreamSynchronize(st);
                throw;
            }
        } catch (const PipeAbort &) {   // another slot's failure is the one reported
            failed[s] = 2;
        } catch (const VhError &e) {
            err[s] = e;
            failed[s] = 1;
            ticket.abort();
        } catch (const std::exception &e) {
            err[s] = VhError{VH_ERR_HIP, e.what()};
            failed[s] = 1;
            ticket.abort();
        }
    }

    void print_trace() {
        fprintf(stderr, "pipe_trace total_ms %.2f\n", now_ms());
        for (int s = 0; s < slots; ++s)
            for (Mark &m : marks[s]) {
                float d[3] = {-1, -1, -1};
                for (int i = 0; i < 3; ++i)
                    if (m.e[i]) {
                        (void)hipEventElapsedTime(&d[i], ev0, m.e[i]);
                        (void)hipEventDestroy(m.e[i]);
                    }
                fprintf(stderr, "pipe_trace slot %d chunk %lld host %.2f %.2f %.2f %.2f %.2f dev %.2f %.2f %.2f\n", s,
                        (long long)m.k, m.h[0], m.h[1], m.h[2], m.h[3], m.h[4], d[0], d[1], d[2]);
            }
        (void)hipEventDestroy(ev0);
    }

    // the slot threads, then the first slot's error if one failed
    void run() {
        p->pins.peak = 0;
        p->staged_spans = 0;
        if (trace) {
            HIP_TRY(hipEventCreate(&ev0));
            HIP_TRY(hipEventRecord(ev0, p->slot[0].b->stream));
        }
        std::vector<std::thread> th;
        for (int s = 1; s < slots; ++s) th.emplace_back([this, s] { slot_loop(s); });
        slot_loop(0);
        for (auto &t : th) t.join();
        for (int s = 0; s < slots; ++s)   // no copy may still touch a pinned buffer when it is released
            (void)hipStreamSynchronize(p->slot[s].b->stream);
        keep.clear();
        if (trace) print_trace();
        for (int s = 0; s < slots; ++s)
            if (failed[s] == 1) throw err[s];
    }
};

extern "C" {

int vh_pipe_create(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t sub, int slots, vh_pipe **out) {
    *out = nullptr;
    API_TRY(ctx, {
        if (sub < 1 || slots < 1 || slots > 8) throw VhError{VH_ERR_ARG, "pipe: sub >= 1, 1 <= slots <= 8"};
        HIP_TRY(hipSetDevice(ctx->device));
        vh_pipe *p = new vh_pipe;
        p->ctx = ctx;
        p->R = R; p->C = C; p->Z = Z; p->sub = sub;
        // a per-node budget of 32 GiB page-locked, shared by the node's ranks (LOCAL_WORLD_SIZE, as
        // torchrun and bench.py set it): 8 ranks pin at most 4 GiB each
        int64_t local_ranks = 1;
        if (const char *e = getenv("LOCAL_WORLD_SIZE")) local_ranks = std::max<int64_t>(1, atoll(e));
        p->pins.cap = ((int64_t)32 << 30) / local_ranks;
        if (const char *e = getenv("VH_PIPE_PIN_CAP")) p->pins.cap = atoll(e);
        const size_t NV = (size_t)sub * R * C * Z;
        try {
            for (int s = 0; s < slots; ++s) {
                p->slot.emplace_back();
                vh_pipe::Slot &q = p->slot.back();
                q.b = vh_new_batch(ctx, R, C, Z, sub);
                q.hp.reserve(NV);
                q.n4.reserve(NV);
                // the chunk's outputs leave the GPU as ONE copy: the per-study scalars and N4 states,
                // then the packed maps.  Small copies (the scalars were two of ~20 / 11 KiB) run as
                // blit kernels (__amd_rocclr_copyBuffer), which wait for a CU like any kernel -- for
                // milliseconds while k_n4_study holds every CU's LDS (r4a trace); one large copy
                // goes to the SDMA engines.
                q.scal = (sizeof(VolScalars) * sub + sizeof(N4State) * sub + 4095) / 4096 * 4096;
                q.u8.reserve(2 * NV + q.scal);   // mask in | scalars + maps out
                HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&q.h2d, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&q.packed, hipEventDisableTiming));
                q.d_pack.reserve((size_t)NV + q.scal);
                q.mb_half = ((size_t)NV / 8 + 1 + 63) / 64 * 64;
                q.mb.reserve(2 * q.mb_half);
                q.sc = reinterpret_cast<VolScalars *>(q.u8 + NV);
                q.st = reinterpret_cast<N4State *>(q.u8 + NV + sizeof(VolScalars) * sub);
                q.res.resize(sub);
            }
        } catch (...) {
            pipe_free(p);
            throw;
        }
        *out = p;
    })
}

int vh_pipe_run(vh_pipe *p, const float *hp, const uint8_t *mask, int64_t n, const vh_run_opts *opts,
                float *n4, uint8_t *defect, uint8_t *defect_border, uint8_t *lb, vh_vdp_result *res) {
    if (!p) return VH_ERR_ARG;
    API_TRY(p->ctx, {
        if (!opts || !hp || !mask || n < 1) throw VhError{VH_ERR_ARG, "pipe: null input or n < 1"};
        HIP_TRY(hipSetDevice(p->ctx->device));
        PipeRun(p, {hp, mask, n, opts, n4, defect, defect_border, lb, res}).run();
    })
}

int vh_pipe_stats(vh_pipe *p, int64_t *pinned_peak_bytes, int64_t *staged_spans) {
    if (!p) return VH_ERR_ARG;
    if (pinned_peak_bytes) *pinned_peak_bytes = p->pins.peak.load();
    if (staged_spans) *staged_spans = p->staged_spans.load();
    return VH_OK;
}

int vh_pipe_destroy(vh_pipe *p) {
    if (p) {
        (void)hipSetDevice(p->ctx->device);
        pipe_free(p);
    }
    return VH_OK;
}

}   // extern "C"
