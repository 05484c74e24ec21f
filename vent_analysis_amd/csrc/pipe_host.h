// pipe_host.h -- the host-to-host pipe's pure host logic (pipe.hip): the staging copies split over
// host threads, the page arithmetic of a caller range, the page-locking budget and the chunk-order
// ticket.  No HIP here: tests/pipe_host_check.cpp builds it with g++ alone under the sanitizers.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#ifndef VH_COPY_THREADS
#define VH_COPY_THREADS 8   // host threads per staging copy (each pipe slot copies on its own)
#endif

// [0, n) cut into at most max_threads non-empty ranges of about chunk bytes or more, every start but
// the first a multiple of align; fn(o, m) takes [o, o + m).  The first range runs on the calling
// thread (alone when n <= chunk), the others on a thread each.
template <class F>
inline void par_ranges(size_t n, size_t chunk, int max_threads, size_t align, F fn) {
    if (!n) return;
    const size_t want = std::min<size_t>((size_t)max_threads, (n + chunk - 1) / chunk);
    const size_t per = ((n + want - 1) / want + align - 1) / align * align;
    std::vector<std::thread> th;
    for (size_t t = 1; t < want && per * t < n; ++t) th.emplace_back(fn, per * t, std::min(per, n - per * t));
    fn((size_t)0, std::min(per, n));
    for (auto &x : th) x.join();
}

// pageable <-> pinned staging copies split over host threads: one thread's memcpy (~5-10 GB/s) bounded
// the whole pipeline at about half the device-resident rate; the copy engines and the
// PCIe link are far from busy at that rate
inline void par_memcpy(void *dst, const void *src, size_t bytes) {
    par_ranges(bytes, (size_t)16 << 20, VH_COPY_THREADS, 1,
               [=](size_t o, size_t m) { memcpy((char *)dst + o, (const char *)src + o, m); });
}

// The mask crosses PCIe as one bit per voxel (bit i % 8 of byte i / 8; the bits past n in the last
// byte are 0).  False (nothing usable in dst) if a byte of src is not 0 / 1.
inline bool par_pack_mask(const uint8_t *src, uint8_t *dst, size_t n) {
    std::atomic<bool> bad{false};
    par_ranges(n, (size_t)8 << 20, VH_COPY_THREADS, 8, [=, &bad](size_t o, size_t m) {   // o a multiple of 8
        uint64_t hi = 0;
        size_t i = o;
        for (; i + 8 <= o + m; i += 8) {
            uint64_t w;
            memcpy(&w, src + i, 8);
            hi |= w;
            dst[i / 8] = (uint8_t)((w * 0x0102040810204080ull) >> 56);   // byte k's bit 0 -> bit k
        }
        if (i < o + m) {
            uint8_t v = 0;
            for (size_t k = 0; i + k < o + m; ++k) {
                hi |= src[i + k];
                v |= (uint8_t)((src[i + k] & 1u) << k);
            }
            dst[i / 8] = v;
        }
        if (hi & 0xFEFEFEFEFEFEFEFEull) bad = true;
    });
    return !bad;
}

// the caller's maps from the packed bytes, defect | border << 1 | LB class << 2 (any of d / b / l may
// be null)
inline void par_unpack_maps(const uint8_t *src, uint8_t *d, uint8_t *b, uint8_t *l, size_t n) {
    par_ranges(n, (size_t)8 << 20, VH_COPY_THREADS, 1, [=](size_t o, size_t m) {
        for (size_t i = o; i < o + m; ++i) {
            const uint8_t v = src[i];
            if (d) d[i] = v & 1u;
            if (b) b[i] = (v >> 1) & 1u;
            if (l) l[i] = v >> 2;
        }
    });
}

// First touch of a caller's output pages on several host threads (hipHostRegister would otherwise
// fault in and zero every untouched page on the calling thread: measured 3.8k vs 5.1k vol/s staged)
inline void par_touch(void *dst, size_t bytes) {
    const size_t page = 4096;
    par_ranges(bytes, (size_t)64 << 20, 2 * VH_COPY_THREADS, page, [=](size_t o, size_t m) {
        volatile char *q = (volatile char *)dst + o;
        for (size_t i = 0; i < m; i += page) q[i] = q[i];
    });
}

// The bytes [s0, s0 + n) of a caller buffer as head + body + tail: the body is the range's whole
// 4096-byte pages, the head and the tail the fragments (< 1 page each) before and after it.  Only an
// eligible body, 1 MiB or more, is worth page-locking.  Consecutive ranges of one buffer never share
// a body page, wherever they are cut.
struct PagePlan {
    size_t head, body_bytes, tail;
    uintptr_t body;   // a page boundary
    bool eligible;
};
inline PagePlan page_plan(uintptr_t s0, size_t n) {
    const uintptr_t pg = 4096, e0 = s0 + n, a = (s0 + pg - 1) / pg * pg, e = e0 / pg * pg;
    PagePlan pl;
    pl.body = a;
    pl.body_bytes = e > a ? e - a : 0;
    pl.head = std::min<size_t>(a - s0, n);
    pl.tail = n - pl.head - pl.body_bytes;
    pl.eligible = pl.body_bytes >= ((size_t)1 << 20);
    return pl;
}

// Caller bytes page-locked in place at one time (used), capped: take() refuses what would pass the
// cap and leaves the count as it was.  peak: the highest count since it was last set.
struct PinBudget {
    int64_t cap = 0;
    std::atomic<int64_t> used{0}, peak{0};
    bool take(int64_t bytes) {
        int64_t cur = used.load();
        do {
            if (cur + bytes > cap) return false;
        } while (!used.compare_exchange_weak(cur, cur + bytes));
        int64_t pk = peak.load();
        while (cur + bytes > pk && !peak.compare_exchange_weak(pk, cur + bytes)) {
        }
        return true;
    }
    void give(int64_t bytes) { used.fetch_sub(bytes); }
};

struct PipeAbort {};   // a pipe slot stopped because another slot failed

// Chunk order across the slot threads: wait(k) returns when chunk k is the current one, pass(k) makes
// k + 1 current.  After abort() every wait throws PipeAbort, but the one whose turn it already is.
class ChunkTicket {
    std::mutex mu;
    std::condition_variable cv;
    int64_t next = 0;
    bool aborted = false;

  public:
    void wait(int64_t k) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return next == k || aborted; });
        if (next != k) throw PipeAbort{};
    }
    void pass(int64_t k) {   // (a chunk that is not the current one changes nothing)
        {
            std::lock_guard<std::mutex> lk(mu);
            if (next == k) next = k + 1;
        }
        cv.notify_all();
    }
    void abort() {
        {
            std::lock_guard<std::mutex> lk(mu);
            aborted = true;
        }
        cv.notify_all();
    }
};
