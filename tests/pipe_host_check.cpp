// The host-to-host pipe's host logic (vent_analysis_amd/csrc/pipe_host.h, the header pipe.hip
// includes): the range splitter and the four split helpers against bytewise references, the page
// plan of a caller range, the pin budget and the chunk ticket under threads.  Built twice by
// tests/test_pipe_host.py: with -fsanitize=address,undefined and with -fsanitize=thread.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "pipe_host.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

using Bytes = std::vector<uint8_t>;
static const size_t MiB = (size_t)1 << 20;

// ok(i) for every i < n, on host threads (the splitter is checked on its own below)
template <class F>
static bool all_of_index(size_t n, F ok) {
    std::atomic<bool> good{true};
    par_ranges(n, MiB, 8, 1, [&](size_t o, size_t m) {
        for (size_t i = o; i < o + m; ++i)
            if (!ok(i)) good = false;
    });
    return good;
}

// ---- the splitter: disjoint, in order, covering [0, n); aligned starts; at most max_threads ranges
static void check_ranges() {
    const size_t ns[] = {0, 1, 7, 8, 9, 4095, 4096, 4097, 100000, MiB + 3};
    const size_t chunks[] = {1, 8, 4096, 65536};
    const int threads[] = {1, 2, 3, 8, 16};
    const size_t aligns[] = {1, 8, 4096};
    for (size_t n : ns)
        for (size_t chunk : chunks)
            for (int mt : threads)
                for (size_t align : aligns) {
                    std::mutex mu;
                    std::vector<std::pair<size_t, size_t>> got;
                    par_ranges(n, chunk, mt, align, [&](size_t o, size_t m) {
                        std::lock_guard<std::mutex> g(mu);
                        got.emplace_back(o, m);
                    });
                    std::sort(got.begin(), got.end());
                    CHECK(got.empty() == (n == 0) && got.size() <= (size_t)mt);
                    if (n && n <= chunk) CHECK(got.size() == 1);
                    size_t at = 0;
                    for (size_t i = 0; i < got.size(); ++i) {
                        CHECK(got[i].first == at);
                        CHECK(got[i].second > 0 && (i == 0 || got[i].first % align == 0));
                        at += got[i].second;
                    }
                    CHECK(at == n);
                }
}

// ---- par_pack_mask against a bytewise reference; a byte that is not 0 / 1 anywhere refuses
static uint8_t mask_at(size_t i) { return (uint8_t)(((i * 2654435761u) >> 7) & 1u); }

static void check_pack_mask() {
    const size_t task = 8 * MiB, big = 2 * task + 5;   // three tasks, the last with a ragged tail
    const size_t ns[] = {0, 1, 7, 8, 9, 63, 64, 65, big};
    for (size_t n : ns) {
        Bytes src(n), dst((n + 7) / 8, 0xAA);
        for (size_t i = 0; i < n; ++i) src[i] = mask_at(i);
        CHECK(par_pack_mask(src.data(), dst.data(), n));
        CHECK(all_of_index(dst.size(), [&](size_t j) {   // (the bits past n in the last byte are 0)
            uint8_t v = 0;
            for (size_t k = 0; k < 8 && j * 8 + k < n; ++k) v |= (uint8_t)(src[j * 8 + k] << k);
            return dst[j] == v;
        }));
        if (n != big) continue;
        const size_t want = (n + task - 1) / task, per = ((n + want - 1) / want + 7) / 8 * 8;
        CHECK(want == 3 && per * 2 < n && (n - per * 2) % 8 != 0);
        const size_t body_end = per * 2 + (n - per * 2) / 8 * 8;   // of the last task
        const size_t at[] = {3, body_end - 3, n - 2};              // first task, last body, ragged tail
        CHECK(at[1] >= per * 2 && at[2] >= body_end);
        for (size_t pos : at)
            for (uint8_t v : {(uint8_t)2, (uint8_t)255}) {
                const uint8_t was = src[pos];
                src[pos] = v;
                CHECK(!par_pack_mask(src.data(), dst.data(), n));
                src[pos] = was;
            }
        CHECK(par_pack_mask(src.data(), dst.data(), n));
    }
}

// The program's own fills and comparisons of whole buffers, single-threaded between the calls under
// test, are left uninstrumented in the thread-sanitizer build: instrumented bytewise they take minutes.
#if defined(__SANITIZE_THREAD__)
#define PLAIN __attribute__((no_sanitize("thread")))
#else
#define PLAIN
#endif
PLAIN static uint8_t packed_at(size_t i) { return (uint8_t)(i % 28); }   // defect | border << 1 | class (<= 6) << 2
PLAIN static uint8_t defect_at(size_t i) { return packed_at(i) & 1; }
PLAIN static uint8_t border_at(size_t i) { return (packed_at(i) >> 1) & 1; }
PLAIN static uint8_t class_at(size_t i) { return packed_at(i) / 4; }
PLAIN static uint8_t pat(size_t i) { return (uint8_t)(i * 131 + (i >> 12)); }
template <uint8_t (*F)(size_t)>
PLAIN static void fill(uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) p[i] = F(i);
}
template <uint8_t (*F)(size_t)>
PLAIN static bool holds(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != F(i)) return false;
    return true;
}

// n bytes that nothing has written yet, and one guard byte behind them
struct Raw {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Raw(size_t n_) : p(new uint8_t[n_ + 1]), n(n_) { p[n] = 0xEE; }
    uint8_t *data() { return p.get(); }
    bool guard_ok() const { return p[n] == 0xEE; }
};

// ---- par_unpack_maps: every byte value 0 .. 27; every combination of null and non-null outputs at
// the small sizes; all outputs, and one with nulls, on both sides of one task and of several
static void check_unpack_maps() {
    const size_t task = 8 * MiB;
    const size_t ns[] = {0, 1, 27, 28, 4099, task, task + 1, 2 * task + 1};   // (1, 2 and 3 tasks)
    for (size_t n : ns)
        for (int combo = 0; combo < 8; ++combo) {
            if (n >= task && combo != 7 && !(combo == 2 && n == task + 1)) continue;
            Raw src(n), d(n), b(n), l(n);
            fill<packed_at>(src.data(), n);
            par_unpack_maps(src.data(), combo & 1 ? d.data() : nullptr, combo & 2 ? b.data() : nullptr,
                            combo & 4 ? l.data() : nullptr, n);
            CHECK(!(combo & 1) || holds<defect_at>(d.data(), n));
            CHECK(!(combo & 2) || holds<border_at>(b.data(), n));
            CHECK(!(combo & 4) || holds<class_at>(l.data(), n));
            CHECK(d.guard_ok() && b.guard_ok() && l.guard_ok());
        }
}

// ---- par_memcpy copies, par_touch changes nothing
static void check_memcpy_touch() {
    const size_t ctask = 16 * MiB, ttask = 64 * MiB;
    {
        Raw src(3 * ctask + 3);
        fill<pat>(src.data(), src.n);
        const size_t ns[] = {0, 1, ctask, ctask + 1, 3 * ctask + 3};
        for (size_t n : ns) {
            Raw dst(n);
            par_memcpy(dst.data(), src.data(), n);
            CHECK(holds<pat>(dst.data(), n) && dst.guard_ok());
        }
    }
    Raw buf(3 * ttask + 3);   // (the largest buffer of this program: three of par_touch's tasks)
    fill<pat>(buf.data(), buf.n);
    const size_t ns[] = {0, 1, ttask, ttask + 1, 3 * ttask + 3};
    for (size_t n : ns) par_touch(buf.data(), n);
    CHECK(holds<pat>(buf.data(), buf.n) && buf.guard_ok());
}

// ---- page plan
static void check_page_plan() {
    const uintptr_t pg = 4096, base = (uintptr_t)1 << 30;
    const size_t lens[] = {0, 1, 4095, 4096, 4097, 8192, MiB - 1, MiB, MiB + 4095, MiB + 4096, MiB + 8191, 3 * MiB + 5};
    const uintptr_t offs[] = {0, 1, 100, 4095, 4096, 4097};
    for (uintptr_t off : offs)
        for (size_t n : lens) {
            const uintptr_t s0 = base + off;
            const PagePlan pl = page_plan(s0, n);
            CHECK(pl.head + pl.body_bytes + pl.tail == n);
            CHECK(pl.body % pg == 0 && pl.body_bytes % pg == 0);
            CHECK(pl.head < pg && pl.tail < pg);
            size_t whole = 0;   // the pages that lie inside [s0, s0 + n), one by one
            for (uintptr_t q = s0 / pg; q * pg < s0 + n; ++q)
                if (q * pg >= s0 && (q + 1) * pg <= s0 + n) ++whole;
            CHECK(pl.body_bytes == whole * pg);
            if (whole) CHECK(pl.body == s0 + pl.head);
            CHECK(pl.eligible == (whole > 0 && whole * pg >= MiB));
        }
    // one buffer cut into consecutive chunks at arbitrary byte offsets: no page in two chunks' bodies
    std::mt19937_64 rng(7);
    for (int trial = 0; trial < 200; ++trial) {
        const uintptr_t s0 = base + rng() % (2 * pg);
        const size_t total = 40 * MiB + rng() % pg;
        std::vector<size_t> cut = {0, total};
        for (int i = 0; i < 12; ++i) cut.push_back(rng() % total);
        std::sort(cut.begin(), cut.end());
        uintptr_t last_end = 0;
        for (size_t i = 0; i + 1 < cut.size(); ++i) {
            const PagePlan pl = page_plan(s0 + cut[i], cut[i + 1] - cut[i]);
            if (!pl.body_bytes) continue;
            CHECK(pl.body >= last_end && pl.body >= s0 + cut[i] && pl.body + pl.body_bytes <= s0 + cut[i + 1]);
            last_end = pl.body + pl.body_bytes;
        }
    }
}

// ---- pin budget: eight threads take and give random sizes against a cap
static void check_pin_budget() {
    PinBudget pb;
    pb.cap = 1000000;
    CHECK(pb.take(900000) && !pb.take(100001) && pb.used == 900000);   // a refusal changes nothing
    CHECK(pb.take(100000) && pb.used == pb.cap && pb.peak == pb.cap);
    pb.give(900000);
    pb.give(100000);
    CHECK(pb.used == 0);
    pb.peak = 0;
    std::atomic<int64_t> held{0};   // accepted and not yet given back: never above the real count
    std::vector<int64_t> largest(8, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(100 + t);
            std::vector<int64_t> mine;
            for (int it = 0; it < 20000; ++it) {
                const int64_t sz = 1 + rng() % 300000;
                if (pb.take(sz)) {
                    CHECK(held.fetch_add(sz) + sz <= pb.cap);
                    largest[t] = std::max(largest[t], sz);
                    mine.push_back(sz);
                }
                CHECK(pb.used <= pb.cap);
                if (mine.size() > 2 || (!mine.empty() && rng() % 2)) {
                    held.fetch_sub(mine.back());
                    pb.give(mine.back());
                    mine.pop_back();
                }
            }
            for (int64_t sz : mine) {
                held.fetch_sub(sz);
                pb.give(sz);
            }
        });
    for (auto &x : th) x.join();
    const int64_t big = *std::max_element(largest.begin(), largest.end());
    CHECK(big > 0 && pb.peak >= big && pb.peak <= pb.cap);
    CHECK(pb.used == 0 && held == 0);
}

// ---- chunk ticket: three slot threads take chunks s, s + 3, ... of 30
static bool aborts(ChunkTicket &t, int64_t k) {
    try {
        t.wait(k);
    } catch (const PipeAbort &) {
        return true;
    }
    return false;
}

static void check_ticket() {
    {
        ChunkTicket tk;
        std::vector<int64_t> order;   // written by the thread whose turn it is: the ticket orders the writes
        std::vector<std::thread> th;
        for (int s = 0; s < 3; ++s)
            th.emplace_back([&, s] {
                for (int64_t k = s; k < 30; k += 3) {
                    tk.wait(k);
                    order.push_back(k);
                    tk.pass(k);
                }
            });
        for (auto &x : th) x.join();
        CHECK(order.size() == 30);
        for (int64_t k = 0; k < 30; ++k) CHECK(order[k] == k);
    }
    // the owner of chunk 7 fails; pass_first: it passes its ticket before the abort, as a failed enqueue does
    for (int pass_first = 0; pass_first < 2; ++pass_first) {
        ChunkTicket tk;
        std::vector<int64_t> order;
        int64_t stopped_at[3] = {-1, -1, -1};
        std::vector<std::thread> th;
        for (int s = 0; s < 3; ++s)
            th.emplace_back([&, s] {
                try {
                    for (int64_t k = s; k < 30; k += 3) {
                        tk.wait(k);
                        if (k == 7) {
                            if (pass_first) tk.pass(k);
                            tk.abort();
                            return;
                        }
                        order.push_back(k);
                        tk.pass(k);
                    }
                } catch (const PipeAbort &) {
                    stopped_at[s] = s;
                }
            });
        for (auto &x : th) x.join();   // (every waiter woke)
        CHECK(stopped_at[0] == 0 && stopped_at[1] == -1 && stopped_at[2] == 2);
        CHECK(order.size() >= 7 && order.size() <= (pass_first ? 9u : 7u));   // chunk 10 never has its turn
        for (size_t i = 0; i < order.size(); ++i) CHECK(order[i] == (int64_t)(i < 7 ? i : i + 1));
    }
    ChunkTicket tk;
    tk.pass(5);   // not the current chunk: nothing changes
    tk.pass(1);
    tk.abort();
    CHECK(!aborts(tk, 0));   // already its turn: no PipeAbort
    CHECK(aborts(tk, 1) && aborts(tk, 2) && aborts(tk, 6));
    tk.pass(0);
    CHECK(!aborts(tk, 1) && aborts(tk, 0));
}

int main() {
    check_ranges();
    check_pack_mask();
    check_unpack_maps();
    check_memcpy_touch();
    check_page_plan();
    check_pin_budget();
    check_ticket();
    printf("pipe host ok\n");
    return 0;
}
