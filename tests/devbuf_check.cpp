// Buf (vent_analysis_amd/csrc/devbuf.h) over a fake allocator: malloc / free, the set of live blocks
// (freeing a block that is not live, or with the other kind, aborts) and a switch that makes the
// k-th allocation from now throw.  Built with -fsanitize=address,undefined by tests/test_devbuf.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "devbuf.h"

static std::map<void *, int> g_live;   // block -> kind
static long g_allocs = 0, g_frees = 0;
static long g_fail_in = 0;             // > 0: that many allocations from now, the last of them throws
struct AllocFailed {};

void *vh_mem_alloc(int kind, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) throw AllocFailed{};
    if (bytes == 0) {
        fprintf(stderr, "allocation of 0 bytes\n");
        abort();
    }
    void *p = malloc(bytes);
    if (!p) abort();
    g_live[p] = kind;
    ++g_allocs;
    return p;
}
void vh_mem_free(int kind, void *p) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) {
        fprintf(stderr, "free of a block that is not live (or of the other kind): %p\n", p);
        abort();
    }
    g_live.erase(it);
    ++g_frees;
    free(p);
}

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

// The N4 lattice group as vh_ensure_n4_workspace keeps it: three buffers indexed with one per-study
// stride, which is named only while all three hold that much.
struct Lattice {
    Buf<float> lat;
    Buf<unsigned long long> numfix;
    Buf<double> den;
    int64_t cap = 0;
    void ensure(size_t nb, int64_t want) {
        if (want > cap) {
            cap = 0;
            lat.reset();
            numfix.reset();
            den.reset();
            lat.reserve(3 * nb * want);
            numfix.reserve(2 * nb * want);
            den.reserve(nb * want);
            cap = want;
        }
    }
    bool sound(size_t nb) const {   // what a kernel launched with stride cap may index
        return cap == 0 || (lat.size() >= 3 * nb * cap && numfix.size() >= 2 * nb * cap && den.size() >= nb * cap);
    }
};

struct Two {
    Buf<float, 1> h;
    Buf<uint8_t> d;
    int tag = 0;
};

static void test_reserve() {
    Buf<int32_t> b;
    CHECK(b.get() == nullptr && b.size() == 0 && !b);
    long a0 = g_allocs, f0 = g_frees;
    CHECK(b.reserve(10));                       // first use allocates
    CHECK(b.size() == 10 && b.get() != nullptr && g_allocs == a0 + 1 && g_frees == f0);
    int32_t *p = b;                             // the implicit conversion
    CHECK(p == b.get());
    p[9] = 7;                                   // (ASan: the block holds 10 elements)
    CHECK(!b.reserve(10) && !b.reserve(3) && !b.reserve(0));   // held size suffices: nothing happens
    CHECK(b.get() == p && b.size() == 10 && g_allocs == a0 + 1 && g_frees == f0);
    CHECK(b.reserve(11));                       // a grow: one free, one allocation
    CHECK(b.size() == 11 && g_allocs == a0 + 2 && g_frees == f0 + 1 && g_live.size() == 1);
    b.get()[10] = 1;
    b.reset();
    CHECK(b.get() == nullptr && b.size() == 0 && g_live.empty());
    b.reset();                                  // twice: nothing is freed twice
    CHECK(b.reserve(0) && b.size() == 1 && b.get() != nullptr);   // n == 0 allocates one element
    b.get()[0] = 3;
    Buf<double, 1> h;                           // the kind reaches the allocator and comes back
    CHECK(h.reserve(4) && g_live.at(h.get()) == 1 && g_live.at(b.get()) == 0);
}

static void test_failure() {
    Buf<double> b;
    CHECK(b.reserve(8));
    long a0 = g_allocs, f0 = g_frees;
    g_fail_in = 1;
    bool threw = false;
    try {
        b.reserve(16);
    } catch (const AllocFailed &) {
        threw = true;
    }
    CHECK(threw && b.get() == nullptr && b.size() == 0);   // empty: the old block went first
    CHECK(g_allocs == a0 && g_frees == f0 + 1 && g_live.empty());
    CHECK(b.reserve(16) && b.size() == 16);                // a later reserve succeeds
    b.get()[15] = 1.0;
    g_fail_in = 1;                                         // a sufficient buffer never reaches the allocator
    CHECK(!b.reserve(16) && g_fail_in == 1);
    g_fail_in = 0;
}

static void test_move() {
    Buf<float> a;
    a.reserve(5);
    float *p = a;
    Buf<float> c(std::move(a));                 // move construction leaves the source empty
    CHECK(c.get() == p && c.size() == 5 && a.get() == nullptr && a.size() == 0);
    Buf<float> d;
    d.reserve(2);
    long f0 = g_frees;
    d = std::move(c);                           // move assignment frees the target's block, takes the source's
    CHECK(d.get() == p && d.size() == 5 && c.get() == nullptr && c.size() == 0 && g_frees == f0 + 1);
    Buf<float> &dr = d;
    d = std::move(dr);                          // self-assignment keeps the block
    CHECK(d.get() == p && d.size() == 5 && g_frees == f0 + 1);

    std::vector<Two> v;                         // as vh_pipe::Slot lives in a std::vector
    std::vector<void *> hs, ds;
    for (int i = 0; i < 40; ++i) {              // (several reallocations of the vector)
        v.emplace_back();
        Two &t = v.back();
        t.h.reserve(3 + i);
        t.d.reserve(1 + i);
        t.tag = i;
        hs.push_back(t.h.get());
        ds.push_back(t.d.get());
    }
    CHECK(g_live.size() == 80 + 1);             // every slot's two blocks, and d's
    for (int i = 0; i < 40; ++i) {
        CHECK(v[i].tag == i && v[i].h.get() == hs[i] && v[i].d.get() == ds[i]);
        CHECK(v[i].h.size() == (size_t)(3 + i) && v[i].d.size() == (size_t)(1 + i));
        v[i].d.get()[i] = 1;
    }
    v.erase(v.begin() + 7);                     // move assignment down the vector
    CHECK(g_live.size() == 78 + 1 && v[7].tag == 8 && v[7].h.get() == hs[8]);
}

// 5^3 then 11^3 lattices on one batch of nb = 2: six allocations.  Allocation k fails, for every k;
// the group stays sound, the call after it rebuilds the whole group, and destruction frees all.
static void test_lattice_group() {
    const size_t nb = 2;
    for (int k = 1; k <= 6; ++k)
        for (int retry = 0; retry < 2; ++retry) {
            CHECK(g_live.empty());
            {
                Lattice L;
                g_fail_in = k;
                int failed_at = 0;
                const int64_t want[3] = {125, 1331, 125};
                for (int c = 0; c < 3 && !failed_at; ++c) {
                    try {
                        L.ensure(nb, want[c]);
                        CHECK(L.sound(nb) && L.cap == (c == 0 ? 125 : 1331));   // the stride never shrinks
                    } catch (const AllocFailed &) {
                        failed_at = c + 1;
                    }
                }
                CHECK(failed_at == (k <= 3 ? 1 : 2) && g_fail_in == 0);
                CHECK(L.cap == 0 && L.sound(nb));          // no stride names a missing buffer
                if (retry) {                               // the next call re-reserves the whole group
                    const long a0 = g_allocs;
                    L.ensure(nb, want[failed_at - 1]);
                    CHECK(g_allocs == a0 + 3 && L.cap == want[failed_at - 1] && L.sound(nb) && g_live.size() == 3);
                    L.lat.get()[3 * nb * L.cap - 1] = 1.f;
                    L.numfix.get()[2 * nb * L.cap - 1] = 1ull;
                    L.den.get()[nb * L.cap - 1] = 1.0;
                }
            }
            CHECK(g_live.empty());                         // destruction freed whatever was held, once
        }
}

int main() {
    {
        test_reserve();
    }
    CHECK(g_live.empty());
    test_failure();
    CHECK(g_live.empty());
    test_move();
    CHECK(g_live.empty());
    test_lattice_group();
    CHECK(g_live.empty() && g_allocs == g_frees);
    printf("devbuf ok: %ld allocations, %ld frees, 0 live\n", g_allocs, g_frees);
    return 0;
}
