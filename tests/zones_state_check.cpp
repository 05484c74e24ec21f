// BatchState (vent_analysis_amd/csrc/batch_state.h): the zones row of the table in DESIGN.md section 3
// -- the guard of a fresh state, the transition with other results present, that a new defect map or a
// selection keeps the result, and that ran, forgot_run and nothing else discard it.  Then the zone rule
// (vent_analysis_amd/csrc/zones_host.h) on small profiles, over both element types its callers use.
// Built with -fsanitize=address,undefined by tests/test_zones_host.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "batch_state.h"
#include "zones_host.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

static bool refuses(const BatchState &s) {
    try {
        s.need_zones();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg.find("vh_batch_zones has not been called") == 0;
    }
    return false;
}

static void test_state() {
    BatchState s;
    CHECK(refuses(s) && !s.fields().zones && !s.has_zones() && s.zone_k() == 0 && s.zone_bins() == 0);
    s.ran(N4Source::n4, true);
    CHECK(refuses(s));
    s.ci_enqueued(17, 1.5);
    s.distribution_enqueued(64);
    s.heterogeneity_enqueued(100);
    s.core_rind_enqueued(3);
    s.components_enqueued(4);
    s.overlay_enqueued();
    const BatchState::Fields before = s.fields();
    s.zones_enqueued(6, 100);
    const BatchState::Fields &f = s.fields();
    CHECK(!refuses(s) && f.zones && s.has_zones() && s.zone_k() == 6 && s.zone_bins() == 100);
    // nothing else changes: the CI stays fresh, the other results keep their parameters
    CHECK(f.result == before.result && f.n4 == before.n4 && f.do_kmeans == before.do_kmeans && f.ci && f.ci_fresh &&
          f.ci_nbs == 17 && f.ci_minvox == 1.5 && f.distribution && f.dist_bins == 64 && f.heterogeneity &&
          f.het_bins == 100 && f.core_rind && f.cr_bands == 3 && f.components && f.cc_classes == 4 && f.overlay &&
          !f.montage && !f.layout && !f.selection && !f.labels && !f.defect && !f.proton && !f.proton_src);
    s.zones_enqueued(32, 7);                             // again with other zones and bins
    CHECK(!refuses(s) && s.zone_k() == 32 && s.zone_bins() == 7 && s.dist_bins() == 64);
    // every transition but ran and forgot_run keeps it
    s.defect_replaced();
    s.selected(false);
    s.selected(true);
    s.labels_built();
    s.ci_enqueued(3, 2.0);
    s.overlay_enqueued();
    s.layout_cached();
    s.montage_enqueued();
    s.distribution_enqueued(8);
    s.heterogeneity_enqueued(9);
    s.core_rind_enqueued(2);
    s.components_enqueued(5);
    s.components_filtered();
    s.proton_uploaded();
    s.proton_src_uploaded();
    CHECK(!refuses(s) && s.zone_k() == 32 && s.zone_bins() == 7);
    s.ran(N4Source::hp, false);                          // a new run discards it
    CHECK(refuses(s) && s.has_run() && !s.fields().zones);
    s.zones_enqueued(2, 1);
    CHECK(!refuses(s) && s.zone_k() == 2 && s.zone_bins() == 1);
    s.forgot_run();                                      // and so does whatever forgets the run
    CHECK(refuses(s) && !s.has_run() && s.fields().ci && s.fields().defect);
}

template <typename P>
static void test_rule() {
    {   // bounds, and both ways to cut {0, 0, 4, 1, 1, 2, 0}
        const std::vector<P> prof = {0, 0, 4, 1, 1, 2, 0};
        int32_t lo, hi;
        int64_t total;
        zn_bounds(prof.data(), (int64_t)prof.size(), lo, hi, total);
        CHECK(lo == 2 && hi == 5 && total == 8);
        std::vector<uint8_t> part(prof.size(), 255);
        zn_axis_parts(prof.data(), (int64_t)prof.size(), 2, ZN_EXTENT, lo, hi, total, part.data());
        CHECK((part == std::vector<uint8_t>{0, 0, 0, 0, 1, 1, 1}));   // below lo: 0; above hi: clamped
        zn_axis_parts(prof.data(), (int64_t)prof.size(), 2, ZN_COUNT, lo, hi, total, part.data());
        CHECK((part == std::vector<uint8_t>{0, 0, 0, 1, 1, 1, 1}));   // cum = 0 0 0 4 5 6 8
        zn_axis_parts(prof.data(), (int64_t)prof.size(), 4, ZN_COUNT, lo, hi, total, part.data());
        CHECK((part == std::vector<uint8_t>{0, 0, 0, 2, 2, 3, 3}));   // part 1 is empty: plane 2 holds half
        zn_axis_parts(prof.data(), (int64_t)prof.size(), 32, ZN_EXTENT, lo, hi, total, part.data());
        CHECK((part == std::vector<uint8_t>{0, 0, 0, 8, 16, 24, 31}));   // p > w
    }
    {   // an empty axis
        const std::vector<P> prof = {0, 0, 0};
        int32_t lo, hi;
        int64_t total;
        zn_bounds(prof.data(), 3, lo, hi, total);
        CHECK(lo == 0 && hi == -1 && total == 0 && zn_split(prof.data(), lo, hi) == 0);
        std::vector<uint8_t> part(3, 255);
        for (int by : {ZN_EXTENT, ZN_COUNT}) {
            zn_axis_parts(prof.data(), 3, 5, by, lo, hi, total, part.data());
            CHECK((part == std::vector<uint8_t>{0, 0, 0}));
        }
    }
    {   // the split: a tie goes to the smallest column; the window is lo + w / 4 .. hi - w / 4
        const std::vector<P> a = {5, 1, 7, 0, 0, 0, 6, 1, 5};         // w = 9, q = 2: candidates 2 .. 6
        CHECK(zn_split(a.data(), 0, 8) == 3);
        const std::vector<P> b = {5, 0, 7, 4, 3, 4, 6, 0, 5};         // the zeros lie outside the window
        CHECK(zn_split(b.data(), 0, 8) == 4);
        const std::vector<P> c = {9, 9, 2, 9, 9, 9, 3, 9, 9};         // the minimum at the window's edge
        CHECK(zn_split(c.data(), 0, 8) == 2);
        const std::vector<P> d = {0, 3, 2, 3, 0};                      // w = 3 < 4: the whole interval
        CHECK(zn_split(d.data(), 1, 3) == 2);
        const std::vector<P> e = {0, 0, 6, 0};                         // a single column: s = lo, side 0 is empty
        CHECK(zn_split(e.data(), 2, 2) == 2);
    }
    CHECK(zn_zone(0, 0, 0, 2, 1) == 1 && zn_zone(2, 1, 0, 2, 1) == 6 && zn_zone(1, 2, 1, 3, 2) == 12);
}

static void test_wide() {
    // totals near 2^31 and p = 32: cum * p needs 64 bits
    const std::vector<int64_t> prof = {1 << 30, (1 << 30) - 2, 1, 1};
    int32_t lo, hi;
    int64_t total;
    zn_bounds(prof.data(), 4, lo, hi, total);
    CHECK(total == ((int64_t)1 << 31));
    std::vector<uint8_t> part(4, 255);
    zn_axis_parts(prof.data(), 4, 32, ZN_COUNT, lo, hi, total, part.data());
    CHECK((part == std::vector<uint8_t>{0, 16, 31, 31}));
    CHECK(zn_part_count(((int64_t)1 << 31) - 1, (int64_t)1 << 31, 32) == 31);
    CHECK(zn_part_extent(((int64_t)1 << 30) - 1, 0, 1 << 30, 32) == 31 && zn_part_extent(1 << 29, 0, 1 << 30, 32) == 16);
}

int main() {
    test_state();
    test_rule<uint32_t>();
    test_rule<int64_t>();
    test_wide();
    printf("zones state ok\n");
    return 0;
}
