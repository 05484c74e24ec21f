// BatchState (vent_analysis_amd/csrc/batch_state.h, the header the library includes): the guards of a
// fresh state, and every transition of the table in DESIGN.md section 3 from the state in which
// everything is set -- exactly the listed members change.  Built with -fsanitize=address,undefined
// by tests/test_batch_state.py.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "batch_state.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

using F = BatchState::Fields;

static bool same(const F &a, const F &b) {
    return a.result == b.result && a.n4 == b.n4 && a.do_kmeans == b.do_kmeans && a.defect == b.defect &&
           a.ci == b.ci && a.ci_nbs == b.ci_nbs && a.ci_minvox == b.ci_minvox && a.labels == b.labels &&
           a.selection == b.selection && a.ci_fresh == b.ci_fresh && a.layout == b.layout &&
           a.overlay == b.overlay && a.montage == b.montage && a.distribution == b.distribution &&
           a.dist_bins == b.dist_bins;
}

// g throws VhError{VH_ERR_ARG, msg}
static bool refuses(const std::function<void()> &g, const char *msg) {
    try {
        g();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg == msg;
    }
    return false;
}
static bool accepts(const std::function<void()> &g) {
    try {
        g();
    } catch (const VhError &) {
        return false;
    }
    return true;
}

static const char *RUN = "vh_batch_run has not been called";
static const char *DEFECT = "no defect maps resident: vh_batch_run or vh_batch_set_defect first";
static const char *KMEANS = "the last vh_batch_run had do_kmeans = 0: no k-means partition";
static const char *CI = "vh_batch_ci has not been called";
static const char *OVERLAY = "vh_batch_overlay has not been called since the last run";
static const char *MONTAGE = "vh_batch_montage has not been called since the last run";
static const char *DIST = "vh_batch_distribution has not been called since the last run";

// every member set, through the transitions alone (selected before ci_enqueued: it makes the CI stale)
static BatchState everything() {
    BatchState s;
    s.ran(N4Source::n4, true);
    s.defect_replaced();
    s.selected(true);
    s.ci_enqueued(17, 1.5);
    s.overlay_enqueued();
    s.layout_cached();
    s.montage_enqueued();
    s.distribution_enqueued(64);
    const F &f = s.fields();
    CHECK(f.result && f.n4 == N4Source::n4 && f.do_kmeans && f.defect && f.ci && f.ci_nbs == 17 &&
          f.ci_minvox == 1.5 && f.labels && f.selection && f.ci_fresh && f.layout && f.overlay && f.montage &&
          f.distribution && f.dist_bins == 64);
    return s;
}

static F clear_derived(F f) {
    f.labels = f.selection = f.ci_fresh = f.layout = f.overlay = f.montage = f.distribution = false;
    return f;
}

static void test_fresh() {
    const BatchState s;
    CHECK(same(s.fields(), F{}));
    const F &f = s.fields();
    CHECK(!f.result && f.n4 == N4Source::none && !f.do_kmeans && !f.defect && !f.ci && !f.labels && !f.selection &&
          !f.ci_fresh && !f.layout && !f.overlay && !f.montage && !f.distribution);
    CHECK(refuses([&] { s.need_run(); }, RUN));
    CHECK(refuses([&] { s.need_defect(); }, DEFECT));
    CHECK(refuses([&] { s.need_kmeans(); }, RUN));        // no run: that comes first, as at every call site
    CHECK(refuses([&] { s.need_ci(); }, CI));
    CHECK(refuses([&] { s.need_overlay(); }, OVERLAY));
    CHECK(refuses([&] { s.need_montage(); }, MONTAGE));
    CHECK(refuses([&] { s.need_distribution(); }, DIST));
    CHECK(!s.has_run() && !s.layout_is_cached() && !s.ci_is_fresh() && !s.selection_on() && !s.labels_valid());
    BatchState r;                                         // a run without k-means: the k-means message
    r.ran(N4Source::hp, false);
    CHECK(accepts([&] { r.need_run(); }) && accepts([&] { r.need_defect(); }));
    CHECK(refuses([&] { r.need_kmeans(); }, KMEANS));
    BatchState d;                                         // an uploaded defect map alone serves the CI
    d.defect_replaced();
    CHECK(accepts([&] { d.need_defect(); }) && refuses([&] { d.need_run(); }, RUN));
}

static void test_guards_when_set() {
    const BatchState s = everything();
    CHECK(accepts([&] { s.need_run(); }) && accepts([&] { s.need_defect(); }) && accepts([&] { s.need_kmeans(); }) &&
          accepts([&] { s.need_ci(); }) && accepts([&] { s.need_overlay(); }) && accepts([&] { s.need_montage(); }) &&
          accepts([&] { s.need_distribution(); }));
    CHECK(s.has_run() && s.layout_is_cached() && s.ci_is_fresh() && s.selection_on() && s.labels_valid());
    CHECK(s.n4_source() == N4Source::n4 && s.ci_nbs() == 17 && s.ci_minvox() == 1.5 && s.dist_bins() == 64);
}

static void test_transitions() {
    const F all = everything().fields();
    {   // ran: the result and the N4 source as given, the derived set cleared, nothing else
        for (N4Source src : {N4Source::hp, N4Source::n4})
            for (bool km : {false, true}) {
                BatchState s = everything();
                s.ran(src, km);
                F want = clear_derived(all);
                want.n4 = src;
                want.do_kmeans = km;
                CHECK(same(s.fields(), want) && s.n4_source() == src);
                CHECK(want.defect && want.ci && want.ci_nbs == 17 && want.dist_bins == 64);   // these survive
            }
    }
    {   // forgot_run: the result gone, no N4 source, the same derived set cleared, nothing else
        BatchState s = everything();
        s.forgot_run();
        F want = clear_derived(all);
        want.result = false;
        want.n4 = N4Source::none;
        CHECK(same(s.fields(), want) && s.n4_source() == N4Source::none);
        CHECK(s.fields().defect && s.fields().ci);          // an uploaded defect map and a present CI survive
        CHECK(refuses([&] { s.need_run(); }, RUN) && refuses([&] { s.need_kmeans(); }, RUN));
        CHECK(accepts([&] { s.need_defect(); }) && accepts([&] { s.need_ci(); }));
        CHECK(refuses([&] { s.need_overlay(); }, OVERLAY) && refuses([&] { s.need_montage(); }, MONTAGE) &&
              refuses([&] { s.need_distribution(); }, DIST));
        // ran and forgot_run clear the same set: after both, only the result and the source differ
        BatchState r = everything();
        r.ran(N4Source::hp, true);
        F a = r.fields(), b = s.fields();
        a.result = b.result = false;
        a.n4 = b.n4 = N4Source::none;
        CHECK(same(a, b));
        s.ran(N4Source::hp, false);                       // and a run after it names its source again
        CHECK(s.has_run() && s.n4_source() == N4Source::hp);
    }
    {   // defect_replaced: from everything, selection off and the CI stale (a cached overlay stays)
        BatchState s = everything();
        s.defect_replaced();
        F want = all;
        want.selection = want.ci_fresh = false;
        CHECK(same(s.fields(), want) && s.fields().overlay && s.fields().ci);
        BatchState t;                                     // from nothing: the uploaded map alone
        t.defect_replaced();
        F w2{};
        w2.defect = true;
        CHECK(same(t.fields(), w2));
    }
    {   // selected: selection on, labels valid only if asked, the CI stale
        BatchState s = everything();
        s.selected(false);
        F want = all;
        want.ci_fresh = false;
        CHECK(same(s.fields(), want) && s.fields().overlay);   // (labels stay valid: false never clears them)
        BatchState t;
        t.ran(N4Source::hp, true);
        const F base = t.fields();
        t.selected(false);
        F w = base;
        w.selection = true;
        CHECK(same(t.fields(), w));
        t.selected(true);
        w.labels = true;
        CHECK(same(t.fields(), w));
    }
    {   // the single-flag transitions, from a run alone
        BatchState t;
        t.ran(N4Source::n4, true);
        const F base = t.fields();
        F w = base;
        t.labels_built();
        w.labels = true;
        CHECK(same(t.fields(), w));
        t.ci_enqueued(9, 0.5);
        w.ci = w.ci_fresh = true;
        w.ci_nbs = 9;
        w.ci_minvox = 0.5;
        CHECK(same(t.fields(), w));
        t.overlay_enqueued();
        w.overlay = true;
        CHECK(same(t.fields(), w));
        t.layout_cached();
        w.layout = true;
        CHECK(same(t.fields(), w));
        t.montage_enqueued();
        w.montage = true;
        CHECK(same(t.fields(), w));
        t.distribution_enqueued(1024);
        w.distribution = true;
        w.dist_bins = 1024;
        CHECK(same(t.fields(), w));
    }
    {   // ... and from everything each leaves all the rest alone
        BatchState s = everything();
        s.labels_built();
        s.overlay_enqueued();
        s.layout_cached();
        s.montage_enqueued();
        CHECK(same(s.fields(), all));
        s.ci_enqueued(3, 2.0);
        s.distribution_enqueued(8);
        F want = all;
        want.ci_nbs = 3;
        want.ci_minvox = 2.0;
        want.dist_bins = 8;
        CHECK(same(s.fields(), want));
    }
}

int main() {
    test_fresh();
    test_guards_when_set();
    test_transitions();
    printf("batch state ok\n");
    return 0;
}
