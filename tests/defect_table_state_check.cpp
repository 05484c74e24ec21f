// BatchState (vent_analysis_amd/csrc/batch_state.h): the defect-table row of the table in DESIGN.md
// section 3 -- the guard of a fresh state, the transition (nothing else changes: the components result
// and the CI stay), that the other enqueues and a new defect map keep the result, and that a new
// labelling, the filter, a run and whatever forgets the run discard it.
// Built with -fsanitize=address,undefined by tests/test_defect_table_host.py.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "batch_state.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

static bool refuses(const BatchState &s) {
    try {
        s.need_defect_table();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg.find("vh_batch_defect_table has not been called") == 0;
    }
    return false;
}

static bool no_components(const BatchState &s) {
    try {
        s.need_components();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG;
    }
    return false;
}

int main() {
    BatchState s;
    CHECK(refuses(s) && !s.fields().defect_table && !s.has_defect_table() && s.dt_rows() == 0 && !s.dt_signal());
    CHECK(no_components(s));                             // what the enqueue asks for first
    s.components_enqueued(1);                            // no run is needed: the mask is an input
    CHECK(refuses(s) && !no_components(s));
    s.defect_table_enqueued(64, false);
    CHECK(!refuses(s) && s.has_defect_table() && s.dt_rows() == 64 && !s.dt_signal() && !s.has_run());
    s.ran(N4Source::n4, true);                           // a run discards it, with the labelling
    CHECK(refuses(s) && no_components(s) && s.has_run());
    s.ci_enqueued(17, 1.5);
    s.distribution_enqueued(64);
    s.zones_enqueued(6, 100);
    s.components_enqueued(3);
    const BatchState::Fields before = s.fields();
    s.defect_table_enqueued(1024, true);
    const BatchState::Fields &f = s.fields();
    CHECK(!refuses(s) && f.defect_table && s.dt_rows() == 1024 && s.dt_signal());
    // nothing else changes: the labelling stays, the CI stays fresh, the other results keep their parameters
    CHECK(f.result == before.result && f.n4 == before.n4 && f.do_kmeans == before.do_kmeans && f.ci && f.ci_fresh &&
          s.ci_is_fresh() && f.ci_nbs == 17 && f.distribution && f.dist_bins == 64 && f.zones && f.zone_k == 6 &&
          f.zone_bins == 100 && f.components && f.cc_classes == 3 && !f.heterogeneity && !f.core_rind && !f.overlay &&
          !f.montage && !f.layout && !f.selection && !f.labels && !f.defect && !f.proton && !f.proton_src);
    s.defect_table_enqueued(5, false);                   // again with other arguments: the last call's
    CHECK(!refuses(s) && s.dt_rows() == 5 && !s.dt_signal() && s.cc_classes() == 3);
    // the other enqueues keep it
    s.ci_enqueued(9, 2.0);
    s.core_rind_enqueued(7);
    s.heterogeneity_enqueued(7);
    s.distribution_enqueued(8);
    s.zones_enqueued(2, 7);
    s.overlay_enqueued();
    s.montage_enqueued();
    s.layout_cached();
    s.labels_built();
    s.proton_uploaded();
    s.proton_src_uploaded();
    CHECK(!refuses(s) && s.dt_rows() == 5);
    s.defect_replaced();                                 // a new defect map does not discard it: the maps the
    CHECK(!refuses(s) && !no_components(s));             // rows refer to are a snapshot
    s.selected(false);
    s.selected(true);
    CHECK(!refuses(s));
    // a new labelling replaces the maps the rows refer to: it discards the table and nothing else
    const BatchState::Fields b2 = s.fields();
    s.components_enqueued(4);
    const BatchState::Fields &g = s.fields();
    CHECK(refuses(s) && !no_components(s) && !g.defect_table && g.cc_classes == 4 && g.result == b2.result &&
          g.ci == b2.ci && g.ci_fresh == b2.ci_fresh && g.core_rind && g.heterogeneity && g.distribution && g.zones &&
          g.overlay && g.montage && g.selection == b2.selection && g.labels == b2.labels && g.defect == b2.defect);
    s.defect_table_enqueued(8, true);
    CHECK(!refuses(s) && s.dt_rows() == 8 && s.dt_signal());
    // the filter relabels into the same buffers: it discards both
    s.components_filtered();
    CHECK(refuses(s) && no_components(s) && s.has_run() && s.fields().zones);
    s.components_enqueued(2);
    s.defect_table_enqueued(8, false);
    CHECK(!refuses(s));
    s.ran(N4Source::hp, false);                          // a new run discards it
    CHECK(refuses(s) && no_components(s) && s.has_run() && !s.fields().defect_table);
    s.components_enqueued(2);
    s.defect_table_enqueued(1, false);
    CHECK(!refuses(s) && s.dt_rows() == 1);
    s.forgot_run();                                      // and so does whatever forgets the run
    CHECK(refuses(s) && no_components(s) && !s.has_run() && s.fields().ci && s.fields().defect);
    s.components_enqueued(5);
    s.defect_table_enqueued(2, false);
    CHECK(!refuses(s) && s.dt_rows() == 2 && !s.has_run());
    printf("defect table state ok\n");
    return 0;
}
