// BatchState (vent_analysis_amd/csrc/batch_state.h): the components row of the table in DESIGN.md
// section 3 -- the guard of a fresh state, the transition without a run and with other results present
// (nothing else changes: the CI stays fresh), that a new defect map, a selection and the other enqueues
// keep the result, and that ran, forgot_run and the filter discard it.
// Built with -fsanitize=address,undefined by tests/test_components_host.py.
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
        s.need_components();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg.find("vh_batch_components has not been called") == 0;
    }
    return false;
}

int main() {
    BatchState s;
    CHECK(refuses(s) && !s.fields().components && !s.has_components() && s.cc_classes() == 0);
    s.components_enqueued(1);                            // no run is needed: the mask is an input
    CHECK(!refuses(s) && s.has_components() && s.cc_classes() == 1 && !s.has_run());
    s.ran(N4Source::n4, true);                           // a run discards it
    CHECK(refuses(s) && s.has_run());
    s.ci_enqueued(17, 1.5);
    s.distribution_enqueued(64);
    s.heterogeneity_enqueued(100);
    s.core_rind_enqueued(3);
    s.overlay_enqueued();
    const BatchState::Fields before = s.fields();
    s.components_enqueued(6);
    const BatchState::Fields &f = s.fields();
    CHECK(!refuses(s) && f.components && s.cc_classes() == 6);
    // nothing else changes: the CI stays fresh, the other results keep their parameters
    CHECK(f.result == before.result && f.n4 == before.n4 && f.do_kmeans == before.do_kmeans && f.ci && f.ci_fresh &&
          s.ci_is_fresh() && f.ci_nbs == 17 && f.distribution && f.dist_bins == 64 && f.heterogeneity &&
          f.het_bins == 100 && f.core_rind && f.cr_bands == 3 && f.overlay && !f.montage && !f.layout &&
          !f.selection && !f.labels && !f.defect && !f.proton && !f.proton_src);
    s.components_enqueued(32);                           // again with other edges
    CHECK(!refuses(s) && s.cc_classes() == 32 && s.cr_bands() == 3);
    // the other enqueues keep it
    s.ci_enqueued(9, 2.0);
    s.core_rind_enqueued(7);
    s.heterogeneity_enqueued(7);
    s.distribution_enqueued(8);
    s.overlay_enqueued();
    s.montage_enqueued();
    s.layout_cached();
    s.labels_built();
    s.proton_uploaded();
    s.proton_src_uploaded();
    CHECK(!refuses(s) && s.cc_classes() == 32 && s.cr_bands() == 7);
    s.defect_replaced();                                 // a new defect map does not discard it: the result is
    CHECK(!refuses(s) && s.cc_classes() == 32);          // a snapshot of the source as it stood at the enqueue
    s.selected(false);
    CHECK(!refuses(s));
    s.selected(true);
    CHECK(!refuses(s));
    // the filter relabels into the same buffers: it discards the result and nothing else
    const BatchState::Fields b2 = s.fields();
    s.components_filtered();
    const BatchState::Fields &g = s.fields();
    CHECK(refuses(s) && !g.components && g.result == b2.result && g.ci == b2.ci && g.ci_fresh == b2.ci_fresh &&
          g.core_rind && g.cr_bands == 7 && g.heterogeneity && g.distribution && g.overlay && g.montage &&
          g.selection == b2.selection && g.labels == b2.labels && g.defect == b2.defect && s.has_run());
    s.components_filtered();                             // without a result: nothing to do
    CHECK(refuses(s));
    s.components_enqueued(2);
    CHECK(!refuses(s) && s.cc_classes() == 2);
    s.ran(N4Source::hp, false);                          // a new run discards it
    CHECK(refuses(s) && s.has_run() && !s.fields().components);
    s.components_enqueued(2);
    CHECK(!refuses(s));
    s.forgot_run();                                      // and so does whatever forgets the run
    CHECK(refuses(s) && !s.has_run() && s.fields().ci && s.fields().defect);
    s.components_enqueued(5);
    CHECK(!refuses(s) && s.cc_classes() == 5 && !s.has_run());
    printf("components state ok\n");
    return 0;
}
