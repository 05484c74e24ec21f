// BatchState (vent_analysis_amd/csrc/batch_state.h): the core-rind row of the table in DESIGN.md
// section 3 -- the guard of a fresh state, the transition without a run and with other results
// present, that a new defect map or a selection keeps the result, and that ran and forgot_run discard
// it with the rest of the derived set.
// Built with -fsanitize=address,undefined by tests/test_core_rind_host.py.
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
        s.need_core_rind();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg.find("vh_batch_core_rind has not been called") == 0;
    }
    return false;
}

int main() {
    BatchState s;
    CHECK(refuses(s) && !s.fields().core_rind && s.cr_bands() == 0);
    s.core_rind_enqueued(1);                             // no run is needed: the mask is an input
    CHECK(!refuses(s) && s.fields().core_rind && s.cr_bands() == 1 && !s.has_run());
    s.ran(N4Source::n4, true);                           // a run discards it
    CHECK(refuses(s) && s.has_run());
    s.ci_enqueued(17, 1.5);
    s.distribution_enqueued(64);
    s.heterogeneity_enqueued(100);
    s.overlay_enqueued();
    const BatchState::Fields before = s.fields();
    s.core_rind_enqueued(3);
    const BatchState::Fields &f = s.fields();
    CHECK(!refuses(s) && f.core_rind && s.cr_bands() == 3);
    // nothing else changes: the CI stays fresh, the other results keep their parameters
    CHECK(f.result == before.result && f.n4 == before.n4 && f.do_kmeans == before.do_kmeans && f.ci && f.ci_fresh &&
          f.ci_nbs == 17 && f.distribution && f.dist_bins == 64 && f.heterogeneity && f.het_bins == 100 &&
          f.overlay && !f.montage && !f.layout && !f.selection && !f.labels && !f.defect && !f.proton &&
          !f.proton_src);
    s.core_rind_enqueued(32);                            // again with other thresholds
    CHECK(!refuses(s) && s.cr_bands() == 32 && s.het_bins() == 100);
    s.heterogeneity_enqueued(7);                         // and the other way round
    CHECK(!refuses(s) && s.cr_bands() == 32 && s.het_bins() == 7);
    s.defect_replaced();                                 // a new defect map does not discard it: the counts
    CHECK(!refuses(s) && s.cr_bands() == 32);            // belong to the map as it stood at the enqueue
    s.selected(false);
    CHECK(!refuses(s) && s.cr_bands() == 32);
    s.selected(true);
    CHECK(!refuses(s));
    s.ran(N4Source::hp, false);                          // a new run does
    CHECK(refuses(s) && s.has_run() && !s.fields().core_rind);
    s.core_rind_enqueued(2);
    CHECK(!refuses(s));
    s.forgot_run();                                      // and so does whatever forgets the run
    CHECK(refuses(s) && !s.has_run() && s.fields().ci && s.fields().defect);
    s.core_rind_enqueued(5);
    CHECK(!refuses(s) && s.cr_bands() == 5 && !s.has_run());
    printf("core rind state ok\n");
    return 0;
}
