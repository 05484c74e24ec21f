// BatchState (vent_analysis_amd/csrc/batch_state.h): the heterogeneity row of the table in DESIGN.md
// section 3 -- the guard of a fresh state, the transition from a run alone and from a state with
// other results present, and that ran and forgot_run discard it with the rest of the derived set.
// Built with -fsanitize=address,undefined by tests/test_heterogeneity_host.py.
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

static const char *HET = "vh_batch_heterogeneity has not been called since the last run";

static bool refuses(const BatchState &s) {
    try {
        s.need_heterogeneity();
    } catch (const VhError &e) {
        return e.code == VH_ERR_ARG && e.msg == HET;
    }
    return false;
}

int main() {
    BatchState s;
    CHECK(refuses(s) && !s.fields().heterogeneity && s.het_bins() == 0);
    s.ran(N4Source::n4, true);
    CHECK(refuses(s));                                   // a run alone enqueues nothing
    s.ci_enqueued(17, 1.5);
    s.distribution_enqueued(64);
    s.overlay_enqueued();
    const BatchState::Fields before = s.fields();
    s.heterogeneity_enqueued(100);
    const BatchState::Fields &f = s.fields();
    CHECK(!refuses(s) && f.heterogeneity && s.het_bins() == 100);
    // nothing else changes: the CI stays fresh, the distribution keeps its bins
    CHECK(f.result == before.result && f.n4 == before.n4 && f.do_kmeans == before.do_kmeans && f.ci && f.ci_fresh &&
          f.ci_nbs == 17 && f.distribution && f.dist_bins == 64 && f.overlay && !f.montage && !f.layout &&
          !f.selection && !f.labels && !f.defect && !f.proton && !f.proton_src);
    s.heterogeneity_enqueued(7);                         // again with other parameters
    CHECK(!refuses(s) && s.het_bins() == 7 && s.dist_bins() == 64);
    s.distribution_enqueued(8);                          // and the other way round
    CHECK(!refuses(s) && s.het_bins() == 7 && s.dist_bins() == 8);
    s.defect_replaced();                                 // a new defect map does not discard it
    s.selected(false);
    CHECK(!refuses(s));
    s.ran(N4Source::hp, false);                          // a new run does
    CHECK(refuses(s) && s.has_run());
    s.heterogeneity_enqueued(1024);
    CHECK(!refuses(s));
    s.forgot_run();                                      // and so does whatever forgets the run
    CHECK(refuses(s) && !s.has_run() && s.fields().ci);
    s.heterogeneity_enqueued(5);                         // the host-buffer form: no run behind it
    CHECK(!refuses(s) && s.het_bins() == 5 && !s.has_run());
    printf("heterogeneity state ok\n");
    return 0;
}
