// BatchState: what a resident batch (vh_batch) holds that is still the last run's, the transitions
// that change it and the guards the entry points raise (the table is in DESIGN.md section 3).
// vh_batch holds one by value as its only record of validity.  Standard headers only.
// vh_batch_upload has no transition: it invalidates nothing (what the last run left is unchanged, and
// the next run reads the new inputs).
#pragma once
#include <cstdint>

#include "vh_error.h"

// the N4 volume the last run's chain read: none without a run, else the batch's d_hp or d_n4
enum class N4Source { none, hp, n4 };

class BatchState {
public:
    struct Fields {
        bool result = false;         // vh_batch_run has run, and nothing since discarded what it left
        N4Source n4 = N4Source::none;
        bool do_kmeans = false;      // the last run's option: its scalars hold a k-means partition
        bool defect = false;         // vh_batch_set_defect uploaded the defect maps
        bool ci = false;             // vh_batch_ci has been enqueued
        int64_t ci_nbs = 0;          // its table's shells and smallest voxel edge (while ci)
        double ci_minvox = 0.0;
        // the derived set: each is the last run's, or newer
        bool labels = false;         // d_km holds the run's k-means labels
        bool selection = false;      // a selection replaced the run's maps (VolScalars::n_sel counts it)
        bool ci_fresh = false;       // the CI was enqueued after the last change of the resident defect maps
        bool layout = false;         // the montage layout is cached
        bool overlay = false;        // vh_batch_overlay has been enqueued
        bool montage = false;        // vh_batch_montage has been enqueued
        bool distribution = false;   // vh_batch_distribution has been enqueued
        int32_t dist_bins = 0;       // its n_bins (while distribution)
        bool heterogeneity = false;  // vh_batch_heterogeneity has been enqueued
        int32_t het_bins = 0;        // its n_bins (while heterogeneity)
        bool core_rind = false;      // vh_batch_core_rind has been enqueued
        int32_t cr_bands = 0;        // its n_thr + 1 (while core_rind)
        bool components = false;     // vh_batch_components has been enqueued, and no filter has reused its buffers
        int32_t cc_classes = 0;      // its n_edges + 1 (while components)
        bool defect_table = false;   // vh_batch_defect_table has been enqueued on that labelling
        int32_t dt_rows = 0;         // its max_rows (while defect_table)
        bool dt_signal = false;      // its norm was not VH_DT_NO_SIGNAL (while defect_table)
        bool zones = false;          // vh_batch_zones has been enqueued
        int32_t zone_k = 0;          // its K, the zones without zone 0 (while zones)
        int32_t zone_bins = 0;       // its n_bins (while zones)
        // an input, like the resident HPvent and mask: no transition but its own changes it
        bool proton = false;         // d_proton holds the batch's proton volumes
        bool proton_src = false;     // d_proton_src holds the proton on its own grid (vh_batch_upload_proton_src)
    };

    // ---- transitions.  An uploaded defect map and a present CI survive ran and forgot_run; a cached
    // overlay survives defect_replaced and selected. ----
    void ran(N4Source source, bool do_kmeans) { f_.result = true; f_.n4 = source; f_.do_kmeans = do_kmeans; clear_derived(); }
    void forgot_run() { f_.result = false; f_.n4 = N4Source::none; clear_derived(); }
    void defect_replaced() { f_.defect = true; f_.selection = f_.ci_fresh = false; }
    void selected(bool with_km) { f_.selection = true; f_.labels = f_.labels || with_km; f_.ci_fresh = false; }
    void labels_built() { f_.labels = true; }
    void ci_enqueued(int64_t nbs, double minvox) { f_.ci = f_.ci_fresh = true; f_.ci_nbs = nbs; f_.ci_minvox = minvox; }
    void overlay_enqueued() { f_.overlay = true; }
    void layout_cached() { f_.layout = true; }
    void montage_enqueued() { f_.montage = true; }
    void distribution_enqueued(int32_t bins) { f_.distribution = true; f_.dist_bins = bins; }
    void heterogeneity_enqueued(int32_t bins) { f_.heterogeneity = true; f_.het_bins = bins; }
    void core_rind_enqueued(int32_t bands) { f_.core_rind = true; f_.cr_bands = bands; }
    // (a new labelling, and the filter's, replace the maps the rows of a defect table refer to)
    void components_enqueued(int32_t classes) { f_.components = true; f_.cc_classes = classes; f_.defect_table = false; }
    void defect_table_enqueued(int32_t rows, bool signal) { f_.defect_table = true; f_.dt_rows = rows; f_.dt_signal = signal; }
    void zones_enqueued(int32_t k, int32_t bins) { f_.zones = true; f_.zone_k = k; f_.zone_bins = bins; }
    void components_filtered() { f_.components = f_.defect_table = false; }   // vh_batch_filter_components relabelled into the same buffers
    void proton_uploaded() { f_.proton = true; }
    void proton_src_uploaded() { f_.proton_src = true; }

    // ---- guards: VH_ERR_ARG, for the entry point to raise before it enqueues anything ----
    void need_run() const { need(f_.result, "vh_batch_run has not been called"); }
    void need_defect() const {
        need(f_.result || f_.defect, "no defect maps resident: vh_batch_run or vh_batch_set_defect first");
    }
    void need_kmeans() const {
        need_run();
        need(f_.do_kmeans, "the last vh_batch_run had do_kmeans = 0: no k-means partition");
    }
    void need_ci() const { need(f_.ci, "vh_batch_ci has not been called"); }
    void need_overlay() const { need(f_.overlay, "vh_batch_overlay has not been called since the last run"); }
    void need_montage() const { need(f_.montage, "vh_batch_montage has not been called since the last run"); }
    void need_distribution() const {
        need(f_.distribution, "vh_batch_distribution has not been called since the last run");
    }
    void need_heterogeneity() const {
        need(f_.heterogeneity, "vh_batch_heterogeneity has not been called since the last run");
    }
    void need_core_rind() const {
        need(f_.core_rind, "vh_batch_core_rind has not been called since the last run or the last edit of the inputs");
    }
    void need_components() const {
        need(f_.components, "vh_batch_components has not been called since the last run, the last edit of the inputs "
                            "or the last vh_batch_filter_components");
    }
    void need_defect_table() const {
        need(f_.defect_table, "vh_batch_defect_table has not been called since the last vh_batch_components, "
                              "vh_batch_filter_components, run or edit of the inputs");
    }
    void need_zones() const {
        need(f_.zones, "vh_batch_zones has not been called since the last run or the last edit of the inputs");
    }
    void need_proton() const { need(f_.proton, "no proton resident: vh_batch_upload_proton first"); }
    void need_proton_src() const {
        need(f_.proton_src, "no proton source resident: vh_batch_upload_proton_src first");
    }

    // ---- queries ----
    bool has_run() const { return f_.result; }
    bool layout_is_cached() const { return f_.layout; }
    bool has_proton() const { return f_.proton; }
    bool has_proton_src() const { return f_.proton_src; }
    bool ci_is_fresh() const { return f_.ci_fresh; }
    bool selection_on() const { return f_.selection; }
    bool labels_valid() const { return f_.labels; }
    N4Source n4_source() const { return f_.n4; }
    int64_t ci_nbs() const { return f_.ci_nbs; }
    double ci_minvox() const { return f_.ci_minvox; }
    int32_t dist_bins() const { return f_.dist_bins; }
    int32_t het_bins() const { return f_.het_bins; }
    int32_t cr_bands() const { return f_.cr_bands; }
    bool has_components() const { return f_.components; }
    int32_t cc_classes() const { return f_.cc_classes; }
    bool has_defect_table() const { return f_.defect_table; }
    int32_t dt_rows() const { return f_.dt_rows; }
    bool dt_signal() const { return f_.dt_signal; }
    bool has_zones() const { return f_.zones; }
    int32_t zone_k() const { return f_.zone_k; }
    int32_t zone_bins() const { return f_.zone_bins; }
    const Fields &fields() const { return f_; }   // everything, read-only (tests/batch_state_check.cpp)

private:
    Fields f_;
    // what a run leaves and the calls after it add: gone with the run's results, whether a new run
    // replaced them (ran) or an edit of the resident inputs discarded them (forgot_run)
    void clear_derived() {
        f_.labels = f_.selection = f_.ci_fresh = false;
        f_.layout = f_.overlay = f_.montage = f_.distribution = f_.heterogeneity = f_.core_rind = false;
        f_.components = f_.defect_table = f_.zones = false;
    }
    static void need(bool ok, const char *msg) { if (!ok) throw VhError{VH_ERR_ARG, msg}; }
};
