// Internal declarations shared by the libventhip translation units (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <new>
#include <set>
#include <mutex>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/vent_hip.h"
#include "vh_error.h"
#include "batch_state.h"
#include "devbuf.h"

#define VH_TPB 256          // threads per block for streaming kernels (4 waves of 64)
#define VH_WAVE 64
#define VH_SORT_TILE 4096   // keys per radix-sort tile (256 threads x 16 keys)
#define VH_SORT_KPT 16
#define VH_MAX_LEVELS 8
#define VH_FFT_P 512
#define VH_MAX_BINS 256

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            throw VhError{_e == hipErrorOutOfMemory ? VH_ERR_NOMEM : VH_ERR_HIP,            \
                          std::string(#expr) + ": " + hipGetErrorString(_e)};               \
    } while (0)

// VH_SYNC_CHECK=1 (diagnostics): every launch is followed by a device sync, so a kernel fault is
// reported at the launch that caused it (file:line) instead of at a later API call
inline bool vh_sync_check() {
    static const bool on = getenv("VH_SYNC_CHECK") != nullptr;
    return on;
}
#define VH_CHECK_LAUNCH()                                                                   \
    do {                                                                                    \
        HIP_TRY(hipGetLastError());                                                         \
        if (vh_sync_check()) {                                                              \
            const hipError_t _s = hipDeviceSynchronize();                                   \
            if (_s != hipSuccess)                                                           \
                throw VhError{VH_ERR_HIP, std::string("after the launch at ") + __FILE__ + \
                                              ":" + std::to_string(__LINE__) + ": " +       \
                                              hipGetErrorString(_s)};                       \
        }                                                                                   \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): the attribute is
// per device, and batches of several contexts / pipeline slots launch from several host threads.
inline void vh_set_max_lds(const void *fn, int bytes) {
    static std::mutex m;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(m);
    if (done.count({fn, dev})) return;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({fn, dev});
}

// Per-volume device scalars (one record per study).
struct VolScalars {
    int64_t n_mask;          // mask != 0
    int64_t n_mask1;         // mask == 1 (N4 label, LungVolume)
    int64_t first_masked;    // raster index of the first mask==1 voxel (N4 bin-range quirk)
    int64_t n_defect;
    int64_t n_lb12;
    int64_t n_km0;
    float mean_anchor;
    float p99;
    double snr;
    int32_t km_iters;
    int32_t pad0;
    double km_c[4];
    int32_t cmin, cmax;      // SNR column box [cmin, cmax)
    int32_t any_row_empty, any_slice_empty;
    int32_t snr_ok;          // 0 when the reference would raise (no masked column > 0)
    int32_t ci_status;       // VH_OK / VH_ERR_MAXRADIUS
    int32_t row_lo, row_hi;  // first / last row holding any masked voxel
    int64_t n_ci;            // defect voxels for CI
    double ci_scalar;
    // k-means' final partition for the defect selection (vh_batch_select_defect), appended so the
    // fields above keep their offsets: the sortable key at cut j + 1 (the smallest value of cluster
    // j + 1), valid where bit j of km_valid is set (cut j + 1 < n); the lowest non-empty cluster
    uint32_t km_cut[3];
    int32_t km_valid;
    int32_t km_low;
    int32_t pad1;
    int64_t n_sel;           // voxels of the last selected defect map
};

// Per-volume N4 iteration state.
struct N4State {
    float bin_min, bin_max, slope;
    int32_t active;          // 1 while the current level is still iterating
    int32_t iters;           // iterations executed in the current level
    int32_t tlast;           // T buffer (0/1) holding the column tables of the last evaluated field
    uint32_t umax_key, umin_key;  // sortable keys: max over all masked, min over all but first
    float u_first;
    float conv_w;            // S7: ITK's float Welford convergence of the last eval (k_n4_welford)
    double conv;
    int32_t iters_level[VH_MAX_LEVELS];
    float conv_level[VH_MAX_LEVELS];
    uint64_t t_start, t_end;   // k_n4_study: device wall clock (wall_clock64) at the workgroup's start / end
    uint32_t hw_id, xcc_id;    // k_n4_study: where the workgroup ran (HW_REG_HW_ID / HW_REG_XCC_ID)
    int32_t pc_rounds, pc_fallbacks;   // k_n4_study: S7 guess-and-verify rounds / serial fallbacks, all iterations
    int32_t pc_pre;            // k_n4_pcw: the last call decided early (PC_PRE): try again on the next one
    // 1 when conv_w of the last S7 call is a certified bound (an early / stage-0 decision: mu's upper
    // and sig's lower bound, enough for the threshold test only), 0 when it is ITK's float measure.
    // A level's last call is never decided early, so conv_level[] is always the exact measure.
    int32_t conv_bound;
};

// Per-axis, per-level B-spline tables (host-built, identical to oracle/n4_oracle.c).
struct AxisTab {
    int32_t n, ncp;
    std::vector<int32_t> base;
    std::vector<float> w;      // [n][4]
    std::vector<double> sw2;   // [n]
};

struct KTimer {
    std::vector<hipEvent_t> ev;   // pairs (start, stop)
    std::vector<int> slots;       // stamped launches: slots of vh_batch::d_kst
    double bytes_per_launch = 0;
    double total_ms = 0;
    int64_t launches = 0;
};

struct vh_ctx {
    int device = 0;
    std::string last_error;
    void *comm = nullptr;           // ncclComm_t
    int nranks = 1, rank = 0;
    // page-locked, device-mapped CI scalars (k_ci_finish stores them there: no readback copy)
    Buf<VolScalars, 1> h_ci_sc;
    // the host-buffer entry points (vh_n4, vh_vdp, ...) share one cached scratch batch per
    // context; mu serialises them, so a context may be used from several host threads
    vh_batch *scratch = nullptr;
    int profile = 0;                // vh_ctx_profile: time the scratch batch's kernel classes
    std::mutex mu;
    // last_error is written by any failing entry point (several host threads may fail at once on
    // one context, and vh_pipe_run does not hold mu): its own lock, and vh_last_error hands out a
    // per-thread copy
    mutable std::mutex err_mu;
    // vh_recon: its own stream and a cached device buffer (input, line transforms, output, twiddles)
    hipStream_t aux = nullptr;
    // RCCL: every collective of the communicator on this one stream, in program order (batches in
    // flight would otherwise issue them on their own streams, which the GPU may run in a different
    // order than another rank does: a deadlock)
    hipStream_t comm_st = nullptr;
    Buf<char> recon_buf;
};

// One study of the batch montage (vh_batch_montage_layout): its crop, how its crop rows split into
// workgroups of k_montage_b, where its image starts in the compact buffer and its first workgroup.
// Entry nb of the array closes the prefix: off = the buffer's size, wg0 = the grid.
struct MtStudy {
    int32_t r0, nr, c0, nc, s0, ns;
    int32_t ncc, nzc;        // column / slice chunks of a crop row (MT_COLS x MT_ZC voxels each)
    int64_t off;             // byte at which the study's image starts (a multiple of VH_MT_ALIGN)
    int64_t wg0;             // first workgroup of the study; an empty study has none
};
#define VH_MT_ALIGN 64
#define VH_MT_COLS 64        // crop columns per workgroup of k_montage_b
#define VH_MT_ZC 32          // crop slices per workgroup

struct vh_batch {
    vh_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;    // every launch and copy of this batch (batches overlap)
    hipStream_t st_n4 = nullptr;     // VH_PRIO: the study kernel alone on a low-priority stream (the
    hipEvent_t ev_n4_pre = nullptr, ev_n4_post = nullptr;   // rest on a high-priority one), joined by events
    hipEvent_t ev_cpre = nullptr, ev_cpost = nullptr;      // the cohort all-reduce on vh_ctx::comm_st
    // Every d_* member (and the pinned h_flags) is a Buf: the batch owns it, it is allocated by
    // reserve() where it is first needed and freed by ~vh_batch.  Adding one takes the member alone.
    Buf<int32_t, 1> h_flags;         // pinned: the sweep driver's per-iteration active counts
    int64_t R = 0, C = 0, Z = 0, V = 0, nb = 0, CZ = 0;
    int64_t max_tiles = 0;
    // inputs / outputs
    Buf<float> d_hp;
    Buf<uint8_t> d_mask;
    Buf<float> d_n4;
    Buf<uint8_t> d_defect, d_border, d_lb;
    // vh_batch_select_defect
    Buf<uint8_t> d_km;               // [nb][V] k-means labels (0 off-mask, else 1 + cluster), on first demand;
                                     //   the last run's while state.labels_valid()
    // mask statistics
    Buf<int32_t> d_colrange;         // [nb][CZ][2]  first/last masked row of each (col, slice) column
    Buf<int32_t> d_colcount;         // [nb][CZ]
    Buf<uint32_t> d_colbits;         // [nb][ceil(R/32)][CZ]  row bitmap of mask == 1 per column
    Buf<uint32_t> d_colbnz;          // [nb][ceil(R/32)][CZ]  row bitmap of mask != 0 per column
    Buf<int64_t> d_colstart;         // [nb][CZ]     exclusive prefix of colcount
    Buf<uint8_t> d_rowany, d_colany, d_sliceany;
    Buf<VolScalars> d_sc;
    Buf<double> d_part;              // [nb][part_blocks][4] deterministic partial sums
    int64_t part_blocks = 0;
    Buf<double> d_snrpart;           // [nb][slab_blocks][4] SNR partial sums (k_snr / k_n4_final)
    int64_t slab_blocks = 0;         // column blocks x 32-row slabs per volume
    bool snr_fused = false;          // k_n4_final computed the SNR partials of this run
    // sort
    Buf<uint32_t> d_keys0, d_keys1;
    Buf<uint32_t> d_tilecnt;         // [nb][256][max_tiles]
    // cohort
    Buf<uint64_t> d_cohort;
    // N4 workspace
    Buf<float> d_L0, d_lat, d_E;
    Buf<unsigned long long> d_numfix;   // [nb][lattice][2] 128-bit fixed-point fit sums (S5)
    Buf<int32_t> d_rowstart;         // [nb][tiles][R] compact offset of each (64-column tile, row)
    Buf<uint64_t> d_rowmask;         // [nb][tiles][R] mask == 1 lanes of each (tile, row)
    Buf<int32_t> d_rrank;            // [nb][tiles][R] raster rank of the first masked voxel of (tile, row)
    Buf<int32_t> d_iscan;            // large volumes: chunk sums of the row-start / raster-rank scans
    Buf<float> d_D;                  // [nb][VS] B_old - B_new (S7 input): compact order (n4), raster order (n4_study)
    Buf<int32_t> d_perm;             // [nb][VS] raster rank -> compact index of the mask == 1 voxels (n4)
    // compact N4 state: mask==1 voxels in tile-row order, volume stride VS
    int64_t VS = 0;
    int rsh = 1;                     // compact voxel index = (row << rsh) | column
    bool keys_fused = false;         // k_n4_final wrote the sort keys of binary-mask volumes
    Buf<float> d_U;                  // [nb][VS] U = L0 - B
    Buf<int32_t> d_ridx;             // [nb][VS] raster index of each compact voxel
    Buf<int32_t> d_cp;               // [nb + 1] chunk prefix (N4_CH voxels per chunk)
    Buf<int32_t> d_cvol;             // [chunks] owning volume
    Buf<uint64_t> d_hpart;           // [chunks][VH_MAX_BINS] per-chunk histograms
    Buf<uint64_t> d_hred;            // [studies][N4_HSL][2][VH_MAX_BINS] slice sums (k_n4_hred)
    Buf<double> d_cpart;             // [chunks][2] per-chunk convergence sums
    int64_t n4_tiles = 0;            // tiles the d_rowstart / d_rowmask / d_rrank rows were laid out for
    std::vector<size_t> lvx_off;     // per level: xst / wk3 / wk2 offsets in d_tabs
    Buf<double> d_P1, d_den;
    Buf<float> d_pcdrift;            // [nb][1024] the study kernel's PC guess offsets (PC_DRIFT)
    Buf<float> d_T;                  // [2][nb][CZ][ncx] per-column lattice contraction (new / previous field)
    Buf<N4State> d_st;
    Buf<int32_t> d_nactive;
    Buf<char> d_tabs;                // device copy of all per-level axis tables
    // per-study strides the kernels index with (the largest request so far), not capacities alone:
    // lat_cap of d_lat / d_numfix / d_den, t_cap of d_T, q2_cap of d_P1.  0 while its group is empty.
    int64_t lat_cap = 0, t_cap = 0, q2_cap = 0;
    std::vector<size_t> tab_off;     // offsets of each (level, axis) table in d_tabs
    vh_n4_params tab_prm{};          // parameters the tables were built for
    bool tabs_valid = false;
    Buf<double2> d_twiddle;          // FFT twiddles (host-computed)
    Buf<char> d_study_lv;            // n4_study.hip: per-level table pointers + iteration caps
    Buf<int32_t> d_study_order;      // n4_study.hip: workgroup -> study, largest study first
    Buf<char> d_pcg;                 // n4.hip k_n4_pcg: per-block guesses / ends / sums, aggregates
    Buf<char> d_study_latg;          // n4_study.hip depth 2: the lattice before the last two updates
    Buf<char> d_stg;                 // n4_study.hip grid form: global sums, records, grid-PC scratch
    Buf<char> d_sortg;               // vdp.hip grid sort: per-chunk digit counts / offsets
    // CI workspace
    Buf<uint32_t> d_bitmap;          // [nb][ceil(V/32)] Fortran-order defect bits
    Buf<int32_t> d_ci_list;          // [nb][V] defect voxel raster indices (compacted)
    Buf<int32_t> d_ci_shell;         // [nb][V]
    Buf<uint32_t> d_ci_hist;         // [nb][ci_nb]
    Buf<int32_t> d_ci_status;        // [nb]
    Buf<unsigned long long> d_ci_count;   // [nb]
    Buf<double> d_ci_map;            // [nb][V] float64 CI map (vh_ci, vh_batch_download_ci)
    // vh_batch_ci (the CI of the resident defect maps)
    Buf<int16_t> d_ci_shell16;       // [nb][V] shell of each defect voxel, -1 elsewhere
    Buf<uint32_t> d_ci_next;         // [nb][64] (one per 256 bytes) next unclaimed slot of the study's defect list (k_ci_walk_b)
    Buf<double> d_ci_radii;          // [state.ci_nbs()] the last table's radii: the batch's own copy, so
                                     //   the float64 map can be expanded after the table is destroyed
    // vh_batch_overlay / vh_batch_montage (export.hip): every buffer on first demand
    Buf<uint8_t> d_ov_rgb;           // [nb][Z][R][C][3] the overlay frames
    Buf<uint32_t> d_ov_mm;           // [nb][2] min / max of |N4| (float bits)
    Buf<float> d_proton;             // [nb][V] the resident proton volumes (vh_batch_upload_proton, or the
                                     //   montage's when it is given one), while state.has_proton()
    Buf<int32_t> d_mt_crop;          // [nb][8] k_crop_layout: r0, nr, c0, nc, s0, ns, status, 0
    Buf<MtStudy> d_mt_st;            // [nb + 1]
    Buf<uint32_t> d_mt_keys;         // [nb][6] crop min / max keys of proton, HPvent, N4
    Buf<int32_t> d_mt_flag;          // [nb] 1: a CI colour index reached prow
    Buf<double> d_mt_parula;         // [prow][3], the largest prow so far
    Buf<uint8_t> d_mt_img;           // the compact image buffer
    std::vector<MtStudy> mt_st;      // host copy of d_mt_st (valid while state.layout_is_cached())
    std::vector<int32_t> mt_status;  // [nb] VH_OK / VH_ERR_EMPTY of the layout
    // vh_batch_distribution (dist.hip): every buffer on first demand
    Buf<uint32_t> d_dist_hist;       // [nb][state.dist_bins()] the last call's histograms
    Buf<unsigned long long> d_dist_out;   // [nb][2] masked voxels below 0 / at or above hi (NaN included)
    Buf<unsigned long long> d_dist_sl;    // [nb][Z][VH_DIST_COLS] slice counts
    // vh_batch_denoise / vh_batch_noise_sigma (denoise.hip): on first demand
    Buf<float> d_dn_prm;             // [nb][2] the last denoise's inv_h2 and bias of each study
    Buf<float> d_dn_sigma;           // [nb] the last noise estimate
    // vh_batch_heterogeneity (heterogeneity.hip): every buffer on first demand
    Buf<float> d_het;                // [nb][V] the last call's CoV maps
    Buf<uint32_t> d_het_hist;        // [nb][state.het_bins()] its histograms
    Buf<unsigned long long> d_het_stats;   // [nb][4] n_in, n_over, n_none, sum_fx
    // vh_batch_core_rind (depth.hip): every buffer on first demand
    Buf<uint16_t> d_cr_map;          // [nb][V] the last call's saturated D2 maps
    Buf<uint16_t> d_cr_g;            // [nb][V] the column distances: scratch of the two kernels (bytes where R <= 510)
    Buf<unsigned long long> d_cr_counts;   // [nb][state.cr_bands()][2] the band's voxels, its defect voxels
    Buf<unsigned long long> d_cr_stats;    // [nb][2] n_mask, max D2
    // vh_batch_components / vh_batch_filter_components (components.hip): every buffer on first demand
    Buf<int32_t> d_cc_root;          // [nb][V] the last labelling's roots: the union-find's parent array
    Buf<uint32_t> d_cc_size;         // [nb][V] its component sizes
    Buf<unsigned long long> d_cc_counts;   // [nb][state.cc_classes()][2] the class's components, their voxels
    Buf<unsigned long long> d_cc_stats;    // [nb][4] n_set, n_comp, the largest key (size << 32 | ~root), unused
    Buf<uint32_t> d_cc_min;          // [nb] the last filter's min_size
    Buf<int32_t> d_cc_keep;          // [nb] its keep_largest
    Buf<unsigned long long> d_cc_picks;    // [nb][8] its picks: the k largest keys of each study, in order
    Buf<unsigned long long> d_cc_kept;     // [nb][2] the components and the voxels it kept
    // vh_batch_defect_table (defect_table.hip): every buffer on first demand
    Buf<unsigned long long> d_dt_rows;     // [nb][state.dt_rows()][VH_DT_COLS] the last call's rows (room for 1024 each)
    Buf<unsigned long long> d_dt_stats;    // [nb][4] n_rows, n_qualifying, voxels in the rows, in the qualifying
    Buf<unsigned long long> d_dt_keys;     // [nb][1024] the rows' keys (size << 32 | ~root), greatest first
    Buf<unsigned long long> d_dt_sel;      // [nb][2] the radix select's prefix and remaining rank
    Buf<unsigned long long> d_dt_cut;      // [nb] the cut-off key of a study with more components than rows (else 0)
    Buf<uint32_t> d_dt_hist;         // [nb][2048] the digit histogram of one pass of the select
    Buf<uint32_t> d_dt_cnt;          // [nb] the keys listed so far
    Buf<uint32_t> d_dt_min;          // [nb] the last call's min_size
    // vh_batch_zones (zones.hip): every buffer on first demand
    Buf<uint32_t> d_zn_prof;        // [nb][R + C + Z] the mask's on voxels of every row, column and slice
    Buf<uint8_t> d_zn_tab;           // [nb][R + C + Z] the part of every row, column (or its side) and slice
    Buf<int32_t> d_zn_geom;          // [nb][8] lo_r, hi_r, lo_c, hi_c, lo_z, hi_z, s, 0
    Buf<uint8_t> d_zn_map;           // [nb][V] the last call's zone maps
    Buf<unsigned long long> d_zn_counts;   // [nb][state.zone_k() + 1][VH_ZONE_COLS]
    Buf<uint32_t> d_zn_hist;         // [nb][state.zone_k() + 1][state.zone_bins()]
    Buf<unsigned long long> d_zn_stats;    // [nb][state.zone_k() + 1][4] n_in, n_below, n_over, sum_fx
    // vh_batch_edit_mask / vh_batch_download_mask (mask_edit.hip): on first demand.  The edits' scratch
    // volumes are d_border (the morphology's other mask) and d_lb (the strokes): a run rewrites both
    Buf<int32_t> d_me_radius;        // [nb] the last edit's radii
    Buf<unsigned long long> d_me_count;   // [nb] voxels != 0 of the resident mask (vh_batch_download_mask)
    // vh_batch_proton_threshold / vh_batch_segment / vh_batch_mask_overlap (segment.hip): on first
    // demand.  The fill writes into d_border and the overlap stages the other mask in d_lb, as the edits do
    Buf<uint32_t> d_sg_pmax;         // [nb] bit pattern of the proton's maximum over its finite voxels >= 0
    Buf<uint32_t> d_sg_hist;         // [nb][256] the proton histogram behind the Otsu cut
    Buf<float> d_sg_thresh;          // [nb] the last segmentation's thresholds
    Buf<unsigned long long> d_sg_count;   // [nb][3] the last overlap counts
    // vh_batch_register / vh_batch_shift (register.hip): on first demand, and nothing another call reads
    Buf<uint32_t> d_rg_max;          // [2][nb] bit patterns of the proton's and the HPvent's maxima over F
    Buf<uint8_t> d_rg_cp, d_rg_cx;   // [nb][V] the 32-level codes of the proton and of the HPvent, 255 invalid
    Buf<uint32_t> d_rg_hist;         // [nb][rg_ns][32][32] the last register call's joint histograms
    Buf<double> d_rg_score;          // [nb][rg_ns] its scores
    int64_t rg_ns = 0;               // its shifts; 0 before any register call
    Buf<int32_t> d_rg_shift;         // [nb][3] the last shift call's shifts
    Buf<float> d_rg_ptmp;            // [nb][V] the proton shift's destination, exchanged with d_proton
    // vh_batch_upload_proton_src / vh_batch_resample_proton (resample.hip): on first demand
    Buf<float> d_proton_src;         // [nb][rs_shape] the proton on its own grid, while state.has_proton_src()
    int64_t rs_shape[3] = {0, 0, 0}; // its shape (Rs, Cs, Zs)
    Buf<int32_t> d_rs_tab;           // [nb][10 (R + C + Z)] the last resampling's tap tables (RsTabs)
    // vh_batch_register_maps (register_maps.hip): on first demand, and nothing another call reads
    Buf<uint32_t> d_rm_max;          // [2][nb] bit patterns of the source's and the HPvent's maxima over F
    Buf<uint8_t> d_rm_cx;            // [nb][V] the 32-level codes of the HPvent, 255 invalid
    Buf<int32_t> d_rm_tab;           // [nb][10 (Kr R + Kc C + Kz Z)] the last call's tap tables
    Buf<uint32_t> d_rm_hist;         // [nb][rm_nc][32][32] its joint histograms
    Buf<double> d_rm_score;          // [nb][rm_nc] its scores
    int64_t rm_nc = 0;               // its candidates; 0 before any register_maps call
    int64_t n4_subbatch = 0;         // volumes per N4 sub-batch (0 = whole batch)
    int32_t n4_mode = 0;             // vh_run_opts.n4_mode
    bool n4_used_study = false;      // the last N4 ran the volume-resident kernel
    // timing
    bool profile = false;
    std::map<std::string, KTimer> timers;
    // stamped timers (cooperative launches): [VH_KST_CAP] first-workgroup starts, then
    // [VH_KST_CAP] last-workgroup ends, device wall clock; kst_n slots handed out since the reset
    Buf<unsigned long long> d_kst;
    int kst_n = 0;
    // last run options
    vh_run_opts opts{};
    // What of all this is still the last run's: the only record of validity (batch_state.h).  api.hip
    // alone changes it, through its named transitions.
    BatchState state;
    // the N4 volume the last run's chain read, resolved where a kernel is launched: d_hp and d_n4 may
    // have been exchanged since (vh_batch_denoise), and without a run there is none to hand to a launch
    const float *n4_last() const {
        state.need_run();
        return state.n4_source() == N4Source::n4 ? d_n4.get() : d_hp.get();
    }
};

// ---- the extern "C" boundary (api.hip, pipe.hip) ----------------------------------------------
int vh_fail(vh_ctx *c, int code, const std::string &msg);

#define API_TRY(ctx, ...)                                                                    \
    try {                                                                                    \
        __VA_ARGS__                                                                          \
    } catch (const VhError &e) {                                                             \
        return vh_fail(ctx, e.code, e.msg);                                                  \
    } catch (const std::bad_alloc &) {                                                       \
        return vh_fail(ctx, VH_ERR_NOMEM, "host allocation failed");                         \
    } catch (const std::exception &e) {                                                      \
        return vh_fail(ctx, VH_ERR_HIP, e.what());                                           \
    } catch (...) {                                                                          \
        return vh_fail(ctx, VH_ERR_HIP, "unknown error");                                    \
    }                                                                                        \
    return VH_OK;

// Every vh_batch_* entry point but vh_batch_destroy: a null handle is VH_ERR_ARG; otherwise API_TRY on
// the batch's context, with its device current.
#define BATCH_TRY(b, ...)                                                                    \
    if (!(b)) return VH_ERR_ARG;                                                             \
    API_TRY((b)->ctx, {                                                                      \
        HIP_TRY(hipSetDevice((b)->ctx->device));                                             \
        __VA_ARGS__                                                                          \
    })

// batches as api.hip makes, frees (after draining their stream) and runs them, for the pipe's slots
vh_batch *vh_new_batch(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t nb);
void vh_free_batch(vh_batch *b);
void vh_run_batch(vh_batch *b, const vh_run_opts &o, int n4_src);
void vh_fill_results(const vh_batch *b, const VolScalars *sc, const N4State *st, vh_vdp_result *res);

// a compact sphere table resident in HBM (vh_ci_table_create): linear offsets for one (R, C)
struct vh_ci_table {
    vh_ctx *ctx = nullptr;
    int64_t R = 0, C = 0, rows = 0, nbs = 0;
    Buf<int32_t> d_offL;             // [rows] px2vec offsets, CI_SENTINEL for duplicate rows
    Buf<int32_t> d_bounds;           // [nbs] shell prefix lengths
    Buf<double> d_radii;             // [nbs] r[b - 1]
    // vh_batch_ci: one event per batch that used the table, recorded on that batch's stream after
    // its CI launches (under ctx->mu); vh_ci_table_destroy waits on all of them before the frees
    mutable std::map<const vh_batch *, hipEvent_t> users;
};

// ---- timing helper ----------------------------------------------------------------------------
// stamped (profiling a cooperative launch): no events; the kernel stamps its own span through
// stamp() (kst_begin / kst_end), because HIP events around hipLaunchCooperativeKernel also time the
// runtime's cooperative handshake (config 5 k_n4_pcg2: 677 us per launch by events against 542 us in
// rocprofv3's trace, whose gaps round the launch are ~13 us each, r6q)
struct ScopedKTimer {
    vh_batch *b;
    KTimer *t;
    hipEvent_t e1 = nullptr;
    unsigned long long *ks = nullptr;
    hipStream_t s = nullptr;   // the stream the timed launches go to (the batch's by default)
    ScopedKTimer(vh_batch *bb, const char *name, double bytes, bool stamped = false,
                 hipStream_t on = nullptr);
    ~ScopedKTimer();
    unsigned long long *stamp() const { return ks; }   // null unless stamped and profiling
};
#define VH_KST_CAP 4096
// a stamped launch's span: thread 0 of every workgroup at its start / end (vector atomics)
__device__ __forceinline__ void kst_begin(unsigned long long *s) {
    if (s && threadIdx.x == 0) atomicMin(s, (unsigned long long)wall_clock64());
}
__device__ __forceinline__ void kst_end(unsigned long long *s) {
    __syncthreads();
    if (s && threadIdx.x == 0) atomicMax(s + VH_KST_CAP, (unsigned long long)wall_clock64());
}

// ---- launchers (defined in vdp.hip / n4.hip / ci.hip) ---------------------------------------
void vh_launch_mask_stats(vh_batch *b);
void vh_launch_vdp_chain(vh_batch *b, const float *d_n4, const vh_run_opts &o);
void vh_launch_snr(vh_batch *b);
void vh_launch_border(vh_batch *b, const uint8_t *d_in, uint8_t *d_out);
// the defect map and border of one thresholding (VH_DEFECT_*) from the resident N4 and scalars; km
// (nullable) also takes the k-means labels.  False, with nothing launched, when the shape has no
// plane-sweep geometry.
bool vh_launch_defect_select(vh_batch *b, const float *d_n4, float thresh, int source, int medfilt,
                             uint8_t *km);
void vh_launch_km_labels(vh_batch *b, const float *d_n4, uint8_t *km);
void vh_launch_n4(vh_batch *b, const vh_n4_params &prm);
void vh_n4_prepare_tables(vh_batch *b, const vh_n4_params &prm);
vh_ci_table *vh_ci_table_build(vh_ctx *ctx, int64_t R, int64_t C, const int16_t *offs, const uint8_t *dup,
                               int64_t rows, const int32_t *bounds, const double *radii, int64_t nbs);
void vh_ci_table_free(vh_ci_table *t);
// form 0: the host-buffer calls (k_ci_walk, int32 shells); 1 / 2: vh_batch_ci with k_ci_walk /
// k_ci_walk_b, shells as int16 in d_ci_shell16
void vh_ci_run(vh_batch *b, const vh_ci_table *t, double minvox, double *d_ci, VolScalars *h_sc = nullptr,
               int form = 0);
int vh_ci_batch_form(const vh_batch *b);   // VH_CI_FORM, read at call time: 1 or 2
void vh_ci_expand(vh_batch *b, double *d_ci);   // d_ci_shell16 -> the float64 map, on the batch's stream
void vh_ci_debug_check();   // VH_DEBUG_BOUNDS builds: raise the CI kernels' first bounds violation
void vh_ensure_n4_workspace(vh_batch *b, const vh_n4_params &prm);

// ---- shared host helpers ----------------------------------------------------------------------
void vh_axis_tables(int n, int ncp, float eps, AxisTab &t);
float vh_bspline_eps(int max_spans);

inline dim3 col_grid(const vh_batch *b) {
    return dim3((unsigned)((b->CZ + VH_TPB - 1) / VH_TPB), (unsigned)b->nb, 1);
}
// row-slab column sweeps: blockIdx.x = slab * col_blocks + column block, slabs of 32 rows (one
// bitmap word of d_colbits / d_colbnz), so a column's rows are walked by R / 32 threads
#define VH_SLAB 32
inline dim3 slab_grid(const vh_batch *b) { return dim3((unsigned)b->slab_blocks, (unsigned)b->nb, 1); }

// calculate_SNR's noise box (Vent_Analysis.py:340-351) for the slab sweeps
struct SnrBox {
    const uint8_t *rowany, *sliceany;
    double *part;                    // [nb][nparts][4]: signal sum, noise sum, noise sum of squares, noise count
    int64_t nparts;
};

// ---- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2key(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// SNR over a 32-row slab: wave 0 sets s_rows[0] = rows inside the noise FOV band (rows 20 ..
// R - 21), s_rows[1] = rows of the box (rows holding mask, row 0 when some row is empty) --
// Vent_Analysis.py:344-351, the quirks as in oracle/vdp_oracle.calculate_snr
__device__ inline void snr_slab_rows(const SnrBox &sb, const VolScalars &s, int64_t b, int64_t R,
                                     int64_t x0, int nr, uint32_t *s_rows) {
    if (threadIdx.x < 64) {
        const int64_t x = x0 + threadIdx.x;
        const bool ok = (int)threadIdx.x < nr;
        const bool fov = ok && x >= 20 && x < R - 20;
        const bool rin = ok && (sb.rowany[b * R + x] || (x == 0 && s.any_row_empty));
        const uint64_t a = __ballot(fov), c = __ballot(rin);
        if (threadIdx.x == 0) { s_rows[0] = (uint32_t)a; s_rows[1] = (uint32_t)c; }
    }
}
// the slab rows of column col that are noise: in the FOV band and outside the box
__device__ inline uint32_t snr_col_noise(const SnrBox &sb, const VolScalars &s, int64_t b,
                                         int64_t Z, int64_t col, const uint32_t *s_rows) {
    const int32_t y = (int32_t)((uint32_t)col / (uint32_t)Z), z = (int32_t)col - y * (int32_t)Z;
    const bool cin = y >= s.cmin && y < s.cmax;
    const bool sin_ = sb.sliceany[b * Z + z] || (z == 0 && s.any_slice_empty);
    return s_rows[0] & ~((cin && sin_) ? s_rows[1] : 0u);
}
// one voxel's contributions (double accumulation, as k_snr always did; a deselected voxel adds
// +0.0, which leaves every sum unchanged).  The noise count is added per slab by snr_count.
__device__ __forceinline__ void snr_add(double (&acc)[4], float v, bool sig, bool noise) {
    const double d = (double)v;
    acc[0] += sig ? d : 0.0;
    const double t = noise ? d : 0.0;
    acc[1] += t;
    acc[2] += t * t;
}
__device__ __forceinline__ void snr_count(double (&acc)[4], uint32_t noise) {
    acc[3] += (double)__popc(noise);
}
// block sums of the 4 partials in a fixed order -> dst[0..3]
__device__ inline void snr_block_write(double (&acc)[4], double (*s_red)[VH_TPB / 64], double *dst) {
    for (int q = 0; q < 4; ++q) {
        double x = acc[q];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0) s_red[q][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double x = 0.0;
        for (int w = 0; w < VH_TPB / 64; ++w) x += s_red[threadIdx.x][w];
        dst[threadIdx.x] = x;
    }
}

// export.hip (rendering after the hot path)
void vh_overlay_launch(hipStream_t s, const float *d_n4, const uint8_t *d_def, int64_t R, int64_t C,
                       int64_t Z, int64_t nb, uint32_t *d_mm, uint8_t *d_rgb);
// the batch renderings (vh_batch_overlay is vh_overlay_launch on the resident buffers)
void vh_crop_layout_launch(vh_batch *b);   // -> d_mt_crop, from the last run's mask statistics
void vh_montage_b_launch(vh_batch *b, bool proton, int64_t prow, bool ci_on);
// dist.hip: the distribution sweep over the resident N4, mask, defect map and LB classes into
// d_dist_hist / d_dist_out / d_dist_sl (zeroed first); vh_dist_takes: the slice counters fit in LDS
#define VH_DIST_MAX_Z 1900
bool vh_dist_takes(const vh_batch *b);
void vh_dist_launch(vh_batch *b, int norm, int n_bins, float hi, float scale);
// denoise.hip: the non-local-means filter of every study, src -> dst (two volumes of the batch), with
// d_prm [nb][2] = inv_h2, bias; vh_denoise_takes: the grid fits.  vh_noise_sigma_launch: d_snrpart
// (after vh_launch_snr) -> d_sigma [nb]
bool vh_denoise_takes(const vh_batch *b);
void vh_denoise_launch(vh_batch *b, const float *src, float *dst, const float *d_prm, int S, int P, int rician);
void vh_noise_sigma_launch(vh_batch *b, float *d_sigma);
// heterogeneity.hip: the CoV map of every study of src (a volume of the batch) over the resident mask,
// without the voxels of defect (nullable) != 0, into map [nb][V], with its summary in d_hist
// [nb][n_bins] and d_stats [nb][4] (both zeroed here); vh_het_takes: the grid fits
bool vh_het_takes(const vh_batch *b);
void vh_het_launch(vh_batch *b, const float *src, const uint8_t *defect, float *map, uint32_t *d_hist,
                   unsigned long long *d_stats, int K, int min_count, int n_bins, float hi, float scale);
// depth.hip: the saturated squared distance to the mask's edge of every study into map [nb][V], with the
// band counts over thr [n_thr] (host) in d_counts [nb][n_thr + 1][2] and d_stats [nb][2] (both zeroed
// here), the defect column from defect (nullable: 0); d_g [nb][V] is its scratch, the column distances;
// vh_depth_takes: the grid fits; vh_depth_form: 0 when the shape's search runs on rows staged in LDS,
// 1 when a row is too long for that and it reads g through the caches
int vh_depth_form(int64_t R, int64_t C, int64_t Z);
bool vh_depth_takes(const vh_batch *b);
void vh_depth_launch(vh_batch *b, const uint8_t *defect, const uint16_t *thr, int n_thr, uint16_t *d_g, uint16_t *map,
                     unsigned long long *d_counts, unsigned long long *d_stats);
// components.hip: the connected components of src [nb][V] (nonzero: set) under conn (4, 8, 6, 26): the
// roots and sizes into root / size [nb][V], the class counts over edges [n_edges] (host) into d_counts
// [nb][n_edges + 1][2] and the summary into d_stats [nb][4] = n_set, n_comp, the largest component's key
// size << 32 | ~root (0: none), unused (both zeroed here).  vh_cc_filter_launch: clears in src the voxels
// whose component (root / size of a labelling of src as it stands) is below d_min [nb] voxels or, where
// d_keep [nb] = k > 0, not among the k largest; kmax = the largest d_keep (<= 8); d_picks [nb][8] is its
// scratch, d_kept [nb][2] = components, voxels kept (both zeroed here).  vh_cc_takes: the grid fits
bool vh_cc_takes(const vh_batch *b);
void vh_cc_launch(vh_batch *b, const uint8_t *src, int conn, const uint32_t *edges, int n_edges, int *root,
                  uint32_t *size, unsigned long long *d_counts, unsigned long long *d_stats);
void vh_cc_filter_launch(vh_batch *b, uint8_t *src, const int *root, const uint32_t *size, const uint32_t *d_min,
                         const int32_t *d_keep, int kmax, unsigned long long *d_picks, unsigned long long *d_kept);
// defect_table.hip: the rows of the components in d_cc_root / d_cc_size with at least d_dt_min [nb]
// voxels, at most max_rows (1..1024) a study, into d_dt_rows [nb][max_rows][VH_DT_COLS] and d_dt_stats
// [nb][4]; norm VH_NORM_* reads the run's N4 and scalars for columns 14..17, VH_DT_NO_SIGNAL leaves them 0.
// Every d_dt_* buffer is reserved by the caller (d_dt_min filled); the others are scratch, zeroed here.
// vh_dt_takes: the grid fits
bool vh_dt_takes(const vh_batch *b);
void vh_dt_launch(vh_batch *b, int max_rows, int norm);
// zones.hip: the zone maps (labels: d_zn_map holds the caller's bytes, else the rule of zones_host.h over
// parts, lateral, by) into d_zn_map with the geometry in d_zn_geom, and the counts of the K + 1 zones over
// the resident N4, mask, defect map, LB classes and zone map into d_zn_counts / d_zn_hist / d_zn_stats
// (zeroed here); vh_zones_takes: the grid fits
bool vh_zones_takes(const vh_batch *b);
void vh_zones_launch(vh_batch *b, bool labels, int K, const int32_t parts[3], int lateral, int by, int norm,
                     int n_bins, float hi, float scale);
// mask_edit.hip: one disc dilation (erode 0) or erosion (erode 1) of every study, src -> dst (two
// mask volumes of the batch), with d_radius [nb] in 0..5 (0: the study is copied);
// vh_mask_edit_takes: the grid fits.  vh_mask_paint_launch: mask = paint(mask != 0, strokes != 0) in
// place, both [nb][V].  vh_mask_count_launch: d_cnt [nb] (zeroed by the caller) += voxels != 0
bool vh_mask_edit_takes(const vh_batch *b);
void vh_mask_morph_launch(vh_batch *b, const uint8_t *src, uint8_t *dst, const int32_t *d_radius, int erode);
void vh_mask_paint_launch(vh_batch *b, uint8_t *mask, const uint8_t *strokes, int how);
void vh_mask_count_launch(vh_batch *b, const uint8_t *mask, unsigned long long *d_cnt);
// segment.hip: vh_proton_stats_launch: the maximum (as bits) and the 256-bin histogram of every study's
// proton (both zeroed here).  vh_segment_launch: seg [nb][V] = the dark pixels of every slice that the
// slice border does not reach, as 0 / 1 bytes, with d_thresh [nb]; vh_segment_takes: the plane is at
// most 512 x 512 and the grid fits.  vh_mask_overlap_launch: d_cnt [nb][3] (zeroed by the caller) +=
// |a != 0|, |o != 0|, |both|, a and o [nb][V] from an allocation's start each
void vh_proton_stats_launch(vh_batch *b, const float *proton, uint32_t *d_pmax_bits, uint32_t *d_hist);
bool vh_segment_takes(const vh_batch *b);
void vh_segment_launch(vh_batch *b, const float *proton, uint8_t *seg, const float *d_thresh);
void vh_mask_overlap_launch(vh_batch *b, const uint8_t *a, const uint8_t *o, unsigned long long *d_cnt);
// the maximum sweep of segment.hip alone: d_max_bits [nb] (zeroed by the caller) = the bit pattern of
// every study's maximum over its finite voxels >= 0; timing class "segment_max_b"
void vh_seg_max_launch(vh_batch *b, const float *x, uint32_t *d_max_bits);
// register.hip: vh_register_launch: the maxima (d_maxb [2][nb]), the codes (d_cp, d_cx [nb][V]), the
// joint histogram of every shift of the search window (d_hist [nb][ns][32][32], zeroed here) and the
// scores (d_score [nb][ns]) of proton against hp; vh_register_takes: the grid fits.
// vh_shift_launch_*: dst(v) = src(v + shift[study]) inside the volume, 0 elsewhere, d_shift [nb][3]
#define RG_INVALID 255u
#define RG_BINS 1024                // 32 x 32
// in F: finite and >= 0 (NaN fails both comparisons; -0.0 is in F and counts as +0.0), as segment.hip
__device__ __forceinline__ bool rg_in_f(float x) { return x >= 0.0f && x <= 3.402823466e+38f; }
// min(255, (int)(x * scale)) >> 3, the product rounded to float32 (one that is not below 255 -- NaN from
// an infinite scale times zero included -- is bin 255, as in k_seg_hist); 255 outside F
__device__ __forceinline__ uint32_t rg_code(float x, float scale) {
    if (!rg_in_f(x)) return RG_INVALID;
    const float p = __fmul_rn(x, scale);
    return (uint32_t)(p < 255.0f ? (int)p : 255) >> 3;
}
bool vh_register_takes(const vh_batch *b);
void vh_register_launch(vh_batch *b, const float *proton, const float *hp, const int32_t search[3],
                        uint32_t *d_maxb, uint8_t *d_cp, uint8_t *d_cx, uint32_t *d_hist, double *d_score);
void vh_register_score_launch(vh_batch *b, const uint32_t *d_hist, const uint32_t *d_maxb, int ns, double *d_score);
void vh_shift_launch_f32(vh_batch *b, const float *src, float *dst, const int32_t *d_shift);
void vh_shift_launch_u8(vh_batch *b, const uint8_t *src, uint8_t *dst, const int32_t *d_shift);
// resample.hip: the tap tables of one study's map as the kernel reads them, 10 (R + C + Z) words: for
// each axis a of n = R, C, Z in turn first int32 [n], count int32 [n], weight float [n][8].
// vh_resample_plan picks the tile and the band from the tables of the whole batch (host copy, [nb] such
// blocks) and says whether the grid fits; vh_resample_launch: dst [nb][R][C][Z] = the resampling of src
// [nb][Rs][Cs][Zs] with d_tab, the device copy of the same tables
struct RsPlan {
    int Rs, Cs, Zs;      // the source shape
    int TC, TZ;          // destination columns and slices of a workgroup's tile
    int BR;              // destination rows of its band
    int span;            // source rows staged for a band: the largest over studies and bands
    int ntc, ntz, nbands;
    int kc, kz;          // the most c-taps of a column and z-taps of a slice in the batch
};
bool vh_resample_plan(const vh_batch *b, const int64_t src_shape[3], const int32_t *h_tab, RsPlan &p);
void vh_resample_launch(vh_batch *b, const RsPlan &p, const float *src, float *dst, const int32_t *d_tab);
// segment.hip's maximum sweep over n voxels per study instead of the batch's V (a source on its own grid)
void vh_seg_max_launch_n(vh_batch *b, const float *x, int64_t n, uint32_t *d_max_bits);
// register_maps.hip: the tap tables of one study's candidate lists as the kernel reads them,
// 10 (Kr R + Kc C + Kz Z) words: the Kr tables of the r list (each first int32 [R], count int32 [R], weight
// float [R][8], as RsTabs), then the Kc of the c list, then the Kz of the z list.  vh_register_maps_plan
// picks the tile, the band and the chunk of the r list from the tables of the whole batch (host copy) and
// says whether the grid fits; vh_register_maps_launch: the maxima (d_maxb [2][nb]: source, HPvent), the
// xenon codes (d_cx [nb][V]), the joint histogram of every candidate (d_hist [nb][nc][32][32], zeroed
// here) and the scores (d_score [nb][nc]) of src [nb][Rs][Cs][Zs] against hp
struct RmPlan {
    int Rs, Cs, Zs;      // the source shape
    int R, C, Z;         // the batch's
    int Kr, Kc, Kz;      // the candidates of each list
    int TC, TZ;          // destination columns and slices of a workgroup's tile
    int BR;              // destination rows of its band
    int span;            // source rows staged for a band and a chunk: the largest over studies, bands, chunks
    int ntc, ntz, nbands;
    int chunk, nchunks;  // r candidates a workgroup serves; chunks of the r list
};
bool vh_register_maps_plan(const vh_batch *b, const int64_t src_shape[3], const int32_t count[3],
                           const int32_t *h_tab, RmPlan &p);
void vh_register_maps_launch(vh_batch *b, const RmPlan &p, const float *src, const float *hp, const int32_t *d_tab,
                             uint32_t *d_maxb, uint8_t *d_cx, uint32_t *d_hist, double *d_score);
void vh_recon_run(hipStream_t st, const double2 *d_in, double2 *d_tmp, double2 *d_out, double2 *d_tw0,
                  double2 *d_tw1, int64_t n0, int64_t n1, int64_t nz);
void vh_montage_run(hipStream_t s, int64_t R, int64_t C, int64_t Z, const void *proton, int p64,
                    const void *hp, int h64, const float *n4, const uint8_t *mborder,
                    const uint8_t *def, const double *ci, const double *parula, int64_t prow,
                    const int64_t crop[6], uint8_t *image);
