/* vent_hip.h -- C-ABI of libventhip.so, the MI355X (gfx950) implementation of the Vent_Analysis
 * voxel hot path (N4 -> mean-anchored / linear-binning / k-means VDP -> defect morphology -> CI).
 *
 * Plain C types only (no torch, no HIP types).  Every function returns an int status (VH_OK = 0)
 * and never throws across the boundary; vh_last_error() gives the message of the last failure on
 * a context.  Host buffers are caller-allocated and C-contiguous in numpy's (rows, cols, slices)
 * order (slice axis fastest, as Vent_Analysis.openSingleDICOM produces, Vent_Analysis.py:179);
 * device buffers are owned by the library.  A context is bound to one GPU; each batch owns its HIP
 * stream.  The host-buffer entry points (vh_n4 ... vh_ci) share a per-context scratch batch behind a
 * per-context mutex, so a context may be used from several host threads; batches are independent.
 *
 * Reference interface each entry point replaces (file:line in thomenr/Vent_Analysis):
 *   vh_n4        Vent_Analysis.N4_bias_correction            Vent_Analysis.py:316-334
 *   vh_snr       Vent_Analysis.calculate_SNR                 Vent_Analysis.py:337-357
 *   vh_border    Vent_Analysis.calculateBorder               Vent_Analysis.py:225-231
 *   vh_vdp       Vent_Analysis.calculate_VDP (post-N4 part)  Vent_Analysis.py:239-263
 *   vh_ci        CI.calculate_CI + Vent_Analysis.calculate_CI CI.py:107-145, Vent_Analysis.py:265-271
 *   vh_ci_table_* / vh_ci_tab  the same with the sphere table resident in HBM (CI.getSpherePix's
 *                cached table, CI.py:33-63, uploaded once)
 *   vh_overlay   Vent_Analysis.exportDICOM (pixel data)       Vent_Analysis.py:381-428
 *   vh_montage   Vent_Analysis.screenShot (montage array)     Vent_Analysis.py:458-520
 *   vh_recon     Vent_Analysis.process_RAW (k-space -> image) Vent_Analysis.py:537-540
 *   vh_batch_*   the same pipeline over a device-resident batch of studies (build-defined)
 *   vh_batch_ci / vh_batch_set_defect / vh_batch_download_ci  calculate_CI of the batch's resident
 *                defect maps (Vent_Analysis.py:265-271) with a per-study status and an int16 shell
 *                map; a vh_ci_table may be destroyed as soon as vh_batch_ci has returned
 *   vh_batch_select_defect / vh_batch_download_defect / vh_batch_km_cuts / vh_defect_map  the defect
 *                map, border and count of the linear-binning or k-means VDP (or the mean-anchored
 *                one again), and the k-means label map, so calculate_CI / exportDICOM / screenShot
 *                can show the defect any of calculate_VDP's three percentages counts (build-defined)
 *   vh_batch_overlay / vh_batch_download_overlay  exportDICOM's pixel data (Vent_Analysis.py:387-393)
 *                of every study from the batch's resident N4 and defect maps
 *   vh_batch_montage_layout / vh_batch_montage / vh_batch_download_montage  cropToData(mask, border=5)
 *                (Vent_Analysis.py:430-456) and screenShot's montage array (:467-495) of every study
 *                from the resident buffers, with calculateBorder(mask) (:225-231) evaluated in place;
 *                only pixels come back.  Their kernel-timing classes are "overlay_b" and "montage_b"
 *                (vh_batch_kernel_time reads them; vh_batch_kernel_names does not list them)
 *   vh_batch_distribution / vh_batch_download_distribution / vh_distribution  the histogram of the
 *                normalised masked signal ("show histogram?", the open item of the reference's list,
 *                Vent_Analysis.py:1019-1026), all six linear-binning class counts (:256; the reference
 *                reports classes 1+2 only, :257) and the slice-wise mask / defect counts, per study from
 *                the resident buffers (build-defined); kernel-timing class "dist_b", not listed either
 *   vh_batch_heterogeneity / vh_batch_download_heterogeneity / vh_heterogeneity  the local
 *                coefficient of variation of the masked signal in a small in-plane window, as a map
 *                specified to the last bit and as exact integer counts whose mean is the ventilation
 *                heterogeneity index, per study from the resident buffers (build-defined);
 *                kernel-timing class "het_b", not listed
 *   vh_batch_core_rind / vh_batch_download_core_rind / vh_core_rind / vh_core_rind_form  the core-rind
 *                analysis: the exact squared in-plane distance of every mask voxel to the mask's edge,
 *                as a map, and the mask and defect voxels of every depth band, per study from the
 *                resident mask and defect map (build-defined); kernel-timing class "depth_b", not listed
 *   vh_batch_components / vh_batch_download_components / vh_batch_filter_components / vh_components /
 *                vh_filter_components  the connected components (4, 8, 6 or 26 neighbours) of the resident
 *                defect map or mask: the canonical root and the size of every voxel's component, counts
 *                per size class, and a filter by size and by rank (build-defined); kernel-timing class
 *                "comp_b", not listed
 *   vh_batch_defect_table / vh_batch_download_defect_table  the defect table: one row per component of
 *                the last vh_batch_components, largest first, with exact integer moments, the bounding
 *                box, the exposed-face counts and fixed-point signal sums (build-defined); kernel-timing
 *                class "dtab_b", not listed
 *   vh_batch_zones / vh_batch_download_zones / vh_zones / vh_zone_parts / vh_zone_split  the regional
 *                analysis: a zone map (left / right lung, thirds, a grid of parts, or the caller's label
 *                volume) and per zone the mask, defect and linear-binning class counts and the histogram
 *                of the normalised signal, per study from the resident buffers (build-defined);
 *                kernel-timing class "zones_b", not listed
 *   vh_batch_noise_sigma / vh_batch_denoise / vh_batch_download_hp / vh_noise_sigma / vh_denoise
 *                the "Denoise Option" of the reference's list (Vent_Analysis.py:1025): an in-plane
 *                non-local-means filter of the resident HPvent, specified to the last bit, and the
 *                noise estimate it needs (build-defined); kernel-timing class "denoise_b", not listed
 *   vh_batch_edit_mask / vh_batch_paint_mask / vh_batch_download_mask / vh_edit_mask
 *                the "edit mask" item of the reference's list (Vent_Analysis.py:1023): per-slice disc
 *                erosion, dilation, opening and closing of the resident masks, paint strokes, and the
 *                mask read back with its voxel count (build-defined); kernel-timing class
 *                "mask_edit_b", not listed
 *   vh_batch_upload_proton / vh_batch_proton_threshold / vh_batch_segment / vh_batch_mask_overlap /
 *   vh_otsu / vh_segment
 *                the "automatic segmentation using proton" item, the last of the reference's list
 *                (Vent_Analysis.py:1024): an Otsu threshold of the proton image, the dark regions of every
 *                slice that its border does not reach, and an opening, specified to the byte; and the
 *                overlap counts against another mask (build-defined); kernel-timing class "segment_b",
 *                not listed
 *   vh_batch_upload_proton_src / vh_batch_resample_proton / vh_batch_download_proton_src /
 *   vh_resample_taps / vh_resample
 *                a proton on its own grid (another matrix, pixel size or slice spacing) resampled onto the
 *                batch's by a separable anti-aliased linear filter, specified to the last bit
 *                (build-defined); kernel-timing class "resample_b", not listed
 *   vh_batch_register_maps / vh_batch_download_register_maps_hist / vh_register_maps_pick /
 *   vh_axis_candidates / vh_register_maps
 *                the fine registration: a grid of candidate maps (scale x sub-voxel offset per axis) of
 *                the resident source proton scored against the HPvent by mutual information, resampled,
 *                coded and counted in one kernel (build-defined); kernel-timing class "register_maps_b",
 *                not listed
 *   vh_pipe_*   the batch pipeline fed from host memory with overlapped transfers (build-defined)
 *   vh_comm_*    cohort histogram all-reduce over RCCL (build-defined, BASELINE config 4)
 */
#ifndef VENT_HIP_H
#define VENT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_ABI_VERSION 8

/* status codes */
#define VH_OK 0
#define VH_ERR_ARG 1          /* bad argument (maps to ValueError/TypeError in the shim) */
#define VH_ERR_HIP 2          /* HIP runtime failure */
#define VH_ERR_NOMEM 3        /* device allocation failed */
#define VH_ERR_MAXRADIUS 4    /* CI: sphere reached the table's last radius (CI.py:101-103, ValueError) */
#define VH_ERR_EMPTY 5        /* empty mask / defect list (Vent_Analysis.py:270 IndexError) */
#define VH_ERR_RCCL 6         /* RCCL failure */
#define VH_ERR_NODEV 7        /* no GPU visible */
#define VH_ERR_INDEX 8        /* index out of range (maps to IndexError): screenShot's parula lookup */

typedef struct vh_ctx vh_ctx;
typedef struct vh_batch vh_batch;
typedef struct vh_ci_table vh_ci_table;

/* N4 parameters; vh_n4_default_params() fills the SimpleITK 2.3.1 defaults the reference runs with
 * (Vent_Analysis.py:330: no setter is called).  ncp is given per numpy axis (rows, cols, slices). */
typedef struct {
    int32_t n_levels;        /* 4  = len(MaximumNumberOfIterations) */
    int32_t max_iters[8];    /* 50, 50, 50, 50 */
    float conv_threshold;    /* 0.001 */
    int32_t ncp[3];          /* 4, 4, 4 control points per axis at level 0 */
    int32_t spline_order;    /* 3 (only 3 supported) */
    int32_t n_bins;          /* 200 histogram bins (<= 256) */
    float wiener_noise;      /* 0.01 */
    float fwhm;              /* 0.15 bias-field FWHM */
    int32_t conv_mode;       /* 0 (default): ITK's convergence measure -- the float (RealType) Welford
                                recurrence over the masked voxels in raster order, whose rounding
                                drift sets SimpleITK's iteration counts; a serial recurrence.
                                1: the exact coefficient of variation it approximates (double,
                                order-free; faster, but stops at different iterations than
                                SimpleITK -- see DESIGN.md §6) */
} vh_n4_params;

/* Per-volume scalars of calculate_VDP / calculate_CI (metadata keys of Vent_Analysis.py:78-103). */
typedef struct {
    double vdp;              /* metadata['VDP']        100*sum(defect)/sum(mask)            :251 */
    double vdp_lb;           /* metadata['VDP_lb']     100*count(LB in {1,2})/sum(mask)     :257 */
    double vdp_km;           /* metadata['VDP_km']     build-defined 1-D k-means (k=4)       :259-261 */
    double defect_volume;    /* metadata['DefectVolume'] litres                              :252 */
    double lung_volume;      /* metadata['LungVolume']   litres                              :166 */
    double km_centres[4];
    double snr;              /* metadata['SNR'] (double accumulation; the shim casts to HPvent's
                                float dtype like numpy)                                      :241 */
    float mean_anchor;       /* np.mean(sorted masked N4) (float32, numpy reduction order)  :246 */
    float p99;               /* sorted[int(0.99 n)]                                          :255 */
    int64_t n_mask;          /* voxels with mask > 0 */
    int64_t n_defect;
    int64_t n_lb12;
    int64_t n_km0;
    int32_t n4_iters[8];     /* N4 iterations executed per level (0 when N4 skipped) */
    float n4_conv[8];        /* last convergence measure per level */
} vh_vdp_result;

/* Options for vh_batch_run. */
typedef struct {
    int32_t do_n4;           /* 1: N4 on HPvent (calculate_VDP);  0: N4 := identity (HPvent) */
    vh_n4_params n4;
    float thresh;            /* mean-anchored threshold (calculate_VDP thresh=0.6) */
    int32_t do_snr;
    int32_t do_kmeans;
    int32_t do_cohort;       /* accumulate the cohort histogram (1024 u64 bins, [0,1.5) of p99-normalised masked N4) */
    int32_t profile;         /* 1: time kernel classes with HIP events (vh_batch_kernel_time) */
    double vox[3];           /* voxel size (mm) for the volume scalars */
    int32_t n4_subbatch;     /* volumes per N4 sub-batch (0 = whole batch); smaller sub-batches
                                keep an iteration's working set in the 256 MiB Infinity Cache */
    int32_t morph3d;         /* build-defined 3-D morphology (BASELINE config 5): 3x3x3 majority
                                (>= 14 of 27, zero padded) and np.gradient != 0 along all three
                                axes, instead of the reference's per-slice medfilt2d / 2-D border */
    int32_t n4_mode;         /* N4 driver: 0 auto, 1 per-iteration sweeps over the batch (any size),
                                2 volume-resident (one workgroup per study, the whole iteration
                                loop in one launch; studies whose N4 state fits in LDS),
                                3 grid form (each study over G cooperating workgroups, one
                                launch per study; auto picks it for a batch of one study) */
} vh_run_opts;

#define VH_COHORT_BINS 1024

/* ---- library / context ---------------------------------------------------------------------- */
int vh_abi_version(void);
const char *vh_status_string(int status);
int vh_device_count(int *n);
void vh_n4_default_params(vh_n4_params *p);
void vh_default_run_opts(vh_run_opts *o);
int vh_create(int device, vh_ctx **out);
int vh_destroy(vh_ctx *ctx);
const char *vh_last_error(const vh_ctx *ctx);
int vh_synchronize(vh_ctx *ctx);

/* ---- host-buffer entry points (one call = upload, compute, download) --------------------------
 * hp: float32, mask: uint8 0/1, shapes [batch][R][C][Z]. */
int vh_n4(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
          int64_t batch, const vh_n4_params *prm, float *out, int32_t *iters /* [batch][n_levels] */,
          float *conv /* [batch][n_levels], nullable */);
int vh_border(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch,
              uint8_t *border);
int vh_snr(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
           int64_t batch, double *snr);
/* calculate_VDP after N4.  hp may be NULL (no SNR).  Outputs: defect / defect_border / lb uint8
 * volumes (any may be NULL), res[batch]. */
int vh_vdp(vh_ctx *ctx, const float *hp, const float *n4, const uint8_t *mask, int64_t R,
           int64_t C, int64_t Z, int64_t batch, float thresh, const double vox[3],
           uint8_t *defect, uint8_t *defect_border, uint8_t *lb, vh_vdp_result *res);
/* Host-buffer form of vh_batch_select_defect / vh_batch_download_defect (declared below) for one
 * call: the post-N4 chain (no N4, no SNR) on the scratch batch, then the selection.  Outputs
 * nullable; VH_ERR_EMPTY for an empty-mask study, like vh_vdp. */
int vh_defect_map(vh_ctx *ctx, const float *n4, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                  int64_t batch, float thresh, int source, int medfilt,
                  uint8_t *defect, uint8_t *border, uint8_t *km, int64_t *count);
/* Cluster index map.  The sphere table comes from the host (reference-identical rows; see
 * vent_analysis_amd/sphere.py): offs int16 [rows][3] (dx,dy,dz), dup uint8 [rows], bounds int32
 * [nb] prefix lengths, radii float64 [nb] (= r[b-1]).  Outputs: ci_array float64 volume,
 * ci_scalar[batch] (95th-percentile CV, Vent_Analysis.py:268-270), shell int32 volume (nullable). */
int vh_ci(vh_ctx *ctx, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
          const int16_t *offs, const uint8_t *dup, int64_t rows, const int32_t *bounds,
          const double *radii, int64_t nb, double minvox, double *ci_array, double *ci_scalar,
          int32_t *shell);
/* The sphere table uploaded once for volumes of R rows and C columns (the px2vec stride of
 * CI.py:65-68): the same arrays as vh_ci; it stays in HBM until vh_ci_table_destroy.  vh_ci_tab is
 * vh_ci with such a table (ci_array and shell nullable): no per-call table work or upload.
 * vh_ci_table_destroy waits for every user of the table first: the host-buffer calls of other
 * threads, and the work vh_batch_ci enqueued with it on any batch's stream. */
int vh_ci_table_create(vh_ctx *ctx, int64_t R, int64_t C, const int16_t *offs, const uint8_t *dup,
                       int64_t rows, const int32_t *bounds, const double *radii, int64_t nb,
                       vh_ci_table **out);
int vh_ci_table_destroy(vh_ci_table *t);
int vh_ci_tab(vh_ctx *ctx, const uint8_t *defect, int64_t R, int64_t C, int64_t Z, int64_t batch,
              const vh_ci_table *t, double minvox, double *ci_array, double *ci_scalar, int32_t *shell);

/* ---- device-resident batch pipeline ---------------------------------------------------------- */
int vh_batch_create(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t batch, vh_batch **out);
int vh_batch_destroy(vh_batch *b);
int vh_batch_upload(vh_batch *b, const float *hp, const uint8_t *mask);
int vh_batch_run(vh_batch *b, const vh_run_opts *opts);      /* enqueue; returns before the GPU ends */
int vh_batch_sync(vh_batch *b);
int vh_batch_download(vh_batch *b, float *n4, uint8_t *defect, uint8_t *defect_border, uint8_t *lb,
                      vh_vdp_result *res /* [batch] */);
/* CI of the batch's resident defect maps, enqueued on the batch's stream; returns before the GPU ends.
 * The maps are the last vh_batch_run's or vh_batch_set_defect's; t is a table of the batch's context
 * and (R, C) with at most 32767 shells.  Leaves the batch's maps and VDP results as they are.
 * VH_CI_FORM (read at call time) picks the walk kernel: 0 / unset auto, 1 the one-study kernel of
 * vh_ci over the batch, 2 the batch form. */
int vh_batch_ci(vh_batch *b, const vh_ci_table *t, double minvox);
/* Replace the resident defect maps (uint8 [nb][V], nonzero = defect): CI of edited or stored maps. */
int vh_batch_set_defect(vh_batch *b, const uint8_t *defect);
/* Waits for the stream.  ci_array f64 [nb][V] and shell int16 [nb][V] (the index into the table's
 * radii, -1 off-defect) are nullable; ci_scalar[nb]; status[nb] is VH_OK, VH_ERR_EMPTY or
 * VH_ERR_MAXRADIUS per study: such a study's scalar is 0.0 and the call still returns VH_OK. */
int vh_batch_download_ci(vh_batch *b, double *ci_array, int16_t *shell, double *ci_scalar, int32_t *status);
/* The defect map of any of the three thresholdings calculate_VDP reports, built on the device from
 * the last vh_batch_run's N4 and scalars.  Each source has a raw map: MEAN float32(N4 / mean_anchor)
 * < thresh (the run's thresh), LB the voxels of linear-binning class 1 or 2, KM the voxels of the
 * lowest non-empty k-means cluster; all inside mask != 0.  medfilt 0 keeps the raw map (2-D border),
 * 1 applies the reference's per-slice 3x3 zero-padded median (2-D border), 2 the build-defined
 * 3x3x3 majority (3-D border), as vh_run_opts.morph3d does.  MEAN with medfilt 1 (2 after a morph3d
 * run) reproduces the run's own defect / defect_border byte for byte. */
#define VH_DEFECT_MEAN 0
#define VH_DEFECT_LB   1
#define VH_DEFECT_KM   2
/* Rebuild the resident defect map and border from the last vh_batch_run's N4 and scalars (enqueue
 * only).  Replaces what vh_batch_run / vh_batch_set_defect left in them; vh_batch_ci, vh_batch_download
 * then see the selected map.  The run's vh_vdp_result values are left as they are.  VH_ERR_ARG,
 * with nothing enqueued: source or medfilt out of range, no vh_batch_run yet, KM after a run with
 * do_kmeans = 0, a shape the plane sweep does not take (more than 816 slices). */
int vh_batch_select_defect(vh_batch *b, int source, int medfilt);
/* Waits for the stream.  All nullable: defect / border / km uint8 [nb][V]; count int64 [nb] (voxels
 * of the selected map; the run's own defect count when no selection followed it); km is computed on
 * demand (needs do_kmeans): 0 off-mask, else 1 + the voxel's cluster in k-means' final partition
 * (an empty cluster's index is skipped: two distinct values give labels 1 and 4). */
int vh_batch_download_defect(vh_batch *b, uint8_t *defect, uint8_t *border, uint8_t *km, int64_t *count);
/* The three k-means cut values per study: the smallest value of clusters 1..3, +inf where the cut
 * is at n; float [nb][3].  (For a histogram display with the cluster edges.) */
int vh_batch_km_cuts(vh_batch *b, float *cuts);
int vh_batch_cohort_hist(vh_batch *b, uint64_t *hist /* [VH_COHORT_BINS] */);
/* Kernel-class timing from HIP events on the context stream (opts.profile = 1).  name is one of
 * the classes listed by vh_batch_kernel_names (';'-separated). */
const char *vh_batch_kernel_names(void);
/* Discard accumulated kernel timings (timings accumulate over vh_batch_run calls). */
int vh_batch_reset_timers(vh_batch *b);
int vh_batch_kernel_time(vh_batch *b, const char *name, double *total_ms, int64_t *launches,
                         double *bytes_per_launch);

/* Kernel-class timing of the host-buffer entry points (vh_ci, vh_vdp, ...): on = 1 makes them time
 * their kernel classes with HIP events on the context's scratch batch (timings accumulate; setting
 * the switch discards them); vh_ctx_kernel_time reads them like vh_batch_kernel_time. */
int vh_ctx_profile(vh_ctx *ctx, int on);
int vh_ctx_kernel_time(vh_ctx *ctx, const char *name, double *total_ms, int64_t *launches);

/* Per-study wall time (microseconds, device wall clock) of the last vh_batch_run's volume-resident
 * N4 kernel (one workgroup per study: the slowest study bounds the launch); zeros when that run did
 * not use it.  us[batch]. */
int vh_batch_study_times(vh_batch *b, double *us);

/* ---- rendering after the hot path ---------------------------------- */
/* exportDICOM's pixel data (Vent_Analysis.py:387-393): BW = uint8(normalize(|N4HPvent|) * 255) in
 * float32, RGB = (BW*(defect==0) + 255*(defect==1), BW*(defect==0), BW*(defect==0)).  n4 float32
 * and defect uint8 volumes [batch][R][C][Z]; rgb uint8 [batch][Z][R][C][3] -- the frame order of
 * np.transpose(RGB, (2,0,1,3)) (:393) and, frame by frame, the PACS branch's RGB[:,:,i,:] (:411). */
int vh_overlay(vh_ctx *ctx, const float *n4, const uint8_t *defect, int64_t R, int64_t C, int64_t Z,
               int64_t batch, uint8_t *rgb);
/* screenShot's montage array (Vent_Analysis.py:467-495) before the text overlay: the 7 x ns grid
 * (blank, blank, proton, HPvent, N4 + mask border, N4 + defects, N4 + parula CI) over the crop
 * crop = {r0, nr, c0, nc, s0, ns} (cropToData(mask, border=5), :430-456), as uint8(IMAGE * 255)
 * [7 nr][ns nc][3].  proton / hp are float32 (is64 = 0) or float64 (is64 = 1); ci float64 or NULL
 * (the reference's blank CI panel); parula float64 [prow][3].  A CI colour index outside the table
 * returns VH_ERR_INDEX (IndexError), a NaN CI VH_ERR_ARG (ValueError). */
int vh_montage(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, const void *proton, int proton_is64,
               const void *hp, int hp_is64, const float *n4, const uint8_t *mask_border,
               const uint8_t *defect, const double *ci, const double *parula, int64_t prow,
               const int64_t crop[6], uint8_t *image);

/* ---- the same renderings of a device-resident batch ------------------------------------------
 * They read what vh_batch_run left resident and bring back pixels only; nothing the run, vh_batch_ci
 * or the selection calls wrote is changed.  Each needs a vh_batch_run on the batch (VH_ERR_ARG
 * otherwise); a new run discards what they enqueued.
 *
 * vh_batch_overlay enqueues vh_overlay for every study: N4 is the volume the last run's chain read
 * (HPvent when do_n4 = 0), defect the resident map as it stands (the run's, vh_batch_set_defect's or
 * vh_batch_select_defect's).  VH_ERR_ARG, with nothing enqueued, for more than 65535 studies or rows.
 * vh_batch_download_overlay waits; rgb uint8 [nb][Z][R][C][3], study i's block byte for byte what
 * vh_overlay returns for that study's downloaded N4 and defect map. */
int vh_batch_overlay(vh_batch *b);
int vh_batch_download_overlay(vh_batch *b, uint8_t *rgb);
/* Where every study's montage lies (waits; the result is kept until the next run).  crop[i] =
 * {r0, nr, c0, nc, s0, ns} is cropToData(mask, border=5) of study i's resident mask: a row, column
 * or slice is non-empty when its mask sum is > 0, index 0 never counts (the reference's quirk), rows
 * and columns widen by 5 and clamp, slices do not.  Study i's image, uint8 [7 nr][ns nc][3], starts
 * at byte offset[i] of the compact buffer (a multiple of 64) and has 21 nr nc ns bytes; offset[nb] is
 * the buffer's size.  A study for which the reference raises IndexError (no counted row, column or
 * slice: an empty mask, a mask only at index 0) has status[i] = VH_ERR_EMPTY, a crop of zeros and no
 * image; the call still returns VH_OK.  All three outputs are nullable. */
int vh_batch_montage_layout(vh_batch *b, int64_t *crop /* [nb][6] */, int64_t *offset /* [nb + 1] */,
                            int32_t *status /* [nb] */);
/* Enqueue vh_montage for every study over its crop: proton float32 [nb][V] (NULL: zeros, what the
 * class substitutes for a missing proton image), HPvent and N4 the resident volumes (N4 as for
 * vh_batch_overlay), each normalised in float32 over the crop; the mask border is
 * calculateBorder(mask) != 0 of the resident mask (0/v masks included), the defect panel shows
 * defect != 0.  The CI panel is drawn only when vh_batch_ci was enqueued after the last change of the
 * resident defect maps (vh_batch_run, vh_batch_set_defect, vh_batch_select_defect), from exactly the
 * float64 values vh_batch_download_ci's ci_array holds; otherwise it is the reference's blank CI
 * panel (N4).  parula float64 [prow][3]; VH_ERR_ARG when prow < 1.  The first call after a run
 * computes the layout if vh_batch_montage_layout has not (it then waits for the stream once).  proton
 * and parula stay valid until the next waiting call on the batch. */
int vh_batch_montage(vh_batch *b, const float *proton, const double *parula, int64_t prow);
/* Waits.  image: offset[nb] bytes, laid out as vh_batch_montage_layout says (the padding between
 * images is not written).  status[i] (nullable): VH_OK, VH_ERR_EMPTY, or VH_ERR_INDEX when a CI colour
 * index int(CI * 64 / 40) of the study's crop reached prow (the IndexError of Vent_Analysis.py:482-484):
 * that study's image bytes are unspecified, the other studies are unaffected. */
int vh_batch_download_montage(vh_batch *b, uint8_t *image, int32_t *status);

/* ---- the ventilation distribution of a device-resident batch -----------------------------------
 * Per study the histogram of the normalised masked signal, and per slice the counts of mask, defect
 * and linear-binning class voxels (slice-wise VDP): one read-only sweep over what the last vh_batch_run
 * left resident; only counts come back, and every count is an exact integer.
 *
 * It reads N4, the volume the run's chain read (HPvent when do_n4 = 0); the resident mask (a voxel
 * counts when mask != 0); the run's LB class volume; and the defect map as it stands (the run's,
 * vh_batch_set_defect's or vh_batch_select_defect's).  The divisor d is the study's mean_anchor
 * (VH_NORM_MEAN) or p99 (VH_NORM_P99) of that run.
 *
 * Histogram: for every voxel with mask != 0, nv = float32(x / d) (IEEE float32 division).  If
 * nv >= 0 && nv < hi the voxel goes to bin min(n_bins - 1, (int)float32(nv * scale)), with
 * scale = (float)n_bins / hi computed once in float32; nv < 0 goes to outside[i][0]; everything else
 * to outside[i][1]: nv >= hi, NaN, and whatever a zero, infinite or NaN d gives under the same
 * pointwise rule.  An empty-mask study gives zeros throughout.  With (VH_NORM_P99, VH_COHORT_BINS,
 * 1.5f) a study's row is the row the cohort histogram (vh_run_opts.do_cohort) sums for it.
 *
 * Slice counts, over all voxels of slice z (mask or not): column 0 counts mask != 0, column 1
 * defect != 0 (not ANDed with the mask: an uploaded map is counted as it is), columns 2..7 the LB
 * classes 1..6 (a class byte outside 1..6 is counted nowhere).
 *
 * vh_batch_distribution enqueues only, and changes nothing the run, vh_batch_ci, the selection calls
 * or the renderings wrote.  It may be called again with other parameters: the download returns the last
 * call's result; a new run discards it.  VH_ERR_ARG, with nothing enqueued: a null batch, no
 * vh_batch_run yet, norm not 0 or 1, n_bins outside 1..1024, hi not finite or <= 0, more than 1900
 * slices.  vh_batch_download_distribution waits; VH_ERR_ARG when vh_batch_distribution has not been
 * enqueued since the last run.  Its kernel-timing class is "dist_b" (vh_batch_kernel_time reads it;
 * vh_batch_kernel_names does not list it).
 *
 * vh_distribution is the host-buffer form for one call, like vh_defect_map: the post-N4 chain (no N4,
 * no SNR) on the scratch batch, then the above with that run's mean-anchored defect map; VH_ERR_EMPTY
 * for an empty-mask study, like vh_vdp. */
#define VH_NORM_MEAN 0   /* nv = float32(N4 / mean_anchor): the domain of calculate_VDP's thresh   */
#define VH_NORM_P99  1   /* nv = float32(N4 / p99): the domain of the LB edges and of the cohort */
#define VH_DIST_COLS 8   /* slice_counts columns: mask, defect, LB class 1..6 */
int vh_batch_distribution(vh_batch *b, int norm, int32_t n_bins, float hi);
int vh_batch_download_distribution(vh_batch *b, uint32_t *hist /* [nb][n_bins] */,
                                   int64_t *outside /* [nb][2] */,
                                   int64_t *slice_counts /* [nb][Z][VH_DIST_COLS] */);   /* all nullable */
int vh_distribution(vh_ctx *ctx, const float *n4, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                    int64_t batch, float thresh, int norm, int32_t n_bins, float hi,
                    uint32_t *hist, int64_t *outside, int64_t *slice_counts);

/* ---- the local ventilation heterogeneity of a device-resident batch ------------------------------
 * The coefficient of variation (CoV) of the signal over the masked pixels of a small in-plane window,
 * as a map, and its summary per study: a histogram, three counts and a fixed-point sum whose mean is
 * the "ventilation heterogeneity index".  Every operation of the map is a correctly-rounded float32
 * add, subtract, multiply, divide or square root in a fixed order (no fused multiply-add), so the map
 * is specified to the last bit (tests/heterogeneity_ref.py is the same arithmetic in numpy); every
 * count of the summary is an exact integer, so it does not depend on the order in which threads add.
 *
 * One study is x (float32 [R][C][Z], the slice axis fastest); every slice is processed on its own, for
 * the reason given for the denoise filter below.  Parameters: radius k (1..5), min_count (2..(2k+1)^2),
 * n_bins (1..1024), hi (finite, 0 < hi <= 16), exclude_defect (0 or 1).
 *
 * The effective mask: M(r, c, z) = (mask != 0), and with exclude_defect also (defect == 0), the
 * resident defect map taken as it stands (the run's, vh_batch_set_defect's or vh_batch_select_defect's).
 *
 * For every voxel with M set, the window offsets (dr, dc) run in raster order, dr outer, each from -k
 * to k.  A neighbour counts when it lies inside the slice and M is set there: there is no clamping and
 * no padding value.
 *   n = the number of counted neighbours (the voxel itself is one)
 *   s = +0; for each counted neighbour in order: s = s + x
 *   m = s / (float)n
 *   q = +0; for each counted neighbour in order: t = x - m;  q = q + t*t   (multiply and add rounded separately)
 * The voxel has a value when n >= min_count and m > 0; then cv = sqrtf(q / (float)(n - 1)) / m.
 *
 * The map, float32 [R][C][Z]: +0 where M is clear, -1 where M is set but there is no value, cv
 * otherwise.  Non-finite input voxels follow the same pointwise rules: nothing special-cases them.
 *
 * The summary, over the voxels with a value: if cv < hi the voxel goes to bin
 * min(n_bins - 1, (int)float32(cv * scale)), with scale = (float)n_bins / hi computed once in float32
 * (the distribution's rule), and adds (int64)float32(cv * 16777216.0f) to a fixed-point sum (the product
 * is exact and below 2^28 because hi <= 16; the conversion truncates); every other valued voxel, NaN
 * included, is counted in n_over.  stats[i] = n_in, n_over, n_none (M set, no value), sum_fx;
 * n_in + n_over + n_none is the number of voxels with M set, and an empty mask gives zeros throughout.
 * The index is sum_fx / 2^24 / n_in, for the caller to compute in double (NaN when n_in == 0).
 *
 * vh_batch_heterogeneity enqueues only.  It reads the volume the last run's chain read (N4, or HPvent
 * when do_n4 = 0), the resident mask and, with exclude_defect, the resident defect map, and changes
 * nothing any other call wrote.  It may be called again with other parameters: the download returns
 * the last call's result; a new run, and whatever forgets the run (vh_batch_denoise, the mask edits,
 * ...), discards it.  VH_ERR_ARG, with nothing enqueued: a null batch, no vh_batch_run yet, any
 * parameter outside the ranges above (and a batch of more than 65535 studies).
 * vh_batch_download_heterogeneity waits; VH_ERR_ARG when vh_batch_heterogeneity has not been enqueued
 * since the last run.  Its kernel-timing class is "het_b" (vh_batch_kernel_time reads it;
 * vh_batch_kernel_names does not list it).
 *
 * vh_heterogeneity is the host-buffer form on the context's scratch batch, for any volume and mask:
 * no run, no N4 and no chain behind it; a caller who wants to exclude defects ANDs them out of the mask. */
int vh_batch_heterogeneity(vh_batch *b, int radius, int32_t min_count, int32_t n_bins, float hi, int exclude_defect);
int vh_batch_download_heterogeneity(vh_batch *b, float *map /* [nb][R][C][Z] */, uint32_t *hist /* [nb][n_bins] */,
                                    int64_t *stats /* [nb][4] */);   /* all nullable */
int vh_heterogeneity(vh_ctx *ctx, const float *x, const uint8_t *mask, int64_t R, int64_t C, int64_t Z, int64_t batch,
                     int radius, int32_t min_count, int32_t n_bins, float hi,
                     float *map, uint32_t *hist, int64_t *stats);

/* ---- the core-rind analysis of a device-resident batch --------------------------------------------
 * Where in the lung the defects lie: at the periphery (the "rind" or "peel") or in the centre (the
 * "core").  Per voxel of the mask the squared in-plane Euclidean distance to the mask's edge, as a
 * map, and per study the mask voxels and the defect voxels of every depth band.  The squared distance
 * is an integer and every summary is an integer count, so the result is exact and does not depend on
 * the order in which threads add (tests/core_rind_ref.py is the same definition in numpy).
 *
 * One study is [R][C][Z], the slice axis fastest; every slice is processed on its own, for the reason
 * given for the denoise filter below.
 *
 * The mask: M(r, c, z) = (mask != 0).  A position outside the slice counts as NOT in M: a lung cut by
 * the field of view has an edge there.  This is deliberately unlike the erosion of vh_batch_edit_mask,
 * which pads with 1; on a mask that stays k + 1 pixels off the slice border the two agree,
 * {D2 > k^2} = erode(mask, k).
 *
 * The distance: for a voxel with M set, D2(r, c, z) = the minimum of (r - r')^2 + (c - c')^2 over the
 * positions (r', c') of slice z with M clear, the one-pixel ring outside the slice included; 0 where
 * M is clear.  So D2 >= 1 on the mask and D2 <= (min(R, C) / 2 + 1)^2.
 *
 * The map, uint16 [R][C][Z]: min(D2, 65535).  The value saturates; only planes of 510 or more on both
 * sides can reach it.
 *
 * The bands: n_thr thresholds (0..31), integers 1 <= thr[0] < thr[1] < ... <= 65535, give n_thr + 1
 * bands; a masked voxel's band is the number of thresholds <= min(D2, 65535).  Band 0 is the outermost
 * rind.  (A depth of at least e pixels, D2 >= e^2, is D2 >= ceil(e^2): the caller rounds up.)
 *
 * The summary per study: counts int64 [n_thr + 1][2], the voxels of M in the band and those of them
 * with defect != 0, the resident defect map taken as it stands at the enqueue (the run's,
 * vh_batch_set_defect's or vh_batch_select_defect's): a later change of the map does not change them.
 * stats int64 [2]: n_mask and the largest D2, unsaturated.  An empty mask gives zeros throughout.  With
 * with_defect = 0 the defect column is 0 and no defect map is needed.
 *
 * vh_batch_core_rind enqueues only (thr is read before it returns).  It reads the resident mask and,
 * with with_defect, the resident defect map, and changes nothing any other call wrote.  It may be
 * called again with other thresholds: the download returns the last call's result; a new run, and
 * whatever forgets the run (vh_batch_denoise, the mask edits, vh_batch_segment, ...), discards it.
 * VH_ERR_ARG, with nothing enqueued: a null batch, n_thr outside 0..31, thresholds that are not
 * strictly increasing or include 0, with_defect outside {0, 1}, with_defect with no defect maps
 * resident (neither a run nor vh_batch_set_defect), a batch of more than 65535 studies.
 * vh_batch_download_core_rind waits; every pointer is nullable; VH_ERR_ARG when vh_batch_core_rind
 * has not been enqueued since the last run or the last call that forgets the run.  Its kernel-timing
 * class is "depth_b" (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * The kernels take every shape a batch accepts.  The search has two forms, chosen by the shape alone:
 * vh_core_rind_form returns 0 when the rows a workgroup searches are staged in LDS (a row of C Z
 * column distances, bytes where R <= 510 and uint16 otherwise, within 60 KiB), 1 when a row is too
 * long for that and the search reads them through the caches (-1 for a dimension below 1).  Both give
 * the same result.
 *
 * vh_core_rind is the host-buffer form on the context's scratch batch, for any mask and (nullable)
 * defect map: no run behind it. */
int vh_batch_core_rind(vh_batch *b, const uint16_t *thr, int32_t n_thr, int with_defect);
int vh_batch_download_core_rind(vh_batch *b, uint16_t *map /* [nb][R][C][Z] */, int64_t *counts /* [nb][n_thr+1][2] */,
                                int64_t *stats /* [nb][2] */);   /* all nullable */
int vh_core_rind(vh_ctx *ctx, const uint8_t *mask, const uint8_t *defect /* nullable */, int64_t R, int64_t C,
                 int64_t Z, int64_t batch, const uint16_t *thr, int32_t n_thr,
                 uint16_t *map, int64_t *counts, int64_t *stats);
int vh_core_rind_form(int64_t R, int64_t C, int64_t Z);

/* ---- the connected components of a device-resident batch ------------------------------------------
 * How many defects there are, how large each one is, and a filter that drops the small ones or keeps
 * the k largest -- of the resident defect map, or of the resident mask (the two lungs after
 * vh_batch_segment).  Every output is an exact integer with one canonical value: no numbering of the
 * labels is left to the implementation, and nothing depends on the order in which threads add
 * (tests/components_ref.py is the same definition in numpy / scipy).
 *
 * One study is [R][C][Z], the slice axis fastest, V = R C Z.  The set: S = (a != 0) of one resident
 * byte volume, source = VH_CC_DEFECT the resident defect map as it stands at the enqueue (the run's,
 * vh_batch_set_defect's or vh_batch_select_defect's), VH_CC_MASK the resident mask.  A position
 * outside the volume is not in S; nothing wraps around.
 *
 * The neighbourhood, conn:   4: |dr| + |dc| = 1, dz = 0          8: max(|dr|, |dc|) = 1, dz = 0
 *                            6: |dr| + |dc| + |dz| = 1          26: max(|dr|, |dc|, |dz|) = 1
 * With 4 and 8 voxels of different slices are never connected: every slice stands on its own, as in
 * the other per-slice analyses.  A component is an equivalence class of S under the transitive closure
 * of the neighbourhood.
 *
 * Per voxel: root int32 [R][C][Z], the smallest linear index (r C + c) Z + z over the voxels of its
 * component, -1 off S: the canonical label.  size uint32 [R][C][Z], the number of voxels of its
 * component, 0 off S.
 *
 * Per study: stats int64 [4] = n_set, n_comp, the size of the largest component (0: none) and that
 * component's root (-1: none); among equal sizes the smaller root wins.  counts int64 [n_edges + 1][2]:
 * edges holds n_edges (0..31) uint32 values 2 <= e[0] < e[1] < ...; a component's class is the number of
 * edges <= its size; counts[k] = {components of class k, voxels in them}.  An empty S gives -1 / 0
 * throughout.
 *
 * The filter: min_size uint32 [nb], each >= 1; keep_largest int32 [nb], 0..8, 0 = no limit (NULL: all
 * 0).  A component's key is (size, -root), ordered lexicographically; its rank is the number of
 * components of the study with a greater key.  A voxel of S is kept when its component has
 * size >= min_size[q] and, where keep_largest[q] = k > 0, rank < k; every other voxel of the source is
 * cleared; a kept voxel keeps its byte value.  kept int64 [nb][2] = {components kept, voxels kept}.
 *
 * vh_batch_components enqueues only (edges is read before it returns).  It reads its source and
 * writes buffers of its own: nothing another call reads changes, so the CI stays fresh.  It may be
 * called again; the download returns the last call's result, a snapshot like the core-rind's defect
 * column: a later change of the source does not change it.  A new run, and whatever forgets the run,
 * discards it.  vh_batch_download_components waits; every pointer is nullable.
 *
 * vh_batch_filter_components labels its source itself -- it does not depend on an earlier
 * vh_batch_components, so it cannot apply stale sizes to a map that has changed since -- in the same
 * device buffers: a download after it is VH_ERR_ARG until the next vh_batch_components.  With
 * VH_CC_MASK it writes the resident mask and forgets the run, exactly as vh_batch_edit_mask does.  With
 * VH_CC_DEFECT it writes the resident defect map, rebuilds the resident border from it (the 2-D
 * calculateBorder of vh_border) and leaves the state vh_batch_set_defect leaves: the CI is no longer
 * fresh, a selection is off, and vh_batch_download_defect's count is NOT updated -- it is the run's,
 * as after vh_batch_set_defect; the filtered count is kept[q][1].  It enqueues only unless kept is
 * given; then it waits.
 *
 * VH_ERR_ARG, with nothing enqueued: a null batch; source or conn out of range; n_edges outside 0..31;
 * edges that are not strictly increasing or are below 2; a null min_size, a min_size of 0, a
 * keep_largest outside 0..8; VH_CC_DEFECT with no defect maps resident (neither a run nor
 * vh_batch_set_defect); a batch of more than 65535 studies; V >= 2^31 (no batch has one); a download
 * without a vh_batch_components since the last run, forget or filter.  The kernel-timing class is
 * "comp_b" (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * The kernels take every shape a batch accepts, in one form: a union-find whose parent array is the
 * root map, tiles of 16 x 16 x min(Z, 24) voxels labelled in LDS and united across their faces; every
 * device loop is bounded because an index strictly decreases along it.
 *
 * vh_components / vh_filter_components are the host-buffer forms on the context's scratch batch, for
 * any byte volume a: no run behind them.  out (nullable) receives the filtered volume. */
#define VH_CC_DEFECT 0
#define VH_CC_MASK 1
int vh_batch_components(vh_batch *b, int source, int conn, const uint32_t *edges, int32_t n_edges);   /* enqueue only */
int vh_batch_download_components(vh_batch *b, int32_t *root /* [nb][R][C][Z] */, uint32_t *size /* [nb][R][C][Z] */,
                                 int64_t *counts /* [nb][n_edges+1][2] */, int64_t *stats /* [nb][4] */);   /* waits; all nullable */
int vh_batch_filter_components(vh_batch *b, int source, int conn, const uint32_t *min_size /* [nb] */,
                               const int32_t *keep_largest /* [nb]; NULL = all 0 */,
                               int64_t *kept /* [nb][2]; nullable; waits when given */);
int vh_components(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch, int conn,
                  const uint32_t *edges, int32_t n_edges, int32_t *root, uint32_t *size, int64_t *counts, int64_t *stats);
int vh_filter_components(vh_ctx *ctx, const uint8_t *a, int64_t R, int64_t C, int64_t Z, int64_t batch, int conn,
                         const uint32_t *min_size, const int32_t *keep_largest, uint8_t *out, int64_t *kept);

/* ---- the defect table of a device-resident batch ----------------------------------------------------
 * Where the big defects are, how large each is, how many slices it spans, how compact and how dark it
 * is: one row per component, largest first, and only the table leaves the device (at most 147 KB per
 * study).  Every entry is an integer combined by integer add / min / max, so nothing depends on the
 * order in which threads add (tests/defect_table_ref.py is the same definition in numpy).
 *
 * The components are those of the last vh_batch_components: its source, its conn, and the resident
 * root and size maps.  A component's key and rank are the filter's: key (size, -root) ordered
 * lexicographically, rank = the number of components of the study with a greater key.
 *
 * A component qualifies when size >= min_size[q] (uint32 [nb], each >= 1).  Row j (0 <= j < max_rows,
 * max_rows 1..VH_DT_MAX_ROWS) holds the component of rank j if it qualifies: the qualifying components
 * are a prefix of the rank order, so n_rows = min(n_qualifying, max_rows).  A row without a component
 * has column 0 = -1 and every other column 0.
 *
 * rows int64 [nb][max_rows][VH_DT_COLS]:
 *    0  root      the component's root            1  size      its voxels
 *    2  sum_r     3  sum_c     4  sum_z           the sums of the voxel indices on each axis
 *    5  min_r     6  max_r     7  min_c     8  max_c     9  min_z    10  max_z    inclusive bounds
 *   11  faces_r  12  faces_c  13  faces_z         the exposed faces normal to each axis
 *   14  n_sig    15  sum_fx   16  min_fx   17  max_fx    the signal columns
 * Faces: for a voxel and each of its two neighbours along an axis, the face is exposed when the
 * neighbour position lies outside the volume or the neighbour's root differs from the voxel's (under
 * conn 4 and 8 slices never join, so faces_z = 2 size: the definition, not a special case).
 * The signal columns, with norm = VH_NORM_MEAN or VH_NORM_P99: x is the N4 volume the last run's chain
 * read, d the run's mean_anchor or p99, nv = float32(x / d).  A voxel counts when 0 <= nv < 64, and then
 * fx = (int64)float32(nv * 16777216.0f), the heterogeneity's fixed point (the bound keeps sum_fx inside
 * int64 at V < 2^31); negative, >= 64, NaN, infinite, or a zero divisor: not counted.  With n_sig = 0,
 * or with norm = VH_DT_NO_SIGNAL, columns 14..17 are 0.
 *
 * stats int64 [nb][4] = n_rows, n_qualifying, the voxels in the rows, the voxels in the qualifying
 * components; the table is truncated where n_rows < n_qualifying.
 *
 * vh_batch_defect_table enqueues only (min_size is read before it returns).  It reads the root and size
 * maps (and x) and writes buffers of its own: nothing another call reads changes, so the CI stays fresh
 * and vh_batch_download_components returns the same bytes before and after.  It may be called again;
 * the download returns the last call's result.  A new vh_batch_components, vh_batch_filter_components,
 * a new run and whatever forgets the run discard it: the events that replace or discard the labelling
 * the rows refer to.  vh_batch_download_defect_table waits; both pointers are nullable.
 *
 * VH_ERR_ARG, with nothing enqueued: a null batch; a null min_size or a min_size of 0; max_rows outside
 * 1..1024; norm not one of the three values; a norm that needs a run when there is none; no
 * vh_batch_components result resident; a download without a vh_batch_defect_table since the last of
 * the discarding events.  The kernel-timing class is "dtab_b" (vh_batch_kernel_time reads it;
 * vh_batch_kernel_names does not list it).
 *
 * The kernels take every shape a batch accepts in one form.  Where a study has more qualifying
 * components than rows, the max_rows-th greatest key is found by a radix select, 11 bits a pass over
 * the 2 ceil(log2(V + 1)) bits of (size, -root); the at most 1024 keys at or above it are sorted in LDS
 * (8 KB); a voxel finds its row by a binary search of its key in that list, and a workgroup combines
 * the voxels of a row in LDS before one global 64-bit atomic per row and column.  Device memory, on
 * first demand, per study: 147 456 B of rows (room for 1024), 8 KB of keys, 8 KB of digit histogram,
 * 64 B of counters and selection state. */
#define VH_DT_COLS 18
#define VH_DT_MAX_ROWS 1024
#define VH_DT_NO_SIGNAL (-1)
int vh_batch_defect_table(vh_batch *b, const uint32_t *min_size /* [nb] */, int32_t max_rows, int norm);  /* enqueue only */
int vh_batch_download_defect_table(vh_batch *b, int64_t *rows /* [nb][max_rows][VH_DT_COLS] */,
                                   int64_t *stats /* [nb][4] */);  /* waits; both nullable */

/* ---- the regional analysis of a device-resident batch ----------------------------------------------
 * Where in the lung the defects lie: the VDP, the class counts and the signal histogram of the left and
 * the right lung, of the upper, middle and lower third, of a grid of parts, or of the zones of a
 * caller's own label volume (lobes from a registered CT).  Every output is an integer, so the result
 * does not depend on the order in which threads add (tests/zones_ref.py is the same definition in
 * numpy; vent_analysis_amd/csrc/zones_host.h is the rule the kernels and the two host functions share).
 *
 * One study is [R][C][Z], the slice axis fastest, V = R C Z.  A voxel is "on" when mask != 0.  Pr[r],
 * Pc[c], Pz[z] are the on voxels of row r, column c and slice z of the study.
 *
 * The bounds of an axis: lo and hi, the first and the last index with P > 0, w = hi - lo + 1.  An empty
 * mask has lo = 0, hi = -1 on every axis and every part index 0.
 *
 * The parts of an axis into p parts (1..32), for every index i of the axis:
 *   by = VH_ZONE_EXTENT  part(i) = clamp(floor((i - lo) p / w), 0, p - 1); indices below lo are in part 0
 *   by = VH_ZONE_COUNT   part(i) = min(p - 1, floor(cum(i) p / total)), cum(i) the sum of P[j] over j < i,
 *                        total the sum of P, in 64-bit integers
 * A part may be empty (p > w, or a plane that holds more than total / p voxels).
 *
 * The lateral split (left and right lung): among the columns lo_c + w_c / 4 .. hi_c - w_c / 4 (integer
 * division: the whole interval where w_c < 4) s is the one with the smallest Pc, the smallest such
 * column on a tie; the side of column c is 0 for c < s and 1 for c >= s.  An empty mask has s = 0.
 *
 * The zone of an on voxel: 1 + (part_r nc + col) pz + part_z with parts = {pr, pc, pz}; with lateral
 * nc = 2, col = the side and pc must be 1; without it nc = pc and col = part_c.  K = pr nc pz <= 32.
 * The zone byte of a voxel off the mask is 0.
 *
 * labels != NULL, the caller's zones: K = n_zones (1..32); labels [nb][V] is copied to the device before
 * the call returns; a byte l in 1..K on an on voxel is zone l, any other byte on an on voxel zone 0,
 * "unassigned"; parts, lateral and by are ignored.  The resident zone map is what was used: the zone
 * byte on on voxels, 0 elsewhere.
 *
 * Per study and zone k = 0..K, over the on voxels of the zone, from the N4 volume the last run's chain
 * read, the resident defect map as it stands at the enqueue, and the run's LB classes:
 *   counts int64 [K + 1][VH_ZONE_COLS]  the voxels, those with defect != 0, those of LB class 1..6
 *   hist uint32 [K + 1][n_bins], stats int64 [K + 1][4] = n_in, n_below, n_over, sum_fx
 * by the distribution's rule: nv = float32(x / d), d the run's mean_anchor (VH_NORM_MEAN) or p99
 * (VH_NORM_P99); for 0 <= nv < hi the bin is min(n_bins - 1, (int)float32(nv * scale)) with
 * scale = (float)n_bins / hi formed once in float32, it counts in n_in, and sum_fx +=
 * (int64)float32(nv * 16777216.0f), the heterogeneity's fixed point: the zone's mean normalised signal
 * is sum_fx / 2^24 / n_in.  nv < 0 counts in n_below; everything else (>= hi, NaN, a zero divisor) in
 * n_over.
 *   geom int32 [8] = lo_r, hi_r, lo_c, hi_c, lo_z, hi_z, s, 0 (s = -1 without lateral and with labels;
 *   with labels the bounds are still the mask's)
 *
 * vh_batch_zones enqueues only, without a host wait (with labels it returns once their copy has left
 * the caller's buffer).  It needs a run, reads what the run and the other calls left and writes buffers
 * of its own: nothing another call reads changes, so the CI stays fresh.  It may be called again: the
 * download returns the last call's result; a new run, and whatever forgets the run, discards it.
 * VH_ERR_ARG, with nothing enqueued: a null batch; no run; norm not VH_NORM_*; n_bins outside 1..256; hi
 * not finite, <= 0 or > 64 (the bound keeps sum_fx inside int64 at V < 2^31); without labels: by not
 * VH_ZONE_*, null parts, a part count below 1, K > 32, lateral outside {0, 1}, lateral with
 * parts[1] != 1; with labels: n_zones outside 1..32; a batch of more than 65535 studies.
 * vh_batch_download_zones waits; every pointer is nullable; VH_ERR_ARG when vh_batch_zones has not been
 * enqueued since the last run or the last call that forgets the run.  The kernel-timing class is
 * "zones_b" (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * The kernels take every shape a batch accepts in one form: the profile, map and count sweeps give a
 * workgroup 256 consecutive (column, slice) pairs and a slab of rows; what does not fit a workgroup's
 * LDS (the slice profile of Z >= 256, the part tables' profiles of R + C + Z > 12288) goes through
 * global integer atomics or global reads.
 *
 * vh_zone_parts / vh_zone_split are the rule on the host, no device needed: the parts of one axis from
 * its profile (n entries, each >= 0) with bounds = {lo, hi}, and the split column of a column profile.
 * VH_ERR_ARG for a null pointer, n < 1, p outside 1..32, by not VH_ZONE_*, a negative entry or a total
 * above 2^57.
 *
 * vh_zones is the host-buffer form on the context's scratch batch: the post-N4 chain of vh_vdp on n4
 * and mask with thresh, then defect (nullable: the chain's map stays) as the resident defect map, then
 * the analysis.  VH_ERR_EMPTY for an empty-mask study, after the outputs are written. */
#define VH_ZONE_EXTENT 0
#define VH_ZONE_COUNT 1
#define VH_ZONE_COLS 8     /* mask, defect (on the mask), LB class 1..6 */
int vh_zone_parts(const int64_t *profile, int64_t n, int32_t p, int by, uint8_t *part /* [n] */, int32_t bounds[2]);
int vh_zone_split(const int64_t *profile, int64_t n, int32_t *s);
int vh_batch_zones(vh_batch *b, const uint8_t *labels /* [nb][V], nullable */, int32_t n_zones,
                   const int32_t parts[3], int lateral, int by, int norm, int32_t n_bins, float hi);   /* enqueue only */
int vh_batch_download_zones(vh_batch *b, uint8_t *map /* [nb][V] */, int64_t *counts /* [nb][K+1][8] */,
                            uint32_t *hist /* [nb][K+1][n_bins] */, int64_t *stats /* [nb][K+1][4] */,
                            int32_t *geom /* [nb][8] */);   /* waits; all nullable */
int vh_zones(vh_ctx *ctx, const float *n4, const uint8_t *mask, const uint8_t *defect /* nullable */, int64_t R,
             int64_t C, int64_t Z, int64_t batch, float thresh, const uint8_t *labels /* nullable */, int32_t n_zones,
             const int32_t parts[3], int lateral, int by, int norm, int32_t n_bins, float hi, uint8_t *map,
             int64_t *counts, uint32_t *hist, int64_t *stats, int32_t *geom);

/* ---- the denoise option of a device-resident batch ("Denoise Option", Vent_Analysis.py:1025) -------
 * An in-plane non-local-means filter of the resident HPvent with a Tukey bisquare weight.  Every
 * operation is a correctly-rounded float32 add, subtract, multiply, divide or square root in a fixed
 * order (no fused multiply-add), so the result is specified to the last bit (tests/denoise_ref.py is
 * the same arithmetic in numpy).
 *
 * The filter, for one study x (float32 [R][C][Z], the slice axis fastest), every slice on its own
 * (slices are 10 mm thick against 1.5 mm pixels: a 3-D patch would mix unrelated anatomy).
 * Parameters: search radius S = search_r (1..5), patch radius P = patch_r (0..2), strength k (a
 * float32), the study's noise sigma (float32, finite, > 0), rician (0: off, else on).  Once per study,
 * in double and then rounded to float32: n = (2P+1)^2, inv_h2 = float32(1 / (2 n (k sigma)^2)),
 * bias = float32(2 sigma^2).  Indices outside the slice are clamped: X(r, c) stands for
 * x[clamp(r, 0, R-1)][clamp(c, 0, C-1)][z], which is np.pad(x, mode='edge') by S + P.
 * For every voxel (r, c, z) the search offsets (dr, dc) run in raster order, dr outer, each from -S
 * to S, with num = den = +0 at the start.  For each offset:
 *   d2 = +0; for the patch offsets (ur, uc) in raster order, ur outer, each from -P to P:
 *       t = X(r+ur, c+uc) - X(r+dr+ur, c+dc+uc);  d2 = d2 + t*t   (multiply and add rounded separately)
 *   u = d2 * inv_h2
 *   w = (u < 1) ? (1-u)*(1-u) : 0      the bisquare weight: compact support, so a dissimilar patch
 *                                      weighs exactly 0, and no exp whose rounding a library decides
 *   num = num + w * Y(r+dr, c+dc);  den = den + w      Y = X, or Y = X*X with rician
 * out = num / den (IEEE float32 division; the centre offset has w = 1, so den >= 1 for finite input);
 * with rician v = out - bias, then out = v > 0 ? sqrtf(v) : 0.  Non-finite input voxels follow the
 * same pointwise rules: nothing special-cases them.
 *
 * The noise estimate: sigma = float32(sqrt(S2 / (2 N))), S2 and N the sum of squares (double) and the
 * count over exactly the voxels calculate_SNR counts as noise (the noise box of Vent_Analysis.py:340-351
 * with its quirks, as vh_snr has it): the Rayleigh maximum-likelihood estimate of a magnitude image's
 * background.  The device sums the doubles in its own fixed order, so against another order the
 * float32 may differ by one ulp.  NaN for a study whose SNR is undefined (no masked column > 0, or
 * no noise voxel).
 *
 * vh_batch_noise_sigma, after vh_batch_upload: the mask statistics and the SNR sweep on the resident
 * HPvent, then waits.  vh_batch_denoise enqueues only: it replaces the resident HPvent with its
 * denoised volume, so the next vh_batch_run (N4, SNR, the VDP chain, the montage's HPvent panel) sees
 * it.  VH_ERR_ARG, with nothing enqueued: a null batch or sigma, search_r outside 1..5, patch_r
 * outside 0..2, a strength that is not finite or <= 0, any sigma that is not finite or <= 0 (and a
 * batch of more than 65535 studies).  Called after a run, either of the two puts the batch back where
 * vh_batch_upload left it (the first rewrites the mask statistics, the second the volume the results
 * came from): the calls that need a run return VH_ERR_ARG until the next one.  vh_batch_download_hp
 * waits and returns the resident HPvent as it stands.  The filter's kernel-timing class is "denoise_b"
 * (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * vh_noise_sigma and vh_denoise are the host-buffer forms on the context's scratch batch. */
int vh_batch_noise_sigma(vh_batch *b, float *sigma /* [nb] */);
int vh_batch_denoise(vh_batch *b, const float *sigma /* [nb] */, float strength, int search_r, int patch_r,
                     int rician);
int vh_batch_download_hp(vh_batch *b, float *hp /* [nb][R][C][Z] */);
int vh_noise_sigma(vh_ctx *ctx, const float *hp, const uint8_t *mask, int64_t R, int64_t C, int64_t Z,
                   int64_t batch, float *sigma);
int vh_denoise(vh_ctx *ctx, const float *hp, int64_t R, int64_t C, int64_t Z, int64_t batch,
               const float *sigma, float strength, int search_r, int patch_r, int rician, float *out);

/* ---- editing the masks of a device-resident batch ("edit mask", Vent_Analysis.py:1023) -------------
 * Disc morphology and paint strokes on the resident mask, in place.  All arithmetic is on bits, so
 * the result is specified exactly (tests/mask_edit_ref.py is the same in numpy).
 *
 * For one study, s(r, c, z) = (mask[r][c][z] != 0).  Every slice is processed on its own (slices are
 * 10 mm thick against 1.5 mm pixels, as for the denoise filter).  The structuring element of radius k
 * (1..5) is the disc D_k = {(dr, dc) : dr^2 + dc^2 <= k^2}, of 5, 13, 29, 49, 81 offsets.
 *   dilate_k:  out(r, c, z) = OR over D_k of s(r + dr, c + dc, z), a position outside the slice
 *              counting as 0
 *   erode_k:   out = AND over D_k of s(r + dr, c + dc, z), a position outside the slice counting as 1,
 *              so the image edge never erodes a mask
 *   open_k  = dilate_k(erode_k(s))          close_k = erode_k(dilate_k(s))
 * With these pads open_k(s) is inside s, s inside close_k(s), and both are idempotent.  The
 * intermediate of open and close is defined on the slice only, and the second step pads it with its
 * own pad value: it is not computed from a padded input.  These are
 * scipy.ndimage.binary_dilation(s, structure=disc[:, :, None]) and binary_erosion(..., border_value=1).
 * Output bytes are 0 / 1.  radius is per study, each 0..5: a study of radius 0 keeps its mask byte for
 * byte (a 0/255 mask stays 0/255), which is how one study of a batch is edited alone.
 *
 * Paint: with p = (strokes != 0) the mask becomes s | p (VH_PAINT_OR), s & ~p (VH_PAINT_ANDNOT), s & p
 * (VH_PAINT_AND) or s ^ p (VH_PAINT_XOR), written as 0 / 1 bytes for every study.
 *
 * vh_batch_edit_mask enqueues only; vh_batch_paint_mask returns once the strokes have left the
 * caller's buffer (it waits for the work enqueued before it, not for its own kernel).  Both replace the
 * resident mask, so the next vh_batch_run (the mask statistics, N4, the VDP chain, the SNR noise box,
 * the montage's crop and mask border) sees the edited one, and both put the batch back where
 * vh_batch_upload left it, exactly as vh_batch_denoise does: the calls that need a run return
 * VH_ERR_ARG until the next one.  radius and strokes may be reused as soon as the call returns.  The
 * resident HPvent, N4 and defect maps are not touched: a map given by vh_batch_set_defect survives.
 * VH_ERR_ARG, with nothing enqueued: a null batch, radius or strokes, op or how out of range, any
 * radius outside 0..5 (and a batch of more than 65535 studies).  The kernel-timing class is
 * "mask_edit_b" (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * vh_batch_download_mask waits and returns the resident mask as it stands -- after an upload, an edit
 * or a run -- and count[i], the voxels != 0 of study i, counted on the device when asked for (an exact
 * integer).  vh_edit_mask is the host-buffer form of vh_batch_edit_mask on the context's scratch
 * batch; out and count are nullable. */
#define VH_MASK_ERODE 0
#define VH_MASK_DILATE 1
#define VH_MASK_OPEN 2
#define VH_MASK_CLOSE 3
#define VH_PAINT_OR 0
#define VH_PAINT_ANDNOT 1
#define VH_PAINT_AND 2
#define VH_PAINT_XOR 3
int vh_batch_edit_mask(vh_batch *b, int op, const int32_t *radius /* [nb] */);
int vh_batch_paint_mask(vh_batch *b, const uint8_t *strokes /* [nb][V] */, int how);
int vh_batch_download_mask(vh_batch *b, uint8_t *mask /* [nb][V] */, int64_t *count /* [nb] */);  /* both nullable */
int vh_edit_mask(vh_ctx *ctx, const uint8_t *mask, int64_t R, int64_t C, int64_t Z, int64_t batch,
                 int op, const int32_t *radius, uint8_t *out, int64_t *count);

/* ---- the lungs from the proton image ("automatic segmentation using proton", Vent_Analysis.py:1024) --
 * In a proton image the lungs are the dark regions that the bright body encloses.  The mask is made in
 * four steps -- a threshold, a flood of the dark pixels from the slice border, the dark pixels the
 * flood did not reach, an opening -- and every step is a max, an integer count or bit logic, so the
 * result is specified exactly (tests/segment_ref.py is the same in numpy).
 *
 * The proton x is float32 [nb][R][C][Z], the slice axis fastest, like HPvent.  It is resident in a
 * buffer of its own, allocated on the first upload: nb * V * 4 bytes, as much again as the HPvent.
 * (The montage, when it is given a proton, stores it in that same buffer and so replaces it.)  Every
 * slice is processed on its own, for the reason given for the denoise filter.
 *
 * Statistics, per study.  F is the set of voxels that are finite and >= 0 (-0.0 counts as +0.0).
 *   pmax   the maximum over F (order-free, hence exact); +0.0 when F is empty
 *   If pmax is not > 0 the study's threshold is NaN and its histogram is all zeros.  Otherwise
 *   scale = 256.0f / pmax (one float32 division), and every voxel of F is counted in bin
 *   min(255, (int)(x * scale)), the product rounded to float32, of a 256-bin uint32 histogram (a product
 *   that is not below 255 -- an infinite scale times zero included -- counts in bin 255).
 *
 * Otsu cut of a histogram h of n_bins >= 2 bins (a host function: no context, no device).  With
 * N = sum h[i], S = sum i h[i] and, for k = 0 .. n_bins - 2, n0(k) = sum over i <= k of h[i] and
 * s0(k) = sum over i <= k of i h[i] (all four exact integers, then converted to double): cuts with
 * n0 == 0 or n0 == N are skipped, and the cut is the lowest k that maximises
 *   d * d / (n0 * (N - n0)),  d = S * n0 - N * s0,
 * evaluated in double in exactly this operation order, no operation contracted.  (This is the
 * between-class variance up to the factor 1 / N^2.)  A histogram with fewer than two occupied bins has
 * no cut: VH_ERR_EMPTY, and the study's threshold is NaN.
 *
 * Threshold.  t = (float)(k + 1) * (pmax / 256.0f): two float32 operations.
 *
 * Segmentation of one slice with threshold t.
 *   dark(r, c) = x < t         (NaN is not dark, -inf is, +inf is not)
 *   reach      = the dark pixels joined to a dark pixel of the slice's border -- row 0, row R - 1,
 *                column 0, column C - 1 -- through dark pixels under 4-connectivity
 *   seg        = dark & ~reach
 * This is scipy.ndimage.binary_fill_holes(~dark) & dark with scipy's default (cross) structure.  The
 * fixed point does not depend on the order in which pixels are visited.
 *
 * Opening.  Where the study's open_radius k is 1..5, seg becomes open_k(seg) exactly as
 * vh_batch_edit_mask defines it above: the same discs and the same pads.  Output bytes are 0 / 1.
 *
 * vh_batch_upload_proton returns once the proton has left the caller's buffer, as vh_batch_upload does,
 * and invalidates nothing.  vh_batch_proton_threshold runs the statistics sweep, waits, and returns the
 * threshold of every study (and pmax and the histograms when asked for); it changes nothing another
 * call reads.  vh_batch_segment enqueues only: it replaces the resident mask, so the next
 * vh_batch_run sees the segmentation, and puts the batch back where vh_batch_upload left it, exactly
 * as vh_batch_edit_mask does; the resident HPvent, N4 and defect maps are not touched.  thresh and
 * open_radius (NULL: every radius 0) may be reused as soon as the call returns.  VH_ERR_ARG, with
 * nothing enqueued: a null batch or thresh, no proton resident, any thresh that is not finite or is
 * <= 0, any radius outside 0..5, a plane of more than 512 rows or 512 columns (and a batch of more than
 * 65535 studies).  The kernel-timing classes are "segment_b" for the fill and "segment_max_b" and "segment_hist_b"
 * for the two passes of the sweep (vh_batch_kernel_time reads them; vh_batch_kernel_names does not list them).  The environment
 * variable VH_SEG_ZC, read at call time, sets how many slices a workgroup of the fill packs into one
 * bit field (1, 2, 4, 8, 16 or 32, where the plane then fits); the result does not depend on it.
 *
 * vh_batch_mask_overlap waits and returns counts[i] = { |resident != 0|, |other != 0|, |both| } of study
 * i, exact integers counted on the device, from which the Dice and Jaccard indices against a manual
 * mask are one line.  It stages other in the buffer the paint strokes use, so like a paint it puts the
 * batch back where vh_batch_upload left it.
 *
 * vh_segment is the host-buffer form on the context's scratch batch: thresh NULL takes the Otsu
 * threshold of every study, and VH_ERR_EMPTY is returned (with thresh_out written, nothing else) when
 * that is NaN for one of them; mask_out, thresh_out and count are nullable.
 *
 * Connectivity across slices and component size filters are vh_batch_components /
 * vh_batch_filter_components (VH_CC_MASK, keep_largest = 2 keeps the two lungs and drops the specks and
 * a trachea that does not touch them).  Not done here: the removal of a trachea that joins a lung,
 * learned segmentation. */
int vh_batch_upload_proton(vh_batch *b, const float *proton /* [nb][V] */);
int vh_batch_proton_threshold(vh_batch *b, float *thresh /* [nb] */, float *pmax /* [nb], nullable */,
                              uint32_t *hist /* [nb][256], nullable */);
int vh_otsu(const uint32_t *hist, int32_t n_bins, int32_t *cut);
int vh_batch_segment(vh_batch *b, const float *thresh /* [nb] */, const int32_t *open_radius /* [nb], NULL = all 0 */);
int vh_batch_mask_overlap(vh_batch *b, const uint8_t *other /* [nb][V] */, int64_t *counts /* [nb][3] */);
int vh_segment(vh_ctx *ctx, const float *proton, int64_t R, int64_t C, int64_t Z, int64_t batch,
               const float *thresh, const int32_t *open_radius, uint8_t *mask_out, float *thresh_out,
               int64_t *count);

/* ---- the proton registered to the xenon image: a rigid integer-voxel shift by mutual information ----
 * The proton and the xenon volume are acquired in separate breath-holds, so the proton is displaced by
 * a few voxels in plane and by up to a slice or two through plane; a mask segmented from it inherits the
 * displacement.  vh_batch_register scores every shift of a small search window by the mutual information
 * of the two images' joint histogram and picks the best; vh_batch_shift applies a shift to the resident
 * proton or mask.  The expensive part is one joint histogram per candidate shift -- integer counts, so
 * it is specified exactly (tests/register_ref.py is the same in numpy); only the score is floating point.
 *
 * All volumes are [nb][R][C][Z], the slice axis fastest.  P is the resident proton, X the resident HPvent
 * as it stands (after a denoise, if one ran).
 *
 * Codes.  Per study and per image, F is the set of voxels that are finite and >= 0 (-0.0 counts as +0.0).
 *   max    the maximum over F; scale = 256.0f / max is one float32 division
 *   The code of a voxel of F is min(255, (int)(x * scale)) >> 3, the product rounded to float32 (a
 *   product that is not below 255 -- an infinite scale times zero included -- gives 255 >> 3): 32
 *   levels.  A voxel outside F is invalid.  For the proton this is the bin of the segment statistics
 *   above, folded by 8.  A study whose proton max or xenon max is not > 0 is unregistrable: status 1,
 *   every score NaN, best shift (0, 0, 0), and its histograms are all zeros.
 *
 * Joint histogram of a shift s = (dr, dc, dz): J_s[a][b], uint32 [32][32], counts the voxels v for which
 * v and v + s are both inside the volume, P(v + s) and X(v) are both valid, a is the code of P(v + s)
 * and b is the code of X(v).  Slices are not processed on their own here: dz couples them.  The counts
 * do not depend on any order and are exact.
 *
 * Search window.  search = (Sr, Sc, Sz) with 0 <= Sr, Sc <= 8, 0 <= Sz <= 2, Sr < R, Sc < C, Sz < Z.  The
 * shifts are all (dr, dc, dz) with |dr| <= Sr, |dc| <= Sc, |dz| <= Sz, indexed
 *   i = ((dz + Sz) (2 Sr + 1) + (dr + Sr)) (2 Sc + 1) + (dc + Sc),   ns = (2 Sr + 1)(2 Sc + 1)(2 Sz + 1) <= 1445.
 *
 * Score.  With n = sum J, Ja the row sums and Jb the column sums, all exact integers,
 *   mi = (1 / n) sum over J > 0 of (double)J * log(((double)J * (double)n) / ((double)Ja * (double)Jb))
 * in double, and mi = 0.0 when n = 0.  Both products are exact in double (they stay below 2^53); where
 * they are equal the quotient is exactly 1.0 and the term exactly 0.0, so a constant image scores
 * exactly 0.0 at every shift.  The summation order is free.  vh_mi is this for a [levels][levels]
 * histogram, 1 <= levels <= 256, on the host (no context, no device).
 *
 * Pick.  The best shift has the largest score; among equal scores the smallest |dr| + |dc| + |dz| wins,
 * then the lowest index i.  A NaN never wins; with nothing but NaN the shift is (0, 0, 0).
 * vh_register_pick is this for one study's scores [ns], on the host; vh_batch_register picks with it.
 *
 * Apply.  Shifting an image A by s gives A'(v) = A(v + s) where v + s is inside the volume and 0
 * elsewhere.  Shifting the proton by its best shift puts it on the xenon's voxels; the same shift moves a
 * mask drawn on the proton.
 *
 * vh_batch_register needs a resident proton, waits, and returns score [nb][ns], best [nb][3] and, when
 * asked for, best_score [nb] (the score at best) and status [nb] (0, or 1: unregistrable).  It changes
 * nothing another call reads: the resident proton, HPvent, mask and a run's results stay as they are.
 * Its device buffers are allocated on the first call and grow with the window: nb * ns * 4 KiB of
 * histograms (1.5 GB for 256 studies at the largest window) and two byte volumes of codes.
 * vh_batch_download_register_hist waits and returns the last call's joint histograms [nb][ns][32][32];
 * VH_ERR_ARG before any register call.
 *
 * vh_batch_shift enqueues only; shift [nb][3] may be reused as soon as the call returns, and every
 * |component| is at most its dimension (a shift by a whole dimension leaves zeros).  VH_SHIFT_PROTON
 * replaces the resident proton and invalidates nothing, as vh_batch_upload_proton does.  VH_SHIFT_MASK
 * replaces the resident mask (bytes are moved as they are), so the next vh_batch_run sees the shifted one,
 * and puts the batch back where vh_batch_upload left it, exactly as vh_batch_edit_mask does; the resident
 * HPvent, N4 and defect maps are not touched.  vh_batch_download_proton waits and returns the resident
 * proton as it stands.
 *
 * vh_register is the host-buffer form on the context's scratch batch; status and shifted_out (the
 * proton shifted by best) are nullable.
 *
 * VH_ERR_ARG, with nothing enqueued or changed: a null batch or a null required pointer, no proton
 * resident (register, VH_SHIFT_PROTON, download_proton), a search outside the limits above, what out of
 * range, a shift beyond its dimension (and a batch of more than 65535 studies).  The kernel-timing
 * classes are "register_b" for the joint histograms, "register_score_b" for the scores, "register_codes_b"
 * for the code pass, "segment_max_b" for the two maximum sweeps and "shift_b" (vh_batch_kernel_time reads
 * them; vh_batch_kernel_names does not list them).
 *
 * Not done here: rotation, deformable registration.  (A proton on another grid than the xenon's comes in
 * through the resampling section below, which also applies a sub-voxel offset; the search over scale and
 * sub-voxel offsets is the fine-registration section after it.) */
#define VH_SHIFT_PROTON 0
#define VH_SHIFT_MASK 1
int vh_batch_register(vh_batch *b, const int32_t search[3], double *score /* [nb][ns] */, int32_t *best /* [nb][3] */,
                      double *best_score /* [nb], nullable */, int32_t *status /* [nb], nullable */);
int vh_batch_download_register_hist(vh_batch *b, uint32_t *hist /* [nb][ns][32][32] */);
int vh_mi(const uint32_t *joint, int32_t levels, double *mi);
int vh_register_pick(const double *score, const int32_t search[3], int32_t best[3]);
int vh_batch_shift(vh_batch *b, int what, const int32_t *shift /* [nb][3] */);
int vh_batch_download_proton(vh_batch *b, float *proton /* [nb][V] */);
int vh_register(vh_ctx *ctx, const float *proton, const float *hp, int64_t R, int64_t C, int64_t Z, int64_t batch,
                const int32_t search[3], double *score, int32_t *best, int32_t *status, float *shifted_out);

/* ---- the proton resampled from its own grid onto the xenon grid of a batch ---------------------------
 * A proton series is rarely on the xenon's grid: a 256 x 256 matrix at half the pixel size, or another
 * slice spacing, is ordinary.  The source proton is staged on the device on its own grid and resampled
 * into the batch's proton buffer by a separable, anti-aliased linear filter whose tap tables are made on
 * the host in double; every device operation is a separately rounded float32 multiply or add in a fixed
 * order (no fused multiply-add), so the result is specified to the last bit (tests/resample_ref.py is the
 * same arithmetic in numpy).  The source stays resident, so it can be resampled again with a refined map
 * (a registration's best shift folded into the offsets) instead of being shifted with zeros pulled in.
 *
 * Volumes.  The source S is float32 [nb][Rs][Cs][Zs], the slice axis fastest; one source shape holds for
 * the whole batch, 1 <= Rs, Cs, Zs <= 1024.  The destination is the batch's [nb][R][C][Z] and lands in the
 * resident proton.
 *
 * Map.  Per study and per axis a (r, c, z) two doubles (scale_a, offset_a): map is double [nb][3][2].
 * Destination index i looks at source coordinate u = scale * (double)i + offset: one multiply and one
 * add in double, not contracted.  Coordinates are in source voxel-index units, voxel centres at the
 * integers.  Limits: scale finite in [0.25, 4], offset finite with |offset| <= 2^20.
 *
 * Taps of one axis (vh_resample_taps, a host function: no context, no device), n_src 1..1024, n_dst
 * 1..2^20.  With w = max(1.0, scale): for integer j, t_j = 1.0 - fabs((double)j - u) / w, in that
 * operation order in double.  The taps are every j with t_j > 0: at most VH_RESAMPLE_TAPS = 8, since they
 * lie in an open interval of length 2 w <= 8.  W is the sum of the t_j in ascending j, starting from 0.0;
 * weight_j = (float)(t_j / W).  Taps with j outside [0, n_src) are dropped after the normalisation, so
 * outside the source counts as zeros, like vh_batch_shift.  The result per destination index is first
 * (the lowest in-range j; 0 when there is none), count (0..8; the in-range taps are contiguous) and
 * weight[8] (the in-range weights from slot 0, the rest 0.0f).
 *
 * Value of destination voxel (r, c, z), with the three tables of its study:
 *   ar = +0.0f
 *   for the r taps, ascending:
 *       ac = +0.0f
 *       for the c taps, ascending:
 *           az = +0.0f
 *           for the z taps, ascending:   az = az + wz * S[jr][jc][jz]
 *           ac = ac + wc * az
 *       ar = ar + wr * ac
 *   out = ar
 * Every multiply and every add is rounded to float32 on its own.  An axis with count 0 gives +0.0f.
 * Non-finite voxels follow the same pointwise rules.  The nested form is exactly separable -- the z-sum
 * depends on (jr, jc, z) only and the c-sum on (jr, c, z) only -- so staging the passes changes no bit.
 * Under the identity map (1, 0) every axis has one tap of weight 1.0f and out = +0.0f + 1.0f * S: the
 * source, with -0.0 become +0.0.
 *
 * vh_batch_upload_proton_src stages the source in a device buffer of its own (allocated or grown on
 * first use: nb * Rs * Cs * Zs * 4 bytes), returns once the caller's buffer is free, and invalidates
 * nothing.  vh_batch_resample_proton builds the nb x 3 tables on the host, uploads them and enqueues the
 * resampling of the resident source into the resident proton; it marks the proton resident exactly as
 * vh_batch_upload_proton does and invalidates nothing else; map may be reused on return.
 * vh_batch_download_proton_src waits and returns the resident source.  vh_resample is the host-buffer
 * form on the context's scratch batch.
 *
 * VH_ERR_ARG, with nothing enqueued or changed: a null batch or a null required pointer, a source shape
 * outside the limits, a map outside the limits or not finite, vh_batch_resample_proton or
 * vh_batch_download_proton_src without a resident source (and a batch of more than 65535 studies, or
 * with a dimension above 2^20, the largest n_dst a tap table is made for).  Every other batch shape is
 * taken.  An upload that fails leaves no source resident.  The kernel-timing class is "resample_b"
 * (vh_batch_kernel_time reads it; vh_batch_kernel_names does not list it).
 *
 * Not done here: rotation, non-diagonal maps (shear, axis exchange), masks resampled from another grid. */
#define VH_RESAMPLE_TAPS 8
int vh_resample_taps(int64_t n_src, int64_t n_dst, double scale, double offset, int32_t *first /* [n_dst] */,
                     int32_t *count /* [n_dst] */, float *weight /* [n_dst][8] */);
int vh_batch_upload_proton_src(vh_batch *b, const float *src /* [nb][Rs][Cs][Zs] */, const int64_t shape[3]);
int vh_batch_resample_proton(vh_batch *b, const double *map /* [nb][3][2] */);
int vh_batch_download_proton_src(vh_batch *b, float *src);
int vh_resample(vh_ctx *ctx, const float *src, const int64_t src_shape[3], int64_t R, int64_t C, int64_t Z,
                int64_t batch, const double *map, float *out /* [batch][R][C][Z] */);

/* ---- fine registration: a search over scale and sub-voxel offset of the resident source --------------
 * The proton and the xenon are two breath-holds at two lung volumes: the lungs differ by a few per cent
 * in size and by a fraction of a voxel in position, and on a 128-voxel axis 3 % of scale moves the lung
 * edge by a voxel.  vh_batch_register_maps scores a grid of candidate resampling maps of the resident
 * SOURCE proton (the resampling section above) against the resident HPvent by the mutual information of
 * the register section, and returns the best map; vh_batch_resample_proton then applies it.  No resampled
 * volume is written: the kernel resamples, codes and counts in one pass.  Every value is the resampler's
 * to the last bit and every count an exact integer (tests/register_maps_ref.py is the same in numpy);
 * only the score is floating point.
 *
 * Candidates.  count = (Kr, Kc, Kz) with 1 <= Kr, Kc <= 17 and 1 <= Kz <= 5, so nc = Kr Kc Kz <= 1445, the
 * ceiling of the integer window.  axis_maps is double [nb][Kr + Kc + Kz][2]: per study the r list, then
 * the c list, then the z list of (scale, offset), every entry within the resampler's limits (scale finite
 * in [0.25, 4], offset finite with |offset| <= 2^20).  Candidate (kr, kc, kz) is the map
 * (r[kr], c[kc], z[kz]) and has index
 *   i = (kz Kr + kr) Kc + kc,
 * the order of the shift index: z slowest, then r, then c.
 *
 * Value.  Q_i(v) is the destination value of the resampling section at voxel v under candidate i's map:
 * the same tap tables (vh_resample_taps), the same nested float32 multiply-then-add order, no
 * contraction -- bit for bit what vh_batch_resample_proton would write with that map.
 *
 * Counted voxels.  A destination voxel is skipped for candidate i when any of its three axes has tap count
 * 0 there, i.e. it looks entirely outside the source.  This is the integer search's "both inside the
 * volume": with a source of the batch's shape, scale 1 and integer offsets -S .. S the histograms are
 * those of vh_batch_register's window (Sr, Sc, Sz) exactly, candidate (kr, kc, kz) being the shift
 * (kr - Sr, kc - Sc, kz - Sz).
 *
 * Codes.  The xenon is coded as in the register section.  For the proton, smax is the maximum over F
 * (finite and >= 0) of the study's whole resident source, scale = 256.0f / smax one float32 division, and
 * code(Q) = min(255, (int)(Q * scale)) >> 3 with the product rounded to float32 (a product that is not
 * below 255 gives 255 >> 3); Q is invalid when it is not finite or is < 0.  One scale per study keeps the
 * codes independent of the candidate.  A study whose smax or xenon maximum is not > 0 is unregistrable:
 * status 1, every score NaN, best = home, and its histograms are all zeros.
 *
 * Histogram and score.  J_i[a][b], uint32 [32][32], counts the counted voxels v with Q_i(v) and X(v) both
 * valid, a the code of Q_i(v) and b the code of X(v); the counts are exact.  The score is the register
 * section's mi of J_i, to its formula (vh_mi is the same on the host).
 *
 * Pick.  home = (hr, hc, hz) defaults to the middle entry (K - 1) / 2 of each list.  The largest score
 * wins; among equal scores the smallest |kr - hr| + |kc - hc| + |kz - hz|, then the lowest index.  A NaN
 * never wins; with nothing but NaN the pick is home.  vh_register_maps_pick is this for one study's
 * scores [nc], on the host (home nullable); vh_batch_register_maps picks with it.
 *
 * Candidate lists.  vh_axis_candidates is a host function (no context, no device) that makes one axis's
 * list around a base (scale0, offset0): factor f scales about the destination centre, then shift d, in
 * destination voxels, moves.  With c = ((double)n_dst - 1.0) / 2.0, entry fi * ns + si of out [nf * ns][2]
 * is
 *   scale = scale0 * f,   offset = offset0 + scale0 * (c * (1.0 - f) + d),
 * every operation a separately rounded double in that order.  VH_ERR_ARG, with nothing written, for a
 * null pointer, nf or ns < 1, n_dst outside 1..2^20 or a result outside the resampler's limits.
 *
 * vh_batch_register_maps needs a resident source, waits, and returns score [nb][nc], best [nb][3] (the
 * picked kr, kc, kz) and, when asked for, best_map [nb][3][2] (the picked list entries as they were
 * given, ready for vh_batch_resample_proton), best_score [nb] and status [nb] (0, or 1: unregistrable).
 * It changes nothing another call reads: the resident source, proton, HPvent, mask and a run's results
 * stay as they are.  Its device buffers are allocated on the first call and grow: nb * nc * 4 KiB of
 * histograms, a byte volume of xenon codes and the nb * (Kr + Kc + Kz) tap tables.
 * vh_batch_download_register_maps_hist waits and returns the last call's histograms [nb][nc][32][32].
 * vh_register_maps is the host-buffer form on the context's scratch batch; best_map and status are
 * nullable.
 *
 * VH_ERR_ARG, with nothing enqueued or changed: a null batch or a null required pointer, no resident
 * source, a count outside its limits, a list entry outside its limits or not finite, home outside its
 * list, vh_batch_download_register_maps_hist before any vh_batch_register_maps call (and a batch of more
 * than 65535 studies or with a dimension above 2^20).  Every other batch and source shape the resampler
 * takes is taken, by the one fused kernel.  The kernel-timing classes are "register_maps_b" for the fused
 * kernel, "register_maps_codes_b" for the xenon codes, "segment_max_b" for the two maximum sweeps and
 * "register_score_b" for the scores (vh_batch_kernel_time reads them; vh_batch_kernel_names does not list
 * them).
 *
 * Not done here: rotation, shear, deformable registration; an optimiser (the caller repeats the search on
 * a finer list around best_map); masks resampled from another grid. */
int vh_batch_register_maps(vh_batch *b, const int32_t count[3], const double *axis_maps /* [nb][Kr+Kc+Kz][2] */,
                           const int32_t *home /* [3], nullable */, double *score /* [nb][nc] */,
                           int32_t *best /* [nb][3] */, double *best_map /* [nb][3][2], nullable */,
                           double *best_score /* [nb], nullable */, int32_t *status /* [nb], nullable */);
int vh_batch_download_register_maps_hist(vh_batch *b, uint32_t *hist /* [nb][nc][32][32] */);
int vh_register_maps_pick(const double *score, const int32_t count[3], const int32_t home[3], int32_t best[3]);
int vh_axis_candidates(double scale0, double offset0, int64_t n_dst, const double *factors, int32_t nf,
                       const double *shifts, int32_t ns, double *out /* [nf * ns][2] */);
int vh_register_maps(vh_ctx *ctx, const float *src, const int64_t src_shape[3], const float *hp, int64_t R, int64_t C,
                     int64_t Z, int64_t batch, const int32_t count[3], const double *axis_maps, const int32_t *home,
                     double *score, int32_t *best, double *best_map, int32_t *status);

/* ---- TWIX raw reconstruction --------------------------------------- */
/* process_RAW's image from raw k-space (Vent_Analysis.py:537-540): for every slice k,
 * fftshift(fft2(fftshift(K[:, :, k]))) in complex128, then np.transpose(., (1, 0, 2))[:, ::-1, :].
 * k: complex128 as interleaved (re, im) doubles, C order [n0][n1][nz]; out: complex128 [n1][n0][nz].
 * (The twix file parse, mapvbvd at :532-536, stays on the host.)  1 <= n0, n1 <= 5120. */
int vh_recon(vh_ctx *ctx, const double *k, int64_t n0, int64_t n1, int64_t nz, double *out);

/* ---- host-to-host pipeline ------------------------------------------------------------------ */
/* Streams n host-resident studies through `slots` device batches of `sub` volumes each (one HIP
 * stream and one host thread per slot, pinned staging per slot): while one slot computes, the
 * others upload their next sub-batch or download their last results.  Outputs are host arrays of
 * n volumes (any may be NULL); res[n].  A ragged last sub-batch is padded with copies of its last
 * study (results discarded).  Build-defined: SURVEY section 8(e) partitioning on one GPU. */
typedef struct vh_pipe vh_pipe;
int vh_pipe_create(vh_ctx *ctx, int64_t R, int64_t C, int64_t Z, int64_t sub, int slots,
                   vh_pipe **out);
int vh_pipe_run(vh_pipe *p, const float *hp, const uint8_t *mask, int64_t n, const vh_run_opts *opts,
                float *n4, uint8_t *defect, uint8_t *defect_border, uint8_t *lb,
                vh_vdp_result *res);
int vh_pipe_destroy(vh_pipe *p);
/* The last vh_pipe_run's peak of caller memory pinned in place (bytes) and the caller ranges that
 * went through the pinned staging instead (not registrable, or past the VH_PIPE_PIN_CAP budget,
 * default 32 GiB per node divided by LOCAL_WORLD_SIZE: a long cohort run never page-locks more than
 * that at once). */
int vh_pipe_stats(vh_pipe *p, int64_t *pinned_peak_bytes, int64_t *staged_spans);
/* This GPU's PCIe link with pinned host memory (bench.py's host-to-host bound): bytes copied H2D
 * alone, D2H alone and both at once on two streams, best of 3; out_gbps = {h2d, d2h, both}. */
int vh_link_probe(vh_ctx *ctx, int64_t bytes, double out_gbps[3]);
/* Page-locked host memory on the context's device (hipHostMalloc) for result arrays the caller
 * reuses: a D2H into it runs at the link rate with no runtime staging.  vh_host_free takes any
 * pointer vh_host_alloc returned (also after vh_destroy). */
int vh_host_alloc(vh_ctx *ctx, int64_t bytes, void **out);
int vh_host_free(void *p);

/* ---- multi-GPU (RCCL over xGMI) -------------------------------------------------------------- */
#define VH_COMM_ID_BYTES 128
int vh_comm_unique_id(uint8_t id[VH_COMM_ID_BYTES]);
int vh_comm_init(vh_ctx *ctx, int nranks, int rank, const uint8_t id[VH_COMM_ID_BYTES]);
/* Sum the batch's device cohort histogram over all ranks of the context's communicator. */
int vh_batch_cohort_allreduce(vh_batch *b);
/* The communicator as RCCL sees it: its rank count (ncclCommCount) and this context's rank
 * (ncclCommUserRank).  bench.py's N > 1 line reports both (ABI 8). */
int vh_comm_info(vh_ctx *ctx, int *nranks, int *rank);
int vh_comm_destroy(vh_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* VENT_HIP_H */
