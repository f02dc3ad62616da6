/*
 * pcseg.h -- C ABI of libpcseg.so, the MI355X (gfx950) implementation of the
 * per-frame segmentation hot path of ssilverman16/particle_col_image_segmentation.
 *
 * The reference has NO FFI of its own (it is pure Python calling scipy /
 * scikit-image); each entry point below replaces the library call or loop the
 * reference makes at the cited file:line.  The Python host layer
 * (particle_col_image_segmentation_amd/) binds these with ctypes; the stub a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every image argument is a DEVICE pointer to a contiguous batch-major,
 *     row-major array (B, H, W) or (B, C, H, W); buffers are caller-owned
 *     (torch tensors' data_ptr()); the library allocates nothing persistent;
 *   - scratch comes from a caller-provided workspace sized by the matching
 *     *_workspace_bytes(B, H, W) query (256-byte aligned device memory); a
 *     workspace's prior contents never affect a result, and nothing beyond
 *     the size the query named is written;
 *   - an output buffer's prior contents never affect a result either (only an
 *     argument documented as accumulated in place is read before it is
 *     written), and nothing outside an output is written;
 *   - work is enqueued on `stream` (a hipStream_t) and every compute entry point
 *     returns without waiting for it: no hidden host synchronisation, fixed
 *     points included (they finish in device-side tail kernels);
 *   - return value: PCSEG_OK or a negative pcseg_status; the message is in
 *     pcseg_last_error() (thread local);
 *   - there is no CPU fallback anywhere: without a HIP device every compute
 *     entry point returns PCSEG_ERR_HIP.
 */
#ifndef PCSEG_H
#define PCSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *pcseg_stream_t; /* hipStream_t */

enum pcseg_status {
    PCSEG_OK = 0,
    PCSEG_ERR_ARG = -1,       /* bad shape / null pointer / unsupported size */
    PCSEG_ERR_HIP = -2,       /* a HIP call or launch failed */
    PCSEG_ERR_WORKSPACE = -3, /* workspace too small */
    PCSEG_ERR_CAPACITY = -4,  /* more labels than the caller's table capacity */
    PCSEG_ERR_CONVERGENCE = -5 /* an iteration passed its bound without reaching its fixed point */
};

/* layout of one row of the region table (int64 each) -- skimage regionprops
 * fields the reference consumes: area (tiff_analysis.py:769-781), centroid sums
 * (:406,844,1054), bbox half-open (:860-863), raster-first pixel (:1041-1044) */
enum pcseg_region_col {
    PCSEG_R_AREA = 0, PCSEG_R_SUM_ROW = 1, PCSEG_R_SUM_COL = 2,
    PCSEG_R_MIN_ROW = 3, PCSEG_R_MIN_COL = 4, PCSEG_R_MAX_ROW1 = 5, PCSEG_R_MAX_COL1 = 6,
    PCSEG_R_FIRST = 7, PCSEG_R_NCOLS = 8
};

int pcseg_version(void);
const char *pcseg_last_error(void);
int pcseg_device_count(void);

/* ---- measurement aid (bench.py's roofline leg): when enabled, every kernel launch is bracketed by hipEvents
 * recorded on the launch stream.  pcseg_timing_report waits for them and writes one line per kernel
 * "name<TAB>launches<TAB>total_ms"; it returns the number of bytes written (needed size when buf is NULL)
 * and clears the records.  Off by default. */
void pcseg_timing_enable(int on);
int pcseg_timing_report(char *buf, size_t buf_bytes);

/* ---- ingest: class map = argmax over the C planes + 1 (what ilastik's
 * "Simple Segmentation" export holds; read at tiff_analysis.py:118-121, 639-642) */
int pcseg_argmax_planes_f32(const float *stack, uint8_t *cls, int B, int C, int H, int W, pcseg_stream_t stream);

/* ---- A1: scipy.ndimage.median_filter(ds_arr, size=5), mode='reflect'
 * (tiff_analysis.py:122, 643) */
int pcseg_median5_u8(const uint8_t *in, uint8_t *out, int B, int H, int W, pcseg_stream_t stream);

/* ---- ingest + A1 + A2 in one call: class map (argmax + 1) -> median_filter(size=5) -> label(z_slice)
 * (tiff_analysis.py:639-643, 743).  Same results as pcseg_argmax_planes_f32, pcseg_median5_u8, pcseg_ccl8_equal_u8 in
 * sequence, but for C <= 5 planes the three tile passes are ONE kernel: the raw class map is never written, the medians
 * are labelled while they sit in LDS.  denoised: uint8 (B,H,W) = the median-filtered class map (what the reference
 * calls ds_arr / z_slice); labels / counts as pcseg_ccl8_equal_u8. */
size_t pcseg_classmap_label_workspace_bytes(int B, int H, int W);
int pcseg_classmap_label_f32(const float *stack, int C, uint8_t *denoised, int32_t *labels, int32_t *counts,
                             int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A2: skimage.measure.label (tiff_analysis.py:743, 260, 829;
 * refine_boundaries.py:64) and scipy.ndimage.label (inside binary_fill_holes).
 * labels: int32 (B,H,W), 0 = background, 1..N in raster order of each
 * component's first pixel; counts[b] = N of frame b (device int32[B]). */
size_t pcseg_ccl_workspace_bytes(int B, int H, int W);
int pcseg_ccl8_equal_u8(const uint8_t *in, int32_t *labels, int32_t *counts, int B, int H, int W,
                        void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_ccl8_bool(const uint8_t *in, int32_t *labels, int32_t *counts, int B, int H, int W,
                    void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_ccl4_bool(const uint8_t *in, int32_t *labels, int32_t *counts, int B, int H, int W,
                    void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
/* renumber a root image (value = linear index of the component's first pixel
 * + 1, 0 = background) into 1..N raster order; `labels` must not alias `roots`. */
int pcseg_compact_labels(const int32_t *roots, int32_t *labels, int32_t *counts, int B, int H, int W,
                         void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A3 + M1: regionprops fields and per-ROI isotope sums
 * (tiff_analysis.py:746-773, 1041-1044; .m:122-135, 186-199).
 * stats: int64 (B, cap, 8) rows as pcseg_region_col; cls_out: uint8 (B, cap) =
 * class-map value at the raster-first pixel (NULL if cls is NULL); sums:
 * float64 (B, cap, C) (NULL if planes is NULL).  Labels above cap are dropped
 * and overflow[b] (device int32[B], may be NULL) is set. */
int pcseg_region_reduce(const int32_t *labels, const uint8_t *cls, const float *planes, int C,
                        int B, int H, int W, int cap, int64_t *stats, uint8_t *cls_out, double *sums,
                        int32_t *overflow, pcseg_stream_t stream);
/* same, but only rows l < counts[b] (device int32[B], e.g. from pcseg_ccl*) are
 * initialised and filled; rows beyond are left untouched. */
int pcseg_region_reduce_n(const int32_t *labels, const int32_t *counts, const uint8_t *cls, const float *planes,
                          int C, int B, int H, int W, int cap, int64_t *stats, uint8_t *cls_out, double *sums,
                          int32_t *overflow, pcseg_stream_t stream);
/* same, with the plane sums restricted to the pixels whose class-map value is in sum_class_bits (bit v = value v,
 * v < 64; 0 = every pixel): the regions of the other classes keep sums of 0 and their planes are not read.  The
 * reference only ever sums isotopes over cell ROIs (tiff_analysis.py:1041-1044). */
int pcseg_region_reduce_sel(const int32_t *labels, const int32_t *counts, const uint8_t *cls, uint64_t sum_class_bits,
                            const float *planes, int C, int B, int H, int W, int cap, int64_t *stats,
                            uint8_t *cls_out, double *sums, int32_t *overflow, pcseg_stream_t stream);

/* (pcseg_region_reduce_sel with planes == NULL but sums != NULL and C >= 1: the integer columns only, the first
 * counts[b] rows of sums are ZEROED -- for pcseg_region_sums2.)
 *
 * Table initialisation alone: the first min(counts[b], cap) rows of stats (B, cap, 8) get the neutral element of the
 * reduction (0 sums, empty bounding box), those of sums (B, cap, C) (C may be 0) are zeroed, overflow[b] (may be NULL)
 * cleared; counts == NULL: every row. */
int pcseg_region_init(const int32_t *counts, int cap, int C, int B, int H, int W, int64_t *stats, double *sums,
                      int32_t *overflow, pcseg_stream_t stream);

/* Plane sums of TWO label images over the same planes in ONE pass (.m:122-135 for the class-map components and for the
 * refined ROIs; the planes are the largest thing a reduction reads): sums_a (B, cap_a, C) += per-label sums of labels_a
 * restricted to the pixels whose class-map value is in sum_class_bits (0 = every pixel), sums_b (B, cap_b, C) += per-label
 * sums of labels_b.  stats_b != NULL: image B's integer columns (pcseg_region_col) are accumulated into stats_b
 * (B, cap_b, 8) / overflow_b by the plane-free pass, launched ahead of the sums.  Every table must have been initialised (pcseg_region_init, or
 * pcseg_region_reduce_sel for image A); without stats_b labels above the capacity are skipped silently.  W % 4 == 0,
 * 16-byte aligned images. */
int pcseg_region_sums2(const int32_t *labels_a, const uint8_t *cls, uint64_t sum_class_bits, int cap_a, double *sums_a,
                       const int32_t *labels_b, int cap_b, double *sums_b, int64_t *stats_b, int32_t *overflow_b,
                       const float *planes, int C, int B, int H, int W, pcseg_stream_t stream);

/* ---- R1: binary_mask = boundary_map < threshold (refine_boundaries.py:44-45) */
int pcseg_threshold_lt_f32(const float *img, float threshold, uint8_t *mask, int B, int H, int W,
                           pcseg_stream_t stream);

/* ---- R2: scipy.ndimage.distance_transform_edt as exact integer squared
 * distance to the nearest zero pixel (refine_boundaries.py:60,
 * tiff_analysis.py:996); the float64 distance is sqrt((double)d2).  cap < 0:
 * exact everywhere; cap >= 0: values above cap are reported as cap + 1.  A
 * frame without any zero pixel follows scipy: virtual zero pixel at (-1, 0).
 * Every shape check_shape admits is exact: squared distances reach (H - 1)^2 + (W - 1)^2 < 2^31 (H * W < 2^30).
 * The threshold members of the EDT family (dilation, particle fill) with a reach of at most 31 pixels -- the radius, or for
 * the particle fill floor(sqrt(max(radius^2, threshold^2 - 1))) -- work on bit words and take any width.  With a larger reach
 * they stage 8 rows of uint16 distances plus the rows' bytes in LDS beside 1056 bytes of the kernel's own:
 * 24 * ((W + 3) & ~3) + 1056 <= 163 840, i.e. W <= 6780; a wider frame is refused ("too wide"), nothing is launched. */
size_t pcseg_edt_workspace_bytes(int B, int H, int W);
int pcseg_edt_sq_u8(const uint8_t *mask, int32_t *d2, int B, int H, int W, int cap,
                    void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
/* fused R1 + R2: mask = img < threshold (also written to mask_out if not NULL).
 * frame_stride = float32 elements between consecutive frames of img (0 = H*W),
 * so that a plane of a (B,C,H,W) stack is read in place (refine_boundaries.py:34). */
int pcseg_edt_sq_lt_f32(const float *img, int64_t frame_stride, float threshold, int32_t *d2, uint8_t *mask_out,
                        int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A6: skimage.morphology.binary_dilation(binary, disk(radius))
 * (tiff_analysis.py:827-828, 990) with binary = ((value_bits >> in) & 1),
 * i.e. `z_slice == v` for one bit and the OR of several classes for several
 * (tiff_analysis.py:812, 816-818); out is 0/1. */
int pcseg_dilate_disk_u8(const uint8_t *in, uint64_t value_bits, int radius, uint8_t *out,
                         int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A6 fused: components of binary_dilation(((value_bits >> in) & 1), disk(radius)) as a union-find parent
 * image (int32 (B,H,W): linear index of a pixel of the same component, -1 = background), computed on a 1-bit image
 * (the dilation is shifts / ORs of 32-row column words).  Feeds pcseg_merge_groups(keys_are_roots = 1). */
size_t pcseg_dilate_ccl_workspace_bytes(int B, int H, int W);
int pcseg_dilate_ccl_roots_u8(const uint8_t *in, uint64_t value_bits, int radius, int32_t *roots,
                              int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
/* the same components WITHOUT a label image, for callers that only look the components up at a few pixels (the merge
 * step reads them at the region centroids, tiff_analysis.py:844-847): dilated_bits = the dilated mask as 32-row column
 * words, uint32 (B, ceil(H/32), W), bit j of word (ch, c) = pixel (32 ch + j, c); run_parent = union-find over the
 * vertical runs of set bits, int32 (B, H, W) of which ONLY the entries at the top pixel of each run (within its word)
 * are written and meaningful.  Feeds pcseg_merge_groups_runs. */
size_t pcseg_dilate_ccl_runs_workspace_bytes(int B, int H, int W);
int pcseg_dilate_ccl_runs_u8(const uint8_t *in, uint64_t value_bits, int radius, uint32_t *dilated_bits,
                             int32_t *run_parent, int B, int H, int W, void *workspace, size_t workspace_bytes,
                             pcseg_stream_t stream);
/* the same for n_masks (<= 4) masks of one class map at once -- get_cell_clusters_from_distances dilates and labels one
 * mask per cell type plus the union of all types (tiff_analysis.py:806-822): the map is read once, every pass behind the
 * bit planes is ONE launch over n_masks * B frames.  value_bits: HOST array [n_masks]; dilated_bits (n_masks, B,
 * ceil(H/32), W); run_parent (n_masks, B, H, W).  Any width and alignment (W % 4 == 0 with a 4-byte aligned map and a
 * 16-byte aligned workspace takes the fast bit setter; pcseg_dilate_ccl_runs_u8 is this call with one mask).
 * Workspace: pcseg_dilate_ccl_runs_workspace_bytes(B * n_masks, H, W). */
int pcseg_dilate_ccl_runs_multi_u8(const uint8_t *in, const uint64_t *value_bits, int n_masks, int radius,
                                   uint32_t *dilated_bits, int32_t *run_parent, int B, int H, int W,
                                   void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A8: fill_particle_area (tiff_analysis.py:982-1015) in one pass pair:
 * out = ds with overlap pixels set to overlap_label, where overlap =
 * (ds == cell_label) & (EDT(ds != particle) < dist_threshold | dilate(ds ==
 * particle, disk(dilation_radius))); overlap_area[b] += count (device int64[B]). */
int pcseg_fill_particle(const uint8_t *ds, uint8_t *out, int particle_label, int cell_label,
                        int overlap_label, int dilation_radius, int dist_threshold, int64_t *overlap_area,
                        int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A7: scipy.ndimage.binary_fill_holes (tiff_analysis.py:880) */
size_t pcseg_fill_holes_workspace_bytes(int B, int H, int W);
int pcseg_fill_holes(const uint8_t *mask, uint8_t *out, int B, int H, int W,
                     void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- R3 + R4: skimage.morphology.local_maxima(distance) and
 * measure.label(local_max) (refine_boundaries.py:63-64) on an int32 image
 * (d2 is order-isomorphic to the float64 distance).  is_max: uint8 (NULL to
 * skip); markers: int32 1..K raster order (NULL to skip); counts: int32[B],
 * the K of every frame: written with the markers only (NULL without them). */
size_t pcseg_local_maxima_workspace_bytes(int B, int H, int W);
int pcseg_local_maxima_i32(const int32_t *img, uint8_t *is_max, int32_t *markers, int32_t *counts,
                           int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- W1: skimage.segmentation.watershed(image, markers, mask=mask),
 * connectivity 1, no compactness, no watershed line (refine_boundaries.py:73).
 * Asynchronous like everything else: the two fixed points (minimax levels, second-level keys) run a fixed number
 * of grid rounds and finish in one-block-per-frame tail kernels, the frames that need the second level / the exact
 * flood are listed and counted on the device.
 * mode 0: parallel flood + proof check, frames that fail the check
 * are re-run by the exact sequential priority flood; mode 1: exact sequential
 * flood for every frame; mode 2: parallel flood only (tie_flags tells which
 * frames are NOT proven exact); add 4 to also run the explicit per-pixel proof
 * check (implied by the component test, kept for verification).  tie_flags:
 * device int32[B] (may be NULL).
 * Test-only bits (at most one of them, never with mode 1; the pipeline never sets them): between two passes of the
 * union-find label assignment, overwrite up to four root entries of its internal parent image per frame, chosen by
 * the frame index b (b % 6: 0 none, 1 2000000000, 2 -1, 3 INT_MIN, 4 a two-cycle of two roots, 5 H*W + 5), to show
 * that every walk over that image is fenced -- a poisoned frame comes back flagged (mode 2) or recomputed by the
 * exact flood (mode 0), never with wrong labels or an access outside its frame:
 *   PCSEG_WS_POISON_BORDER  first level, before the cross-tile border pass (roots named from a union-find tile seam)
 *   PCSEG_WS_POISON_LABEL   first level, before the label pass
 *   PCSEG_WS_POISON_LEVEL2  second level (listed frames, active tiles), before its label passes
 * frame_stride: as for pcseg_edt_sq_lt_f32 (0 = H*W).
 * img: any float32 but NaN -- -0.0 and +0.0 are one level, infinities and subnormals are ordinary levels; a NaN
 * inside the mask is outside the contract (the reference's comparisons are unordered there, the labels undefined). */
enum pcseg_ws_poison { PCSEG_WS_POISON_BORDER = 8, PCSEG_WS_POISON_LABEL = 16, PCSEG_WS_POISON_LEVEL2 = 32 };
size_t pcseg_watershed_workspace_bytes(int B, int H, int W);
/* measurement aid: out[0] = 64x64 tiles the minimax relaxation actually processed (marked tiles over all rounds;
 * kept in a counter on the current device and read with a blocking copy, i.e. after everything queued so far),
 * out[1] = relaxation grid launches (including the rounds that find nothing marked), out[2] = watershed
 * calls since the last reset (process-wide).  reset != 0 synchronises the device. */
void pcseg_watershed_counters(int64_t *out, int reset);
int pcseg_watershed4_f32(const float *img, int64_t frame_stride, const int32_t *markers, const uint8_t *mask,
                         int32_t *out, int32_t *tie_flags, int B, int H, int W, int mode,
                         void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- A6 tail: get_merged_regions grouping (tiff_analysis.py:843-878).
 * region_list[b][k] (k < n_list[b]) is the reference's og_cell_regions as
 * 0-based row indices into the (B, cap, 8) stats table, in list order.  key =
 * dilated_labels at the truncated centroid; list entries sharing a non-zero
 * key form one group, groups numbered 1.. in the order of their first member;
 * group_of[b][k] = group id or 0 (centroid on a zero pixel -> dropped, :848).
 * region_list / group_of: int32 (B, list_cap); n_list / n_groups: int32[B].
 * keys_are_roots != 0: `dilated_labels` is the parent image of pcseg_dilate_ccl_roots_u8 (no numbering pass needed,
 * groups only need "same component").
 * An entry outside [0, cap), a region of area 0 and a region whose centroid lies outside the frame get group 0 too;
 * entries of group_of at or beyond n_list[b] are not written.
 * Every grouping entry point below is ONE launch of the same kernel, one block per frame (and mask): they differ in
 * where a key comes from (label image, parent image, run components) and in whether the member sums are wanted.
 * The workspace is only touched by frames that list more than 4096 regions (shorter lists are grouped in LDS). */
size_t pcseg_merge_groups_workspace_bytes(int B, int list_cap);
int pcseg_merge_groups(const int32_t *dilated_labels, int keys_are_roots, const int64_t *stats,
                       const int32_t *region_list, const int32_t *n_list, int32_t *group_of, int32_t *n_groups,
                       int B, int H, int W, int cap, int list_cap, void *workspace, size_t workspace_bytes,
                       pcseg_stream_t stream);
/* the same grouping on the run-based components of pcseg_dilate_ccl_runs_u8 (workspace: pcseg_merge_groups_workspace_bytes) */
int pcseg_merge_groups_runs(const uint32_t *dilated_bits, const int32_t *run_parent, const int64_t *stats,
                            const int32_t *region_list, const int32_t *n_list, int32_t *group_of, int32_t *n_groups,
                            int B, int H, int W, int cap, int list_cap, void *workspace, size_t workspace_bytes,
                            pcseg_stream_t stream);

/* get_merged_regions' grouping AND the member sums of its groups (tiff_analysis.py:843-878) in ONE launch, on the
 * run-based components of pcseg_dilate_ccl_runs_u8: what pcseg_merge_groups_runs followed by pcseg_group_reduce
 * computes, with the list of type slot `slot` read in place from the (B, n_slots, cap) region lists and (B, n_slots)
 * list lengths pcseg_classify_regions writes (list capacity = cap).  group_of int32 (B, cap): every entry below the
 * list length is written; n_groups int32[B]; group_stats int64 (B, cap, 8): rows below n_groups[b] are written.
 * Workspace: pcseg_merge_groups_workspace_bytes(B, cap). */
int pcseg_merge_groups_fused(const uint32_t *dilated_bits, const int32_t *run_parent, const int64_t *stats,
                             const int32_t *region_lists, const int32_t *n_lists, int slot, int n_slots,
                             int32_t *group_of, int32_t *n_groups, int64_t *group_stats, int B, int H, int W, int cap,
                             void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* pcseg_merge_groups_fused for n_masks (<= 4) masks in ONE launch: dilated_bits (n_masks, B, ceil(H/32), W) and run_parent
 * (n_masks, B, H, W) as pcseg_dilate_ccl_runs_multi_u8 leaves them, mask m grouped over the list of type slot slots[m]
 * (HOST array); group_of (n_masks, B, cap), n_groups (n_masks, B), group_stats (n_masks, B, cap, 8).
 * Workspace: pcseg_merge_groups_workspace_bytes(B * n_masks, cap). */
int pcseg_merge_groups_fused_multi(const uint32_t *dilated_bits, const int32_t *run_parent, const int64_t *stats,
                                   const int32_t *region_lists, const int32_t *n_lists, const int32_t *slots, int n_masks,
                                   int n_slots, int32_t *group_of, int32_t *n_groups, int64_t *group_stats, int B, int H,
                                   int W, int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* member sums of the groups of a caller's own group_of (what pcseg_merge_groups_fused adds up in its own launch):
 * group_stats int64 (B, list_cap, 8) = area, sum_row, sum_col, min_row, min_col, max_row+1, max_col+1, members
 * (tiff_analysis.py:855-872) */
int pcseg_group_reduce(const int64_t *stats, const int32_t *region_list, const int32_t *n_list,
                       const int32_t *group_of, const int32_t *n_groups, int64_t *group_stats,
                       int B, int H, int W, int cap, int list_cap, pcseg_stream_t stream);

/* ---- A3 tail + A4: the per-region loop of get_cell_positions_and_areas
 * (tiff_analysis.py:754-781) and the region lists get_cell_clusters_from_distances
 * builds (:794-796).  Class tables are HOST arrays: class_slot[256] maps a class
 * value to a cell-type slot (255 = none), class_particle[256] flags "Particle",
 * min_cell / min_cluster [n_slots] are MIN_CELL_AREA / MIN_CLUSTER_AREA (:54-60).
 * Outputs (device): kind (B,cap) 0 none / 1 cell / 2 cluster; slot_of (B,cap);
 * cells (B,cap) = 1 for cells, int(area // mean cell area) for clusters, -1 when
 * the reference would raise (clusters but no single cell; nan_flag[b] = 1);
 * particle_area int64[B]; type_stats int64 (B,4,4) = n_cells, n_clusters,
 * sum of cell areas, first region index; region_list int32 (B,5,cap): per slot
 * cells then clusters in label order, row 4 = the "combined" list (types in the
 * order of their first region); n_list int32 (B,5). */
int pcseg_classify_regions(const int64_t *stats, const uint8_t *cls_out, const int32_t *counts,
                           const uint8_t *class_slot, const uint8_t *class_particle,
                           const int32_t *min_cell, const int32_t *min_cluster, int n_slots,
                           uint8_t *kind, uint8_t *slot_of, int32_t *cells, int64_t *particle_area,
                           int64_t *type_stats, int32_t *region_list, int32_t *n_list, int32_t *nan_flag,
                           int B, int cap, pcseg_stream_t stream);

/* ---- C14: nearest distance from every point of a (na, 2) float64 set to a (nb, 2) set = min(pdist2(a, b), [], 2)
 * (.m:260-263 between the two ROI classes, .m:301-305 to the aggregate boundary, one frame and one brute-force block at a
 * time; the batched, pruned route to a mask's surface is pcseg_surface_points + pcseg_surface_distances); out_a: float64[na]. */
int pcseg_nearest_dist_f64(const double *a, int na, const double *b, int nb, double *out_a, pcseg_stream_t stream);

/* ---- C6: combine_cell_positions_and_clusters (tiff_analysis.py:252-287):
 * out = dapi with every 8-connected component of (dapi == 1) whose overlap
 * with (other == 1) exceeds `threshold` of its area set to 2. */
size_t pcseg_overlap_workspace_bytes(int B, int H, int W);
int pcseg_remove_overlapping(const uint8_t *dapi, const uint8_t *other, double threshold, uint8_t *out,
                             int B, int H, int W, void *workspace, size_t workspace_bytes,
                             pcseg_stream_t stream);

/* ---- per-ROI table output (SURVEY.md 8b output formats / 8e: what the ranks all-gather): the fixed-capacity
 * per-frame tables of the calls above, compacted on the device into dense float64 row tables.
 *   rois   (n, 5 + C + n_ratios)   frame, label, area, centroid_row, centroid_col, S_0.., ratios (.m:136-139 form:
 *                                  S[num] / sum of S[den...]); one row per refined ROI that owns a pixel
 *   cells  (n, 14 + C + n_ratios)  frame, label, class, kind (1 cell, 2 cluster), area, centroid (2), bbox (4), cells,
 *                                  group, group_combined, S_0.., ratios; one row per cell / cluster region
 *   groups (n, 11)                 frame, slot (4 = combined), group, area, centroid (2), bbox (4), members
 *   frames int64 (B, 17)           n_labels, n_rois, particle_area, particle_area + overlap, tie_flag, then per
 *                                  cell-type slot: present, count, area in pixels (tiff_analysis.py:1018-1038
 *                                  before its two round(x, 5), which the host applies)
 * pcseg_table_layout counts and scans (totals: device int64[6] = rows of rois, cells, groups, then the number of frames
 * with overflow / ws_overflow / nan_flag set, so that one read-back serves the caller's checks too); the caller reads the
 * totals, allocates, and pcseg_table_write fills the tables.  The workspace then holds the frames' row counts and row
 * offsets (layout: table_offsets() in csrc/table_common.h, the only definition); it is the `table_workspace` that
 * pcseg_cell_distances, pcseg_neighbours_pack_cells, pcseg_surface_pack_cells and pcseg_refined_table_write read, opaque
 * to callers.  Both asynchronous on `stream`; every pointer of the
 * struct is a device pointer, group_of / n_groups / group_stats entries may be NULL (slot absent / merged = False). */
typedef struct pcseg_table_inputs {
    int32_t B, cap, C, n_ratios;
    const int64_t *frame_ids;                                   /* (B) id written into column 0 */
    const int32_t *counts; const int64_t *stats; const uint8_t *cls_out; const double *cc_sums;  /* class-map components */
    const uint8_t *kind; const uint8_t *slot_of; const int32_t *cells;                            /* pcseg_classify_regions */
    const int64_t *particle_area; const int64_t *overlap_area; const int64_t *type_stats; const int32_t *tie_flags;
    const int32_t *region_list; const int32_t *n_list;          /* (B, 5, cap), (B, 5) */
    const int32_t *group_of[5]; const int32_t *n_groups[5]; const int64_t *group_stats[5];       /* (B, cap), (B), (B, cap, 8) */
    const int32_t *n_markers; const int64_t *ws_stats; const double *ws_sums;                     /* refined ROIs */
    int32_t ratio_num[8]; int32_t ratio_den[8][4];              /* plane indices, -1 = unused */
    const int32_t *overflow; const int32_t *ws_overflow; const int32_t *nan_flag;  /* per-frame flags (B), may be NULL */
} pcseg_table_inputs;
size_t pcseg_table_workspace_bytes(int B, int cap);
int pcseg_table_layout(const pcseg_table_inputs *in, int64_t *totals, void *workspace, size_t workspace_bytes,
                       pcseg_stream_t stream);
int pcseg_table_write(const pcseg_table_inputs *in, double *rois, double *cells, double *groups, int64_t *frames,
                      void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- C14 for a batch (HCN_nanosims_rois_activity_distance_5iso_YG.m:260-268): dist[i] = distance from row i of the dense
 * `cells` table pcseg_table_write has just filled to the nearest row of the OTHER of the two cell types (slots 0 and 1 of
 * class_slot, a HOST array class value -> slot) in the same frame, / (size / raster) (the script: size 512, raster 19);
 * positions (centroid_col + 1, centroid_row + 1) as MATLAB's regionprops reports them; NaN for rows without an entry
 * (another type, or a frame in which one of the two types is absent).  `workspace` is the one pcseg_table_layout /
 * pcseg_table_write used (it holds the frames' row offsets).  PARITY UNPINNED (no MATLAB here). */
int pcseg_cell_distances(const double *cells, int64_t n_rows, int ncol, const uint8_t *class_slot, double raster, double size,
                         double *dist, int B, const void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- goal 3 of refine_boundaries.py:8-12 (per-strain nearest neighbours and pair distances), batched: points in
 * frame-contiguous order -- xy device float64 (n, 2), slot device int32 (n) in 0..K-1 (any other value: the point takes
 * part in nothing and gets NaN / -1), id device int32 (n), frame_offsets device int64 (B + 1), K <= 4, n < 2^24.
 *   dist  device float64 (n, K): for point i and slot t, sqrt(min d2) / scale over the OTHER points j of slot t in i's
 *         frame (excluded by index: a duplicate position gives 0); d2 = dx*dx + dy*dy, each product and the sum rounded
 *         on their own (no FMA; pcseg_cell_distances is compiled to fma(dx, dx, dy*dy), up to 1 ulp apart); NaN when there is no candidate
 *   nn_id device int32 (n, K): id of that neighbour, the smallest id among equal minimal d2; -1 when there is none
 *   pair_hist device int64 (B, K (K + 1) / 2, m + 2), rows in (slot_a <= slot_b) order: [n_pairs, bin_0 .. bin_m-1, over]
 *         over the unordered pairs of the frame, bin k = edges[k] <= d < edges[k + 1], over = d >= edges[m], so that
 *         bins + over = n_pairs = n_a (n_a - 1) / 2 or n_a n_b.  edges: HOST float64 (n_edges = m + 1, 2..1025),
 *         edges[0] == 0, strictly increasing; edges == NULL, n_edges == 0, pair_hist == NULL: no histogram.
 * pcseg_neighbours_pack_cells: the points of the dense `cells` table pcseg_table_write has just filled -- xy =
 * (centroid_col + 1, centroid_row + 1), slot = class_slot[class] (a HOST array, 255 -> -1), id = label -- and the
 * frames' offsets (B + 1); `table_workspace`: see pcseg_table_layout. */
size_t pcseg_neighbours_workspace_bytes(int64_t n_points, int B, int K, int n_edges);
int pcseg_point_neighbours(const double *xy, const int32_t *slot, const int32_t *id, const int64_t *frame_offsets, int64_t n_points,
                           int B, int K, double scale, const double *edges, int n_edges, double *dist, int32_t *nn_id,
                           int64_t *pair_hist, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_neighbours_pack_cells(const double *cells, int ncol, const uint8_t *class_slot, int B, const void *table_workspace,
                                size_t table_workspace_bytes, double *xy, int32_t *slot, int32_t *id, int64_t *frame_offsets,
                                pcseg_stream_t stream);

/* ---- random-labelling envelopes of those pair histograms (csrc/mixing.hip): the points stay, the slots are shuffled.
 * xy / slot / frame_offsets / K / scale / edges as for pcseg_point_neighbours (edges required, n_edges = m + 1);
 * frame_keys device int64 (B): the id of every frame (its low 24 bits enter the generator).  The typed points of a frame
 * are those with 0 <= slot < K, in the caller's order, i = 0 .. n_t - 1; every other point takes part in nothing.
 * Labelling p = 0 is the observed one; for p = 1 .. n_perm, with rem[s] = the frame's typed points of slot s, tot = n_t,
 * for i = 0 .. n_t - 1 (all uint64, mod 2^64):
 *     c = ((key & 0xFFFFFF) << 40) ^ (p << 24) ^ i;  z = c * 0x9E3779B97F4A7C15 + seed;
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31;
 *     r = (z * tot) >> 64 (the high half of the 128-bit product);  label_p(i) = the smallest s with r < rem[0] + .. +
 *     rem[s];  rem[s] -= 1;  tot -= 1
 * (sequential sampling without replacement: every arrangement with the observed per-slot counts equally likely up to the
 * 2^-40 bias of the multiply-high; a frame's result depends on its key, not on its place in the batch).
 *   counts   device int64 (B, n_perm + 1, Q, m), Q = K (K + 1) / 2 rows in (slot_a <= slot_b) order, or NULL (then the
 *            workspace holds them: pcseg_mixing_workspace_bytes(.., with_counts = 1)): N_p = the unordered pairs of typed
 *            points whose labels under p are {a, b} and whose distance lies in bin k (pcseg_point_neighbours' bin rule
 *            to the bit; pairs at d >= edges[m] are not counted)
 *   envelope device int64 (12, B, Q, m): obs = N_0, then over p = 1 .. n_perm lo = min, hi = max, sum, n_le = #{p: N_p <=
 *            obs}, n_ge = #{p: N_p >= obs}; then the same six of the cumulative counts C_p[k] = N_p[0] + .. + N_p[k].
 *            With n_perm = 0 everything but obs and the cumulative obs is 0.
 * Exact integers, the same bits for the same arguments.  Every count is a 64-bit integer: a frame has fewer than 2^24
 * points, so fewer than 2^47 pairs, and the sums over at most 65535 permutations stay below 2^63 -- nothing can wrap, and
 * a batch of n_points >= 2^24 is rejected with PCSEG_ERR_ARG like every other bad argument: K outside 1..4, edges that
 * pcseg_point_neighbours would reject, n_perm outside 0..65535, a null pointer (counts excepted); a short workspace gives
 * PCSEG_ERR_WORKSPACE.  pcseg_mixing_workspace_bytes returns 0 for sizes it rejects.  pcseg_mixing_tile: the points of
 * one LDS tile of the pair walk (larger frames are walked tile against tile). */
size_t pcseg_mixing_workspace_bytes(int64_t n_points, int B, int K, int n_edges, int n_perm, int with_counts);
int pcseg_pair_label_mixing(const double *xy, const int32_t *slot, const int64_t *frame_offsets, const int64_t *frame_keys,
                            int64_t n_points, int B, int K, double scale, const double *edges, int n_edges, int n_perm,
                            uint64_t seed, int64_t *counts, int64_t *envelope, void *workspace, size_t workspace_bytes,
                            pcseg_stream_t stream);
int pcseg_mixing_tile(void);

/* ---- goal 2 of refine_boundaries.py:1-12 (refined ROIs related to the class-map components they split), batched.
 * pcseg_label_parent: labels_a (class-map components) and labels_r (refined ROIs), device int32 (B, H, W), any width
 * and alignment; counts_r device int32 (B).  ov(r, a) = #pixels with labels_r = r and labels_a = a, a >= 1 (pixels on
 * a = 0 or r = 0 count for nothing); rows r = 1 .. min(counts_r[b], cap) (row r - 1 of the (B, cap) outputs; other rows
 * 0), labels_r above that are skipped.
 *   parent    device int32 (B, cap): the a maximising ov(r, a), the smallest on ties; 0 when there is none
 *   parent_px device int32 (B, cap): ov(r, parent);  n_overlap device int32 (B, cap): #distinct a with ov(r, a) > 0
 *   cls_r     device uint8 (B, cap), may be NULL: cls_a[b, parent - 1] (cls_a device uint8 (B, cap), may be NULL: 0)
 *   overflow  device int32 (B): 1 when a parent label exceeds cap (its class is unknown; parent itself stays exact)
 *   n_spilled device int32 (1), may be NULL: the rows with more than 16 distinct a (resolved by the exact bounding-box pass)
 * stats_r (device int64 (B, cap, 8), may be NULL: the whole frame) gives the refined ROIs' bounding boxes in columns 3..6
 * as pcseg_region_reduce writes them.  Exact and deterministic; nothing goes back to the host.
 *
 * pcseg_refined_layout / pcseg_refined_table_write: the refined tables from the struct below (device pointers, the
 * pcseg_classify_regions outputs of the class-map components and of the refined ROIs, the latter run on (ws_stats, cls_r,
 * n_markers)), asynchronous on `stream`:
 *   refined    (n_rois, 11)  frame, label, parent, parent_px, n_overlap, class, kind, cells, area, centroid_row,
 *                            centroid_col; one row per row of `rois`, in its order
 *   resolution (n_cells, 5)  frame, label, children, resolved, cells_integrated; one row per row of `cells`, in its order.
 *                            children = #refined ROIs of kind >= 1 whose parent is the row; resolved = cluster with >= 2
 *                            children; cells_integrated = 1 (cell), sum of the children's cells (resolved), the row's
 *                            own cells (residual cluster), -1 when a term it uses is -1
 *   frames     (B, 2 + 5 n_slots)  frame, refined nan flag, then per slot: refined cells, refined clusters, resolved,
 *                            residual, count_integrated (sum of cells_integrated over the slot's rows, -1 if one is -1)
 *   xy / slot / id / frame_offsets (all or none): the refined rows of kind >= 1 as pcseg_point_neighbours points --
 *                            (centroid_col + 1, centroid_row + 1), slot_r, label -- and their frames' offsets (B + 1).
 * pcseg_refined_layout's totals (device int64[2]) = {points, frames with parent_overflow set}; `table_workspace` is the
 * one pcseg_table_layout / pcseg_table_write used (the row offsets of `rois` and `cells`). */
typedef struct pcseg_refined_inputs {
    int32_t B, cap, n_slots;
    const int64_t *frame_ids;                                                                    /* (B) */
    const int32_t *counts; const uint8_t *kind; const uint8_t *slot_of; const int32_t *cells;   /* class-map components */
    const int32_t *n_markers; const int64_t *ws_stats;                                           /* refined ROIs */
    const int32_t *parent; const int32_t *parent_px; const int32_t *n_overlap; const uint8_t *cls_r;  /* pcseg_label_parent */
    const uint8_t *kind_r; const uint8_t *slot_r; const int32_t *cells_r; const int64_t *type_stats_r;
    const int32_t *nan_flag_r;                                                 /* pcseg_classify_regions on the refined ROIs */
    const int32_t *parent_overflow;                                            /* (B) overflow of pcseg_label_parent, may be NULL */
} pcseg_refined_inputs;
size_t pcseg_label_parent_workspace_bytes(int B, int H, int W, int cap);
int pcseg_label_parent(const int32_t *labels_a, const int32_t *labels_r, const int32_t *counts_r, const int64_t *stats_r,
                       const uint8_t *cls_a, int32_t *parent, int32_t *parent_px, int32_t *n_overlap, uint8_t *cls_r,
                       int32_t *overflow, int32_t *n_spilled, int B, int H, int W, int cap, void *workspace,
                       size_t workspace_bytes, pcseg_stream_t stream);
size_t pcseg_refined_workspace_bytes(int B, int cap);
int pcseg_refined_layout(const pcseg_refined_inputs *in, int64_t *totals, void *workspace, size_t workspace_bytes,
                         pcseg_stream_t stream);
int pcseg_refined_table_write(const pcseg_refined_inputs *in, const void *table_workspace, size_t table_workspace_bytes,
                              double *refined, double *resolution, double *frames, double *xy, int32_t *slot, int32_t *id,
                              int64_t *frame_offsets, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- distance of every cell to the particle surface and colonisation profiles, batched
 * (HCN_nanosims_rois_activity_distance_5iso_YG.m:271-309, data_dist_nearest_bound.csv).
 * Surface S of the mask M = ((value_bits >> in) & 1): the pixels of M with a 4-neighbour outside M, pixels outside the
 * image counting as outside M (the point set of bwboundaries).  Any width and alignment.
 * pcseg_surface_points (no host read-back):
 *   bits    device uint32 (B, H, ceil(W / 32)): S as bit words, bit j of word w of a row = column 32 w + j, 0 beyond W
 *   counts  device int64 (B): #S per frame;  offsets device int64 (B + 1): their exclusive prefix, offsets[B] = total
 *   area    device int64 (B), may be NULL: #M per frame
 *   points  device int32 (points_cap, 2), may be NULL with points_cap = 0: (row, col) of S in raster order, frame by frame
 *           (count -> scan -> write: the order never depends on scheduling); points beyond points_cap are not written
 * pcseg_surface_distances: queries in frame-contiguous order -- rc device float64 (n, 2) = (row, col), 0-based,
 * frame_offsets device int64 (B + 1), n < 2^31 -- against the bits.  d2(q, s) = fl(fl(dr*dr) + fl(dc*dc)) (no FMA),
 *   dist    device float64 (n): sqrt(min d2) / scale;  nearest device int32 (n, 2): the surface point of minimal d2, the
 *           smallest raster index row * W + col among equal d2;  NaN, -1, -1 for a frame without surface, and for a query
 *           with a NaN coordinate or one beyond +-2^24
 *   inside  device uint8 (n), may be NULL: mask != 0 at pixel (floor(row + 0.5), floor(col + 0.5)) (mask: device uint8
 *           (B, H, W), may be NULL: 0), 0 outside the image and for a query without distance
 *   counts  as pcseg_surface_points wrote them, may be NULL (a frame without surface is then searched in full)
 *   hist    device int64 (B, 2, K, m + 2), with edges (HOST float64, n_edges = m + 1 in 2..1025, edges[0] == 0, strictly
 *           increasing; needs slot device int32 (n), mask and K <= 4): per frame, side (0 outside, 1 inside) and slot
 *           [n, bin_0 .. bin_m-1, over] over the queries that have a distance and a slot in 0..K-1, bin k = edges[k] <= d <
 *           edges[k + 1], over = d >= edges[m], n = bins + over.  edges == NULL, n_edges == 0, hist == NULL: none
 *   rows_visited device int32 (n), may be NULL: image rows whose words the search read (a measurement aid)
 * The search is exact and pruned: one wave per query, rows outward from the query's row, a row skipped once
 * fl(dr*dr) > best d2 (strictly), words walked left / right of the query column until a bit or the bound.
 * Workspace of both: pcseg_surface_workspace_bytes(B, H, W).
 * pcseg_surface_thresholds (HOST only, touches no device): out[k] = the smallest integer n >= 0 with
 * sqrt((double)n) / scale >= edges[k] (INT64_MAX if none up to 2^53), so that for an integer squared distance D2
 * edges[k] <= sqrt(D2) / scale  <=>  D2 >= out[k].
 * pcseg_surface_shells: D2(p) = exact squared distance of every pixel to S (pcseg_edt_sq_u8 on the image that is 0 on S),
 * shells device int64 (B, 2, m + 2) = per frame and side (mask at the pixel) [n_px, bin_0 .. bin_m-1, over] with the bins
 * of pcseg_surface_thresholds; every pixel of a frame without surface is `over`.  B <= 65535.
 * Workspace: pcseg_surface_shells_workspace_bytes(B, H, W).
 * pcseg_surface_pack_cells: the queries of the dense `cells` table pcseg_table_write has just filled -- rc =
 * (centroid_row, centroid_col) as the table prints them, slot = class_slot[class] (a HOST array, 255 -> -1), id = label --
 * and the frames' offsets; `table_workspace`: see pcseg_table_layout.  pcseg_surface_pack_refined: rc of the
 * refined points pcseg_refined_table_write packed (id = refined label, frame_offsets) = their centroids as the `refined`
 * table prints them, from ws_stats device int64 (B, cap, 8). */
size_t pcseg_surface_workspace_bytes(int B, int H, int W);
int pcseg_surface_points(const uint8_t *in, uint64_t value_bits, uint32_t *bits, int64_t *counts, int64_t *offsets, int64_t *area,
                         int32_t *points, int64_t points_cap, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_surface_distances(const double *rc, const int32_t *slot, const int64_t *frame_offsets, int64_t n_points,
                            const uint32_t *bits, const int64_t *counts, const uint8_t *mask, int B, int H, int W, double scale,
                            const double *edges, int n_edges, int K, double *dist, int32_t *nearest, uint8_t *inside, int64_t *hist,
                            int32_t *rows_visited, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_surface_thresholds(const double *edges, int n_edges, double scale, int64_t *out);
size_t pcseg_surface_shells_workspace_bytes(int B, int H, int W);
int pcseg_surface_shells(const uint32_t *bits, const int64_t *counts, const uint8_t *mask, int B, int H, int W, double scale,
                         const double *edges, int n_edges, int64_t *shells, void *workspace, size_t workspace_bytes,
                         pcseg_stream_t stream);
int pcseg_surface_pack_cells(const double *cells, int ncol, const uint8_t *class_slot, int B, const void *table_workspace,
                             size_t table_workspace_bytes, double *rc, int32_t *slot, int32_t *id, int64_t *frame_offsets,
                             pcseg_stream_t stream);
int pcseg_surface_pack_refined(const int64_t *ws_stats, int cap, const int32_t *id, const int64_t *frame_offsets, int64_t n_points,
                               int B, double *rc, pcseg_stream_t stream);

/* ---- per-ROI shape: what RegionProperties offers beyond the fields the reference reads itself (every public function
 * hands such objects back: tiff_analysis.py:742-883, 1018; HCN_nanosims_rois_activity_distance_5iso_YG.m:104, 173 asks for
 * regionprops(red, 'all')) -- second moments, axes, eccentricity, orientation, perimeter; scikit-image 0.18.3 conventions.
 * pcseg_region_shape: labels device int32 (B, H, W), any width and alignment (the class-map components or the refined
 * ROIs); counts device int32 (B).  shape_out device int64 (B, cap, 8), rows l = 1 .. min(counts[b], cap) (row l - 1; the
 * others stay untouched), all exact integers over the label's pixels, absolute image coordinates:
 *   0, 1, 2  sum r^2, sum r c, sum c^2
 *   3, 4, 5  n_1, n_sqrt2, n_mid: border pixels by the weight class of skimage.measure.perimeter(region.image, 4)
 *   6        n_border: all border pixels;  7: 0
 * border pixel: a pixel of the label with a 4-neighbour of another label (outside the image counts as another label);
 * its value v = 1 + 2 #(4-neighbours that are border pixels OF THE SAME LABEL) + 10 #(such diagonal neighbours);
 * v in {5,7,15,17,25,27} -> n_1, {21,33} -> n_sqrt2, {13,23} -> n_mid.  Labels above min(counts[b], cap) are skipped;
 * overflow[b] (device int32 (B), may be NULL) is cleared and then set when a label exceeds cap.  B <= 65535.
 * pcseg_shape_properties: stats device int64 (B, cap, 8) (pcseg_region_col rows of the same labels), shape as above; out
 * device float64 (B, cap, 12), rows below min(counts[b], cap); NaN for a label without pixel.  With A the area, P = (A sum
 * r^2 - (sum r)^2) / A^2, Q the same in c, R = (A sum r c - sum r sum c) / A^2 (numerators exact in 128-bit integers):
 *   0, 1, 2  inertia tensor [[a, b], [b, c]] = [[Q, -R], [-R, P]]
 *   3, 4     l1, l2 = ((P + Q) +- sqrt((P - Q)^2 + 4 R^2)) / 2, l2 clipped at 0
 *   5, 6     major, minor axis length = 4 sqrt(l1), 4 sqrt(l2);  7: eccentricity = l1 == 0 ? 0 : sqrt(1 - l2 / l1)
 *   8        orientation = a - c == 0 ? (b < 0 ? -pi/4 : pi/4) : atan2(-2 b, c - a) / 2
 *   9        equivalent diameter = sqrt(4 A / pi);  10: extent = A / bounding-box area
 *   11       perimeter = n_1 + n_sqrt2 sqrt 2 + n_mid (1 + sqrt 2) / 2
 * in pixels; every operation rounded on its own (no FMA). */
size_t pcseg_region_shape_workspace_bytes(int B, int H, int W);
int pcseg_region_shape(const int32_t *labels, const int32_t *counts, int64_t *shape_out, int32_t *overflow, int B, int H, int W,
                       int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_shape_properties(const int64_t *stats, const int64_t *shape, const int32_t *counts, double *out, int B, int cap,
                           pcseg_stream_t stream);

/* ---- per-ROI convexity: is this blob one cell or a clump (tiff_analysis.py:776-781 counts a cluster's cells as area //
 * mean cell area; refine_boundaries.py:5-7 expects clusters the watershed does not split) -- convex area, solidity, Feret
 * diameter, Euler number; scikit-image 0.18.3 conventions, every value exact.
 * pcseg_region_hull: labels device int32 (B, H, W), any width and alignment; counts device int32 (B); stats device int64
 * (B, cap, 8), the pcseg_region_col rows of the same labels (area and bounding box are read: a ROI is looked for inside
 * the box its row names, held to the frame, and nowhere else -- a row that does not belong to the image gives a wrong
 * answer, never an access outside it).  hull_out device int64 (B, cap, 4), rows l = 1 .. min(counts[b], cap) (row l - 1; the
 * others stay untouched; zeros for a label without pixel).  In doubled coordinates a pixel (r, c) owns the four points
 * (2r +- 1, 2c), (2r, 2c +- 1) (convex_hull_image(offset_coordinates=True)):
 *   0  convex_area: the pixel centres (2r, 2c) in the CLOSED convex hull of the points of the label's pixels (a centre on a
 *      hull edge counts; pixels of other labels count); these pixels are the convex image
 *   1  feret_sq4: the largest squared distance between points of the pixels OF THE CONVEX IMAGE (which reaches further than
 *      the hull of the label's own points); feret_diameter_max = sqrt(feret_sq4 / 4)
 *   2  euler number, 8-connectivity: (Q1 - Q3 - 2 QD) / 4 over all 2 x 2 windows of the zero-padded indicator of the label
 *      (one, three, exactly the two diagonal pixels set; windows over the frame's edge count)
 *   3  0
 * Labels need not be connected.  overflow[b] (device int32 (B), may be NULL) = counts[b] > cap: the image is not searched
 * for labels, a label above min(counts[b], cap) is never looked at.  B <= 65535.  Asynchronous, nothing is allocated.
 * pcseg_hull_properties: out device float64 (B, cap, 4), rows below min(counts[b], cap); NaN for a label without pixel:
 *   0  convex_area;  1  solidity = area / convex_area (one division);  2  feret_diameter_max = sqrt(feret_sq4 / 4.0), in
 *   pixels;  3  euler_number */
size_t pcseg_region_hull_workspace_bytes(int B, int H, int W, int cap);
int pcseg_region_hull(const int32_t *labels, const int32_t *counts, const int64_t *stats, int64_t *hull_out, int32_t *overflow, int B,
                      int H, int W, int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_hull_properties(const int64_t *stats, const int64_t *hull, const int32_t *counts, double *out, int B, int cap,
                          pcseg_stream_t stream);

/* ---- nearest-label transform, territories and adjacency (csrc/voronoi.hip): how much of the frame a ROI has to itself and
 * which ROIs are its neighbours.  All values are exact integers.
 * A SITE is a pixel whose label l lies in 1 .. cap and, with sel (device uint8 (B, cap), may be NULL), has sel[b, l - 1] != 0; a
 * label outside 1 .. cap is never a site and never an index.
 * pcseg_nearest_label_i32: labels device int32 (B, H, W), any width and alignment.  For every pixel p
 *   d2   (device int32 (B, H, W)) = min over the frame's sites q of (pr - qr)^2 + (pc - qc)^2 (0 on a site),
 *   near (device int32 (B, H, W)) = the SMALLEST label among the sites at that minimum (a site: its own label),
 *   site (device int32 (B, H, W), may be NULL) = the raster index of the nearest site of label near, the smallest index among equals
 *   (scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True) with the ties decided).
 * A frame without site: d2 = -1, near = 0, site = -1 everywhere (scipy's virtual pixel is not reproduced).  Shapes as
 * pcseg_edt_sq_u8 (check_shape), B <= 65535.
 * A pixel BELONGS to label near iff d2 >= 0 and d2 <= R2 (R2 < 0: unbounded).
 * pcseg_territory_labels: out[i] = near[i] where the pixel belongs to it, else 0, over n pixels (skimage.segmentation.expand_labels).
 * pcseg_territory_reduce: mask device uint8 (B, H, W), may be NULL; out device int64 (B, cap, 4), row l - 1 over the pixels that
 * belong to l (near outside 1 .. cap is ignored): 0 territory_px, 1 territory_on_px (those with mask != 0), 2 reach2_max (the
 * largest d2 among them), 3 clipped (1 if one of them lies on the frame's outer row or column).  Every row is written (zeros for
 * a label that owns nothing).  cap < 2^30.
 * pcseg_territory_pairs: a LINK is an unordered pair of 4-neighbour pixels that both belong to a label, to different ones; each
 * is counted once (right and down neighbour).  Per frame an open-addressing table of pair_cap slots keyed by (a, b), a < b,
 * holds border (links between a and b) and contact (those with d2 = 0 at both ends: the labels touch in the label image).
 * overflow[b] (device int32 (B)) = 1 where a frame has more pairs than pair_cap: links are dropped then, nothing is written
 * outside the table and no thread waits.  offsets (device int64 (B + 1)): first row of every frame among the compacted rows;
 * totals (device int64 (2)) = {rows, frames with overflow}: the one host read between the two calls.
 * pcseg_territory_pairs_write (same workspace, untouched in between): key (device int64 (rows)) = a << 32 | b, frame (device
 * int32 (rows)) = b's position in the batch, counts (device int32 (rows, 2)) = border, contact; rows of a frame in table order
 * (sort by key for (a, b) order).  With degree (device int32 (B, cap, 2 n_types), ZEROED by the caller) and slot_of (device
 * uint8 (B, cap), a value >= n_types: no type): degree[b, a - 1, slot_of[b]] += 1 for every pair (both directions), and at
 * n_types + slot for every pair with contact > 0.  Asynchronous, nothing is allocated. */
size_t pcseg_nearest_label_workspace_bytes(int B, int H, int W);
int pcseg_nearest_label_i32(const int32_t *labels, const uint8_t *sel, int cap, int32_t *d2, int32_t *near, int32_t *site, int B,
                            int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_territory_labels(const int32_t *near, const int32_t *d2, int64_t R2, int32_t *out, int64_t n, pcseg_stream_t stream);
int pcseg_territory_reduce(const int32_t *near, const int32_t *d2, const uint8_t *mask, int64_t R2, int cap, int64_t *out, int B,
                           int H, int W, pcseg_stream_t stream);
size_t pcseg_territory_pairs_workspace_bytes(int B, int pair_cap);
int pcseg_territory_pairs(const int32_t *near, const int32_t *d2, int64_t R2, int pair_cap, int32_t *overflow, int64_t *offsets,
                          int64_t *totals, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_territory_pairs_write(int pair_cap, const int64_t *offsets, const uint8_t *slot_of, int cap, int n_types, int64_t *key,
                                int32_t *frame, int32_t *counts, int32_t *degree, int B, const void *workspace,
                                size_t workspace_bytes, pcseg_stream_t stream);

/* ---- agreement of two label images (csrc/agreement.hip): the contingency table of a truth image T and a test image S, and
 * per-label / per-frame agreement figures from it.  All values but the IoUs are exact integers.
 * T, S device int32 (B, H, W), any width and alignment.  A value outside 0 .. cap_t (S: 0 .. cap_s) is read as 0; negative
 * values silently (as pcseg_thin_labels), a value above its cap raises bit 2 (value 2) of the frame's overflow word.
 * n(t, s) = pixels with T = t and S = s; A_t = sum over s >= 0 of n(t, s), B_s = sum over t >= 0 of n(t, s).
 * pcseg_label_contingency: per frame an open-addressing table of pair_cap slots keyed by t << 32 | s that holds every pair with
 * n > 0 except (0, 0) -- pairs with the background included, so the marginals are row sums and n(0, 0) = H W - sum.  overflow
 * (device int32 (B)): bit 1 (value 1) where the frame has more pairs than pair_cap -- pairs are dropped then, nothing is written
 * outside the table and no thread waits --, bit 2 as above.  offsets (device int64 (B + 1)): first row of every frame among
 * the compacted rows; totals (device int64 (2)) = {rows, frames with overflow bit 1}: the one host read between the two calls.
 * One read of each image; cap_t, cap_s, pair_cap >= 1, shapes as pcseg_edt_sq_u8 (check_shape), B <= 65535.
 * pcseg_contingency_write (same workspace, untouched in between): key (device int64 (rows)) = t << 32 | s, frame (device int32
 * (rows)) = the frame's position in the batch, n (device int64 (rows)); rows of a frame in table order (not deterministic; sort
 * by key for (t, s) order).
 * pcseg_agreement_match: key, n device int64 (rows) SORTED by (frame, key), offsets as above, rows = offsets[B]; rows with a label
 * above its cap are ignored.  thresholds: HOST float64 (n_thr), n_thr <= 8, 0.5 <= tau <= 1.  Written (every element):
 *   area_t device int64 (B, cap_t) = A_t, area_s device int64 (B, cap_s) = B_s
 *   for a pair t >= 1, s >= 1 with n > 0: U = A_t + B_s - n, iou = (double)n / (double)U (one division)
 *   best_t device int32 (B, cap_t, 3): 0 the best partner of t -- the s >= 1 with the largest n / U, compared exactly (n U' against
 *   n' U in unsigned 64 bits), the smallest s among equals, 0 if none --, 1 its n, 2 the number of s >= 1 with n(t, s) > 0;
 *   iou_t device float64 (B, cap_t): the partner's iou, NaN without one;  best_s (B, cap_s, 3), iou_s (B, cap_s): the mirror image
 *   match_t device uint8 (B, cap_t), match_s (B, cap_s): bit k set where the label's best partner has 2 n > U and iou >= tau_k
 *   (2 n > U means n > A_t / 2 and n > B_s / 2: at most one such partner per label, on both sides, and it is the best one -- no
 *   assignment problem, no dependence on order)
 *   frame_ints device int64 (B, 6 + n_thr): 0 n_truth (t >= 1 with A_t > 0), 1 n_rois (s >= 1 with B_s > 0), 2 N1 = sum over
 *   t >= 1 of A_t, 3 S_pp = sum over t >= 1, s >= 0 of n^2, 4 S_a = sum over t >= 1 of A_t^2, 5 S_b = sum over s >= 0 of (sum over
 *   t >= 1 of n(t, s))^2, 6 + k TP_k = truth labels matched at tau_k.
 * Rows of labels without pixel stay zero / NaN.  Asynchronous, nothing is allocated. */
size_t pcseg_contingency_workspace_bytes(int B, int pair_cap);
int pcseg_label_contingency(const int32_t *labels_t, const int32_t *labels_s, int cap_t, int cap_s, int pair_cap, int32_t *overflow,
                            int64_t *offsets, int64_t *totals, int B, int H, int W, void *workspace, size_t workspace_bytes,
                            pcseg_stream_t stream);
int pcseg_contingency_write(int pair_cap, const int64_t *offsets, int64_t *key, int32_t *frame, int64_t *n, int B,
                            const void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_agreement_match(const int64_t *key, const int64_t *n, const int64_t *offsets, int64_t rows, int cap_t, int cap_s,
                          const double *thresholds, int n_thr, int64_t *area_t, int64_t *area_s, int32_t *best_t, double *iou_t,
                          int32_t *best_s, double *iou_s, uint8_t *match_t, uint8_t *match_s, int64_t *frame_ints, int B,
                          pcseg_stream_t stream);

/* ---- borders between touching regions and the merge of over-segmented regions by border strength (csrc/borders.hip): what
 * skimage.graph.rag_boundary + cut_threshold do after a watershed, and the classical merge of basins over a low pass.
 * Inputs.  L device int32 (B, H, W), any width and alignment.  V device float32, frame b at V + b * value_stride (elements,
 *   >= H * W; rows contiguous): a (B, H, W) image or one plane of a (B, C, H, W) stack.
 * Labels.  A label outside 0 .. cap is read as 0; a label above cap raises bit 2 (value 2) of the frame's overflow word, as in
 *   pcseg_label_contingency.
 * Links.  A LINK is an unordered pair of pixels p, q that are 4-neighbours (conn = 4) or 8-neighbours (conn = 8) with labels
 *   a = L[p] >= 1, b = L[q] >= 1, a != b.  Every link is counted exactly once.  A link's value is max(V[p], V[q]): the ridge
 *   between the two regions, whichever side of the cut it fell on.
 * Values.  V is read as a probability: a NaN is read as 0, a value outside [0, 1] is clamped; either raises bit 4 (value 4).
 * Per pair (a < b) with at least one link:
 *   links   the number of links
 *   saddle  the smallest link value, the exact float32 (non-negative floats order like their bit patterns)
 *   sum     the sum over the links of rint(value * 2^32), an unsigned 64-bit integer.  A float32 in [2^-9, 1] is a multiple of
 *           2^-32: for such values (the k/100 maps included) sum is the exact sum; below 2^-9 a value is off by at most 2^-33.
 *           sum does not depend on any order of addition: results are reproducible bit for bit from run to run.
 *   mean    = sum / (links * 2^32), left to the caller (in float64: the correctly rounded quotient when sum < 2^53)
 * Merge rule.  below is a float64 in [0, 1].  by = PCSEG_BORDER_BY_MEAN: the pair is JOINED iff sum < rint(below * 2^32) * links, in
 *   unsigned 64-bit integers, strictly.  by = PCSEG_BORDER_BY_SADDLE: JOINED iff saddle < (float)below.  The GROUPS are the connected
 *   components of the joined pairs over the labels 1 .. count, count = counts[b] held to 0 .. cap (counts NULL: cap).  One
 *   pass: weights are not updated after a union (cut_threshold, not merge_hierarchical); links and sum are additive, so a
 *   second call on the merged image is the exact second round.
 * Numbering.  Groups are numbered 1 .. m in the order of their smallest member.  map device int32 (B, cap + 1), old label to new
 *   label: map[b, 0] = 0, map[b, l] = 0 for l > count; n_merged[b] = m; the merged image is map[b, L].  A region that touches
 *   nothing keeps a group of its own, relative order is preserved, and with no joined pair the map is the identity on 1 .. count.
 * pcseg_label_borders: per frame an open-addressing table of pair_cap slots (24 bytes each) keyed by a << 32 | b.  overflow (device
 *   int32 (B)): bit 1 (value 1) where the frame has more pairs than pair_cap -- pairs are dropped then, nothing is written outside
 *   the table and no thread waits --, bits 2 and 4 as above.  offsets (device int64 (B + 1)), totals (device int64 (2)) = {rows,
 *   frames with bit 1}: the one host read between the two calls, as for pcseg_territory_pairs.  L and V are read once each.
 *   cap, pair_cap >= 1, cap < 2^30, shapes as pcseg_edt_sq_u8 (check_shape), B <= 65535.
 * pcseg_label_borders_write (same workspace, untouched in between): key (device int64 (rows)) = a << 32 | b, frame (device int32
 *   (rows)), links (device int32 (rows)), sum (device int64 (rows)), saddle (device float32 (rows)); rows of a frame in table order.
 * pcseg_border_merge (same workspace, straight after pcseg_label_borders: nothing is read back): flags is that call's overflow
 *   array.  A frame with bit 1 keeps map as the identity on 1 .. count and n_merged = count: its merge is no result.  Bit 8 (value
 *   8) is raised where a walk of the grouping met a parent entry outside its fence (a workspace overwritten while the call ran):
 *   never a fault or an endless loop, and no result either.  Parents live in LDS where cap + 1 <= lds_labels, else in the workspace.
 * pcseg_relabel_map: out[b, p] = map[b, L[b, p]], 0 where L is outside 0 .. cap; out device int32 (B, H, W), may not alias L.
 * pcseg_border_block: HOST int32 (3) = rows and columns of a block of the fill kernel, lds_labels.
 * Asynchronous, nothing is allocated; fill -> merge -> relabel can be captured in a graph. */
#define PCSEG_BORDER_BY_MEAN 0
#define PCSEG_BORDER_BY_SADDLE 1
int pcseg_border_block(int32_t *rows_cols_lds);
size_t pcseg_label_borders_workspace_bytes(int B, int pair_cap, int cap);
int pcseg_label_borders(const int32_t *labels, const float *values, int64_t value_stride, int cap, int conn, int pair_cap,
                        int32_t *overflow, int64_t *offsets, int64_t *totals, int B, int H, int W, void *workspace,
                        size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_label_borders_write(int pair_cap, int cap, const int64_t *offsets, int64_t *key, int32_t *frame, int32_t *links, int64_t *sum,
                              float *saddle, int B, const void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_border_merge(int pair_cap, int cap, const int32_t *counts, double below, int by, int32_t *flags, int32_t *map,
                       int32_t *n_merged, int B, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_relabel_map(const int32_t *labels, const int32_t *map, int cap, int32_t *out, int B, int H, int W, pcseg_stream_t stream);

/* ---- per-ROI skeletons (csrc/skeleton.hip): exact Guo-Hall thinning, every label on its own -- the union over l of
 * skimage.morphology.thin(labels == l) of scikit-image 0.18.3 -- and per ROI the length and the ends / junctions of its
 * skeleton.  Integers only.
 * pcseg_thin_labels: labels device int32 (B, H, W), any width and alignment; values <= 0 are background, labels may touch and
 * need not be consecutive.  A neighbour counts only if it is alive and carries the centre's label; outside the frame is
 * background.  With N = sum 2^i b[i], b[0..7] = E, NE, N, NW, W, SW, S, SE (indices mod 8):
 *   G1   exactly one i in {0, 2, 4, 6} has !b[i] && (b[i + 1] || b[i + 2])
 *   G2   min(n1, n2) in {2, 3}, n1 = #{k in {1, 3, 5, 7}: b[k] || b[k - 1]}, n2 = #{k: b[k] || b[k + 1]}
 *   G3   !((b[1] || b[2] || !b[7]) && b[0])        G3'  !((b[5] || b[6] || !b[3]) && b[4])
 * the first sub-iteration deletes the alive pixels with G1 && G2 && G3, the second, on its result, those with G1 && G2 && G3';
 * a full iteration is the pair.  It stops after the first full iteration that deletes nothing or after max_iter full
 * iterations (max_iter < 0: no limit; 0: none).  peel device uint16 (B, H, W): 0 background, 65535 the pixel survives (the
 * skeleton), otherwise the 1-based sub-iteration that deleted it (odd: first table; full iteration (s + 1) / 2).  iters
 * device int32 (B): the full iterations of the frame that deleted a pixel.  The call WAITS for the stream (two counters per
 * launch decide whether another one follows) and cannot be captured into a graph; H + W full iterations without an end
 * return PCSEG_ERR_CONVERGENCE ("thinning did not converge").  B <= 65535.
 * pcseg_region_skeleton: labels and peel as above, counts device int32 (B); table device int64 (B, cap, 6), rows l = 1 ..
 * min(counts[b], cap) (row l - 1; the others stay untouched, labels above are ignored; zeros for a label without pixel).
 * Links join skeleton pixels (peel == 65535) of EQUAL label: two 4-adjacent ones form an orthogonal link, two diagonal ones
 * a diagonal link only if neither of the two pixels 4-adjacent to both is a skeleton pixel of that label (an L-corner is two
 * links, not three).  The degree of a pixel is its number of links.
 *   0  skel_px   1  n_orth   2  n_diag   3  n_end (degree 1)   4  n_junction (degree >= 3)
 *   5  passes: (max s + 1) / 2 over the label's deleted pixels, 0 if none
 * Asynchronous, nothing is allocated.
 * pcseg_skeleton_properties: stats device int64 (B, cap, 8) (pcseg_region_col rows of the same labels), out device float64
 * (B, cap, 2), rows below min(counts[b], cap); NaN for a label without pixel:
 *   0  length_px = n_orth + n_diag * sqrt(2.0) (one rounded product, one rounded sum, no FMA)
 *   1  width_px = area / length_px (one division; inf for a one-pixel skeleton) */
size_t pcseg_thin_labels_workspace_bytes(int B, int H, int W);
int pcseg_thin_labels(const int32_t *labels, uint16_t *peel, int32_t *iters, int B, int H, int W, int max_iter, void *workspace,
                      size_t workspace_bytes, pcseg_stream_t stream);
size_t pcseg_region_skeleton_workspace_bytes(int B, int H, int W, int cap);
int pcseg_region_skeleton(const int32_t *labels, const uint16_t *peel, const int32_t *counts, int64_t *table, int B, int H, int W,
                          int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_skeleton_properties(const int64_t *stats, const int64_t *table, const int32_t *counts, double *out, int B, int cap,
                              pcseg_stream_t stream);

/* ---- grayscale morphological reconstruction and h-maxima / h-minima (csrc/reconstruct.hip):
 * skimage.morphology.reconstruction, h_maxima and h_minima of scikit-image 0.18.3 for 2-D frames, exact.
 * pcseg_reconstruct_{i32,f64}: seed, mask, out device (B, H, W), out distinct from both inputs, NaN-free; conn 8 (the 3 x 3
 * footprint) or 4; method PCSEG_RECONSTRUCT_DILATION: out = the largest R with seed <= R <= mask in which every value above
 * the seed is carried along a connected path of pixels whose mask is at least that value, i.e. the fixed point of
 * R <- max(R, min(mask, max of R over the neighbourhood)) from R = min(seed, mask), nothing outside the frame;
 * PCSEG_RECONSTRUCT_EROSION: its mirror image (min and max change places).  -0.0 is read as +0.0.  flags device int32 (B),
 * written by the call: PCSEG_RECONSTRUCT_SEED_BEYOND_MASK where a seed pixel lies above (erosion: below) its mask pixel --
 * scikit-image raises there, the call clamps the seed to the mask --, PCSEG_RECONSTRUCT_NOT_CONVERGED where the frame's tail
 * loop reached max_rounds rounds (<= 0: (tiles of a frame + 64) * 64, the watershed's cap; H * W cannot be reached by any
 * image): out is then NO fixed point and must not be used.  The launch sequence is fixed -- nothing is read back, nothing
 * allocated -- so the call can be captured into a graph.  B <= 65535.  The first 32 int32 of the workspace are counters of
 * the last call: [r], 1 <= r < 6, the tiles listed for grid round r (round 0 visits every tile), [16] the tiles those
 * rounds visited, [17] the tiles the tail kernel visited, [18] the most tail rounds of a frame.
 * h_maxima(image, h) = (image - reconstruction by dilation of shift(image) under image) >= h, all zero in a frame with
 * h > max - min (the test is per frame); h_minima its mirror.  sign -1: h_maxima, +1: h_minima; h > 0.
 * pcseg_hmax_range_*: range device uint64 (B, 2), opaque (order keys of each frame's minimum and maximum).
 * pcseg_hmax_shift_i32: seed = image -+ h clipped to int32; _f64: (image - h) - (2e-15 |image|) or (image + h) + (2e-15
 * |image|), one rounding per operation in that order; _edt: from the squared distance d2, dist = sqrt((double)d2) and
 * seed = the float64 h_maxima shift of dist.
 * pcseg_hmax_mark_*: out uint8 = residue >= h, residue = image - rec (sign -1) or rec - image (sign +1), zero where h
 * exceeds the frame's range; range_of_d2 = 1: range holds pcseg_hmax_range_i32 of d2 and the image is its square root
 * (range = sqrt(max d2) - sqrt(min d2)). */
#define PCSEG_RECONSTRUCT_DILATION 0
#define PCSEG_RECONSTRUCT_EROSION 1
#define PCSEG_RECONSTRUCT_SEED_BEYOND_MASK 1
#define PCSEG_RECONSTRUCT_NOT_CONVERGED 2
size_t pcseg_reconstruct_workspace_bytes(int B, int H, int W);
int pcseg_reconstruct_i32(const int32_t *seed, const int32_t *mask, int32_t *out, int32_t *flags, int B, int H, int W, int conn,
                          int method, int max_rounds, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_reconstruct_f64(const double *seed, const double *mask, double *out, int32_t *flags, int B, int H, int W, int conn,
                          int method, int max_rounds, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);
int pcseg_hmax_range_i32(const int32_t *img, uint64_t *range, int B, int H, int W, pcseg_stream_t stream);
int pcseg_hmax_range_f64(const double *img, uint64_t *range, int B, int H, int W, pcseg_stream_t stream);
int pcseg_hmax_shift_i32(const int32_t *img, int64_t h, int sign, int32_t *seed, int B, int H, int W, pcseg_stream_t stream);
int pcseg_hmax_shift_f64(const double *img, double h, int sign, double *seed, int B, int H, int W, pcseg_stream_t stream);
int pcseg_hmax_shift_edt(const int32_t *d2, double h, double *dist, double *seed, int B, int H, int W, pcseg_stream_t stream);
int pcseg_hmax_mark_i32(const int32_t *img, const int32_t *rec, int64_t h, int sign, const uint64_t *range, uint8_t *out, int B,
                        int H, int W, pcseg_stream_t stream);
int pcseg_hmax_mark_f64(const double *img, const double *rec, double h, int sign, const uint64_t *range, int range_of_d2,
                        uint8_t *out, int B, int H, int W, pcseg_stream_t stream);

/* ---- X1 (north_star extension; refine_boundaries.py:22 imports skimage.filters and never calls it): the library
 * SURVEY.md 8a names is the oracle -- skimage.filters.threshold_otsu(float32 image, nbins=256), pinned by
 * tests/golden/extensions.npz.  pcseg_otsu_f32: threshold[b] (device float64 (B,), the value is the float32 bin
 * centre the library returns; a constant frame returns its value), plus the histogram it was taken from: hist device
 * int64 (B,256) over each frame's own [min, max] with numpy.histogram's float32 binning, lohi device float32 (B,2).
 * Entirely on the device, asynchronous on `stream`.  pcseg_otsu_hist_f32: the histogram alone. */
int pcseg_otsu_f32(const float *img, double *threshold, int64_t *hist, float *lohi, int B, int H, int W,
                   pcseg_stream_t stream);
int pcseg_otsu_hist_f32(const float *img, int64_t *hist, float *lohi, int B, int H, int W,
                        pcseg_stream_t stream);

/* ---- X2 (north_star extension, no reference call site): 3x3 square binary
 * erosion (erode != 0, outside = True) or dilation (outside = False). */
int pcseg_morph3x3(const uint8_t *mask, uint8_t *out, int erode, int B, int H, int W, pcseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCSEG_H */
