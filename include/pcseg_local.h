/*
 * pcseg_local.h -- local neighbourhoods: per-query ring counts of set pixels and per-point ring counts of other points
 * (csrc/local_counts.hip), compiled into the same libpcseg.so as pcseg.h and pcseg_spatial.h: same conventions (device
 * pointers to contiguous batch-major arrays, caller-owned outputs of which every element is written, a caller-provided
 * workspace sized by the matching query whose prior contents never matter, work enqueued on `stream` without a host wait,
 * PCSEG_OK or a negative pcseg_status with the message in pcseg_last_error()).  All values are exact integers.
 */
#ifndef PCSEG_LOCAL_H
#define PCSEG_LOCAL_H

#include "pcseg_spatial.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- set pixels in distance rings around query pixels.
 * planes  device uint8 (B, H, W), any width and alignment: bit c of a pixel is set when the pixel belongs to set c, c < C,
 *         1 <= C <= 8; higher bits are ignored
 * queries device int32 (n, 2) = (row, col), in frame-contiguous order; frame_offsets device int64 (B + 1), from 0 to n
 * edges   HOST float64, n_edges = m + 1 in 2..1025, edges[0] == 0, strictly increasing, in units of `scale` pixels per unit
 *         (the rules of pcseg_window_pairs)
 * thr     = pcseg_surface_thresholds(edges, n_edges, scale): a pixel q is in ring k of query p when thr[k] <= (pr - qr)^2 +
 *         (pc - qc)^2 < thr[k + 1]
 * reach   R of pcseg_window_reach, with the same limit PCSEG_WINDOW_MAX_REACH
 * A query may lie anywhere with |row|, |col| < 2^24: on the border, outside the image, farther than R from it.  Pixels
 * outside the image belong to no set: such a query simply counts fewer pixels, or none.
 *   counts device int32 (n, C, m): [i, c, k] = the pixels of set c in ring k of query i, in the query's own frame; the query
 *          pixel itself is counted, in ring 0, when it is in the set
 *   area   device int64 (B, C): [b, c] = the pixels of set c in frame b
 * planes, queries, frame_offsets and edges are NOT WRITTEN.  A ring holds fewer than (2 R + 1)^2 < 2^25 pixels: int32 cannot
 * wrap.  All arithmetic is integer: the same bits whatever the order of the adds.
 * Limits: the shapes of pcseg_window_pairs (H, W <= 32768, H W < 2^30), B <= 65535, 0 <= n < 2^31 (n == 0: only area is
 * written; queries and counts are then not read or written), R <= PCSEG_WINDOW_MAX_REACH; these, a null pointer, a scale
 * that is not positive and finite and edges that pcseg_surface_thresholds rejects are PCSEG_ERR_ARG before anything is
 * enqueued; a short workspace gives PCSEG_ERR_WORKSPACE.
 * Workspace: pcseg_disk_counts_workspace_bytes(B, C, H, W, n_edges, reach) with reach from pcseg_window_reach (0 for
 * arguments the entry refuses).  pcseg_local_rows (HOST only): the image rows one pass of a query's wave covers when
 * m == 1 (with more bins a pass covers fewer rows; frames and reaches beyond it are walked pass by pass);
 * pcseg_local_bins (HOST only): the bins of one pass (more bins are walked chunk by chunk). */
int pcseg_local_rows(void);
int pcseg_local_bins(void);
size_t pcseg_disk_counts_workspace_bytes(int B, int C, int H, int W, int n_edges, int64_t reach);
int pcseg_disk_counts(const uint8_t *planes, int B, int C, int H, int W, const int32_t *queries, const int64_t *frame_offsets,
                      int64_t n_queries, double scale, const double *edges, int n_edges, int32_t *counts, int64_t *area,
                      void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- other points in distance rings around every point.
 * xy / slot / frame_offsets / n_points / B / K / scale / edges exactly as pcseg_point_neighbours takes them (edges
 * required), K <= 4, n < 2^24.
 *   counts device int32 (n, K, m): [i, t, k] = the OTHER points j of slot t in i's frame whose distance falls in bin k.
 *          "Other" means excluded by index: a duplicate position counts in bin 0.  Bin k follows the bin rule of
 *          pcseg_point_neighbours' pair_hist to the bit (d2 = dx*dx + dy*dy, each product and the sum rounded on its own, no
 *          FMA, against the same per-edge thresholds on d2); pairs at or beyond edges[m] are not counted.  A point whose slot
 *          is outside 0..K-1 takes part in nothing, and its row is all -1.
 * So the sum of counts[i, b, k] over the points i of slot a of a frame is pair_hist[a <= b][1 + k] of that frame, twice it
 * when a == b.  A frame has fewer than 2^24 points: int32 cannot wrap.
 * Bad arguments (those pcseg_point_neighbours rejects, n_edges == 0, a null pointer) are PCSEG_ERR_ARG before anything is
 * enqueued; a short workspace gives PCSEG_ERR_WORKSPACE.  Workspace: pcseg_point_counts_workspace_bytes(n_points, B, K,
 * n_edges) (0 for arguments the entry refuses).  pcseg_local_point_tile (HOST only): the candidates one pass of a point's
 * wave compares (larger frames are walked pass by pass). */
int pcseg_local_point_tile(void);
size_t pcseg_point_counts_workspace_bytes(int64_t n_points, int B, int K, int n_edges);
int pcseg_point_counts(const double *xy, const int32_t *slot, const int64_t *frame_offsets, int64_t n_points, int B, int K,
                       double scale, const double *edges, int n_edges, int32_t *counts, void *workspace, size_t workspace_bytes,
                       pcseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PCSEG_LOCAL_H */
