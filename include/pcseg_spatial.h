/*
 * pcseg_spatial.h -- spatial statistics on top of the tables of pcseg.h, compiled into the same libpcseg.so: same
 * conventions (device pointers to contiguous batch-major arrays, caller-owned buffers, a caller-provided workspace sized
 * by the matching query whose prior contents never matter, work enqueued on `stream` without a host wait, PCSEG_OK or a
 * negative pcseg_status with the message in pcseg_last_error()).
 */
#ifndef PCSEG_SPATIAL_H
#define PCSEG_SPATIAL_H

#include "pcseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- clustering against chance: exact window pair counts (the set covariance of the window in which points can sit,
 * summed over the lags of every distance bin).
 * mask   device uint8 (B, H, W), any width and alignment: non-zero = the pixel is in the window M of its frame
 * edges  HOST float64, n_edges = m + 1 in 2..1025, edges[0] == 0, strictly increasing, in units of `scale` pixels per unit
 * thr    = pcseg_surface_thresholds(edges, n_edges, scale): a lag (dy, dx) lies in bin k when thr[k] <= dy^2 + dx^2 <
 *          thr[k + 1], which is edges[k] <= sqrt(d2) / scale < edges[k + 1] as pcseg_point_neighbours and
 *          pcseg_surface_shells round it
 * gamma(dy, dx) = #{(y, x) : M[y, x] and M[y + dy, x + dx]}, pixels outside the image counting as outside the window
 * reach  R = floor(sqrt(thr[m] - 1)), the largest max(|dy|, |dx|) of a lag below the last threshold (thr[m] >= 1 because
 *          the edges increase from 0).  pcseg_window_reach (HOST only, touches no device) writes it to *reach.
 *   hist  device int64 (B, m + 2) = [n_px, bin_0 .. bin_m-1, over]: n_px = A = #M; bin_k = the sum of gamma(dy, dx) over
 *         ALL lags, both signs of dy and dx, the zero lag included, with thr[k] <= dy^2 + dx^2 < thr[k + 1]; over =
 *         A^2 - the sum of the bins.  The row without n_px sums to A^2: ordered pixel pairs, self pairs included.  An
 *         empty mask gives a row of zeros.
 *   lags  device int64 (B, R + 1, 2 R + 1), may be NULL (then NOT WRITTEN): gamma(dy, dx) for dy = 0 .. R, dx = -R .. R
 *         (the other half plane: gamma(-dy, -dx) = gamma(dy, dx)).  Lags that reach beyond the image count 0.
 * mask and edges are NOT WRITTEN.  H W < 2^30 (as everywhere), so gamma fits 32 bits and A^2 < 2^60; all arithmetic is
 * integer: the same bits whatever the order of the adds.
 * Limits: B <= 65535; R <= PCSEG_WINDOW_MAX_REACH, else PCSEG_ERR_ARG before anything is enqueued (a reach larger than
 * the image is no error); a null pointer (lags excepted), a bad shape, a scale that is not positive and finite and edges
 * that pcseg_surface_thresholds rejects are PCSEG_ERR_ARG too; a short workspace gives PCSEG_ERR_WORKSPACE.
 * Workspace: pcseg_window_pairs_workspace_bytes(B, H, W, n_edges, reach) with reach from pcseg_window_reach (0 for
 * sizes it rejects).  pcseg_window_rows (HOST only): the image rows one block of the lag walk holds in LDS. */
#define PCSEG_WINDOW_MAX_REACH 2048
int pcseg_window_reach(const double *edges, int n_edges, double scale, int64_t *reach);
int pcseg_window_rows(void);
size_t pcseg_window_pairs_workspace_bytes(int B, int H, int W, int n_edges, int64_t reach);
int pcseg_window_pairs(const uint8_t *mask, int B, int H, int W, double scale, const double *edges, int n_edges, int64_t *hist,
                       int64_t *lags, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PCSEG_SPATIAL_H */
