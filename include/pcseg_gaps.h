/*
 * pcseg_gaps.h -- edge-to-edge gaps between the ROIs of a label image (csrc/gaps.hip), compiled into the same libpcseg.so
 * as pcseg.h: same conventions (device pointers to contiguous batch-major arrays, caller-owned buffers, a caller-provided
 * workspace sized by the matching query whose prior contents never matter, work enqueued on `stream` without a host wait,
 * PCSEG_OK or a negative pcseg_status with the message in pcseg_last_error()).  All values are exact integers.
 */
#ifndef PCSEG_GAPS_H
#define PCSEG_GAPS_H

#include "pcseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the widest frame of the two entries below: one row of the search's stage ((W + 2) cells of 8 bytes) must fit 128 KB of
 * LDS.  A wider frame is PCSEG_ERR_ARG (its size query answers 0); it is never mis-computed. */
#define PCSEG_GAPS_MAX_WIDTH 16382

/* ---- nearest OTHER label.
 * A SITE is a pixel whose label l lies in 1 .. cap and, with sel (device uint8 (B, cap), may be NULL), has sel[b, l - 1] != 0
 * (the sites of pcseg_nearest_label_i32).  labels device int32 (B, H, W), any width and alignment.  For every pixel p
 *   d2   (device int32 (B, H, W)) = min of (pr - qr)^2 + (pc - qc)^2 over the frame's sites q with labels[q] != labels[p],
 *   near (device int32 (B, H, W)) = the SMALLEST label among those sites at that minimum.
 * Labels are compared as raw integers: a pixel whose label is 0, not selected or outside 1 .. cap never carries a site's label
 * and gets pcseg_nearest_label_i32's (d2, near).  Labels need not be connected.  With r2 >= 0 sites farther than r2 (d2 > r2)
 * are ignored (a site at exactly r2 counts); r2 < 0: unbounded.  d2 = -1, near = 0 where there is no such site: a frame
 * without site, a pixel whose label every site of the frame carries, nothing within r2.  Every pixel of d2 and near is written;
 * labels and sel are NOT WRITTEN.
 * Limits: the shapes of pcseg_edt_sq_u8 (H, W <= 32768, H W < 2^30), W <= PCSEG_GAPS_MAX_WIDTH, B <= 65535, cap >= 1; these
 * and a null pointer (sel excepted) are PCSEG_ERR_ARG before anything is enqueued, a short workspace PCSEG_ERR_WORKSPACE.
 * Workspace: pcseg_nearest_other_label_workspace_bytes(B, H, W) (0 for shapes the entry refuses). */
size_t pcseg_nearest_other_label_workspace_bytes(int B, int H, int W);
int pcseg_nearest_other_label_i32(const int32_t *labels, const uint8_t *sel, int cap, int64_t r2, int32_t *d2, int32_t *near, int B,
                                  int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

/* ---- gaps per label and type slot.
 * live device uint8 (B, cap): non-zero = label l (row l - 1) is a ROI of the table; slot_of device uint8 (B, cap): its type
 * slot, a value >= K: no type.  For a live label l and a slot t < K, over the pixels p with labels[p] == l and the pixels q
 * whose label m != l is live with slot_of[m] == t:
 *   gap2    (device int32 (B, cap, K))[b, l - 1, t] = min |p - q|^2   (1: the two ROIs touch along an edge, 2: at a corner),
 *   partner (device int32 (B, cap, K))[b, l - 1, t] = the smallest m that attains it.
 * -1 / 0 where there is no such pair, or none with |p - q|^2 <= r2 (r2 >= 0; r2 < 0: unbounded), for a live label without
 * pixel and for EVERY row of a label that is not live: all B cap K elements of both outputs are written.  The gap of a pair
 * is symmetric, so with m = partner[l - 1, t] and s = slot_of[l] < K: gap2[m - 1, s] <= gap2[l - 1, t], equal where
 * partner[m - 1, s] == l (m may have a nearer ROI of slot s than l).  K in 1 .. 4; labels, live and slot_of are NOT WRITTEN.
 * Limits and statuses as pcseg_nearest_other_label_i32, and cap < 2^30.
 * Workspace: pcseg_label_gaps_workspace_bytes(B, H, W, cap, K) (0 for arguments the entry refuses). */
size_t pcseg_label_gaps_workspace_bytes(int B, int H, int W, int cap, int K);
int pcseg_label_gaps(const int32_t *labels, const uint8_t *live, const uint8_t *slot_of, int cap, int K, int64_t r2, int32_t *gap2,
                     int32_t *partner, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PCSEG_GAPS_H */
