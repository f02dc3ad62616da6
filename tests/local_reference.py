"""numpy restatement of the local neighbourhood counts (include/pcseg_local.h) and of the neighbourhood table on top of them,
written from the definitions.  No tests in here: tests/test_local_counts_cpu.py and tests/test_gpu_local_counts.py compare
against it, by equality."""
import numpy as np


def disk_counts(planes, queries, frame_offsets, thresholds, C):
    """``(counts, area)`` of ``pcseg_disk_counts``: for every query a loop over ALL pixels of its frame -- the squared distance,
    its ring by ``thr[k] <= d2 < thr[k + 1]``, one count per set whose bit the pixel carries.  ``planes`` (B, H, W) uint8,
    ``queries`` (n, 2) = (row, col), ``frame_offsets`` (B + 1,), ``thresholds`` (m + 1,) int64.  int64 (n, C, m) and (B, C)."""
    planes = np.asarray(planes, np.uint8)
    thr = np.asarray(thresholds, np.int64)
    B, H, W = planes.shape
    m = thr.shape[0] - 1
    queries = np.asarray(queries, np.int64).reshape(-1, 2)
    counts = np.zeros((queries.shape[0], C, m), np.int64)
    frame = np.searchsorted(np.asarray(frame_offsets, np.int64), np.arange(queries.shape[0]), side="right") - 1
    rows, cols = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    for i, (pr, pc) in enumerate(queries):
        d2 = (rows - pr) ** 2 + (cols - pc) ** 2
        k = np.searchsorted(thr, d2, side="right") - 1
        for c in range(C):
            sel = (((planes[frame[i]] >> c) & 1) != 0) & (k >= 0) & (k < m)
            counts[i, c] = np.bincount(k[sel], minlength=m)[:m]
    area = np.stack([((planes >> c) & 1).reshape(B, -1).sum(axis=1) for c in range(C)], axis=1).astype(np.int64)
    return counts, area


def point_counts(xy, slot, frame_offsets, K, scale, edges):
    """``counts`` of ``pcseg_point_counts``: a loop over all ordered pairs i != j of a frame's points; point_neighbours'
    formula, d = sqrt(dx*dx + dy*dy) / scale (every operation rounded on its own), bin k = edges[k] <= d < edges[k + 1]; the
    row of a point whose slot is outside 0 .. K - 1 is -1, and it is counted for nobody.  int64 (n, K, m)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    slot = np.asarray(slot, np.int64)
    edges = np.asarray(edges, np.float64)
    foff = np.asarray(frame_offsets, np.int64)
    m = edges.shape[0] - 1
    out = np.zeros((xy.shape[0], K, m), np.int64)
    for b in range(foff.shape[0] - 1):
        for i in range(foff[b], foff[b + 1]):
            if not 0 <= slot[i] < K:
                out[i] = -1
                continue
            for j in range(foff[b], foff[b + 1]):
                if j == i or not 0 <= slot[j] < K:
                    continue
                dx, dy = xy[i, 0] - xy[j, 0], xy[i, 1] - xy[j, 1]
                d = np.sqrt(dx * dx + dy * dy) / scale
                k = int(np.searchsorted(edges, d, side="right")) - 1
                if 0 <= k < m:
                    out[i, slot[j], k] += 1
    return out


def pair_hist_bins(xy, slot, frame_offsets, K, scale, edges):
    """The bins of ``pcseg_point_neighbours``' pair_hist from all UNORDERED pairs: int64 (B, K (K + 1) / 2, m)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    slot = np.asarray(slot, np.int64)
    edges = np.asarray(edges, np.float64)
    foff = np.asarray(frame_offsets, np.int64)
    m = edges.shape[0] - 1
    index = {(a, b): q for q, (a, b) in enumerate((a, b) for a in range(K) for b in range(a, K))}
    out = np.zeros((foff.shape[0] - 1, len(index), m), np.int64)
    for b in range(foff.shape[0] - 1):
        for i in range(foff[b], foff[b + 1]):
            for j in range(i + 1, foff[b + 1]):
                if not (0 <= slot[i] < K and 0 <= slot[j] < K):
                    continue
                dx, dy = xy[i, 0] - xy[j, 0], xy[i, 1] - xy[j, 1]
                k = int(np.searchsorted(edges, np.sqrt(dx * dx + dy * dy) / scale, side="right")) - 1
                if 0 <= k < m:
                    out[b, index[(min(slot[i], slot[j]), max(slot[i], slot[j]))], k] += 1
    return out


def window_queries(points_rc):
    """the pixel (floor(row + 0.5), floor(col + 0.5)) of every point; pixel 0 for a NaN coordinate"""
    q = np.floor(np.asarray(points_rc, np.float64).reshape(-1, 2) + 0.5)
    return np.clip(np.where(np.isnan(q), 0.0, q), -(2.0 ** 24 - 1), 2.0 ** 24 - 1).astype(np.int64)


def columns(names):
    out = ["frame", "label", "slot", "in_window", "bin", "r_lo_um", "r_hi_um", "win_px", "cum_win_px"]
    for n in names:
        out += [c % n for c in ("n_%s", "cum_n_%s", "px_%s", "cum_px_%s", "expected_%s", "cum_expected_%s")]
    return out + ["own_frac", "own_px_frac"]


def neighbourhood_rows(frame_ids, xy, points_rc, slot, ids, frame_offsets, planes, edges, scale, thresholds, K):
    """The ``neighbourhoods`` table from the definitions: ``planes`` bit 0 the window, bit 1 + t the pixels of slot t.  A point
    is in the window when bit 0 is set at its rounded centroid (inside the image); the others get slot -1 for the counting.
    Float64, every operation rounded on its own: expected = (N_t * win_px) / A, NaN where A == 0; the fractions NaN where their
    denominator is 0; every count column NaN for a point outside the window."""
    planes = np.asarray(planes, np.uint8)
    B, H, W = planes.shape
    slot = np.asarray(slot, np.int64)
    edges = np.asarray(edges, np.float64)
    foff = np.asarray(frame_offsets, np.int64)
    m = edges.shape[0] - 1
    n = slot.shape[0]
    q = window_queries(points_rc)
    frame = np.searchsorted(foff, np.arange(n), side="right") - 1
    ok = ~np.isnan(np.asarray(points_rc, np.float64).reshape(-1, 2)).any(axis=1)
    ok &= (q[:, 0] >= 0) & (q[:, 0] < H) & (q[:, 1] >= 0) & (q[:, 1] < W)
    inside = np.zeros(n, bool)
    inside[ok] = (planes[frame[ok], q[ok, 0], q[ok, 1]] & 1) != 0
    typed = (slot >= 0) & (slot < K)
    near = point_counts(xy, np.where(inside, slot, -1), foff, K, scale, edges)
    px, area = disk_counts(planes, q, foff, thresholds, 1 + K)
    n_in = np.array([[int((typed & inside & (frame == b) & (slot == t)).sum()) for t in range(K)] for b in range(B)], np.int64).reshape(B, K)
    rows = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in np.nonzero(typed)[0]:
            b, s = frame[i], slot[i]
            A = np.float64(area[b, 0])
            cn, cp = np.cumsum(near[i], axis=1), np.cumsum(px[i], axis=1)
            win, cwin = px[i, 0].astype(np.float64), cp[0].astype(np.float64)
            cols = [win, cwin]
            for t in range(K):
                N = np.float64(n_in[b, t] - (1 if t == s else 0))
                exp, cexp = (N * win) / A, (N * cwin) / A
                if A == 0:
                    exp, cexp = np.full(m, np.nan), np.full(m, np.nan)
                cols += [near[i, t].astype(np.float64), cn[t].astype(np.float64), px[i, 1 + t].astype(np.float64),
                         cp[1 + t].astype(np.float64), exp, cexp]
            for own, tot in ((cn[s], cn.sum(axis=0)), (cp[1 + s], cp[1:].sum(axis=0))):
                frac = own.astype(np.float64) / tot.astype(np.float64)
                cols.append(np.where(tot == 0, np.nan, frac))
            cols = np.stack(cols, axis=1)
            if not inside[i]:
                cols[:] = np.nan
            head = np.stack([np.full(m, float(frame_ids[b])), np.full(m, float(ids[i])), np.full(m, float(s)),
                             np.full(m, float(inside[i])), np.arange(m, dtype=np.float64), edges[:-1], edges[1:]], axis=1)
            rows.append(np.concatenate([head, cols], axis=1))
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 11 + 6 * K))
