"""numpy restatement of the window pair counts (include/pcseg_spatial.h) and of the clustering table on top of them.
No tests in here: tests/test_window_pairs_cpu.py and tests/test_gpu_window_pairs.py compare against it, by equality."""
import numpy as np


def lag_table_brute(mask, R):
    """gamma(dy, dx) for dy = 0 .. R, dx = -R .. R from ALL pairs of window pixels: int64 (R + 1, 2 R + 1)."""
    ys, xs = np.nonzero(np.asarray(mask))
    out = np.zeros((R + 1, 2 * R + 1), np.int64)
    if ys.size == 0:
        return out
    dy = (ys[None, :] - ys[:, None]).ravel()
    dx = (xs[None, :] - xs[:, None]).ravel()
    keep = (dy >= 0) & (dy <= R) & (np.abs(dx) <= R)
    return np.bincount(dy[keep] * (2 * R + 1) + dx[keep] + R, minlength=out.size).astype(np.int64).reshape(out.shape)


def lag_table_fft(mask, R):
    """The same table as the zero-padded rfft2 autocorrelation, rounded to the nearest integer."""
    m = (np.asarray(mask) != 0).astype(np.float64)
    H, W = m.shape
    f = np.fft.rfft2(m, s=(2 * H, 2 * W))
    ac = np.rint(np.fft.irfft2(f * np.conj(f), s=(2 * H, 2 * W))).astype(np.int64)  # ac[dy % 2H, dx % 2W]
    out = np.zeros((R + 1, 2 * R + 1), np.int64)
    Ry, Rx = min(R, H - 1), min(R, W - 1)
    dy = np.arange(Ry + 1)
    dx = np.arange(-Rx, Rx + 1)
    out[:Ry + 1, R - Rx:R + Rx + 1] = ac[dy[:, None] % (2 * H), dx[None, :] % (2 * W)]
    return out


def reach(thresholds):
    """R = floor(sqrt(thr[m] - 1)): the largest max(|dy|, |dx|) of a lag below the last threshold."""
    v = int(thresholds[-1]) - 1
    r = int(np.sqrt(float(v)))
    while r * r > v:
        r -= 1
    while (r + 1) * (r + 1) <= v:
        r += 1
    return r


def window_hist(mask, thresholds, table=None):
    """``[n_px, bin_0 .. bin_m-1, over]`` (int64) of one frame: every lag of both half planes, the zero lag included, in
    the bin k with ``thr[k] <= dy^2 + dx^2 < thr[k + 1]``; over = n_px^2 - the bins.  ``table``: a lag table of reach
    ``reach(thresholds)`` to bin (default: the brute one)."""
    thr = np.asarray(thresholds, np.int64)
    m = thr.shape[0] - 1
    R = reach(thr)
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    Rc = min(R, max(H, W) - 1)  # lags beyond the image count nothing
    g = lag_table_brute(mask, Rc) if table is None else np.asarray(table)[:Rc + 1, R - Rc:R + Rc + 1]
    dy = np.arange(Rc + 1, dtype=np.int64)[:, None]
    dx = np.arange(-Rc, Rc + 1, dtype=np.int64)[None, :]
    k = np.searchsorted(thr, dy * dy + dx * dx, side="right") - 1
    weight = np.where(dy > 0, 2, 1) * g  # gamma(-dy, -dx) = gamma(dy, dx)
    A = int(mask.sum())
    out = np.zeros(m + 2, np.int64)
    out[0] = A
    keep = k < m
    np.add.at(out, 1 + k[keep], weight[keep])
    out[m + 1] = A * A - int(out[1:m + 1].sum())
    return out


def clustering_rows(frame_ids, edges, obs, slot_in, slot_out, window):
    """The ``clustering`` table from exact integers: ``obs`` (B, Q, m) pair counts of the in-window points per slot pair
    (a <= b order), ``slot_in`` / ``slot_out`` (B, K) points inside / left out, ``window`` (B, m + 2) of :func:`window_hist`.
    Float64, every operation rounded on its own: expected = (npairs * G) / (A * A), ratio = obs / expected; NaN where A == 0
    or expected == 0; the cumulative columns from the integer prefix sums."""
    obs, window = np.asarray(obs, np.int64), np.asarray(window, np.int64)
    slot_in, slot_out = np.asarray(slot_in, np.int64), np.asarray(slot_out, np.int64)
    B, Q, m = obs.shape
    K = slot_in.shape[1]
    edges = np.asarray(edges, np.float64)
    rows = []

    def derived(npairs, o, g, A):
        with np.errstate(divide="ignore", invalid="ignore"):
            exp = (npairs * g.astype(np.float64)) / (A * A)
            exp = np.where((A == 0) | (exp == 0), np.nan, exp)
            return exp, o.astype(np.float64) / exp

    for b in range(B):
        A = np.float64(window[b, 0])
        G = window[b, 1:m + 1]
        cG = np.cumsum(G)
        q = 0
        for a in range(K):
            for c in range(a, K):
                na, nb = int(slot_in[b, a]), int(slot_in[b, c])
                npairs = np.float64(na * (na - 1) // 2 if a == c else na * nb)
                o, co = obs[b, q], np.cumsum(obs[b, q])
                exp, ratio = derived(npairs, o, G, A)
                cexp, cratio = derived(npairs, co, cG, A)
                for k in range(m):
                    rows.append([frame_ids[b], a, c, k, edges[k], edges[k + 1], na, nb, slot_out[b, a], slot_out[b, c],
                                 o[k], G[k], exp[k], ratio[k], co[k], cG[k], cexp[k], cratio[k]])
                q += 1
    return np.array(rows, np.float64).reshape(-1, 18)
