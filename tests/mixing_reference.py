"""The random-labelling test of the pair-distance histograms (include/pcseg.h, pcseg_pair_label_mixing) restated in numpy:
the labelling rule word for word (uint64 arithmetic, vectorised over the permutations), the counts by brute force on
point_neighbours' formula (d = sqrt(dx*dx + dy*dy) / scale, bin k = edges[k] <= d < edges[k + 1]) and the envelope."""
import numpy as np

FIELDS = ("obs", "lo", "hi", "sum", "n_le", "n_ge")
M64 = (1 << 64) - 1


def labellings(slots, K, P, key, seed):
    """(P + 1, n_t) labels of the typed points (``slots``: their observed slots in the caller's order); row 0 = observed."""
    slots = np.asarray(slots, np.int64)
    n_t = slots.shape[0]
    lab = np.empty((P + 1, n_t), np.int64)
    lab[0] = slots
    rem = np.tile(np.bincount(slots, minlength=K)[:K].astype(np.uint64), (P, 1))
    p = np.arange(1, P + 1, dtype=np.uint64)
    head = np.uint64((key & 0xFFFFFF) << 40) ^ (p << np.uint64(24))
    u = np.uint64
    with np.errstate(over="ignore"):
        for i in range(n_t):
            tot = u(n_t - i)
            z = (head ^ u(i)) * u(0x9E3779B97F4A7C15) + u(seed & M64)
            z ^= z >> u(30); z *= u(0xBF58476D1CE4E5B9)
            z ^= z >> u(27); z *= u(0x94D049BB133111EB)
            z ^= z >> u(31)
            r = ((z >> u(32)) * tot + (((z & u(0xFFFFFFFF)) * tot) >> u(32))) >> u(32)  # high half of z * tot (tot < 2^24)
            s = (r[:, None] >= np.cumsum(rem, axis=1)).sum(axis=1)  # the smallest slot with r < rem[0] + .. + rem[s]
            lab[1:, i] = s
            rem[np.arange(P), s] -= u(1)
    return lab


def envelope(counts):
    """(B, P + 1, Q, m) counts -> dict of the twelve (B, Q, m) tensors."""
    out = {}
    for pre, c in (("", counts), ("cum_", np.cumsum(counts, axis=3))):
        obs, sh = c[:, 0], c[:, 1:]
        zero = np.zeros_like(obs)
        has = sh.shape[1] > 0
        vals = (obs, sh.min(axis=1) if has else zero, sh.max(axis=1) if has else zero, sh.sum(axis=1),
                (sh <= obs[:, None]).sum(axis=1), (sh >= obs[:, None]).sum(axis=1))
        out.update((pre + k, v.astype(np.int64)) for k, v in zip(FIELDS, vals))
    return out


def mixing(xy, slot, foff, K, scale, edges, P, seed=0, keys=None):
    """counts (B, P + 1, Q, m) int64 of the points ``xy`` (n, 2), ``slot`` (n,), frames ``foff`` (B + 1,)."""
    B, m, Q = len(foff) - 1, len(edges) - 1, K * (K + 1) // 2
    pidx = np.zeros((K, K), np.int64)
    for q, (a, b) in enumerate((a, b) for a in range(K) for b in range(a, K)):
        pidx[a, b] = pidx[b, a] = q
    counts = np.zeros((B, P + 1, Q, m), np.int64)
    for f in range(B):
        lo, hi = int(foff[f]), int(foff[f + 1])
        typed = np.nonzero((slot[lo:hi] >= 0) & (slot[lo:hi] < K))[0] + lo
        lab = labellings(slot[typed], K, P, f if keys is None else int(keys[f]), seed)
        X, Y = xy[typed, 0], xy[typed, 1]
        I, J = np.triu_indices(len(typed), 1)
        dx, dy = X[I] - X[J], Y[I] - Y[J]
        k = np.searchsorted(edges, np.sqrt(dx * dx + dy * dy) / scale, side="right") - 1
        I, J, k = I[k < m], J[k < m], k[k < m]
        for p in range(P + 1):
            counts[f, p] = np.bincount(pidx[lab[p, I], lab[p, J]] * m + k, minlength=Q * m).reshape(Q, m)
    return counts
