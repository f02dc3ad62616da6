"""The borders between touching regions and the merge by border strength (csrc/borders.hip, ops.label_borders /
merge_by_border; the definitions: include/pcseg.h) restated in numpy, with scipy's connected components for the grouping.
Imported by test_borders_cpu.py (which checks it on hand-made images) and test_gpu_borders.py.  No GPU here."""
from fractions import Fraction

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

TWO32 = 2 ** 32
# (row, column) steps of the link directions: right, down, down-right, down-left
STEPS = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}


def read_labels(L, cap):
    """Labels as the definitions read them, and bit 2 (value 2) where one lies above the cap."""
    L = np.asarray(L).astype(np.int64)
    return np.where((L < 0) | (L > cap), 0, L), (2 if (L > cap).any() else 0)


def read_values(V):
    """Values as probabilities: NaN -> 0, clamped to [0, 1]; bit 4 (value 4) where that changed one."""
    V = np.asarray(V, np.float32)
    bad = np.isnan(V) | (V < 0) | (V > 1)
    out = np.where(np.isnan(V), np.float32(0), np.clip(V, np.float32(0), np.float32(1))).astype(np.float32) + np.float32(0)
    return out, (4 if bad.any() else 0)


def shifted(x, dr, dc):
    """The two views of x whose elements are (dr, dc) apart: p, q with q = p + (dr, dc); dr >= 0."""
    H, W = x.shape
    if dc >= 0:
        return x[:H - dr, :W - dc], x[dr:, dc:]
    return x[:H - dr, -dc:], x[dr:, :W + dc]


def frame_borders(L, V, conn=8, cap=None):
    """One frame: a, b (a < b), links, sum (int64), saddle (float32), sorted by (a, b), and the flag bits 2 and 4."""
    cap = max(int(np.max(L)), 1) if cap is None else cap
    lab, f_l = read_labels(L, cap)
    val, f_v = read_values(V)
    keys, fixed, ridge = [], [], []
    for dr, dc in STEPS[conn]:
        lp, lq = shifted(lab, dr, dc)
        vp, vq = shifted(val, dr, dc)
        on = (lp >= 1) & (lq >= 1) & (lp != lq)
        keys.append((np.minimum(lp, lq)[on] << 32) | np.maximum(lp, lq)[on])
        v = np.maximum(vp, vq)[on]
        ridge.append(v)
        fixed.append(np.rint(v.astype(np.float64) * TWO32).astype(np.int64))
    keys, fixed, ridge = np.concatenate(keys), np.concatenate(fixed), np.concatenate(ridge)
    uniq, inv = np.unique(keys, return_inverse=True)
    links = np.zeros(len(uniq), np.int64)
    total = np.zeros(len(uniq), np.int64)
    saddle = np.full(len(uniq), np.inf, np.float32)
    np.add.at(links, inv, 1)
    np.add.at(total, inv, fixed)
    np.minimum.at(saddle, inv, ridge)
    return uniq >> 32, uniq & 0xFFFFFFFF, links, total, saddle, f_l | f_v


def exact_mean(total, links):
    """sum / (links 2^32) correctly rounded to float64, through Fraction."""
    return np.array([float(Fraction(int(s), int(n) * TWO32)) for s, n in zip(total, links)], np.float64)


def borders(L, V, conn=8, cap=None):
    """ops.label_borders restated for a batch (B, H, W): the same keys as numpy arrays, rows sorted by (frame, a, b)."""
    L = np.asarray(L)
    cap = max(int(L.max()), 1) if cap is None else cap
    cols = {k: [] for k in ("frame", "a", "b", "links", "sum", "saddle")}
    flags = []
    for f in range(L.shape[0]):
        a, b, links, total, saddle, fl = frame_borders(L[f], V[f], conn, cap)
        for k, v in zip(("frame", "a", "b", "links", "sum", "saddle"), (np.full(len(a), f, np.int64), a, b, links, total, saddle)):
            cols[k].append(v)
        flags.append(fl)
    out = {k: np.concatenate(v) for k, v in cols.items()}
    out["mean"] = exact_mean(out["sum"], out["links"])
    out["overflow"] = np.array(flags, np.int32)
    out["pairs_per_frame"] = np.array([len(v) for v in cols["a"]])
    return out


def joined(links, total, saddle, below, by="mean"):
    """The merge rule, per pair: integers for the mean, float32 for the saddle; strict."""
    if by == "mean":
        t = int(np.rint(np.float64(below) * TWO32))
        return np.array([int(s) < t * int(n) for s, n in zip(total, links)], bool)
    return np.asarray(saddle, np.float32) < np.float32(below)


def group_map(a, b, join, count, cap):
    """map (cap + 1,) and m: the connected components of the joined pairs over the nodes 1 .. count, numbered by each
    component's smallest member; 0 at 0 and above count.  Pairs with a label above count are no edges."""
    a, b, join = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(join, bool)
    keep = join & (a >= 1) & (b >= 1) & (a <= count) & (b <= count)
    out = np.zeros(cap + 1, np.int32)
    if count < 1:
        return out, 0
    g = coo_matrix((np.ones(int(keep.sum()), np.int8), (a[keep] - 1, b[keep] - 1)), shape=(count, count))
    m, comp = connected_components(g, directed=False)
    # smallest member of every component, then rank the components by it
    smallest = np.full(m, count + 1, np.int64)
    np.minimum.at(smallest, comp, np.arange(1, count + 1))
    rank = np.empty(m, np.int64)
    rank[np.argsort(smallest)] = np.arange(1, m + 1)
    out[1:count + 1] = rank[comp]
    return out, int(m)


def merge(L, V, below, by="mean", conn=8, counts=None, cap=None):
    """ops.merge_by_border restated: (merged, n_merged, map, flags) as numpy arrays."""
    L = np.asarray(L)
    B = L.shape[0]
    cap = max(int(L.max()), 1) if cap is None else cap
    merged = np.zeros(L.shape, np.int32)
    maps = np.zeros((B, cap + 1), np.int32)
    n_merged = np.zeros(B, np.int32)
    flags = np.zeros(B, np.int32)
    for f in range(B):
        count = cap if counts is None else min(max(int(counts[f]), 0), cap)
        a, b, links, total, saddle, flags[f] = frame_borders(L[f], V[f], conn, cap)
        maps[f], n_merged[f] = group_map(a, b, joined(links, total, saddle, below, by), count, cap)
        merged[f] = maps[f][read_labels(L[f], cap)[0]]
    return merged, n_merged, maps, flags


def float_bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
