"""Spatial statistics on the device: clustering against chance (include/pcseg_spatial.h, csrc/window_pairs.hip).

The entries of ``pcseg_spatial.h`` live in the same ``libpcseg.so``; this module holds their signature table, sets the
prototypes on ``_lib.load()``'s handle and enters the library through ``ops._call`` with the argument checks of ``ops``
("The argument contract of ops": a tensor that is not on the device, or of another dtype, is a ``TypeError``;
another rank or shape a ``ValueError``; a non-contiguous input is copied).
"""
import collections
import ctypes
from ctypes import c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from . import _lib, ops

_P, _I = c_void_p, c_int
# name -> (restype, argtypes); mirrors include/pcseg_spatial.h one to one
SIGNATURES = {
    "pcseg_window_reach": (c_int, [_P, _I, c_double, _P]),
    "pcseg_window_rows": (c_int, []),
    "pcseg_window_pairs_workspace_bytes": (c_size_t, [_I, _I, _I, _I, c_int64]),
    "pcseg_window_pairs": (c_int, [_P, _I, _I, _I, c_double, _P, _I, _P, _P, _P, c_size_t, _P]),
}
MAX_REACH = 2048  # PCSEG_WINDOW_MAX_REACH
_bound = None


def _load():
    """``_lib.load()``'s handle with the prototypes of ``pcseg_spatial.h`` declared on it (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def window_rows():
    """The image rows one block of the lag walk holds in LDS (taller frames are walked chunk by chunk)."""
    return int(_load().pcseg_window_rows())


def window_reach(edges, scale):
    """Host only: the reach R of the bins, the largest ``max(|dy|, |dx|)`` of a pixel lag with ``sqrt(dy^2 + dx^2) / scale <
    edges[-1]`` as the kernels round it.  ``ValueError`` for edges the library refuses."""
    e, n_edges = ops._edges_arg(edges)
    out = ctypes.c_int64(0)
    if e is None or _load().pcseg_window_reach(e.ctypes.data, n_edges, float(scale), ctypes.byref(out)):
        msg = _lib.load().pcseg_last_error() if e is not None else b"no edges"
        raise ValueError("window_reach: %s" % (msg.decode() if msg else "?"))
    return int(out.value)


def _reach_within_limit(edges, scale):
    R = window_reach(edges, scale)
    if R > MAX_REACH:
        raise ValueError("the reach of the last edge is %d px, the limit is %d (PCSEG_WINDOW_MAX_REACH)" % (R, MAX_REACH))
    return R


def window_pair_counts(mask, edges, scale, lags=False):
    """Exact pair counts of a window, per distance bin (csrc/window_pairs.hip).  ``mask`` (B, H, W) uint8 (or bool) CUDA
    tensor, non-zero = the pixel is in the window; ``edges`` m + 1 increasing values from 0 (m <= 1024) in units of
    ``scale`` pixels per unit.  Returns ``hist`` int64 (B, m + 2) = ``[n_px, bin_0 .. bin_m-1, over]``: the ORDERED pairs of
    window pixels (self pairs included) whose distance d lies in ``edges[k] <= d < edges[k + 1]`` -- the bin rule of
    :func:`ops.point_neighbours` and :func:`ops.surface_shells` to the bit -- and ``over`` = the rest of the ``n_px ** 2``
    pairs.  With ``lags`` also ``lag_table`` int64 (B, R + 1, 2 R + 1), R = :func:`window_reach`: ``gamma(dy, dx) =
    #{(y, x): M[y, x] and M[y + dy, x + dx]}`` for dy = 0 .. R, dx = -R .. R (the other half plane is its mirror image).
    ``ValueError``, before anything is enqueued, for edges the library refuses and for a reach above ``MAX_REACH`` px; a
    reach larger than the image is fine.  Exact integers, bit for bit reproducible."""
    mask = ops._req(mask, torch.uint8, 3)
    B, H, W = mask.shape
    e, n_edges = ops._edges_arg(edges)
    R = _reach_within_limit(e, scale)
    if B < 1:
        hist = torch.zeros((0, n_edges + 1), dtype=torch.int64, device=mask.device)
        return (hist, torch.zeros((0, R + 1, 2 * R + 1), dtype=torch.int64, device=mask.device)) if lags else hist
    nbytes = _load().pcseg_window_pairs_workspace_bytes(B, H, W, n_edges, R)
    if not nbytes:
        raise ValueError("window_pair_counts: a batch of shape %s is not supported" % ((B, H, W),))
    dev = mask.device
    hist = torch.empty((B, n_edges + 1), dtype=torch.int64, device=dev)
    table = torch.empty((B, R + 1, 2 * R + 1), dtype=torch.int64, device=dev) if lags else None
    ops._call("window_pairs", mask, B, H, W, float(scale), e, n_edges, hist, table, ws=(ops._ws(nbytes, dev), nbytes))
    return (hist, table) if lags else hist


def pair_expectation(pair_hist, slot_counts, window_hist):
    """Observed pair counts against complete spatial randomness on the window, on the device.  ``pair_hist`` int64 (B, Q, m +
    2) of :func:`ops.point_neighbours` over the points IN the window (Q = K (K + 1) / 2 slot pairs, a <= b), ``slot_counts``
    int64 (B, K) = those points per slot, ``window_hist`` int64 (B, m + 2) of :func:`window_pair_counts` with the same edges.
    With G the window's bin, A = n_px and npairs = n_a (n_a - 1) / 2 (a == b) or n_a n_b: ``expected = (npairs * G) / (A * A)``
    and ``ratio = obs / expected`` in float64, each operation rounded on its own, NaN where A == 0 or expected == 0; the
    ``cum_*`` fields apply the same expressions to the integer prefix sums over the bins (the K-function form).  Returns a
    dict of (B, Q, m) tensors: ``obs``, ``cum_obs``, ``window_pairs``, ``cum_window_pairs`` int64 and ``expected``, ``ratio``,
    ``cum_expected``, ``cum_ratio`` float64; and ``npairs`` int64 (B, Q)."""
    pair_hist = ops._req(pair_hist, torch.int64, 3)
    slot_counts = ops._req(slot_counts, torch.int64, 2)
    window_hist = ops._req(window_hist, torch.int64, 2)
    B, Q, m = pair_hist.shape[0], pair_hist.shape[1], pair_hist.shape[2] - 2
    K = slot_counts.shape[1]
    if m < 1 or Q != K * (K + 1) // 2 or slot_counts.shape[0] != B or tuple(window_hist.shape) != (B, m + 2):
        raise ValueError("pair_hist (B, K (K + 1) / 2, m + 2), slot_counts (B, K) and window_hist (B, m + 2) do not match")
    dev = pair_hist.device
    ia = torch.tensor([a for a in range(K) for b in range(a, K)], dtype=torch.int64, device=dev)
    ib = torch.tensor([b for a in range(K) for b in range(a, K)], dtype=torch.int64, device=dev)
    na, nb = slot_counts[:, ia], slot_counts[:, ib]
    npairs = torch.where((ia == ib)[None, :], na * (na - 1) // 2, na * nb)
    obs = pair_hist[:, :, 1:m + 1]
    G = window_hist[:, None, 1:m + 1].expand(B, Q, m)
    A = window_hist[:, 0].to(torch.float64)[:, None, None].expand(B, Q, m)
    nan = torch.full((B, Q, m), float("nan"), dtype=torch.float64, device=dev)

    def derived(o, g):
        # every operand is a tensor: one correctly rounded product, product and quotient each (no reciprocal, no fusing)
        exp = (npairs.to(torch.float64)[:, :, None] * g.to(torch.float64)) / (A * A)
        exp = torch.where((A == 0) | (exp == 0), nan, exp)
        return exp, o.to(torch.float64) / exp

    cum_obs, cum_G = torch.cumsum(obs, dim=2), torch.cumsum(G, dim=2)
    expected, ratio = derived(obs, G)
    cum_expected, cum_ratio = derived(cum_obs, cum_G)
    return {"obs": obs, "window_pairs": G, "expected": expected, "ratio": ratio, "cum_obs": cum_obs, "cum_window_pairs": cum_G,
            "cum_expected": cum_expected, "cum_ratio": cum_ratio, "npairs": npairs}


CLUSTERING_COLUMNS = ("frame", "slot_a", "slot_b", "bin", "r_lo_um", "r_hi_um", "n_a", "n_b", "n_out_a", "n_out_b", "obs",
                      "window_pairs", "expected", "ratio", "cum_obs", "cum_window_pairs", "cum_expected", "cum_ratio")


def clustering_columns(edges):
    """The column lists of ``FramePipeline.clustering``'s two tables for ``edges`` (m + 1 values)."""
    m = len(np.asarray(edges, np.float64).reshape(-1)) - 1
    return {"window_pairs": ["frame", "n_px"] + ["bin_%d" % k for k in range(m)] + ["over"], "clustering": list(CLUSTERING_COLUMNS)}


def _points_in_window(points_rc, frame_offsets, mask):
    """(n,) bool: the window is set at pixel ``(floor(row + 0.5), floor(col + 0.5))`` of the point's frame -- the rule of
    :func:`ops.surface_distances`' ``inside``; False outside the image and for a NaN coordinate."""
    rc = ops._req(points_rc, torch.float64, 2)
    foff = ops._req(frame_offsets, torch.int64, 1)
    mask = ops._req(mask, torch.uint8, 3)
    B, H, W = mask.shape
    if rc.shape[1] != 2 or foff.shape[0] != B + 1:
        raise ValueError("points_rc must be (n, 2) and frame_offsets (B + 1,) for the mask's B frames")
    n = rc.shape[0]
    pr, pc = torch.floor(rc[:, 0] + 0.5), torch.floor(rc[:, 1] + 0.5)
    ok = (pr >= 0) & (pr <= H - 1) & (pc >= 0) & (pc <= W - 1)
    frame = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=rc.device), foff[1:] - foff[:-1], output_size=n)
    zero = torch.zeros_like(pr)
    idx = (frame * H + torch.where(ok, pr, zero).to(torch.int64)) * W + torch.where(ok, pc, zero).to(torch.int64)
    return ok & (mask.reshape(-1)[idx] != 0)


_WindowSlots = collections.namedtuple("_WindowSlots", "inside typed slot_in frame n_in n_out")


def _window_slots(points, points_rc, mask, K):
    """The points of a packed set against a window, for the tables that count only the points IN it: ``inside`` (n,) bool
    (:func:`_points_in_window`), ``typed`` (n,) bool (slot in 0 .. K - 1), ``slot_in`` (n,) int32 = the slot, -1 outside the
    window, ``frame`` (n,) int64 and ``n_in`` / ``n_out`` int64 (B, K): the typed points per frame and slot in the window and
    left out."""
    dev = mask.device
    B = mask.shape[0]
    foff = points.frame_offsets
    inside = _points_in_window(points_rc, foff, mask)
    typed = (points.slot >= 0) & (points.slot < K)
    slot_in = torch.where(inside, points.slot, torch.full_like(points.slot, -1))
    n = points.slot.shape[0]
    frame = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=dev), foff[1:] - foff[:-1], output_size=n)
    key = frame * K + points.slot.clamp(0, K - 1).to(torch.int64)
    count = lambda sel: torch.zeros((B * K,), dtype=torch.int64, device=dev).index_add_(0, key, sel.to(torch.int64)).reshape(B, K)
    return _WindowSlots(inside, typed, slot_in, frame, count(typed & inside), count(typed & ~inside))


def _clustering_tables(points, points_rc, mask, edges, scale, K, frame_ids):
    """The two tables of ``FramePipeline.clustering`` (which describes them) for one packed point set: ``points``
    (:class:`ops.Points`, coordinates as :func:`ops.point_neighbours` takes them), ``points_rc`` (n, 2) float64 (row, col) of
    the same points, 0-based, ``mask`` uint8 (B, H, W) the window, ``edges`` in units of ``scale`` pixels per unit, ``K`` type
    slots, ``frame_ids`` (B,) numpy.  Returns float64 CUDA tensors ``window_pairs`` (B, m + 3) and ``clustering`` (B Q m, 18)."""
    dev = mask.device
    B = mask.shape[0]
    K = int(K)
    foff = points.frame_offsets
    ws = _window_slots(points, points_rc, mask, K)
    slot_in, n_in, n_out = ws.slot_in, ws.n_in, ws.n_out
    _, _, pair_hist = ops.point_neighbours(points.coords, slot_in, points.ids, foff, K, scale, edges)
    window = window_pair_counts(mask, edges, scale)
    ex = pair_expectation(pair_hist, n_in, window)
    Q, m = pair_hist.shape[1], pair_hist.shape[2] - 2
    fid = torch.as_tensor(np.asarray(frame_ids, np.float64)).to(dev)
    ab = torch.tensor([(a, b) for a in range(K) for b in range(a, K)], dtype=torch.int64, device=dev)
    e = torch.as_tensor(np.asarray(edges, np.float64).reshape(-1)).to(dev)
    bins = torch.stack([torch.arange(m, dtype=torch.float64, device=dev), e[:-1], e[1:]], dim=1)
    per_pair = lambda t: t.to(torch.float64)[:, :, None, None].expand(B, Q, m, 1)  # (B, Q) -> a column
    col = lambda k: ex[k].to(torch.float64)[:, :, :, None]
    rows = torch.cat([fid[:, None, None, None].expand(B, Q, m, 1), ab.to(torch.float64)[None, :, None, :].expand(B, Q, m, 2),
                      bins[None, None].expand(B, Q, m, 3), per_pair(n_in[:, ab[:, 0]]), per_pair(n_in[:, ab[:, 1]]),
                      per_pair(n_out[:, ab[:, 0]]), per_pair(n_out[:, ab[:, 1]])]
                     + [col(k) for k in CLUSTERING_COLUMNS[10:]], dim=3).reshape(B * Q * m, len(CLUSTERING_COLUMNS))
    return {"window_pairs": torch.cat([fid[:, None], window.to(torch.float64)], dim=1), "clustering": rows}
