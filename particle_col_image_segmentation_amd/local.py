"""Local neighbourhoods on the device: what lies within each distance of ONE cell (include/pcseg_local.h,
csrc/local_counts.hip).

``neighbours`` and ``gaps`` give every cell's nearest partner, ``pair_hist``, ``mixing`` and ``clustering`` one number per frame,
slot pair and distance bin.  This module gives the per-cell marks of those statistics: how many cells of each strain, how many
pixels of each strain and how much of the window lie in each distance ring around a cell -- the local K-function of Getis and
Franklin with its edge-correction term, and a segregation index per cell.  Summed over the cells of a frame the point counts are
``clustering``'s observed counts; summed over the window's pixels the ring counts are ``spatial.window_pair_counts``' bins.

The entries of ``pcseg_local.h`` live in the same ``libpcseg.so``; this module holds their signature table, sets the prototypes
on ``_lib.load()``'s handle and enters the library through ``ops._call`` with the argument checks of ``ops`` ("The
argument contract of ops": a tensor that is not on the device, or of another dtype, is a ``TypeError``; another rank or shape a
``ValueError``; a non-contiguous input is copied).
"""
from ctypes import c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from . import _lib, ops, spatial

_P, _I = c_void_p, c_int
# name -> (restype, argtypes); mirrors include/pcseg_local.h one to one
SIGNATURES = {
    "pcseg_local_rows": (c_int, []),
    "pcseg_local_bins": (c_int, []),
    "pcseg_disk_counts_workspace_bytes": (c_size_t, [_I, _I, _I, _I, _I, c_int64]),
    "pcseg_disk_counts": (c_int, [_P, _I, _I, _I, _I, _P, _P, c_int64, c_double, _P, _I, _P, _P, _P, c_size_t, _P]),
    "pcseg_local_point_tile": (c_int, []),
    "pcseg_point_counts_workspace_bytes": (c_size_t, [c_int64, _I, _I, _I]),
    "pcseg_point_counts": (c_int, [_P, _P, _P, c_int64, _I, _I, c_double, _P, _I, _P, _P, c_size_t, _P]),
}
MAX_SETS = 8
_bound = None


def _load():
    """``_lib.load()``'s handle with the prototypes of ``pcseg_local.h`` declared on it (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def local_rows():
    """The image rows one pass of a query's wave covers with a single bin (more bins: fewer rows per pass)."""
    return int(_load().pcseg_local_rows())


def local_bins():
    """The bins one pass of a query's wave covers (more bins are walked chunk by chunk)."""
    return int(_load().pcseg_local_bins())


def local_point_tile():
    """The candidates one pass of a point's wave compares in :func:`point_counts` (larger frames: pass by pass)."""
    return int(_load().pcseg_local_point_tile())


def _checked_edges(edges, scale):
    """``ops._edges_arg``, and ``ValueError`` for edges or a scale that ``pcseg_surface_thresholds`` (host only: the rules of
    ``pcseg_point_neighbours``) refuses -- before any launch."""
    e, n_edges = ops._edges_arg(edges)
    out = np.zeros(max(n_edges, 1), np.int64)
    if e is None or _load().pcseg_surface_thresholds(e.ctypes.data, n_edges, float(scale), out.ctypes.data):
        msg = _lib.load().pcseg_last_error() if e is not None else b"no edges"
        raise ValueError("edges: %s" % (msg.decode() if msg else "?"))
    return e, n_edges


def disk_counts(planes, queries, frame_offsets, edges, scale, sets=MAX_SETS):
    """Set pixels in distance rings around query pixels (csrc/local_counts.hip).  ``planes`` (B, H, W) uint8 CUDA tensor, bit c
    of a pixel set = the pixel belongs to set c, for c < ``sets`` (1 .. 8; higher bits are ignored); ``queries`` (n, 2) int32 =
    (row, col) in frame-contiguous order, ``frame_offsets`` (B + 1,) int64; ``edges`` m + 1 increasing values from 0 (m <= 1024)
    in units of ``scale`` pixels per unit.  Returns ``(counts, area)``: ``counts`` int32 (n, sets, m), the pixels q of set c in
    the query's own frame with ``edges[k] <= |p - q| / scale < edges[k + 1]`` -- the bin rule of
    :func:`spatial.window_pair_counts` to the bit; the query pixel itself counts, in ring 0, when it is in the set -- and
    ``area`` int64 (B, sets), the pixels of every set per frame.  A query may lie on the border, outside the image or farther
    from it than the reach (|row|, |col| < 2^24): pixels outside the image belong to no set.  ``ValueError``, before anything is
    enqueued, for edges the library refuses and for a reach above ``spatial.MAX_REACH`` px.  Without a frame both results are
    empty; without a query ``counts`` is empty and only the areas are counted.  Exact integers, bit for bit reproducible."""
    planes = ops._req(planes, torch.uint8, 3)
    queries = ops._req(queries, torch.int32, 2)
    foff = ops._req(frame_offsets, torch.int64, 1)
    B, H, W = planes.shape
    n, C = queries.shape[0], int(sets)
    if queries.shape[1] != 2 or foff.shape[0] != B + 1:
        raise ValueError("queries must be (n, 2) and frame_offsets (B + 1,) for the planes' B frames")
    if not 1 <= C <= MAX_SETS:
        raise ValueError("1 to %d sets" % MAX_SETS)
    e, n_edges = ops._edges_arg(edges)
    R = spatial._reach_within_limit(e, scale)
    dev = planes.device
    m = n_edges - 1
    if B < 1:
        return torch.zeros((0, C, m), dtype=torch.int32, device=dev), torch.zeros((0, C), dtype=torch.int64, device=dev)
    nbytes = _load().pcseg_disk_counts_workspace_bytes(B, C, H, W, n_edges, R)
    if not nbytes:
        raise ValueError("disk_counts: a batch of shape %s is not supported" % ((B, H, W),))
    counts = torch.empty((n, C, m), dtype=torch.int32, device=dev)
    area = torch.empty((B, C), dtype=torch.int64, device=dev)
    ops._call("disk_counts", planes, B, C, H, W, queries if n else None, foff, n, float(scale), e, n_edges, counts if n else None, area,
              ws=(ops._ws(nbytes, dev), nbytes))
    return counts, area


def point_counts(xy, slot, frame_offsets, K, scale, edges):
    """Other points in distance rings around every point (csrc/local_counts.hip).  ``xy`` (n, 2) float64, ``slot`` (n,) int32 and
    ``frame_offsets`` (B + 1,) int64 CUDA tensors as :func:`ops.point_neighbours` takes them, ``K`` <= 4 type slots, ``edges``
    m + 1 increasing values from 0 in units of ``scale``.  Returns ``counts`` int32 (n, K, m): for point i and slot t the OTHER
    points of slot t in i's frame (excluded by index: a duplicate position counts in bin 0) whose distance lies in ``edges[k]
    <= d < edges[k + 1]`` -- the bin rule of :func:`ops.point_neighbours`' ``pair_hist`` to the bit; pairs at or beyond the last
    edge are not counted.  The row of a point whose slot is outside 0 .. K - 1 is all -1, and it is counted for nobody.
    ``ValueError`` for edges the library refuses.  Exact integers, bit for bit reproducible."""
    xy = ops._req(xy, torch.float64, 2)
    slot = ops._req(slot, torch.int32, 1)
    foff = ops._req(frame_offsets, torch.int64, 1)
    n, B, K = xy.shape[0], foff.shape[0] - 1, int(K)
    if xy.shape[1] != 2 or slot.shape[0] != n:
        raise ValueError("xy must be (n, 2) with n slots")
    if not 1 <= K <= 4:
        raise ValueError("1 to 4 type slots")
    e, n_edges = _checked_edges(edges, scale)
    dev = xy.device
    if n < 1:
        return torch.zeros((0, K, n_edges - 1), dtype=torch.int32, device=dev)
    if B < 1:
        raise ValueError("%d points but no frame: frame_offsets must be (B + 1,)" % n)
    counts = torch.empty((n, K, n_edges - 1), dtype=torch.int32, device=dev)
    nbytes = _load().pcseg_point_counts_workspace_bytes(n, B, K, n_edges)
    if not nbytes:
        raise ValueError("point_counts: %d points in %d frames are not supported" % (n, B))
    ops._call("point_counts", xy, slot, foff, n, B, K, float(scale), e, n_edges, counts, ws=(ops._ws(nbytes, dev), nbytes))
    return counts


NEIGHBOURHOOD_COLUMNS = ("frame", "label", "slot", "in_window", "bin", "r_lo_um", "r_hi_um", "win_px", "cum_win_px")
_PER_SLOT = ("n_%s", "cum_n_%s", "px_%s", "cum_px_%s", "expected_%s", "cum_expected_%s")


def neighbourhood_columns(names, edges=None):
    """The columns of :func:`neighbourhood_tables` for the type slots ``names`` (their names, or their number); they do not
    depend on ``edges``."""
    names = ["%d" % k for k in range(names)] if isinstance(names, int) else [str(n) for n in names]
    return list(NEIGHBOURHOOD_COLUMNS) + [c % n for n in names for c in _PER_SLOT] + ["own_frac", "own_px_frac"]


def window_queries(points_rc):
    """(n, 2) int32: the pixel ``(floor(row + 0.5), floor(col + 0.5))`` of every point -- the rule of
    ``spatial._points_in_window``; a NaN coordinate gives pixel 0 (such a point is in no window) and coordinates are clipped
    to +-(2^24 - 1)."""
    rc = ops._req(points_rc, torch.float64, 2)
    lim = float((1 << 24) - 1)
    return torch.nan_to_num(torch.floor(rc + 0.5), nan=0.0).clamp(-lim, lim).to(torch.int32)


def set_planes(window, class_map, class_slot):
    """The ``planes`` of :func:`neighbourhood_tables`: bit 0 where ``window`` (uint8 (B, H, W)) is non-zero, bit 1 + t where
    ``class_slot`` (256 values on the host: class value -> type slot, 255 = none) maps the pixel of ``class_map`` (uint8 (B, H,
    W)) to slot t -- the 256-entry look-up, applied as one compare per typed class value."""
    window = ops._req(window, torch.uint8, 3)
    class_map = ops._req(class_map, torch.uint8, 3)
    if window.shape != class_map.shape:
        raise ValueError("window and class_map must have one shape")
    slot = np.asarray(class_slot, np.uint8).reshape(256)
    planes = (window != 0).to(torch.uint8)
    for value in np.nonzero(slot < 7)[0]:  # the few class values that carry a type: one compare each, no widened copy of the map
        planes |= (class_map == int(value)).to(torch.uint8) << (1 + int(slot[value]))
    return planes


def neighbourhood_tables(points, points_rc, planes, edges, scale, K, frame_ids):
    """The table of ``FramePipeline.neighbourhoods`` (which describes it) for one packed point set: ``points``
    (:class:`ops.Points`, coordinates as :func:`ops.point_neighbours` takes them), ``points_rc`` (n, 2) float64 (row, col) of the
    same points, 0-based, ``planes`` uint8 (B, H, W): bit 0 the window, bit 1 + t the pixels of type slot t, ``edges`` in units
    of ``scale`` pixels per unit, ``K`` type slots, ``frame_ids`` (B,) numpy.  Returns ``{"neighbourhoods": float64 CUDA tensor
    (typed points x m, 11 + 6 K)}``.  Everything but the derived columns is an exact integer; the derived ones are torch
    operations on tensors, each rounded on its own."""
    planes = ops._req(planes, torch.uint8, 3)
    dev = planes.device
    B, K = planes.shape[0], int(K)
    e = np.asarray(edges, np.float64).reshape(-1)
    m = e.shape[0] - 1
    foff = points.frame_offsets
    inside, typed, slot_in, frame, n_in, _ = spatial._window_slots(points, points_rc, planes & 1, K)
    near = point_counts(points.coords, slot_in, foff, K, scale, e)                          # (n, K, m), -1 outside the window
    px, area = disk_counts(planes, window_queries(points_rc), foff, e, scale, sets=1 + K)   # (n, 1 + K, m), (B, 1 + K)
    rows = torch.nonzero(typed)[:, 0]
    r = rows.shape[0]
    fid = torch.as_tensor(np.asarray(frame_ids, np.float64)).to(dev)
    f64 = lambda t: t.to(torch.float64)
    own = points.slot[rows].to(torch.int64)
    seen = inside[rows]
    near, px = near[rows].to(torch.int64), px[rows].to(torch.int64)
    cum_near, cum_px = torch.cumsum(near, dim=2), torch.cumsum(px, dim=2)
    win, cum_win = f64(px[:, 0]), f64(cum_px[:, 0])                                          # (r, m)
    A = f64(area[frame[rows], 0])[:, None].expand(r, m)
    others = n_in[frame[rows]] - torch.nn.functional.one_hot(own, K).to(torch.int64)        # (r, K): N_t, less the row itself
    nan = torch.full((r, m), float("nan"), dtype=torch.float64, device=dev)
    cols = [fid[frame[rows]][:, None].expand(r, m), f64(points.ids[rows])[:, None].expand(r, m), f64(own)[:, None].expand(r, m),
            f64(seen)[:, None].expand(r, m), torch.arange(m, dtype=torch.float64, device=dev)[None, :].expand(r, m),
            torch.as_tensor(e[:-1]).to(dev)[None, :].expand(r, m), torch.as_tensor(e[1:]).to(dev)[None, :].expand(r, m)]
    counted = [win, cum_win]
    for t in range(K):
        N = f64(others[:, t])[:, None].expand(r, m)
        # every operand is a tensor: one correctly rounded product and one quotient each (no reciprocal, no fusing)
        expected, cum_expected = (N * win) / A, (N * cum_win) / A
        counted += [f64(near[:, t]), f64(cum_near[:, t]), f64(px[:, 1 + t]), f64(cum_px[:, 1 + t]), torch.where(A == 0, nan, expected),
                    torch.where(A == 0, nan, cum_expected)]
    pick = own[:, None, None].expand(r, 1, m)
    for cum, tot in ((cum_near, cum_near.sum(dim=1)), (cum_px[:, 1:], cum_px[:, 1:].sum(dim=1))):
        frac = f64(torch.gather(cum, 1, pick)[:, 0]) / f64(tot)
        counted.append(torch.where(tot == 0, nan, frac))
    counted = [torch.where(seen[:, None], c, nan) for c in counted]
    return {"neighbourhoods": torch.stack(cols + counted, dim=2).reshape(r * m, 11 + 6 * K)}
