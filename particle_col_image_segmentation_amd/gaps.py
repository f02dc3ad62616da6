"""Edge-to-edge gaps on the device: the nearest OTHER ROI of every strain (include/pcseg_gaps.h, csrc/gaps.hip).

The gap of two ROIs is the smallest distance between a pixel of one and a pixel of the other -- what matters for the
interaction of rods and clusters whose centroids lie many pixels from their rims.  The entries of ``pcseg_gaps.h`` live in the
same ``libpcseg.so``; this module holds their signature table, sets the prototypes on ``_lib.load()``'s handle and enters the
library through ``ops._call`` with the argument checks of ``ops`` ("The argument contract of ops": a tensor that
is not on the device, or of another dtype, is a ``TypeError``; another rank or shape a ``ValueError``; a non-contiguous input
is copied).
"""
from ctypes import c_int, c_int64, c_size_t, c_void_p

import torch

from . import _lib, ops

_P, _I = c_void_p, c_int
# name -> (restype, argtypes); mirrors include/pcseg_gaps.h one to one
SIGNATURES = {
    "pcseg_nearest_other_label_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_nearest_other_label_i32": (c_int, [_P, _P, _I, c_int64, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_label_gaps_workspace_bytes": (c_size_t, [_I, _I, _I, _I, _I]),
    "pcseg_label_gaps": (c_int, [_P, _P, _P, _I, _I, c_int64, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
}
MAX_WIDTH = 16382  # PCSEG_GAPS_MAX_WIDTH
_bound = None


def _load():
    """``_lib.load()``'s handle with the prototypes of ``pcseg_gaps.h`` declared on it (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def _width_within_limit(shape):
    if shape[2] > MAX_WIDTH:
        raise ValueError("a frame of %d columns: the limit is %d (PCSEG_GAPS_MAX_WIDTH)" % (shape[2], MAX_WIDTH))


def nearest_other_label(labels, sel=None, cap=None, r2=-1):
    """The exact nearest-label transform that leaves out the pixel's OWN label (csrc/gaps.hip): ``labels`` (B, H, W) int32 CUDA
    tensor of any width and alignment; a site is a pixel with a label in 1 .. ``cap`` (default: the width of ``sel``, else the
    largest label) that ``sel`` ((B, cap) uint8 / bool, optional) keeps -- the sites of :func:`ops.nearest_label`.  Returns
    ``(d2, near)``, int32 (B, H, W): the squared distance to the nearest site whose label differs from the pixel's, and the
    SMALLEST label among those sites at that distance.  Labels are compared as raw integers, so a pixel that carries no site's
    label (0, not selected, outside 1 .. cap) gets :func:`ops.nearest_label`'s pair.  With ``r2`` >= 0 sites farther than
    ``r2`` are ignored (one at exactly ``r2`` counts).  -1, 0 where there is no such site: a frame without site, a frame whose
    sites all carry the pixel's label, nothing within ``r2``.  ``ValueError`` for a frame wider than ``MAX_WIDTH``."""
    labels = ops._label_batch(labels)
    B, H, W = labels.shape
    if sel is not None:
        sel = ops._req(sel, torch.uint8, 2)
        if cap is None:
            cap = sel.shape[1]
        if tuple(sel.shape) != (B, int(cap)):
            raise ValueError("sel must be (B, cap)")
    _width_within_limit(labels.shape)
    if cap is None:
        cap = ops._default_cap(labels)
    cap = int(cap)
    dev = labels.device
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    near = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    if B < 1 or H < 1 or W < 1:
        return d2, near
    nbytes = _load().pcseg_nearest_other_label_workspace_bytes(B, H, W)
    if not nbytes:
        raise ValueError("nearest_other_label: a batch of shape %s is not supported" % ((B, H, W),))
    ops._call("nearest_other_label_i32", labels, sel, cap, int(r2), d2, near, B, H, W, ws=(ops._ws(nbytes, dev), nbytes))
    return d2, near


def label_gaps(labels, live, slot_of, n_types, r2=-1):
    """The smallest gap of every ROI to the ROIs of each type slot (csrc/gaps.hip).  ``labels`` (B, H, W) int32 CUDA tensor,
    ``live`` (B, cap) uint8 / bool: label l (row l - 1) is a ROI; ``slot_of`` (B, cap) uint8: its type slot, a value >=
    ``n_types`` (1 .. 4): no type.  Returns ``(gap2, partner)``, int32 (B, cap, n_types): for a live label l and slot t the
    smallest squared distance between a pixel of l and a pixel of a live label m != l of slot t (1: they touch along an edge,
    2: at a corner), and the smallest m that attains it; -1, 0 where there is none (within ``r2`` if ``r2`` >= 0), for a live
    label without pixel and for every row of a label that is not live.  Exact integers, bit for bit reproducible."""
    labels = ops._label_batch(labels)
    B, H, W = labels.shape
    live = ops._req(live, torch.uint8, 2)
    cap = live.shape[1]
    if live.shape[0] != B:
        raise ValueError("live must be (B, cap) for the labels' B frames, got %s" % (tuple(live.shape),))
    slot_of = ops._req(slot_of, torch.uint8, 2)
    if tuple(slot_of.shape) != (B, cap):
        raise ValueError("slot_of must have live's shape %s, got %s" % ((B, cap), tuple(slot_of.shape)))
    K = int(n_types)
    if not 1 <= K <= 4:
        raise ValueError("1 to 4 type slots")
    _width_within_limit(labels.shape)
    dev = labels.device
    gap2 = torch.empty((B, cap, K), dtype=torch.int32, device=dev)
    partner = torch.empty((B, cap, K), dtype=torch.int32, device=dev)
    if B < 1 or cap < 1:
        return gap2, partner
    nbytes = _load().pcseg_label_gaps_workspace_bytes(B, H, W, cap, K)
    if not nbytes:
        raise ValueError("label_gaps: a batch of shape %s with %d labels is not supported" % ((B, H, W), cap))
    ops._call("label_gaps", labels, live, slot_of, cap, K, int(r2), gap2, partner, B, H, W, ws=(ops._ws(nbytes, dev), nbytes))
    return gap2, partner


GAP_COLUMNS = ("frame", "label", "slot")


def _names(names_or_K):
    return ["%d" % k for k in range(names_or_K)] if isinstance(names_or_K, int) else [str(n) for n in names_or_K]


def gap_columns(names):
    """The columns of :func:`gap_rows` for the type slots ``names`` (their names, or their number)."""
    names = _names(names)
    return (list(GAP_COLUMNS) + ["gap_um_%s" % n for n in names] + ["gap_label_%s" % n for n in names]
            + ["gap_px2_%s" % n for n in names])


def gap_rows(labels, live, slot_of, frame_ids, scale, names_or_K, r2=-1):
    """The ``gaps`` table of one label batch: :func:`label_gaps` on the whole batch, then the rows ``live`` in (frame, label)
    order as float64 ``[frame, label, slot, gap_um_<type>.., gap_label_<type>.., gap_px2_<type>..]`` (:func:`gap_columns`):
    ``gap_um = sqrt(float64(gap_px2)) / scale`` -- one correctly rounded square root and one division --, NaN where there is
    no partner; ``gap_label`` and ``gap_px2`` are -1 there (the conventions of ``neighbours``).  ``frame_ids`` (B,) CUDA
    tensor, ``scale`` pixels per um."""
    K = len(_names(names_or_K))
    live = ops._req(live, torch.uint8, 2)
    gap2, partner = label_gaps(labels, live, slot_of, max(K, 1), r2)
    b, l, head = ops._row_head(live != 0, slot_of, frame_ids)
    g = gap2[b, l][:, :K].to(torch.float64)
    some = g >= 0
    um = ops._over(torch.sqrt(torch.where(some, g, torch.zeros_like(g))), float(scale))
    um = torch.where(some, um, torch.full_like(um, float("nan")))
    who = torch.where(some, partner[b, l][:, :K].to(torch.float64), torch.full_like(g, -1.0))
    return torch.cat([torch.stack(head, dim=1), um, who, g], dim=1)
